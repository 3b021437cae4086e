// fold_kernels.hpp — the ordered fold of the carry and the release: rows of job columns, grouped into segments by a
// stable sort, are summed into the staged offers and the staged user state.  GIVE_BACK = false takes the rows' resources (the carry: a
// kept placement uses its offer), true gives them back (the release: a finished task frees its host).
//
// The order rule: every fp64 sum runs over the rows of its segment in the segment's order, left to right, one add after another from
// 0.0.  One workgroup per segment stages a chunk of rows in LDS with coalesced gathers and lets ONE lane per column chain the adds.  No
// fp64 atomics, no tree, no negated accumulator: the chain is the definition, and the sum meets the column in one literal + or -.
#pragma once
#include "common.hpp"

// the row columns a fold gathers (null columns: all 0 / no request).  j_index: position -> row; null: the row is the position itself
struct CarryJobs {
  const uint32_t* j_index;
  const double *cpus, *mem, *gpus, *disk_req;
  const uint32_t *gpu_model, *disk_type;
  const int32_t* ports;
  const double* scal[3];
};
static __device__ __forceinline__ unsigned fold_index(const CarryJobs& j, unsigned i) { return j.j_index ? j.j_index[i] : i; }
// the offer columns a fold changes: `in` the staged ones (null: all 0), `out` the engine's own copy ([M] each, [M][slots] the maps;
// null where the staged offers have no such column and the fold makes none)
struct CarryOfferCols {
  double *cpus, *mem, *run_cpus, *run_mem, *scal[3], *gpu_count, *disk_space;
  int32_t *run_count, *num_tasks, *ports;
};
struct CarryOfferIn {
  const double *cpus, *mem, *run_cpus, *run_mem, *scal[3], *gpu_count, *disk_space;
  const int32_t *run_count, *num_tasks, *ports;
  const uint8_t* k8s;
  const uint32_t *gpu_model, *disk_type;
  unsigned gpu_slots, disk_slots;
};

// a sum meets what is FREE in an offer / what is IN USE (an offer's running totals, a user's usage)
template <bool GIVE_BACK, class T>
static __device__ __forceinline__ T fold_free(T x, T sum) { return GIVE_BACK ? x + sum : x - sum; }
template <bool GIVE_BACK, class T>
static __device__ __forceinline__ T fold_used(T x, T sum) { return fold_free<!GIVE_BACK>(x, sum); }

// ---- per offer ------------------------------------------------------------------------------------------------------------------------
// One wave per offer (its segment is a handful of rows).  Lanes 0..4 chain cpus, mem and the three named scalars; lane 5 walks the gpu
// map, lane 6 the disk map, lane 7 adds the port counts.  Taking: `out` is a fresh copy and every offer's row is written.  Giving back:
// copy_all != 0 likewise; 0: out is the set the carry of this advance has just written (in == out, one wave owns one row) and a row
// without entries is left alone; *clamped counts the rows whose run_count / num_tasks would have gone below 0 and stopped there.
constexpr int FOLD_OT = COOK_WAVE;
template <bool GIVE_BACK>
COOK_KERNEL void fold_offers(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_end,
                             unsigned M, unsigned copy_all, CarryJobs j, CarryOfferIn in, CarryOfferCols out, unsigned* __restrict__ clamped) {
  __shared__ double t_sum[5][FOLD_OT];
  __shared__ double t_gpus[FOLD_OT], t_disk[FOLD_OT];
  __shared__ uint32_t t_model[FOLD_OT], t_dtype[FOLD_OT];
  __shared__ int32_t t_ports[FOLD_OT];
  const unsigned v = blockIdx.x, tid = threadIdx.x;
  if (v >= M) return;  // (uniform per workgroup)
  const unsigned lo = seg_start[v], hi = seg_end[v];
  if constexpr (GIVE_BACK)
    if (lo >= hi && !copy_all) return;
  const bool k8s = in.k8s && in.k8s[v];
  const unsigned gs = in.gpu_slots, ds = in.disk_slots;
  double acc = 0.0;
  long long iacc = 0;
  double slot[COOK_MAX_RES_SLOTS] = {0.0, 0.0, 0.0, 0.0};
  uint32_t slot_key[COOK_MAX_RES_SLOTS] = {0u, 0u, 0u, 0u};
  if (tid == 5 && in.gpu_count)
    for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
      if (s < gs) slot[s] = in.gpu_count[(size_t)v * gs + s], slot_key[s] = in.gpu_model ? in.gpu_model[(size_t)v * gs + s] : 0u;
  if (tid == 6 && in.disk_space)
    for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
      if (s < ds) slot[s] = in.disk_space[(size_t)v * ds + s], slot_key[s] = in.disk_type ? in.disk_type[(size_t)v * ds + s] : 0u;
  for (unsigned base = lo; base < hi; base += FOLD_OT) {
    const unsigned n = hi - base < (unsigned)FOLD_OT ? hi - base : (unsigned)FOLD_OT;
    if (tid < n) {
      const unsigned jj = fold_index(j, perm[base + tid]);
      t_sum[0][tid] = j.cpus[jj];
      t_sum[1][tid] = j.mem[jj];
      for (unsigned s = 0; s < 3u; ++s) t_sum[2 + s][tid] = j.scal[s] ? j.scal[s][jj] : __longlong_as_double(0x7FF8000000000000ll);
      t_gpus[tid] = j.gpus ? j.gpus[jj] : 0.0;
      t_model[tid] = j.gpu_model ? j.gpu_model[jj] : 0u;
      t_disk[tid] = j.disk_req ? j.disk_req[jj] : -1.0;
      t_dtype[tid] = j.disk_type ? j.disk_type[jj] : 0u;
      t_ports[tid] = j.ports ? j.ports[jj] : 0;
    }
    __syncthreads();
    if (tid < 5u) {
      for (unsigned t = 0; t < n; ++t) {
        const double r = t_sum[tid][t];
        if (r == r) acc = acc + r;  // (NaN: the row has no request under this name; cpus and mem are never NaN)
      }
    } else if (tid == 5u) {
      for (unsigned t = 0; t < n; ++t) {
        const double g = t_gpus[t];
        const uint32_t key = t_model[t];
        if (k8s && g > 0.0 && key != 0u)
          for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
            if (s < gs && slot_key[s] == key) slot[s] = fold_free<GIVE_BACK>(slot[s], g);
      }
    } else if (tid == 6u) {
      for (unsigned t = 0; t < n; ++t) {
        const double d = t_disk[t];
        const uint32_t key = t_dtype[t];
        if (k8s && d >= 0.0 && key != 0u)
          for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
            if (s < ds && slot_key[s] == key) slot[s] = fold_free<GIVE_BACK>(slot[s], d);
      }
    } else if (tid == 7u) {
      for (unsigned t = 0; t < n; ++t) iacc += t_ports[t] > 0 ? t_ports[t] : 0;
    }
    __syncthreads();
  }
  const int cnt = (int)(hi - lo);
  if (tid == 0u) {
    const int rc = fold_used<GIVE_BACK>(in.run_count ? in.run_count[v] : 0, cnt), nt = fold_used<GIVE_BACK>(in.num_tasks ? in.num_tasks[v] : 0, cnt);
    out.cpus[v] = fold_free<GIVE_BACK>(in.cpus[v], acc);
    out.run_cpus[v] = fold_used<GIVE_BACK>(in.run_cpus ? in.run_cpus[v] : 0.0, acc);
    out.run_count[v] = GIVE_BACK && rc < 0 ? 0 : rc;
    out.num_tasks[v] = GIVE_BACK && nt < 0 ? 0 : nt;
    if constexpr (GIVE_BACK)
      if (rc < 0 || nt < 0) atomicAdd(clamped, 1u);
  } else if (tid == 1u) {
    out.mem[v] = fold_free<GIVE_BACK>(in.mem[v], acc);
    out.run_mem[v] = fold_used<GIVE_BACK>(in.run_mem ? in.run_mem[v] : 0.0, acc);
  } else if (tid < 5u) {
    for (unsigned s = 0; s < 3u; ++s)  // (constant indices: the argument structures stay in registers)
      if (tid == 2u + s && out.scal[s]) out.scal[s][v] = fold_free<GIVE_BACK>(in.scal[s][v], acc);
  } else if (tid == 5u) {
    if (out.gpu_count)
      for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
        if (s < gs) out.gpu_count[(size_t)v * gs + s] = slot[s];
  } else if (tid == 6u) {
    if (out.disk_space)
      for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
        if (s < ds) out.disk_space[(size_t)v * ds + s] = slot[s];
  } else if (tid == 7u) {
    out.ports[v] = (int32_t)fold_free<GIVE_BACK>((long long)(in.ports ? in.ports[v] : 0), iacc);
  }
}

// ---- per user, and the pool --------------------------------------------------------------------------------------------------------
// A user's segment can hold thousands of rows (the user sizes are Zipf-skewed), and the pool's "segment" is every row.  One workgroup
// per segment: all threads gather the NEXT chunk of rows into registers while lanes 0..2 chain cpus / mem / gpus over the chunk in LDS,
// so the gathers are coalesced and in flight while the adds chain.  -> the three sums in lanes 0..2 of the workgroup and, with COUNT,
// the number of rows summed in every thread.
constexpr int FOLD_UT = 256;
struct CarryRow { double c, m, g; unsigned ok; };
static __device__ __forceinline__ CarryRow fold_row(const CarryJobs& j, unsigned i) {
  const unsigned jj = fold_index(j, i);
  return CarryRow{j.cpus[jj], j.mem[jj], j.gpus ? j.gpus[jj] : 0.0, 1u};
}
// position of a sort — with perm null, the position itself — -> its row
struct RowsSorted {
  static constexpr bool FILTER = false;
  const uint32_t* perm;
  CarryJobs j;
  __device__ __forceinline__ CarryRow operator()(unsigned p) const { return fold_row(j, perm ? perm[p] : p); }
};

// Load: position -> CarryRow; Load::FILTER: a row may come back with ok = 0 and then counts nothing
template <bool COUNT, class Load>
static __device__ __forceinline__ double chain3(const Load& load, unsigned lo, unsigned hi, unsigned* n_summed) {
  __shared__ double t_val[3][FOLD_UT];
  __shared__ unsigned t_ok[FOLD_UT], t_cnt;  // (only with COUNT or Load::FILTER)
  const unsigned tid = threadIdx.x;
  double acc = 0.0;
  unsigned cnt = 0;
  CarryRow nx = lo + tid < hi ? load(lo + tid) : CarryRow{};
  for (unsigned base = lo; base < hi; base += FOLD_UT) {
    t_val[0][tid] = nx.c, t_val[1][tid] = nx.m, t_val[2][tid] = nx.g;
    if constexpr (COUNT || Load::FILTER) t_ok[tid] = nx.ok;
    __syncthreads();
    nx = base + FOLD_UT + tid < hi ? load(base + FOLD_UT + tid) : CarryRow{};
    const unsigned n = hi - base < (unsigned)FOLD_UT ? hi - base : (unsigned)FOLD_UT;
    if (tid < 3u) {
      for (unsigned t = 0; t < n; ++t)
        if (!Load::FILTER || t_ok[t]) acc = acc + t_val[tid][t];
    } else if constexpr (COUNT) {
      if (tid == 3u)
        for (unsigned t = 0; t < n; ++t) cnt += t_ok[t];
    }
    __syncthreads();
  }
  if constexpr (COUNT) {
    if (tid == 3u) t_cnt = cnt;
    __syncthreads();
    *n_summed = t_cnt;
  }
  return acc;
}

// usage arrays in place (each user is one workgroup's, read before it is written).  Taking spends the tokens too; they may be null
// (none staged, the host replaced them, or the engine's own limiters spend: limiter_host.hpp).  Giving back leaves them alone and counts the segment's length.
template <bool GIVE_BACK, class Load>
COOK_KERNEL void fold_users(Load load, const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_end, unsigned U,
                            double* __restrict__ ucount, double* __restrict__ ucpus, double* __restrict__ umem, double* __restrict__ ugpus,
                            int64_t* __restrict__ tokens) {
  const unsigned u = blockIdx.x, tid = threadIdx.x;
  if (u >= U) return;
  const unsigned lo = seg_start[u], hi = seg_end[u];
  if (lo >= hi) return;  // (x + 0.0 == x for every x a sum from +0.0 can reach: nothing to write)
  unsigned n = hi - lo;
  const double acc = chain3<!GIVE_BACK>(load, lo, hi, &n);
  if (tid == 0u) ucpus[u] = fold_used<GIVE_BACK>(ucpus[u], acc);
  else if (tid == 1u) umem[u] = fold_used<GIVE_BACK>(umem[u], acc);
  else if (tid == 2u) ugpus[u] = fold_used<GIVE_BACK>(ugpus[u], acc);
  else if (tid == 3u) {
    ucount[u] = fold_used<GIVE_BACK>(ucount[u], (double)n);
    if (!GIVE_BACK && tokens) tokens[u] = tokens[u] - (int64_t)n;
  }
}

// out[0..3] = {count, cpus, mem, gpus} over the rows at ALL positions [0, n) in order (one workgroup); the host adds or subtracts them
template <bool GIVE_BACK, class Load>
COOK_KERNEL void fold_pool(Load load, unsigned n, double* __restrict__ out) {
  if (blockIdx.x != 0u) return;
  unsigned cnt = n;
  const double acc = chain3<!GIVE_BACK>(load, 0u, n, &cnt);
  if (threadIdx.x < 3u) out[1u + threadIdx.x] = acc;
  else if (threadIdx.x == 3u) out[0] = (double)cnt;
}
