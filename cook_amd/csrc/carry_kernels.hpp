// carry_kernels.hpp — device side of the carry (cook_cycle_run_queue_carry*): a queue cycle's advance moves the last
// cycle's KEPT placements (job_to_offer >= 0, offer not skipped: q_mark_removed's predicate) into the staged offers and the staged
// user state.
//
// Index spaces: i = considered position of the pool's last cycle (j2o[i] its offer, j_index[i] its pending ordinal = its row in the
//               staged job columns); p = position in a stable sort of the considered positions by key; v = offer; u = user.
// The order rule: every fp64 sum runs over the kept jobs of its segment in CONSIDERED order, left to right, one add after another
// from 0.0, which is the order in which the placement itself accumulated "assigned this call".  So: keys -> the STABLE radix passes of
// sort.hpp (equal keys keep considered order) -> segment bounds -> one workgroup per segment that stages a chunk of job rows in LDS
// with coalesced gathers and lets ONE lane per column chain the adds.  No fp64 atomics, no tree: the chain is the definition.
#pragma once
#include "common.hpp"

// the job columns a fold gathers through j_index (null columns: all 0 / no request)
struct CarryJobs {
  const uint32_t* j_index;
  const double *cpus, *mem, *gpus, *disk_req;
  const uint32_t *gpu_model, *disk_type;
  const int32_t* ports;
  const double* scal[3];
};
// the offer columns the carry changes: `in` the staged ones (null: all 0), `out` the engine's own copy ([M] each, [M][slots] the maps;
// null where the staged offers have no such column and the carry makes none)
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

static __device__ __forceinline__ bool carry_kept(const int32_t* __restrict__ j2o, const uint8_t* __restrict__ offer_skipped, unsigned i) {
  const int o = j2o[i];
  return o >= 0 && !(offer_skipped && offer_skipped[o]);
}

// key of considered job i: its offer / its user when its placement is kept, else the sentinel M / U (sorted behind every segment).
// okey or ukey may be null.
COOK_KERNEL void carry_keys(const int32_t* __restrict__ j2o, unsigned k, const uint8_t* __restrict__ offer_skipped,
                            const uint32_t* __restrict__ j_index, const uint32_t* __restrict__ j_user, unsigned M, unsigned U,
                            uint64_t* __restrict__ okey, uint64_t* __restrict__ ukey) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const bool hit = carry_kept(j2o, offer_skipped, i);
  if (okey) okey[i] = hit ? (uint64_t)(unsigned)j2o[i] : (uint64_t)M;
  if (ukey) {
    const unsigned u = hit ? j_user[j_index[i]] : U;
    ukey[i] = (uint64_t)(u < U ? u : U);
  }
}

// seg_start / seg_end are zero beforehand (a key without kept jobs keeps the empty segment [0, 0))
COOK_KERNEL void carry_seg_bounds(const uint32_t* __restrict__ perm, const uint64_t* __restrict__ key, unsigned k, unsigned n_seg,
                                  uint32_t* __restrict__ seg_start, uint32_t* __restrict__ seg_end) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= k) return;
  const uint64_t x = key[perm[p]];
  if (x >= n_seg) return;
  if (p == 0 || key[perm[p - 1]] != x) seg_start[x] = p;
  if (p + 1 == k || key[perm[p + 1]] != x) seg_end[x] = p + 1;
}

// ---- per offer ------------------------------------------------------------------------------------------------------------------------
// One wave per offer (its segment is a handful of jobs).  Lanes 0..4 chain cpus, mem and the three named scalars; lane 5 walks the gpu
// map, lane 6 the disk map, lane 7 adds the port counts.  Every offer's row is written: the columns are a fresh copy.
constexpr int CARRY_OT = COOK_WAVE;
COOK_KERNEL void carry_fold_offers(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ seg_start,
                                   const uint32_t* __restrict__ seg_end, unsigned M, CarryJobs j, CarryOfferIn in, CarryOfferCols out) {
  __shared__ double t_sum[5][CARRY_OT];
  __shared__ double t_gpus[CARRY_OT], t_disk[CARRY_OT];
  __shared__ uint32_t t_model[CARRY_OT], t_dtype[CARRY_OT];
  __shared__ int32_t t_ports[CARRY_OT];
  const unsigned v = blockIdx.x, tid = threadIdx.x;
  if (v >= M) return;  // (uniform per workgroup)
  const unsigned lo = seg_start[v], hi = seg_end[v];
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
  for (unsigned base = lo; base < hi; base += CARRY_OT) {
    const unsigned n = hi - base < (unsigned)CARRY_OT ? hi - base : (unsigned)CARRY_OT;
    if (tid < n) {
      const unsigned jj = j.j_index[perm[base + tid]];
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
        if (r == r) acc = acc + r;  // (NaN: the job has no request under this name; cpus and mem are never NaN in a placed job)
      }
    } else if (tid == 5u) {
      for (unsigned t = 0; t < n; ++t) {
        const double g = t_gpus[t];
        const uint32_t key = t_model[t];
        if (k8s && g > 0.0 && key != 0u)
          for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
            if (s < gs && slot_key[s] == key) slot[s] = slot[s] - g;
      }
    } else if (tid == 6u) {
      for (unsigned t = 0; t < n; ++t) {
        const double d = t_disk[t];
        const uint32_t key = t_dtype[t];
        if (k8s && d >= 0.0 && key != 0u)
          for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
            if (s < ds && slot_key[s] == key) slot[s] = slot[s] - d;
      }
    } else if (tid == 7u) {
      for (unsigned t = 0; t < n; ++t) iacc += t_ports[t] > 0 ? t_ports[t] : 0;
    }
    __syncthreads();
  }
  const int cnt = (int)(hi - lo);
  if (tid == 0u) {
    out.cpus[v] = in.cpus[v] - acc;
    out.run_cpus[v] = (in.run_cpus ? in.run_cpus[v] : 0.0) + acc;
    out.run_count[v] = (in.run_count ? in.run_count[v] : 0) + cnt;
    out.num_tasks[v] = (in.num_tasks ? in.num_tasks[v] : 0) + cnt;
  } else if (tid == 1u) {
    out.mem[v] = in.mem[v] - acc;
    out.run_mem[v] = (in.run_mem ? in.run_mem[v] : 0.0) + acc;
  } else if (tid < 5u) {
    for (unsigned s = 0; s < 3u; ++s)  // (constant indices: the argument structures stay in registers)
      if (tid == 2u + s && out.scal[s]) out.scal[s][v] = in.scal[s][v] - acc;
  } else if (tid == 5u) {
    if (out.gpu_count)
      for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
        if (s < gs) out.gpu_count[(size_t)v * gs + s] = slot[s];
  } else if (tid == 6u) {
    if (out.disk_space)
      for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
        if (s < ds) out.disk_space[(size_t)v * ds + s] = slot[s];
  } else if (tid == 7u) {
    out.ports[v] = (int32_t)((long long)(in.ports ? in.ports[v] : 0) - iacc);
  }
}

// ---- per user, and the pool --------------------------------------------------------------------------------------------------------
// A user's segment can hold thousands of jobs (the user sizes are Zipf-skewed), and the pool's "segment" is every kept job.  One
// workgroup per segment: all threads gather the NEXT chunk of rows into registers while lanes 0..2 chain cpus / mem / gpus over the chunk
// in LDS, so the gathers are coalesced and in flight while the adds chain.  -> the three sums in lanes 0..2 of the workgroup, the
// number of jobs summed in every thread.
constexpr int CARRY_UT = 256;
struct CarryRow {
  double c, m, g;
  unsigned ok;
};
// FILTER: the segment is the considered positions [lo, hi) themselves and only the kept ones count (the pool); else perm[lo .. hi)
template <bool FILTER>
static __device__ __forceinline__ CarryRow carry_load_row(const uint32_t* __restrict__ perm, unsigned p, unsigned hi,
                                                          const int32_t* __restrict__ j2o, const uint8_t* __restrict__ offer_skipped,
                                                          const CarryJobs& j) {
  CarryRow r{0.0, 0.0, 0.0, 0u};
  if (p >= hi) return r;
  const unsigned i = FILTER ? p : perm[p];
  if (FILTER && !carry_kept(j2o, offer_skipped, i)) return r;
  const unsigned jj = j.j_index[i];
  r.c = j.cpus[jj], r.m = j.mem[jj], r.g = j.gpus ? j.gpus[jj] : 0.0, r.ok = 1u;
  return r;
}
template <bool FILTER>
static __device__ __forceinline__ double carry_chain3(const uint32_t* __restrict__ perm, unsigned lo, unsigned hi,
                                                      const int32_t* __restrict__ j2o, const uint8_t* __restrict__ offer_skipped,
                                                      const CarryJobs& j, unsigned* n_summed) {
  __shared__ double t_val[3][CARRY_UT];
  __shared__ unsigned t_ok[CARRY_UT];
  __shared__ unsigned t_cnt;
  const unsigned tid = threadIdx.x;
  double acc = 0.0;
  unsigned cnt = 0;
  CarryRow nx = carry_load_row<FILTER>(perm, lo + tid, hi, j2o, offer_skipped, j);
  for (unsigned base = lo; base < hi; base += CARRY_UT) {
    t_val[0][tid] = nx.c, t_val[1][tid] = nx.m, t_val[2][tid] = nx.g, t_ok[tid] = nx.ok;
    __syncthreads();
    nx = carry_load_row<FILTER>(perm, base + CARRY_UT + tid, hi, j2o, offer_skipped, j);
    const unsigned n = hi - base < (unsigned)CARRY_UT ? hi - base : (unsigned)CARRY_UT;
    if (tid < 3u) {
      for (unsigned t = 0; t < n; ++t)
        if (!FILTER || t_ok[t]) acc = acc + t_val[tid][t];
    } else if (tid == 3u) {
      for (unsigned t = 0; t < n; ++t) cnt += t_ok[t];
    }
    __syncthreads();
  }
  if (tid == 3u) t_cnt = cnt;
  __syncthreads();
  *n_summed = t_cnt;
  return acc;
}

// usage arrays and tokens in place (each user is one workgroup's, read before it is written); tokens may be null (none staged, or
// the host replaced them)
COOK_KERNEL void carry_fold_users(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ seg_start,
                                  const uint32_t* __restrict__ seg_end, unsigned U, CarryJobs j, double* __restrict__ ucount,
                                  double* __restrict__ ucpus, double* __restrict__ umem, double* __restrict__ ugpus,
                                  int64_t* __restrict__ tokens) {
  const unsigned u = blockIdx.x, tid = threadIdx.x;
  if (u >= U) return;
  const unsigned lo = seg_start[u], hi = seg_end[u];
  if (lo >= hi) return;  // (x + 0.0 == x for every x a sum from +0.0 can reach: nothing to write)
  unsigned n = 0;
  const double acc = carry_chain3<false>(perm, lo, hi, (const int32_t*)nullptr, (const uint8_t*)nullptr, j, &n);
  if (tid == 0u) ucpus[u] = ucpus[u] + acc;
  else if (tid == 1u) umem[u] = umem[u] + acc;
  else if (tid == 2u) ugpus[u] = ugpus[u] + acc;
  else if (tid == 3u) {
    ucount[u] = ucount[u] + (double)n;
    if (tokens) tokens[u] = tokens[u] - (int64_t)n;
  }
}

// out[0..3] = {count, cpus, mem, gpus} over ALL kept jobs in considered order (one workgroup)
COOK_KERNEL void carry_fold_pool(const int32_t* __restrict__ j2o, unsigned k, const uint8_t* __restrict__ offer_skipped, CarryJobs j,
                                 double* __restrict__ out) {
  if (blockIdx.x != 0u) return;
  unsigned n = 0;
  const double acc = carry_chain3<true>((const uint32_t*)nullptr, 0u, k, j2o, offer_skipped, j, &n);
  if (threadIdx.x < 3u) out[1u + threadIdx.x] = acc;
  else if (threadIdx.x == 3u) out[0] = (double)n;
}
