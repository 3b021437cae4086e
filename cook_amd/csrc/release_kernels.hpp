// release_kernels.hpp — device side of the release (cook_cycle_run_queue_release*), the inverse of the carry: a queue
// cycle's advance gives the resources of a short list of FINISHED tasks back to the staged offers, takes them out of the staged user
// state and removes them from the groups' running-cotask lists.
//
// Index spaces: t = entry of the list (list order = the order rule's order); p = position in a stable sort of the entries by key;
//               v = offer (row of the staged offers); u = user; g = group; x = row of the groups' running-cotask table (CSR by g).
// The order rule: every fp64 sum runs over the entries of its segment in LIST order, left to right, one add after another from 0.0.
// So: keys -> the STABLE radix passes of sort.hpp (equal keys keep list order) -> segment bounds (carry_seg_bounds) -> one wave per
// offer / one workgroup per user that stages a chunk of entries in LDS and lets ONE lane per column chain the adds.  No fp64 atomics,
// no tree: the chain is the definition.  The fold kernels are the carry's with the sign turned and the rows read from the list itself.
#pragma once
#include "carry_kernels.hpp"
#include "common.hpp"
#include "scan.hpp"

// words of QueueBufs::counters behind the advance's two: read back in the advance's one synchronisation
constexpr unsigned REL_CNT_NO_ROW = 2, REL_CNT_CLAMPED = 3, REL_CNT_MISSING = 4, REL_CNT_WORDS = 8;

// the list's columns on the device (null columns: all 0 / no request)
struct ReleaseList {
  const uint32_t *host, *user, *group;
  const double *cpus, *mem, *gpus, *disk_req;
  const uint32_t *gpu_model, *disk_type;
  const int32_t* ports;
  const double* scal[3];
};

// host id -> row of the staged offers; the table is 0xFF-filled beforehand (a host without a row keeps 0xFFFFFFFF).  One row per host:
// the release is refused while two staged offers share a host.
COOK_KERNEL void release_host_rows(const uint32_t* __restrict__ o_host, unsigned M, unsigned n_hosts, uint32_t* __restrict__ h2row) {
  const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= M) return;
  const uint32_t h = o_host[v];
  if (h < n_hosts) h2row[h] = v;
}

// keys of entry t: its row or the sentinel M, its user or U, its group or G.  h2row null: the greatest host id of the staged offers is
// not known (offers built on the device) — the row is looked up in o_host itself.  counters[REL_CNT_NO_ROW] += entries without a row,
// one atomic per wave.  okey, ukey or gkey may be null.
COOK_KERNEL void release_keys(ReleaseList l, unsigned n, const uint32_t* __restrict__ h2row, unsigned n_hosts,
                              const uint32_t* __restrict__ o_host, unsigned M, unsigned U, unsigned G, uint64_t* __restrict__ okey,
                              uint64_t* __restrict__ ukey, uint64_t* __restrict__ gkey, unsigned* __restrict__ counters) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  bool no_row = false;
  if (t < n) {
    if (okey) {
      const uint32_t h = l.host[t];
      unsigned v = M;
      if (h2row) {
        if (h < n_hosts && h2row[h] < M) v = h2row[h];
      } else {
        for (unsigned x = 0; x < M; ++x)
          if (o_host[x] == h) {
            v = x;
            break;
          }
      }
      okey[t] = (uint64_t)v;
      no_row = v == M;
    }
    if (ukey) {
      const unsigned u = l.user[t];
      ukey[t] = (uint64_t)(u < U ? u : U);
    }
    if (gkey) {
      const unsigned g = l.group ? l.group[t] : G;
      gkey[t] = (uint64_t)(g < G ? g : G);
    }
  }
  const unsigned long long b = __ballot(no_row);
  if (lane_id() == 0 && b) atomicAdd(&counters[REL_CNT_NO_ROW], (unsigned)__popcll(b));
}

// ---- per offer ------------------------------------------------------------------------------------------------------------------------
// One wave per offer, as carry_fold_offers: lanes 0..4 chain cpus, mem and the three named scalars; lane 5 walks the gpu map, lane 6 the
// disk map, lane 7 adds the port counts.  copy_all != 0: `out` is a fresh set of columns and every row is written; 0: out is the set the
// carry of this advance has just written (in == out, one wave owns one row) and a row without entries is left alone.
constexpr int RELEASE_OT = COOK_WAVE;
COOK_KERNEL void release_fold_offers(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ seg_start,
                                     const uint32_t* __restrict__ seg_end, unsigned M, unsigned copy_all, ReleaseList l, CarryOfferIn in,
                                     CarryOfferCols out, unsigned* __restrict__ counters) {
  __shared__ double t_sum[5][RELEASE_OT];
  __shared__ double t_gpus[RELEASE_OT], t_disk[RELEASE_OT];
  __shared__ uint32_t t_model[RELEASE_OT], t_dtype[RELEASE_OT];
  __shared__ int32_t t_ports[RELEASE_OT];
  const unsigned v = blockIdx.x, tid = threadIdx.x;
  if (v >= M) return;  // (uniform per workgroup)
  const unsigned lo = seg_start[v], hi = seg_end[v];
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
  for (unsigned base = lo; base < hi; base += RELEASE_OT) {
    const unsigned n = hi - base < (unsigned)RELEASE_OT ? hi - base : (unsigned)RELEASE_OT;
    if (tid < n) {
      const unsigned t = perm[base + tid];
      t_sum[0][tid] = l.cpus[t];
      t_sum[1][tid] = l.mem[t];
      for (unsigned s = 0; s < 3u; ++s) t_sum[2 + s][tid] = l.scal[s] ? l.scal[s][t] : __longlong_as_double(0x7FF8000000000000ll);
      t_gpus[tid] = l.gpus ? l.gpus[t] : 0.0;
      t_model[tid] = l.gpu_model ? l.gpu_model[t] : 0u;
      t_disk[tid] = l.disk_req ? l.disk_req[t] : -1.0;
      t_dtype[tid] = l.disk_type ? l.disk_type[t] : 0u;
      t_ports[tid] = l.ports ? l.ports[t] : 0;
    }
    __syncthreads();
    if (tid < 5u) {
      for (unsigned t = 0; t < n; ++t) {
        const double r = t_sum[tid][t];
        if (r == r) acc = acc + r;  // (NaN: no request under this name)
      }
    } else if (tid == 5u) {
      for (unsigned t = 0; t < n; ++t) {
        const double g = t_gpus[t];
        const uint32_t key = t_model[t];
        if (k8s && g > 0.0 && key != 0u)
          for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
            if (s < gs && slot_key[s] == key) slot[s] = slot[s] + g;
      }
    } else if (tid == 6u) {
      for (unsigned t = 0; t < n; ++t) {
        const double d = t_disk[t];
        const uint32_t key = t_dtype[t];
        if (k8s && d >= 0.0 && key != 0u)
          for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
            if (s < ds && slot_key[s] == key) slot[s] = slot[s] + d;
      }
    } else if (tid == 7u) {
      for (unsigned t = 0; t < n; ++t) iacc += t_ports[t] > 0 ? t_ports[t] : 0;
    }
    __syncthreads();
  }
  const int cnt = (int)(hi - lo);
  if (tid == 0u) {
    const int rc = (in.run_count ? in.run_count[v] : 0) - cnt, nt = (in.num_tasks ? in.num_tasks[v] : 0) - cnt;
    out.cpus[v] = in.cpus[v] + acc;
    out.run_cpus[v] = (in.run_cpus ? in.run_cpus[v] : 0.0) - acc;
    out.run_count[v] = rc > 0 ? rc : 0;
    out.num_tasks[v] = nt > 0 ? nt : 0;
    if (rc < 0 || nt < 0) atomicAdd(&counters[REL_CNT_CLAMPED], 1u);
  } else if (tid == 1u) {
    out.mem[v] = in.mem[v] + acc;
    out.run_mem[v] = (in.run_mem ? in.run_mem[v] : 0.0) - acc;
  } else if (tid < 5u) {
    for (unsigned s = 0; s < 3u; ++s)  // (constant indices: the argument structures stay in registers)
      if (tid == 2u + s && out.scal[s]) out.scal[s][v] = in.scal[s][v] + acc;
  } else if (tid == 5u) {
    if (out.gpu_count)
      for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
        if (s < gs) out.gpu_count[(size_t)v * gs + s] = slot[s];
  } else if (tid == 6u) {
    if (out.disk_space)
      for (unsigned s = 0; s < (unsigned)COOK_MAX_RES_SLOTS; ++s)
        if (s < ds) out.disk_space[(size_t)v * ds + s] = slot[s];
  } else if (tid == 7u) {
    out.ports[v] = (int32_t)((long long)(in.ports ? in.ports[v] : 0) + iacc);
  }
}

// ---- per user, and the pool --------------------------------------------------------------------------------------------------------
// One workgroup per segment, as carry_chain3: all threads gather the NEXT chunk of entries into registers while lanes 0..2 chain
// cpus / mem / gpus over the chunk in LDS.  perm null: the segment is the list positions [lo, hi) themselves (the pool).
// -> the three sums in lanes 0..2 of the workgroup.
constexpr int RELEASE_UT = 256;
static __device__ __forceinline__ CarryRow release_load_row(const uint32_t* __restrict__ perm, unsigned p, unsigned hi, const ReleaseList& l) {
  CarryRow r{0.0, 0.0, 0.0, 0u};
  if (p >= hi) return r;
  const unsigned t = perm ? perm[p] : p;
  r.c = l.cpus[t], r.m = l.mem[t], r.g = l.gpus ? l.gpus[t] : 0.0, r.ok = 1u;
  return r;
}
static __device__ __forceinline__ double release_chain3(const uint32_t* __restrict__ perm, unsigned lo, unsigned hi, const ReleaseList& l) {
  __shared__ double t_val[3][RELEASE_UT];
  const unsigned tid = threadIdx.x;
  double acc = 0.0;
  CarryRow nx = release_load_row(perm, lo + tid, hi, l);
  for (unsigned base = lo; base < hi; base += RELEASE_UT) {
    t_val[0][tid] = nx.c, t_val[1][tid] = nx.m, t_val[2][tid] = nx.g;
    __syncthreads();
    nx = release_load_row(perm, base + RELEASE_UT + tid, hi, l);
    const unsigned n = hi - base < (unsigned)RELEASE_UT ? hi - base : (unsigned)RELEASE_UT;
    if (tid < 3u)
      for (unsigned t = 0; t < n; ++t) acc = acc + t_val[tid][t];
    __syncthreads();
  }
  return acc;
}

// usage arrays in place (each user is one workgroup's, read before it is written)
COOK_KERNEL void release_fold_users(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ seg_start,
                                    const uint32_t* __restrict__ seg_end, unsigned U, ReleaseList l, double* __restrict__ ucount,
                                    double* __restrict__ ucpus, double* __restrict__ umem, double* __restrict__ ugpus) {
  const unsigned u = blockIdx.x, tid = threadIdx.x;
  if (u >= U) return;
  const unsigned lo = seg_start[u], hi = seg_end[u];
  if (lo >= hi) return;
  const double acc = release_chain3(perm, lo, hi, l);
  if (tid == 0u) ucpus[u] = ucpus[u] - acc;
  else if (tid == 1u) umem[u] = umem[u] - acc;
  else if (tid == 2u) ugpus[u] = ugpus[u] - acc;
  else if (tid == 3u) ucount[u] = ucount[u] - (double)(hi - lo);
}

// out[0..3] = {count, cpus, mem, gpus} over ALL entries in list order (one workgroup)
COOK_KERNEL void release_fold_pool(unsigned n, ReleaseList l, double* __restrict__ out) {
  if (blockIdx.x != 0u) return;
  const double acc = release_chain3((const uint32_t*)nullptr, 0u, n, l);
  if (threadIdx.x < 3u) out[1u + threadIdx.x] = acc;
  else if (threadIdx.x == 3u) out[0] = (double)n;
}

// ---- the groups' running cotasks ------------------------------------------------------------------------------------------------------
// One wave per group that has a segment.  For each entry in turn (list order) the lanes look at 64 rows of the group's list at a time,
// first chunk first: a ballot of the lanes whose row holds the entry's host and is not yet claimed, the lowest such lane claims its row
// (claimed[] is zero beforehand; a row is only ever looked at by the same lane of the same wave).  An entry that finds no row is
// missing: counters[REL_CNT_MISSING], one atomic per wave.
COOK_KERNEL void release_group_mark(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ seg_start,
                                    const uint32_t* __restrict__ seg_end, unsigned G, const uint32_t* __restrict__ host,
                                    const uint32_t* __restrict__ g_off, const uint32_t* __restrict__ g_host, unsigned n_rows_max,
                                    uint8_t* __restrict__ claimed, unsigned* __restrict__ counters) {
  const unsigned g = blockIdx.x, lane = threadIdx.x;
  if (g >= G) return;  // (uniform per workgroup)
  const unsigned lo = seg_start[g], hi = seg_end[g];
  if (lo >= hi) return;
  unsigned r0 = g_off[g], r1 = g_off[g + 1];
  if (r1 > n_rows_max) r1 = n_rows_max;  // (never: the table has at most n_rows_max rows)
  if (r0 > r1) r0 = r1;
  unsigned missing = 0;
  for (unsigned p = lo; p < hi; ++p) {
    const uint32_t h = host[perm[p]];
    bool found = false;
    for (unsigned base = r0; base < r1 && !found; base += COOK_WAVE) {
      const unsigned x = base + lane;
      const bool mine = x < r1 && g_host[x] == h && !claimed[x];
      const unsigned long long b = __ballot(mine);
      if (b) {
        if (lane == (unsigned)(__ffsll(b) - 1)) claimed[x] = 1;
        found = true;
      }
    }
    if (!found) ++missing;
  }
  if (lane == 0u && missing) atomicAdd(&counters[REL_CNT_MISSING], missing);
}

// a row of the table survives unless claimed; rows behind the table's end (the launch is sized by an upper bound) count nothing
struct LoadUnclaimed {
  const uint8_t* claimed;
  const uint32_t* n_rows;  // the table's row count on the device: g_off + G
  __device__ __forceinline__ SumI operator()(unsigned x) const { return SumI{(x < *n_rows && !claimed[x]) ? 1 : 0}; }
};

// the survivors keep their order, and a CSR's groups lie one behind the other: the compacted table is the old one without the claimed
// rows, and group g starts at the number of survivors in front of its old start.  incl = inclusive scan of LoadUnclaimed.
COOK_KERNEL void release_group_offsets(const SumI* __restrict__ incl, const uint32_t* __restrict__ old_off, unsigned G,
                                       uint32_t* __restrict__ new_off) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > G) return;
  const unsigned x = old_off[g];
  new_off[g] = x ? (uint32_t)incl[x - 1].v : 0u;
}
COOK_KERNEL void release_group_compact(const uint8_t* __restrict__ claimed, const SumI* __restrict__ incl, const uint32_t* __restrict__ n_rows,
                                       unsigned n_rows_max, const uint32_t* __restrict__ old_host, const uint32_t* __restrict__ old_attr,
                                       uint32_t* __restrict__ new_host, uint32_t* __restrict__ new_attr) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_rows_max || x >= *n_rows || claimed[x]) return;
  const unsigned d = (unsigned)incl[x].v - 1u;
  new_host[d] = old_host[x];
  new_attr[d] = old_attr ? old_attr[x] : 0u;
}
