// release_kernels.hpp — device side of the release (cook_cycle_run_queue_release*), the inverse of the carry: a queue
// cycle's advance gives the resources of a short list of FINISHED tasks back to the staged offers, takes them out of the staged user
// state and removes them from the groups' running-cotask lists.  Here: the keys, the host rows and the groups; the fold of the offers,
// the users and the pool is fold_kernels.hpp, giving back, with the list's columns as its rows.
//
// Index spaces: t = entry of the list (list order = the order rule's order); p = position in a stable sort of the entries by key;
//               v = offer (row of the staged offers); u = user; g = group; x = row of the groups' running-cotask table (CSR by g).
// The order rule: every fp64 sum runs over the entries of its segment in LIST order (keys -> stable sort -> carry_seg_bounds -> the fold).
#pragma once
#include "carry_kernels.hpp"
#include "scan.hpp"

// words of QueueBufs::counters behind the advance's two: read back in the advance's one synchronisation
constexpr unsigned REL_CNT_NO_ROW = 2, REL_CNT_CLAMPED = 3, REL_CNT_MISSING = 4, REL_CNT_WORDS = 12;  // (behind the release's: the churn's, the reservations', the limiters')

// the list's columns on the device (null columns: all 0 / no request)
struct ReleaseList {
  const uint32_t *host, *user, *group;
  const double *cpus, *mem, *gpus, *disk_req;
  const uint32_t *gpu_model, *disk_type;
  const int32_t* ports;
  const double* scal[3];
  // the fold's rows: entry t is row t
  CarryJobs rows() const { return CarryJobs{nullptr, cpus, mem, gpus, disk_req, gpu_model, disk_type, ports, {scal[0], scal[1], scal[2]}}; }
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
