// queue_kernels.hpp — device side of the queue cycles (cook_cycle_run_queue*): the standing ranked queue that match cycles consume
// between two ranks, as pool-name->pending-jobs-atom is in the reference (scheduler.clj:1360, remove-matched-jobs-from-pending-jobs
// :790-795, called at :1506-1508; the Kubernetes pool handler removes every considered job, :1792-1794).
//
// Index spaces: q = rank position in the standing queue (e->ranked); i = considered position of the pool's last cycle (cons_pos[i] its
//               rank position, or i itself without the considerable filters; j2o[i] its offer; j_index[i] its pending ordinal);
//               g = group; x = row of the groups' running-cotask table (CSR by g).
// The advance: mark -> scan -> compact of the queue, and the fold of the kept matches' cotasks into a new CSR (count -> scan ->
// copy the old rows, append the new ones).  Integers only: no sum-order question, counts are exact.
#pragma once
#include "autoscale_kernels.hpp"
#include "common.hpp"
#include "scan.hpp"

// removed[] and add_cnt[] are zero beforehand.  A considered job leaves the queue iff it has a kept match (remove_all: in any case);
// a kept match with a group becomes a running cotask of that group (fold != 0).  counters[0] = jobs removed, [1] = cotasks to fold,
// one atomic per wave each.
COOK_KERNEL void q_mark_removed(const uint32_t* __restrict__ cons_pos, const int32_t* __restrict__ j2o, unsigned k, unsigned n,
                                const uint8_t* __restrict__ offer_skipped, unsigned remove_all, const uint32_t* __restrict__ j_index,
                                const uint32_t* __restrict__ j_group, unsigned G, unsigned fold, int* __restrict__ removed,
                                unsigned* __restrict__ add_cnt, unsigned* __restrict__ counters) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  bool rem = false, cot = false;
  if (i < k) {
    const int o = j2o[i];
    const bool hit = o >= 0 && !(offer_skipped && offer_skipped[o]);
    const unsigned q = cons_pos ? cons_pos[i] : i;
    rem = (hit || remove_all) && q < n;
    if (rem) removed[q] = 1;
    if (hit && fold && j_group) {
      const unsigned g = j_group[j_index[i]];
      if (g < G) {
        cot = true;
        atomicAdd(&add_cnt[g], 1u);
      }
    }
  }
  const unsigned long long br = __ballot(rem), bc = __ballot(cot);
  if (lane_id() == 0) {
    if (br) atomicAdd(&counters[0], (unsigned)__popcll(br));
    if (bc) atomicAdd(&counters[1], (unsigned)__popcll(bc));
  }
}

// the survivors keep their order (`remove` is order-preserving): incl = inclusive scan of 1 - removed
COOK_KERNEL void q_compact_ranked(const int* __restrict__ removed, const SumI* __restrict__ incl, unsigned n,
                                  const uint32_t* __restrict__ ranked, uint32_t* __restrict__ out) {
  const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n || removed[q]) return;
  out[(unsigned)incl[q].v - 1] = ranked[q];
}

// a group's new row count: the rows it has plus the cotasks this advance folds in
struct LoadGroupRows {
  const uint32_t* old_off;  // may be NULL: no running cotasks so far
  const unsigned* add_cnt;
  __device__ __forceinline__ SumI operator()(unsigned g) const {
    return SumI{(int)((old_off ? old_off[g + 1] - old_off[g] : 0u) + add_cnt[g])};
  }
};

COOK_KERNEL void q_fold_offsets(const SumI* __restrict__ incl, unsigned G, uint32_t* __restrict__ new_off) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  if (g == 0) new_off[0] = 0u;
  new_off[g + 1] = (uint32_t)incl[g].v;
}

// the rows a group has already, to the head of its new list (their order kept)
COOK_KERNEL void q_fold_copy_old(const uint32_t* __restrict__ old_off, const uint32_t* __restrict__ old_host,
                                 const uint32_t* __restrict__ old_attr, unsigned G, unsigned n_old, const uint32_t* __restrict__ new_off,
                                 uint32_t* __restrict__ new_host, uint32_t* __restrict__ new_attr) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_old) return;
  unsigned lo = 0, hi = G;  // the last g with old_off[g] <= x (the groups in front of it may be empty)
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (old_off[mid] <= x) lo = mid;
    else hi = mid;
  }
  const unsigned d = new_off[lo] + (x - old_off[lo]);
  new_host[d] = old_host[x];
  new_attr[d] = old_attr ? old_attr[x] : 0u;
}

// one row per kept match with a group, behind the group's old rows: run_host = the offer's host, run_attr = that offer's value of the
// group's attribute key (0 = absent).  Unique, balanced and attribute-equals read a group's rows as a set / as counts, so the order
// inside a list is free: the slot comes from a cursor per group (zero beforehand).
COOK_KERNEL void q_fold_append(const int32_t* __restrict__ j2o, unsigned k, const uint8_t* __restrict__ offer_skipped,
                               const uint32_t* __restrict__ j_index, const uint32_t* __restrict__ j_group, unsigned G,
                               const uint32_t* __restrict__ old_off, const uint32_t* __restrict__ new_off, unsigned* __restrict__ cursor,
                               const uint32_t* __restrict__ o_host, const uint32_t* __restrict__ o_attr, unsigned n_attr,
                               const uint32_t* __restrict__ g_attr_key, uint32_t* __restrict__ new_host, uint32_t* __restrict__ new_attr) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int o = j2o[i];
  if (o < 0 || (offer_skipped && offer_skipped[o])) return;
  const unsigned g = j_group[j_index[i]];
  if (g >= G) return;
  const unsigned had = old_off ? old_off[g + 1] - old_off[g] : 0u;
  const unsigned d = new_off[g] + had + atomicAdd(&cursor[g], 1u);
  const uint32_t key = g_attr_key[g];
  new_host[d] = o_host[o];
  new_attr[d] = (o_attr && key < n_attr) ? o_attr[(size_t)o * n_attr + key] : 0u;
}
