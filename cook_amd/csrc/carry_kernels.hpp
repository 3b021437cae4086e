// carry_kernels.hpp — device side of the carry (cook_cycle_run_queue_carry*): a queue cycle's advance moves the last
// cycle's KEPT placements (job_to_offer >= 0, offer not skipped: q_mark_removed's predicate) into the staged offers and the staged
// user state.  Here: the keys, the segment bounds and the pool's loader; the fold itself is fold_kernels.hpp, taking.
//
// Index spaces: i = considered position of the pool's last cycle (j2o[i] its offer, j_index[i] its pending ordinal = its row in the
//               staged job columns); p = position in a stable sort of the considered positions by key; v = offer; u = user.
// The order rule: every fp64 sum runs over the kept jobs of its segment in CONSIDERED order, the order in which the placement itself
// accumulated "assigned this call".  So: keys -> the STABLE radix passes of sort.hpp (equal keys keep that order) -> bounds -> the fold.
#pragma once
#include "fold_kernels.hpp"

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
// considered position -> its row when its placement is kept (the carry's pool: the segment is the considered positions themselves)
struct RowsKept {
  static constexpr bool FILTER = true;
  const int32_t* j2o;
  const uint8_t* offer_skipped;
  CarryJobs j;
  __device__ __forceinline__ CarryRow operator()(unsigned i) const { return carry_kept(j2o, offer_skipped, i) ? fold_row(j, i) : CarryRow{}; }
};
