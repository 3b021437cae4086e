// churn_kernels.hpp — device side of the host churn (cook_cycle_run_queue_hosts*): a queue cycle's advance takes the rows
// of the hosts that LEAVE out of the staged offers and puts the rows that JOIN in, behind the carry, the groups' fold and the release
// (which still index the old rows).  A stable compaction plus an ordered insertion over every offer column: mark -> the joins sorted
// by anchor -> ONE scan -> a source map -> ONE gather.
//
// Index spaces: r = row of the OLD table (M_old rows; r = M_old: "behind the last old row"); t = entry of the leave list; i = entry of
//               the join list (list order = the order rule's order); p = position in a stable sort of the joins by anchor row;
//               d = row of the NEW table.  src[d] = r for an old row that stays, M_old + i for join i.
// The order rule: old rows keep their relative order; join i lands directly in front of its anchor's OLD position, joins of one anchor
// in list order (keys -> the STABLE radix passes -> carry_seg_bounds), whether or not the anchor itself leaves.
#pragma once
#include "offer_table.hpp"
#include "release_kernels.hpp"

// word of QueueBufs::counters behind the release's: leave_host entries that have no row
constexpr unsigned CHURN_CNT_MISSING = 5;
static_assert(CHURN_CNT_MISSING > REL_CNT_MISSING && CHURN_CNT_MISSING < REL_CNT_WORDS, "the churn's counter lies behind the release's");

// the gather's arguments (by pointer: three column sets do not fit a batched kernel's argument block)
struct ChurnGather {
  OfferCols<false> old, join;
  OfferCols<true> out;
  unsigned M_old, n_join, M_new;
  OfferDims dims;
};

// host id -> row of the OLD table or M (none): through the release's host-indexed table, or (h2row null: the greatest host id is far
// above the row count) by a look through o_host itself
static __device__ __forceinline__ unsigned churn_row_of(uint32_t h, const uint32_t* __restrict__ h2row, unsigned n_hosts,
                                                        const uint32_t* __restrict__ o_host, unsigned M) {
  if (h2row) return (h < n_hosts && h2row[h] < M) ? h2row[h] : M;
  for (unsigned x = 0; x < M; ++x)
    if (o_host[x] == h) return x;
  return M;
}

// keep[] is 1 beforehand.  Entry t of the leave list clears its row's keep, or is missing: counters[CHURN_CNT_MISSING], one atomic per
// wave.  Entry i of the join list gets its anchor's row as key (COOK_NONE_U32, or a host without a row — the host refuses those —: M).
COOK_KERNEL void churn_mark(const uint32_t* __restrict__ leave_host, unsigned n_leave, const uint32_t* __restrict__ join_before, unsigned n_join,
                            const uint32_t* __restrict__ h2row, unsigned n_hosts, const uint32_t* __restrict__ o_host, unsigned M,
                            uint8_t* __restrict__ keep, uint64_t* __restrict__ akey, unsigned* __restrict__ counters) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  bool missing = false;
  if (t < n_leave) {
    const unsigned r = churn_row_of(leave_host[t], h2row, n_hosts, o_host, M);
    if (r < M) keep[r] = 0;
    missing = r >= M;
  }
  if (t < n_join) {
    const uint32_t h = join_before ? join_before[t] : 0xFFFFFFFFu;
    akey[t] = (uint64_t)(h == 0xFFFFFFFFu ? M : churn_row_of(h, h2row, n_hosts, o_host, M));
  }
  const unsigned long long b = __ballot(missing);
  if (lane_id() == 0 && b) atomicAdd(&counters[CHURN_CNT_MISSING], (unsigned)__popcll(b));
}

// what position r of the old table (r = M: its end) puts into the new one: itself if it stays, and the joins anchored at it
struct LoadChurnRows {
  const uint8_t* keep;
  const uint32_t *seg_start, *seg_end;  // the joins' segments by anchor row, [M + 1]; null: no joins
  unsigned M;
  __device__ __forceinline__ unsigned joins(unsigned r) const { return seg_start ? seg_end[r] - seg_start[r] : 0u; }
  __device__ __forceinline__ unsigned stays(unsigned r) const { return (r < M && keep[r]) ? 1u : 0u; }
  __device__ __forceinline__ SumI operator()(unsigned r) const { return SumI{(int)(stays(r) + joins(r))}; }
};

// src[] from the ONE inclusive scan of LoadChurnRows over [0, M]: with excl[r] = incl[r] - rows(r), an old row r that stays lands at
// excl[r] + joins(r), and the p-th join of anchor a at excl[a] + p.  Thread x handles old row x and the join at sorted position x.
COOK_KERNEL void churn_source(LoadChurnRows rows, const SumI* __restrict__ incl, const uint32_t* __restrict__ perm,
                              const uint64_t* __restrict__ akey, unsigned n_join, unsigned M_new, uint32_t* __restrict__ src) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned M = rows.M;
  if (x < M && rows.stays(x)) {
    const unsigned d = (unsigned)incl[x].v - 1u;  // (its own 1 is the last of its position's rows)
    if (d < M_new) src[d] = x;
  }
  if (x < n_join) {
    const unsigned i = perm[x];
    const unsigned a = (unsigned)akey[i];
    if (a <= M) {
      const unsigned d = (unsigned)incl[a].v - rows.stays(a) - rows.joins(a) + (x - rows.seg_start[a]);
      if (d < M_new) src[d] = M + i;
    }
  }
}

template <class T>
static __device__ __forceinline__ void churn_move(T* __restrict__ out, const T* __restrict__ old, const T* __restrict__ join, unsigned width,
                                                  unsigned d, unsigned s, unsigned M_old, T none) {
  if (!out) return;
  const bool from_old = s < M_old;
  const T* __restrict__ col = from_old ? old : join;
  const size_t row = from_old ? s : s - M_old;
  for (unsigned x = 0; x < width; ++x) out[(size_t)d * width + x] = col ? col[row * width + x] : none;
}

// One thread per NEW row: every column the new table has (offer_columns) moves with its row.  A column the source lacks (the joins'
// list may leave out what the staged table has) gives the value a NULL column means for every row, the list's `none`.  src is
// 0xFF-filled beforehand: a row nobody claimed is left alone.
COOK_KERNEL void churn_gather(const ChurnGather* __restrict__ gp, const uint32_t* __restrict__ src) {
  const unsigned d = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned M_old = gp->M_old;
  if (d >= gp->M_new) return;
  const unsigned s = src[d];
  if (s >= M_old + gp->n_join) return;
  offer_columns([&](const auto& col) {
    churn_move(col.col(gp->out), col.col(gp->old), col.col(gp->join), gp->dims.width(col.kind), d, s, M_old, col.none);
  });
}
