// reserve_kernels.hpp — device side of the rebalancer's host reservations kept across match cycles (cook_cycle_set_reservations,
// cook_cycle_run_queue_reserve*): the reference's atom {job-uuid->reserved-host, launched-job-uuids}
// (rebalancer.clj:419-432 reserve-hosts!, scheduler.clj:1050-1057 update-host-reservations!) as a list, a column, a bitmap and a byte
// per pending row.
//
// Index spaces: i = considered position of the pool's last cycle (j2o[i] its offer, j_index[i] its pending row); r = pending row
//               (cook_cycle_stage's pending_jobs); x = entry of the reservation list (rv_job[x] = r or COOK_NONE_U32, rv_host[x] a
//               host ID, not an offer row: the host churn moves no reservation).
// An entry with a row is ALIVE iff col[rv_job[x]] == rv_host[x]: the release and the retire write -1 into the column and nothing
// into the list, and a row is in the list at most once (the host refuses a second).  An entry without a row (a job of another pool)
// is alive until the list is replaced.
#pragma once
#include "churn_kernels.hpp"

// words of QueueBufs::counters behind the churn's: reservations the kept matches released, list entries dropped as launched
constexpr unsigned RESV_CNT_RELEASED = 6, RESV_CNT_DROPPED = 7;
static_assert(RESV_CNT_RELEASED > CHURN_CNT_MISSING && RESV_CNT_DROPPED < REL_CNT_WORDS, "the reservations' counters lie behind the churn's");

// update-host-reservations! over the last cycle's kept matches (the predicate of q_mark_removed): the row joins `launched`, its
// reservation — if it holds one — goes.  counters[RESV_CNT_RELEASED]: one atomic per wave.
COOK_KERNEL void resv_release(const int32_t* __restrict__ j2o, unsigned k, const uint8_t* __restrict__ offer_skipped,
                              const uint32_t* __restrict__ j_index, unsigned n_rows, int32_t* __restrict__ col,
                              uint8_t* __restrict__ launched, unsigned* __restrict__ counters) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  bool rel = false;
  if (i < k) {
    const int o = j2o[i];
    const unsigned r = j_index[i];
    if (o >= 0 && !(offer_skipped && offer_skipped[o]) && r < n_rows) {
      launched[r] = 1;
      rel = col[r] >= 0;
      if (rel) col[r] = -1;
    }
  }
  const unsigned long long b = __ballot(rel);
  if (lane_id() == 0 && b) atomicAdd(&counters[RESV_CNT_RELEASED], (unsigned)__popcll(b));
}

// every old reservation goes: the column back to -1 (the list itself is overwritten by the upload behind this kernel)
COOK_KERNEL void resv_retire(const uint32_t* __restrict__ rv_job, unsigned n_list, unsigned n_rows, int32_t* __restrict__ col) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_list) return;
  const uint32_t r = rv_job[x];
  if (r < n_rows) col[r] = -1;
}

// (apply dissoc reservations launched-job-uuids): entry x becomes a reservation unless its row is in `launched` (which the host
// clears behind this kernel).  counters[RESV_CNT_DROPPED]: one atomic per wave.
COOK_KERNEL void resv_install(const uint32_t* __restrict__ rv_job, const uint32_t* __restrict__ rv_host, unsigned n_list, unsigned n_rows,
                              const uint8_t* __restrict__ launched, int32_t* __restrict__ col, unsigned* __restrict__ counters) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x;
  bool drop = false;
  if (x < n_list) {
    const uint32_t r = rv_job[x];
    if (r < n_rows) {
      drop = launched[r] != 0;
      if (!drop) col[r] = (int32_t)rv_host[x];
    }
  }
  const unsigned long long b = __ballot(drop);
  if (lane_id() == 0 && b) atomicAdd(&counters[RESV_CNT_DROPPED], (unsigned)__popcll(b));
}

// the bitmap (zero beforehand, n_words words) from the live list, and every entry's liveness for cook_cycle_fetch_reservations
COOK_KERNEL void resv_bits(const uint32_t* __restrict__ rv_job, const uint32_t* __restrict__ rv_host, unsigned n_list, unsigned n_rows,
                           const int32_t* __restrict__ col, unsigned n_words, uint32_t* __restrict__ bits, uint8_t* __restrict__ rv_live) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_list) return;
  const uint32_t r = rv_job[x], h = rv_host[x];
  const bool live = r < n_rows ? col[r] == (int32_t)h : r == 0xFFFFFFFFu;
  rv_live[x] = live ? 1 : 0;
  if (live && (h >> 5) < n_words) atomicOr(&bits[h >> 5], 1u << (h & 31));
}
