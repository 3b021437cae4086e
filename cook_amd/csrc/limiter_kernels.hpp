// limiter_kernels.hpp — device side of the per-user-per-pool launch-rate limiters kept across match cycles (cook_cycle_set_limiters,
// cook_cycle_set_clock, cook_cycle_limiters_spend): the reference's token bucket filter
// (rate_limit/token_bucket_filter.clj, rate_limit/generic.clj) as four columns over the staged users.
//
// Per user u: rate[u] tokens per millisecond (per_minute / 60000.0, one fp64 division), bucket[u], tokens[u] (may be negative),
// last[u] (ms).  lim_earned is earn-tokens as a pure function: the considerable filter compares with it on the fly
// (cons_rate_limit), lim_commit_earn stores it for the users whose jobs reached that stage, lim_spend runs it at the spend time.
// Everything is per-user work over integers and ONE fp64 multiply per earn: no sum, no order to keep.
#pragma once
#include "common.hpp"

struct LimState {
  int64_t tokens, last;
};
constexpr double LIM_PRODUCT_MAX = 4611686018427387904.0;  // 2^62: where the product is clamped before conversion (the reference would throw)

// earn-tokens (token_bucket_filter.clj): t' = max(t, last); d = trunc((t' - last) * rate); d != 0: last = t', tokens = min(tokens + d,
// bucket); d == 0: nothing changes — last stays, so the fraction of a token is not lost
static __host__ __device__ __forceinline__ LimState lim_earned(double rate, int64_t bucket, LimState s, int64_t t) {
  const int64_t t1 = t > s.last ? t : s.last;
  if (t1 == s.last) return s;
  double p = (double)(t1 - s.last) * rate;
  if (p > LIM_PRODUCT_MAX) p = LIM_PRODUCT_MAX;
  const int64_t d = (int64_t)p;
  if (d == 0) return s;
  const int64_t x = s.tokens + d;
  return LimState{x < bucket ? x : bucket, t1};
}

// what the rate-limit stage of the considerable filter reads (tokens null: no limiters of the engine's own, the staged tokens_left
// counts); clock == 0: nobody earns
struct LimView {
  const double* rate;
  const int64_t *bucket, *tokens, *last;
  int64_t now;
  int clock;
};
static __device__ __forceinline__ int64_t lim_tokens_now(const LimView& v, unsigned u) {
  const LimState s{v.tokens[u], v.last[u]};
  return v.clock ? lim_earned(v.rate[u], v.bucket[u], s, v.now).tokens : s.tokens;
}

// words of a read-back that the limiters' counters ride in: behind the considerable filter's length (d_counters + LIM_F_LEN ..), and
// in QueueBufs::counters behind the reservations' (release_kernels.hpp sizes REL_CNT_WORDS for them)
constexpr unsigned LIM_F_LEN = 44, LIM_F_EARNED = 45, LIM_F_DEBT = 46, LIM_F_WORDS = 3;
constexpr unsigned LIM_CNT_USERS = 8, LIM_CNT_SPENT = 9;

// cook_cycle_set_limiters: entry x of the list becomes user user[x]'s state (user null: entry x is user x)
COOK_KERNEL void lim_install(const uint32_t* __restrict__ user, const double* __restrict__ per_minute, const int64_t* __restrict__ in_bucket,
                             const int64_t* __restrict__ in_tokens, const int64_t* __restrict__ in_last, unsigned n, unsigned U,
                             double* __restrict__ rate, int64_t* __restrict__ bucket, int64_t* __restrict__ tokens, int64_t* __restrict__ last) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n) return;
  const unsigned u = user ? user[x] : x;
  if (u >= U) return;  // (the host refused such a list)
  rate[u] = per_minute[x] / 60000.0;  // generic.clj:50
  bucket[u] = in_bucket[x];
  tokens[u] = in_tokens[x];
  last[u] = in_last[x];
}

// the kept placements of the pool's last cycle per user (the predicate of q_mark_removed, the fold and the carry); kept[] is 0 beforehand
COOK_KERNEL void lim_count_kept(const int32_t* __restrict__ j2o, unsigned k, const uint8_t* __restrict__ offer_skipped,
                                const uint32_t* __restrict__ j_index, const uint32_t* __restrict__ j_user, unsigned n_rows, unsigned U,
                                unsigned* __restrict__ kept) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int o = j2o[i];
  if (o < 0 || (offer_skipped && offer_skipped[o])) return;
  const unsigned r = j_index[i];
  if (r >= n_rows) return;
  const unsigned u = j_user[r];
  if (u < U) atomicAdd(&kept[u], 1u);
}

// spend-tokens for every user with kept placements: earn(spend_ms) when a clock is given, then tokens = min(tokens - n, bucket); last is
// the earn's.  Leaves kept[] zero for the next spend.  counters[LIM_CNT_USERS] += users that spent, [LIM_CNT_SPENT] += their tokens
COOK_KERNEL void lim_spend(unsigned* __restrict__ kept, unsigned U, const double* __restrict__ rate, const int64_t* __restrict__ bucket,
                           int64_t* __restrict__ tokens, int64_t* __restrict__ last, int64_t spend_ms, int clock,
                           unsigned* __restrict__ counters) {
  const unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned n = 0;
  if (u < U) {
    n = kept[u];
    if (n) {
      kept[u] = 0u;
      LimState s{tokens[u], last[u]};
      if (clock) s = lim_earned(rate[u], bucket[u], s, spend_ms);
      const int64_t x = s.tokens - (int64_t)n, b = bucket[u];
      tokens[u] = x < b ? x : b;
      last[u] = s.last;
    }
  }
  const unsigned long long any = __ballot(n != 0u);
  if (any) {  // (one pair of atomics per wave)
    unsigned sum = n;
    for (int d = COOK_WAVE / 2; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, COOK_WAVE);
    if (lane_id() == 0) atomicAdd(&counters[LIM_CNT_USERS], (unsigned)__popcll(any)), atomicAdd(&counters[LIM_CNT_SPENT], sum);
  }
}

// behind cons_rate_limit: the users with a job at the rate-limit stage (passed + rate_limited > 0) keep the earn the filter compared
// with; everybody else's state stays, fraction and all.  fcnt[LIM_F_EARNED] += users whose state moved, fcnt[LIM_F_DEBT] += users
// whose tokens are below 0 behind this cycle's earn
COOK_KERNEL void lim_commit_earn(const uint32_t* __restrict__ passed, const uint32_t* __restrict__ rate_limited, unsigned U,
                                 const double* __restrict__ rate, const int64_t* __restrict__ bucket, int64_t* __restrict__ tokens,
                                 int64_t* __restrict__ last, int64_t now, int clock, unsigned* __restrict__ fcnt) {
  const unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
  bool moved = false, debt = false;
  if (u < U) {
    LimState s{tokens[u], last[u]};
    if (clock && passed[u] + rate_limited[u] > 0u) {
      const LimState e = lim_earned(rate[u], bucket[u], s, now);
      moved = e.last != s.last || e.tokens != s.tokens;
      if (moved) tokens[u] = e.tokens, last[u] = e.last;
      s = e;
    }
    debt = s.tokens < 0;
  }
  const unsigned long long bm = __ballot(moved), bd = __ballot(debt);
  if (lane_id() == 0) {
    if (bm) atomicAdd(&fcnt[LIM_F_EARNED], (unsigned)__popcll(bm));
    if (bd) atomicAdd(&fcnt[LIM_F_DEBT], (unsigned)__popcll(bd));
  }
}
