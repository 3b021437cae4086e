// sweep_kernels.hpp — device side of cook_sweep_running: the lingering-task killer (get-lingering-tasks, scheduler.clj:1888-1912),
// the straggler handler (handle-stragglers :1955-1986 over find-stragglers :quantile-deviation, group.clj:17-44) and the cancelled-task
// killer (killable-cancelled-tasks, scheduler.clj:1988-1996) over the cluster's running set.
//
// Index spaces: i = running row (0 .. n-1); g = straggler group (0 .. G-1); j = successful instance (0 .. NS-1, the groups' CSR,
//               group g owns [off[g], off[g+1])).
// Order of the launches: sw_groups (readiness and the quantile's index, from the CSR alone) -> sw_keys ((g, s) per successful instance)
// -> the radix sort of sort.hpp -> sw_select (the idx-th smallest s of every ready group) -> sw_rows (the three killers per row) ->
// the scan of the reason bits (its last entry holds the three list lengths) -> [lengths and error words read back] -> sw_scatter.
#pragma once
#include "common.hpp"
#include "scan.hpp"

// control words (device, zeroed per call apart from the two minima, which start at COOK_NONE_U32)
constexpr unsigned SW_READY = 0, SW_ERR = 1, SW_BAD_ROW = 2, SW_BAD_SUCC = 3, SW_CTL_WORDS = 4;
constexpr unsigned SW_ERR_GROUP = 1u;  // a type-1 group's quantile / multiplier / job_count, or a type > 1
constexpr unsigned SW_ERR_OFF = 2u;    // succ_off decreases
constexpr unsigned SW_S_BITS = 31;     // s <= INT32_MAX (t/in-seconds is an int): the key is (g << 31) | s

struct SweepTimes {
  int64_t now_ms, default_timeout_ms, max_timeout_ms;
};

// t/in-seconds of the interval [start, end] (Interval and Seconds.secondsIn throw outside 0 .. INT32_MAX s): -1 where the reference throws
static __host__ __device__ __forceinline__ int64_t sw_in_seconds(int64_t start, int64_t end) {
  if (start == INT64_MIN || end < start) return -1;
  const uint64_t s = ((uint64_t)end - (uint64_t)start) / 1000u;  // exact: end >= start
  return s > (uint64_t)INT32_MAX ? -1 : (int64_t)s;
}

// per group: gsel[g] = the quantile's index idx if the group is of type 1 and ready, else -1; thr[g] = NaN (sw_select fills the ready
// ones); the ready groups counted with one atomic per wave
COOK_KERNEL void sw_groups(const uint8_t* __restrict__ type, const double* __restrict__ quantile, const double* __restrict__ multiplier,
                           const uint32_t* __restrict__ job_count, const uint32_t* __restrict__ off, unsigned G, unsigned NS,
                           int* __restrict__ gsel, double* __restrict__ thr, unsigned* __restrict__ ctl) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  bool ready = false;
  unsigned err = 0;
  if (g < G) {
    const unsigned lo = off[g], hi = off[g + 1];
    if (lo > hi || hi > NS) err |= SW_ERR_OFF;
    int sel = -1;
    const unsigned t = type[g];
    if (t > 1u) {
      err |= SW_ERR_GROUP;  // (find-stragglers has no method for it)
    } else if (t == 1u) {
      const double q = quantile[g], m = multiplier[g];
      const uint32_t jc = job_count[g];
      // api.clj:495-497: 0 < q < 1, multiplier > 1 (both comparisons are false for NaN; the upper bound keeps +inf out)
      if (!(q > 0.0 && q < 1.0) || !(m > 1.0 && m <= 1.7976931348623157e308) || jc > (uint32_t)INT32_MAX) {
        err |= SW_ERR_GROUP;
      } else if (!(err & SW_ERR_OFF)) {
        // quantile-job-idx = (int (* (dec (count jobs)) quantile)): 0 jobs give trunc(-q) = 0
        const int idx = (int)((double)((int64_t)jc - 1) * q);
        if (hi - lo > (unsigned)idx) sel = idx, ready = true;
      }
    }
    gsel[g] = sel;
    thr[g] = __builtin_nan("");
    if (err) atomicOr(&ctl[SW_ERR], err);
  }
  const unsigned long long b = __ballot(ready);
  if (lane_id() == 0 && b) atomicAdd(&ctl[SW_READY], (unsigned)__popcll(b));
}

// per successful instance: its group (the last g with off[g] <= j: empty groups share their offset with the next one) and the key
// (g << 31) | s.  s is evaluated, and its interval checked, only in ready type-1 groups; elsewhere s = 0, so that an interval the
// reference never looks at neither fails the call nor spills into the group bits.
COOK_KERNEL void sw_keys(const uint32_t* __restrict__ off, unsigned G, unsigned NS, const int64_t* __restrict__ s_start,
                         const int64_t* __restrict__ s_end, int64_t now_ms, const int* __restrict__ gsel, uint64_t* __restrict__ key,
                         unsigned* __restrict__ ctl) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= NS) return;
  unsigned lo = 0, hi = G;  // off[lo] <= j < off[hi] (off[0] = 0, off[G] = NS: checked on the host)
  while (hi - lo > 1u) {
    const unsigned mid = (lo + hi) >> 1;
    if (off[mid] <= j) lo = mid;
    else hi = mid;
  }
  uint64_t s = 0;
  if (gsel[lo] >= 0) {
    const int64_t e = s_end[j];
    const int64_t v = sw_in_seconds(s_start[j], e < 0 ? now_ms : e);  // (tools.clj:670-676 task-run-time: no end-time -> now)
    if (v < 0) atomicMin(&ctl[SW_BAD_SUCC], j);
    else s = (uint64_t)v;
  }
  key[j] = ((uint64_t)lo << SW_S_BITS) | s;
}

// per ready group: threshold = (double)(the idx-th smallest s) * multiplier (group.clj:38-41; the sorted run of g starts at off[g])
COOK_KERNEL void sw_select(const int* __restrict__ gsel, const uint32_t* __restrict__ off, const uint32_t* __restrict__ perm,
                           const uint64_t* __restrict__ key, const double* __restrict__ multiplier, unsigned G, double* __restrict__ thr) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int sel = gsel[g];
  if (sel < 0) return;
  const uint64_t s = key[perm[off[g] + (unsigned)sel]] & ((1ull << SW_S_BITS) - 1ull);
  thr[g] = (double)s * multiplier[g];
}

// per running row: the three killers' bits (what: which of them run).  A running row of a ready group whose own interval the reference
// cannot take (or a group index out of range) lowers ctl[SW_BAD_ROW].  The lists are counted by the scan that places them: a count
// per wave here, one atomic per wave on three words, made this kernel take 447 us at a million rows on the MI355X (the atomics of
// 15 625 waves on one address serialise); without them it takes 13.5 us.
COOK_KERNEL void sw_rows(const int64_t* __restrict__ start, const uint8_t* __restrict__ unknown, const int64_t* __restrict__ max_rt,
                         const uint8_t* __restrict__ cancelled, const uint32_t* __restrict__ group, unsigned n, unsigned what,
                         SweepTimes t, const int* __restrict__ gsel, const double* __restrict__ thr, unsigned G,
                         uint8_t* __restrict__ reason, unsigned* __restrict__ ctl) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    unsigned bits = 0;
    const int64_t st = (what & 3u) ? start[i] : INT64_MIN;
    bool bad = false;
    if ((what & 1u) && st != INT64_MIN && st <= t.now_ms) {
      // get-lingering-tasks: (time/after? now (plus start (min max-runtime max-timeout))), max-runtime get-else the default; now - start
      // as an unsigned difference (exact for start <= now) against a limit >= 0: no sum that can overflow
      const int64_t rt = max_rt ? max_rt[i] : -1;
      const int64_t lim = rt >= 0 ? (rt < t.max_timeout_ms ? rt : t.max_timeout_ms)
                                  : (t.default_timeout_ms < t.max_timeout_ms ? t.default_timeout_ms : t.max_timeout_ms);
      if ((uint64_t)t.now_ms - (uint64_t)st > (uint64_t)lim) bits |= 1u;
    }
    if ((what & 2u) && group) {
      const uint32_t g = group[i];
      if (g != COOK_NONE_U32) {
        if (g >= G) {
          bad = true;
        } else if (gsel[g] >= 0 && !(unknown && unknown[i])) {  // find-stragglers keeps :instance.status/running only
          const int64_t s = sw_in_seconds(st, t.now_ms);
          if (s < 0) bad = true;
          else if ((double)s > thr[g]) bits |= 2u;  // Clojure's > on an int and a double compares in double
        }
      }
    }
    if ((what & 4u) && cancelled && cancelled[i]) bits |= 4u;
    reason[i] = (uint8_t)bits;
    if (bad) atomicMin(&ctl[SW_BAD_ROW], i);
  }
}

// the three list positions of every row in one scan
struct SumI3 {
  int v[3];
  static __host__ __device__ __forceinline__ SumI3 zero() { return SumI3{{0, 0, 0}}; }
};
static __host__ __device__ __forceinline__ SumI3 combine(const SumI3& a, const SumI3& b) {
  return SumI3{{a.v[0] + b.v[0], a.v[1] + b.v[1], a.v[2] + b.v[2]}};
}
static __device__ __forceinline__ SumI3 shfl_up_v(const SumI3& v, unsigned d) {
  return SumI3{{__shfl_up(v.v[0], d, COOK_WAVE), __shfl_up(v.v[1], d, COOK_WAVE), __shfl_up(v.v[2], d, COOK_WAVE)}};
}
struct LoadReason3 {
  const uint8_t* reason;
  __device__ __forceinline__ SumI3 operator()(unsigned i) const {
    const int b = reason[i];
    return SumI3{{b & 1, (b >> 1) & 1, (b >> 2) & 1}};
  }
};

// lingering ++ stragglers ++ cancelled, each in row order: the k-th list starts at base[k]
COOK_KERNEL void sw_scatter(const uint8_t* __restrict__ reason, const SumI3* __restrict__ incl, unsigned n, unsigned base_s, unsigned base_c,
                            uint32_t* __restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned b = reason[i];
  if (!b) return;
  const SumI3 p = incl[i];
  if (b & 1u) out[(unsigned)p.v[0] - 1u] = i;
  if (b & 2u) out[base_s + (unsigned)p.v[1] - 1u] = i;
  if (b & 4u) out[base_c + (unsigned)p.v[2] - 1u] = i;
}
