// user_stats_kernels.hpp — device side of cook_user_stats / cook_user_stats_multi: the arithmetic of cook.monitor's
// set-stats-counters! (monitor.clj:40-116, 177-207) over the per-user order a rank run left on the device.
//
// Index spaces: B = position in a pool's per-user order (rank_gather's s_use / s_pending / s_user, segments seg_start..seg_end);
//               u = a pool's user id;  g = the caller's (group) user id (u itself, or user_map[u] in the multi form).
//
// Oracle-defined summation order (the reference reduces in Datomic query / hash-map order, which is unpinned):
//  - per user: left to right in the user's task order (tools.clj:614-641), running and pending tasks separately; in the multi form over
//    the concatenation of the member pools' segments in the order the engines are passed;
//  - "all": left to right over the users in id order.
// Every sum is bit-identical to that sequential sum for ANY fp64 inputs: the parallel forms track exactness (common.hpp, TwoSum) over
// EVERY prefix they stand for, and whatever is flagged is folded again left to right.
#pragma once
#include "common.hpp"
#include "scan.hpp"

// running {jobs, cpus, mem} and waiting {jobs, cpus, mem} side by side; bad bit 1: a running sum rounded, bit 2: a waiting one
struct SumRW {
  double rj, rc, rm, wj, wc, wm;
  unsigned bad;
  static __host__ __device__ __forceinline__ SumRW zero() { return SumRW{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u}; }
};
static __host__ __device__ __forceinline__ unsigned rw_inexact(double ac, double am, double bc, double bm, double sc, double sm) {
  return (two_sum_err(ac, bc, sc) != 0.0 || two_sum_err(am, bm, sm) != 0.0) ? 1u : 0u;
}
static __host__ __device__ __forceinline__ SumRW combine(const SumRW& a, const SumRW& b) {
  SumRW r;
  r.rj = a.rj + b.rj;  // task counts < 2^53: always exact
  r.rc = a.rc + b.rc;
  r.rm = a.rm + b.rm;
  r.wj = a.wj + b.wj;
  r.wc = a.wc + b.wc;
  r.wm = a.wm + b.wm;
  r.bad = a.bad | b.bad | rw_inexact(a.rc, a.rm, b.rc, b.rm, r.rc, r.rm) | (rw_inexact(a.wc, a.wm, b.wc, b.wm, r.wc, r.wm) << 1);
  return r;
}
static __device__ __forceinline__ SumRW shfl_up_v(const SumRW& v, unsigned d) {
  SumRW r;
  r.rj = __shfl_up(v.rj, d, COOK_WAVE);
  r.rc = __shfl_up(v.rc, d, COOK_WAVE);
  r.rm = __shfl_up(v.rm, d, COOK_WAVE);
  r.wj = __shfl_up(v.wj, d, COOK_WAVE);
  r.wc = __shfl_up(v.wc, d, COOK_WAVE);
  r.wm = __shfl_up(v.wm, d, COOK_WAVE);
  r.bad = __shfl_up(v.bad, d, COOK_WAVE);
  return r;
}

// a row of the rank's per-user order as a running or a waiting contribution (the pending-aware counterpart of LoadRunningU4)
struct LoadTaskRW {
  const SumU4* use;
  const uint8_t* pending;
  __device__ __forceinline__ SumRW operator()(unsigned i) const {
    const SumU4 x = use[i];
    if (pending[i]) return SumRW{0.0, 0.0, 0.0, 1.0, x.cpus, x.mem, 0u};
    return SumRW{1.0, x.cpus, x.mem, 0.0, 0.0, 0.0, 0u};
  }
};
// rows [off, off + 6) of the per-user result [U][4][3] as one SumRW (off 0: running + waiting, off 6: starved + waiting-under-quota)
struct LoadUserRows {
  const double* rows;
  unsigned off;
  __device__ __forceinline__ SumRW operator()(unsigned g) const {
    const double* p = rows + (size_t)g * 12 + off;
    return SumRW{p[0], p[1], p[2], p[3], p[4], p[5], 0u};
  }
};

// java.lang.Math.min / max on doubles (clojure.lang.Numbers min / max of two doubles): NaN wins, -0.0 < 0.0
static __device__ __forceinline__ double jmin(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  if (a == 0.0 && b == 0.0) return __longlong_as_double(__double_as_longlong(a) | __double_as_longlong(b));
  return a <= b ? a : b;
}
// (max x 0) of a double and the long 0 (monitor.clj:100): x when x > 0, NaN stays NaN, else 0
static __device__ __forceinline__ double clj_max0(double x) { return (x != x || x > 0.0) ? x : 0.0; }

// one pool of a stats call, as the combine / fold-again kernels see it (device memory, one entry per engine)
struct UsPool {
  const SumRW* pre;          // the pool's segmented scan over its per-user order
  const SumU4* use;          // rank_gather's rows
  const uint8_t* pending;
  const uint32_t* seg_start;
  const uint32_t* seg_end;   // nullptr: the pool holds no task
  const uint32_t* inv;       // [n_users]: g -> the pool's user id, 0xFFFFFFFF = none
  double* carry;             // [U_pool][4]: the group's {running cpus, mem, waiting cpus, mem} in front of this pool (pools after the first)
};

// ---- what a call wants cleared: the per-(group)-user flags and the five counts, in ONE launch -----------------------------------
COOK_KERNEL void us_init(uint32_t* __restrict__ flags, unsigned n_users, unsigned* __restrict__ counts, unsigned nblk) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 8) counts[i] = 0u;
  for (unsigned g = i; g < n_users; g += nblk * blockDim.x) flags[g] = 0u;
}

// inv[map[u]] = u for the users of one pool (map == nullptr: the identity); inv preset to 0xFF bytes
COOK_KERNEL void us_invert(const uint32_t* __restrict__ map, unsigned n_pool_users, uint32_t* __restrict__ inv) {
  const unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n_pool_users) inv[map ? map[u] : u] = u;
}

// the users whose prefix sums in this pool involved an inexact addition (bit 1 running, bit 2 waiting): every prefix counts, not only
// the segment's last — an exact total does not make the sequential prefixes in front of it exact
COOK_KERNEL void us_mark(const SumRW* __restrict__ pre, const uint32_t* __restrict__ s_user, const uint32_t* __restrict__ map, unsigned n,
                         uint32_t* __restrict__ flags) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned b = pre[i].bad;
  if (!b) return;
  const unsigned u = s_user[i];
  const unsigned g = map ? map[u] : u;
  if ((flags[g] & b) != b) atomicOr(&flags[g], b);
}

// per group user: the pools' segment totals added in pool order (exactness tracked); what stands in front of pool i is kept as that
// pool's carry for us_check.  Writes rows 0 (running) and 1 (waiting) of out[g][4][3].
COOK_KERNEL void us_combine(const UsPool* __restrict__ pools, unsigned n_pools, unsigned n_users, uint32_t* __restrict__ flags,
                            double* __restrict__ out) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_users) return;
  SumRW acc = SumRW::zero();
  for (unsigned i = 0; i < n_pools; ++i) {
    const UsPool p = pools[i];
    if (!p.seg_end) continue;
    const unsigned u = p.inv[g];
    if (u == 0xFFFFFFFFu) continue;
    const unsigned b = p.seg_end[u];
    if (b == 0u) continue;  // (rank_init: the user has no task in this pool)
    if (i > 0) {
      double* c = p.carry + (size_t)u * 4;
      c[0] = acc.rc, c[1] = acc.rm, c[2] = acc.wc, c[3] = acc.wm;
    }
    SumRW t = p.pre[b - 1];
    t.bad = 0u;  // (the segment's own flags are us_mark's)
    acc = combine(acc, t);
  }
  if (acc.bad) atomicOr(&flags[g], acc.bad);
  double* o = out + (size_t)g * 12;
  o[0] = acc.rj, o[1] = acc.rc, o[2] = acc.rm;
  o[3] = acc.wj, o[4] = acc.wc, o[5] = acc.wm;
}

// a pool after the first: carry + every prefix of the user's segment must be exact, else the group user is folded again
COOK_KERNEL void us_check(const SumRW* __restrict__ pre, const uint32_t* __restrict__ s_user, const uint32_t* __restrict__ map,
                          const double* __restrict__ carry, unsigned n, uint32_t* __restrict__ flags) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned u = s_user[i];
  const double* c = carry + (size_t)u * 4;
  const SumRW x = pre[i];
  const unsigned b = rw_inexact(c[0], c[1], x.rc, x.rm, c[0] + x.rc, c[1] + x.rm) |
                     (rw_inexact(c[2], c[3], x.wc, x.wm, c[2] + x.wc, c[3] + x.wm) << 1);
  if (!b) return;
  const unsigned g = map ? map[u] : u;
  if ((flags[g] & b) != b) atomicOr(&flags[g], b);
}

// ... folded left to right over the pools' segments in pool order, one thread per flagged group user (fractional inputs only)
COOK_KERNEL void us_fold(const UsPool* __restrict__ pools, unsigned n_pools, unsigned n_users, const uint32_t* __restrict__ flags,
                         double* __restrict__ out) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_users) return;
  const unsigned f = flags[g];
  if (!f) return;
  double rc = 0.0, rm = 0.0, wc = 0.0, wm = 0.0;
  for (unsigned i = 0; i < n_pools; ++i) {
    const UsPool p = pools[i];
    if (!p.seg_end) continue;
    const unsigned u = p.inv[g];
    if (u == 0xFFFFFFFFu) continue;
    for (unsigned r = p.seg_start[u], e = p.seg_end[u]; r < e; ++r) {
      const SumU4 x = p.use[r];
      if (p.pending[r])
        wc += x.cpus, wm += x.mem;
      else
        rc += x.cpus, rm += x.mem;
    }
  }
  double* o = out + (size_t)g * 12;
  if (f & 1u) o[1] = rc, o[2] = rm;
  if (f & 2u) o[4] = wc, o[5] = wm;
}

// ---- starved / waiting-under-quota / the counts (monitor.clj:69-116, 184-194) ---------------------------------------------------
// out[g] rows 0 / 1 hold running / waiting (jobs 0: the user is absent from that map); fills rows 2 / 3 and the state bits.
// counts: [0] total, [1] starved, [2] waiting-under-quota, [3] hungry, [4] satisfied (one atomic per wave and count)
COOK_KERNEL void us_classify(double* __restrict__ out, unsigned n_users, const double* __restrict__ s_cpus,
                             const double* __restrict__ s_mem, const double* __restrict__ q_count, const double* __restrict__ q_cpus,
                             const double* __restrict__ q_mem, const double* __restrict__ q_gpus,
                             const uint8_t* __restrict__ extra_positive, uint8_t* __restrict__ state, unsigned* __restrict__ counts) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  bool run = false, wait = false, starved = false, under = false;
  if (g < n_users) {
    double* o = out + (size_t)g * 12;
    const double rj = o[0], rc = o[1], rm = o[2], wj = o[3], wc = o[4], wm = o[5];
    run = rj > 0.0;
    wait = wj > 0.0;
    // absent running stats count as 0.0 in the tests; the merges differ (monitor.clj:75-78, 97-100)
    const double urj = run ? rj : 0.0, urc = run ? rc : 0.0, urm = run ? rm : 0.0;
    const double sc = s_cpus[g], sm = s_mem[g];
    starved = wait && urc < sc && urm < sm;
    const double qn = q_count[g], qc = q_cpus[g], qm = q_mem[g];
    under = wait && urj < qn && urc < qc && urm < qm && 0.0 < q_gpus[g] && (!extra_positive || extra_positive[g] != 0);
    double st[3] = {0.0, 0.0, 0.0}, uq[3] = {0.0, 0.0, 0.0};
    if (starved) {  // (merge-with min waiting (merge-with - share running)): :jobs only exists in running
      st[0] = run ? jmin(wj, rj) : wj;
      st[1] = jmin(wc, run ? sc - rc : sc);
      st[2] = jmin(wm, run ? sm - rm : sm);
    }
    if (under) {  // (merge-with min waiting (merge-with #(max (- %1 %2) 0) promised running))
      uq[0] = jmin(wj, run ? clj_max0(qn - rj) : qn);
      uq[1] = jmin(wc, run ? clj_max0(qc - rc) : qc);
      uq[2] = jmin(wm, run ? clj_max0(qm - rm) : qm);
    }
    o[6] = st[0], o[7] = st[1], o[8] = st[2];
    o[9] = uq[0], o[10] = uq[1], o[11] = uq[2];
    state[g] = (uint8_t)((run ? 1u : 0u) | (wait ? 2u : 0u) | (starved ? 4u : 0u) | (under ? 8u : 0u));
  }
  const unsigned long long b_total = __ballot(run || wait), b_starved = __ballot(starved), b_under = __ballot(under),
                           b_hungry = __ballot(wait && !starved), b_sat = __ballot(run && !wait);
  if (lane_id() == 0) {
    if (b_total) atomicAdd(&counts[0], (unsigned)__popcll(b_total));
    if (b_starved) atomicAdd(&counts[1], (unsigned)__popcll(b_starved));
    if (b_under) atomicAdd(&counts[2], (unsigned)__popcll(b_under));
    if (b_hungry) atomicAdd(&counts[3], (unsigned)__popcll(b_hungry));
    if (b_sat) atomicAdd(&counts[4], (unsigned)__popcll(b_sat));
  }
}

// ---- the "all" rows (add-aggregated-stats, monitor.clj:59-67) and the counts into the result block -------------------------------
// pre_a / pre_b: plain scans over the users of rows 0-1 / 2-3.  One workgroup: the OR of every prefix's bad bits, then the columns whose
// prefixes rounded are folded again left to right (one thread per column), the others are the scans' last prefixes.
// res: [0..11] all[4][3], then the five counts as doubles.
COOK_KERNEL void us_finish(const SumRW* __restrict__ pre_a, const SumRW* __restrict__ pre_b, const double* __restrict__ out,
                           unsigned n_users, const unsigned* __restrict__ counts, double* __restrict__ res) {
  __shared__ unsigned bad_s;
  if (threadIdx.x == 0) bad_s = 0u;
  __syncthreads();
  unsigned bad = 0u;
  for (unsigned g = threadIdx.x; g < n_users; g += blockDim.x) bad |= pre_a[g].bad | (pre_b[g].bad << 2);
  for (int d = 32; d >= 1; d >>= 1) bad |= __shfl_xor(bad, d, COOK_WAVE);
  if (lane_id() == 0 && bad) atomicOr(&bad_s, bad);
  __syncthreads();
  bad = bad_s;
  const unsigned k = threadIdx.x;  // column k of all[4][3]
  if (k < 12) {
    double v = 0.0;
    if (n_users) {
      const SumRW a = pre_a[n_users - 1], b = pre_b[n_users - 1];
      const double last[12] = {a.rj, a.rc, a.rm, a.wj, a.wc, a.wm, b.rj, b.rc, b.rm, b.wj, b.wc, b.wm};
      v = last[k];
      if ((k % 3) != 0 && (bad >> (k / 3)) & 1u) {
        v = 0.0;
        for (unsigned g = 0; g < n_users; ++g) v += out[(size_t)g * 12 + k];
      }
    }
    res[k] = v;
  }
  if (k < 5) res[12 + k] = (double)counts[k];
}
