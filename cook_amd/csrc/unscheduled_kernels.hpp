// unscheduled_kernels.hpp — device side of cook_unscheduled: the three reasons of cook.unscheduled/reasons that need the user's whole
// task list (unscheduled.clj:37-77 how-job-would-exceed-resource-limits / check-exceeds-limit with quotas and with shares, :128-158
// check-queue-position), for every row of the task table or for a list of rows, over the per-user order a rank run left on the device.
//
// Index spaces: A = task row of the staged cook_tasks;  B = position in the per-user order (rank_gather's s_use / s_pending / s_user,
//               segments seg_start..seg_end, permB[B] = A);  u = user id;  k = output index (A itself, or the index into `rows`).
//
// A segment holds the user's running and pending rows INTERLEAVED by the key of tools.clj:614-632 (rank_build_keys: user, -priority,
// then the running rows by start time and task id in front of the pending ones by job id — start = Long.MAX_VALUE and task = nil for
// a pending row): it is `sorted-tasks` of check-queue-position as it stands, so a user's list is its segment without the pending rows
// outside the window, and nothing is sorted here.
//
// Oracle-defined summation order (the reference's is (conj running-jobs job) over a Datomic result): the user's running rows left to
// right in that order, starting from the first of them, the job's own resources last.  The running sums are per user; they are the
// scan's last prefix when EVERY prefix of the user's segment was formed by exact additions (common.hpp "exact-sum tracking"), else
// the user is folded again left to right (un_user_sums).
#pragma once
#include "common.hpp"
#include "scan.hpp"

// running {count, cpus, mem, gpus} of the rows so far and the number of listed rows so far
struct SumUL {
  double count, cpus, mem, gpus;
  unsigned listed, bad;
  static __host__ __device__ __forceinline__ SumUL zero() { return SumUL{0.0, 0.0, 0.0, 0.0, 0u, 0u}; }
};
static __host__ __device__ __forceinline__ SumUL combine(const SumUL& a, const SumUL& b) {
  SumUL r;
  r.count = a.count + b.count;  // task counts < 2^53: always exact
  r.cpus = a.cpus + b.cpus;
  r.mem = a.mem + b.mem;
  r.gpus = a.gpus + b.gpus;
  r.listed = a.listed + b.listed;
  const bool inexact = two_sum_err(a.cpus, b.cpus, r.cpus) != 0.0 || two_sum_err(a.mem, b.mem, r.mem) != 0.0 ||
                       two_sum_err(a.gpus, b.gpus, r.gpus) != 0.0;
  r.bad = a.bad | b.bad | (inexact ? 1u : 0u);
  return r;
}
static __device__ __forceinline__ SumUL shfl_up_v(const SumUL& v, unsigned d) {
  SumUL r;
  r.count = __shfl_up(v.count, d, COOK_WAVE);
  r.cpus = __shfl_up(v.cpus, d, COOK_WAVE);
  r.mem = __shfl_up(v.mem, d, COOK_WAVE);
  r.gpus = __shfl_up(v.gpus, d, COOK_WAVE);
  r.listed = __shfl_up(v.listed, d, COOK_WAVE);
  r.bad = __shfl_up(v.bad, d, COOK_WAVE);
  return r;
}

// is the row at position i of the per-user order in its user's list?  (running: always; pending: the caller's window mask by task row)
static __device__ __forceinline__ bool un_listed(const uint8_t* __restrict__ s_pending, const uint32_t* __restrict__ permB,
                                                 const uint8_t* __restrict__ in_window, unsigned i) {
  return !s_pending[i] || !in_window || in_window[permB[i]] != 0;
}

struct LoadUnsched {
  const SumU4* use;
  const uint8_t* pending;
  const uint32_t* permB;
  const uint8_t* in_window;  // by task row, or nullptr = every pending row
  __device__ __forceinline__ SumUL operator()(unsigned i) const {
    const unsigned l = un_listed(pending, permB, in_window, i) ? 1u : 0u;
    if (pending[i]) return SumUL{0.0, 0.0, 0.0, 0.0, l, 0u};
    const SumU4 x = use[i];
    // the fold starts from the user's first RUNNING row and keeps a -0.0 there; the scan adds the pending rows' +0.0, which does not
    const bool negz = __double_as_longlong(x.cpus) == LLONG_MIN || __double_as_longlong(x.mem) == LLONG_MIN ||
                      __double_as_longlong(x.gpus) == LLONG_MIN;
    return SumUL{1.0, x.cpus, x.mem, x.gpus, l, negz ? 1u : 0u};
  }
};

// ---- what a call wants preset, in ONE launch: no user rounded, every list empty, nobody ahead ----------------------------------------
COOK_KERNEL void un_init(uint32_t* __restrict__ flags, uint32_t* __restrict__ list_len, uint32_t* __restrict__ ahead, unsigned n_users,
                         unsigned nblk) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  for (unsigned u = i; u < n_users; u += nblk * blockDim.x) flags[u] = 0u, list_len[u] = 0u;
  for (unsigned k = i; k < n_users * COOK_UNSCHED_AHEAD; k += nblk * blockDim.x) ahead[k] = COOK_NONE_U32;
}

// ---- per position of the per-user order: the users with ANY rounded prefix (not only the segment's last: an exact total does not make
// the sequential prefixes in front of it exact), the first ten listed rows of every user, and every user's list length.  The listed
// count of the scan names a row's place in its user's list, so a segment of any length needs no walk.
COOK_KERNEL void un_lists(const SumUL* __restrict__ pre, const uint32_t* __restrict__ s_user, const uint8_t* __restrict__ s_pending,
                          const uint32_t* __restrict__ permB, const uint8_t* __restrict__ in_window,
                          const uint32_t* __restrict__ seg_end, unsigned n, uint32_t* __restrict__ flags,
                          uint32_t* __restrict__ list_len, uint32_t* __restrict__ ahead) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const SumUL p = pre[i];
  const unsigned u = s_user[i];
  if (p.bad) flags[u] = 1u;
  if (p.listed <= COOK_UNSCHED_AHEAD && un_listed(s_pending, permB, in_window, i)) ahead[(size_t)u * COOK_UNSCHED_AHEAD + (p.listed - 1u)] = permB[i];
  if (i + 1u == seg_end[u]) list_len[u] = p.listed;
}

// ---- per user: the running {count, cpus, mem, gpus}; a flagged user folded left to right over its running rows (fractional inputs only)
COOK_KERNEL void un_user_sums(const SumUL* __restrict__ pre, const SumU4* __restrict__ s_use, const uint8_t* __restrict__ s_pending,
                              const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_end,
                              const uint32_t* __restrict__ flags, unsigned n_users, double* __restrict__ run /*[U][4]*/) {
  const unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_users) return;
  double n = 0.0, c = 0.0, m = 0.0, g = 0.0;
  if (seg_end && seg_end[u] != 0u) {  // (rank_init: 0 = the user has no row in this pool; no seg_end at all: an empty table)
    const unsigned a = seg_start[u], b = seg_end[u];
    const SumUL t = pre[b - 1];
    n = t.count, c = t.cpus, m = t.mem, g = t.gpus;
    if (flags[u]) {
      bool first = true;
      for (unsigned i = a; i < b; ++i) {
        if (s_pending[i]) continue;
        const SumU4 x = s_use[i];
        if (first) {
          c = x.cpus, m = x.mem, g = x.gpus;
          first = false;
        } else {
          c += x.cpus, m += x.mem, g += x.gpus;
        }
      }
    }
  }
  double* o = run + (size_t)u * 4;
  o[0] = n, o[1] = c, o[2] = m, o[3] = g;
}

// pos[permB[i]] = i: task row -> position in the per-user order (a call with a list of rows)
COOK_KERNEL void un_invert(const uint32_t* __restrict__ permB, unsigned n, uint32_t* __restrict__ pos) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pos[permB[i]] = i;
}

struct UnLimits {  // per user, device memory
  const double *q_count, *q_cpus, *q_mem, *q_gpus, *s_cpus, *s_mem, *s_gpus;
};

// ---- per output: the row's place in its user's list, and for a pending row the user's running sums + its own against both limits.
// rows == nullptr: thread i stands for position i of the per-user order and writes at its task row; else for rows[i], at index i.
COOK_KERNEL void un_classify(const SumUL* __restrict__ pre, const SumU4* __restrict__ s_use, const uint8_t* __restrict__ s_pending,
                             const uint32_t* __restrict__ s_user, const uint32_t* __restrict__ permB,
                             const uint8_t* __restrict__ in_window, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ pos,
                             unsigned n_out, const double* __restrict__ run, const uint32_t* __restrict__ list_len, UnLimits lim,
                             uint32_t* __restrict__ reasons, uint32_t* __restrict__ queue_pos, double* __restrict__ total) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  const unsigned b = rows ? pos[rows[i]] : i;   // position in the per-user order
  const unsigned k = rows ? i : permB[i];       // where the answer goes
  const unsigned u = s_user[b];
  const bool pending = s_pending[b] != 0;
  const bool listed = un_listed(s_pending, permB, in_window, b);
  const unsigned qp = listed ? pre[b].listed - 1u : list_len[u];
  unsigned r = (qp > 0u ? COOK_UNSCHED_QUEUE_POSITION : 0u) | (listed ? 0u : COOK_UNSCHED_AT_LEAST);
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  if (pending) {
    const SumU4 x = s_use[b];
    const double* ru = run + (size_t)u * 4;
    if (ru[0] == 0.0) {  // no running row: the reduce of one usage map is that map
      t[0] = 1.0, t[1] = x.cpus, t[2] = x.mem, t[3] = x.gpus;
    } else {
      t[0] = ru[0] + 1.0, t[1] = ru[1] + x.cpus, t[2] = ru[2] + x.mem, t[3] = ru[3] + x.gpus;
    }
    r |= (t[0] > lim.q_count[u] ? COOK_UNSCHED_QUOTA_COUNT : 0u) | (t[1] > lim.q_cpus[u] ? COOK_UNSCHED_QUOTA_CPUS : 0u) |
         (t[2] > lim.q_mem[u] ? COOK_UNSCHED_QUOTA_MEM : 0u) | (t[3] > lim.q_gpus[u] ? COOK_UNSCHED_QUOTA_GPUS : 0u) |
         (t[1] > lim.s_cpus[u] ? COOK_UNSCHED_SHARE_CPUS : 0u) | (t[2] > lim.s_mem[u] ? COOK_UNSCHED_SHARE_MEM : 0u) |
         (t[3] > lim.s_gpus[u] ? COOK_UNSCHED_SHARE_GPUS : 0u);
  }
  reasons[k] = r;
  queue_pos[k] = qp;
  double* o = total + (size_t)k * 4;
  o[0] = t[0], o[1] = t[1], o[2] = t[2], o[3] = t[3];
}
