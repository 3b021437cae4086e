// autoscale_kernels.hpp — device side of cook_cycle_autoscale: the queue of handle-resource-offers-autoscaling-helper
// (scheduler.clj:1283-1335), i.e. the ranked queue of the pool's last cycle without the jobs that cycle matched.
//
// Index spaces: q = rank position (e->ranked, and the cycle's gathered queue columns ConsBufs::q_*);
//               i = considered position (0 .. k-1: ConsBufs::result[i] is its rank position, m_j2o[i] its offer);
//               a = position in Q' (the ranked queue without the kept matches, remove-matched-jobs-from-pending-jobs :790-795);
//               c = candidate position (the filters' survivors over Q', cons_run_device's result holds their a).
// The filter chain itself is cons_run_device's (considerable_host.hpp), run on its own work set.
#pragma once
#include "common.hpp"
#include "scan.hpp"

// kept matches: considered job i is matched iff it got an offer and filter-matches-for-ratelimit (:887-924) did not drop the matches of
// that offer's compute cluster.  matched[] is zero beforehand; m is counted with one atomic per wave.
COOK_KERNEL void as_mark_matched(const uint32_t* __restrict__ cons_pos, const int32_t* __restrict__ j2o, unsigned k,
                                 const uint8_t* __restrict__ offer_skipped, int* __restrict__ matched, unsigned* __restrict__ n_matched) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  bool hit = false;
  if (i < k) {
    const int o = j2o[i];
    hit = o >= 0 && !(offer_skipped && offer_skipped[o]);
    if (hit) matched[cons_pos[i]] = 1;
  }
  const unsigned long long b = __ballot(hit);
  if (lane_id() == 0 && b) atomicAdd(n_matched, (unsigned)__popcll(b));
}

struct LoadUnmatched {
  const int* matched;
  __device__ __forceinline__ SumI operator()(unsigned q) const { return SumI{1 - matched[q]}; }
};

// Q': the unmatched jobs in rank order as the filters' queue columns, and the rank position of each
COOK_KERNEL void as_compact_queue(const int* __restrict__ matched, const SumI* __restrict__ incl, unsigned n,
                                  const double* __restrict__ cpus, const double* __restrict__ mem, const double* __restrict__ gpus,
                                  const uint32_t* __restrict__ user, double* __restrict__ a_cpus, double* __restrict__ a_mem,
                                  double* __restrict__ a_gpus, uint32_t* __restrict__ a_user, uint32_t* __restrict__ a_rpos) {
  const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n || matched[q]) return;
  const unsigned a = (unsigned)incl[q].v - 1;
  a_cpus[a] = cpus[q];
  a_mem[a] = mem[q];
  a_gpus[a] = gpus[q];
  a_user[a] = user[q];
  a_rpos[a] = q;
}

// caches/recent-synthetic-pod-job-uuids as a per-task flag (the indices are checked on the host)
COOK_KERNEL void as_exclude_flags(const uint32_t* __restrict__ tasks, unsigned n, uint8_t* __restrict__ excluded) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) excluded[tasks[i]] = 1;
}

// candidate c -> its task index; keep[c] = 0 for an excluded task (excluded NULL: none is, and `task` is the output as it stands)
COOK_KERNEL void as_candidate_tasks(const uint32_t* __restrict__ cand, unsigned len, const uint32_t* __restrict__ a_rpos,
                                    const uint32_t* __restrict__ ranked, const uint8_t* __restrict__ excluded, uint32_t* __restrict__ task,
                                    int* __restrict__ keep) {
  const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= len) return;
  const uint32_t t = ranked[a_rpos[cand[c]]];
  task[c] = t;
  if (excluded) keep[c] = excluded[t] ? 0 : 1;
}

// Out: the candidates that are not excluded, in order (removed after the take, :1319: no refill)
COOK_KERNEL void as_compact_out(const uint32_t* __restrict__ task, const int* __restrict__ keep, const SumI* __restrict__ incl,
                                unsigned len, uint32_t* __restrict__ out, unsigned* __restrict__ n_out) {
  const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= len) return;
  if (keep[c]) out[(unsigned)incl[c].v - 1] = task[c];
  if (c == len - 1) *n_out = (unsigned)incl[c].v;
}
