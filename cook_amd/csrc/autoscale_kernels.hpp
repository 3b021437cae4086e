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

// ---- cook_cycle_autoscale_clusters: Out distributed to the pool's autoscaling compute clusters and cut per cluster -------------------
// (distribute-jobs-to-compute-clusters, scheduler.clj:1078-1103; autoscale!'s cut, kubernetes/compute_cluster.clj:642-663).  Integers only.
// Index spaces: c = position in Out (its storage holds `len` slots, of which the first *n_live count when an exclude list compacted it);
//               b = bin: cluster 0 .. n-1, n = :no-acceptable-compute-cluster; (b, blk) = cell b * nb + blk of the per-block counts.
constexpr unsigned AS_MAX_CLUSTERS = 32;
constexpr unsigned AS_BINS = AS_MAX_CLUSTERS + 1;
constexpr int AS_THREADS = 256;
constexpr unsigned AS_DEAD = 0xFFu, AS_OUTSTANDING = 0x80u;  // a slot's code: its bin (| AS_OUTSTANDING: it has a pod there), AS_DEAD behind Out's end
constexpr unsigned AS_FIRST_TEN = 10;

static __device__ __forceinline__ unsigned as_min_u(unsigned a, unsigned b) { return a < b ? a : b; }

struct AsClusterTab {  // the cluster table in the kernel arguments: scalar loads, no global load per lane
  unsigned n;
  uint32_t location[AS_MAX_CLUSTERS];
  uint32_t max_launch[AS_MAX_CLUSTERS];  // max-launchable clamped to [0, 2^32 - 1]
};
struct AsOutOff {
  uint32_t off[AS_MAX_CLUSTERS + 1];
};
struct AsDistOut {  // what the host reads back (zeroed before)
  unsigned assigned[AS_MAX_CLUSTERS], outstanding[AS_MAX_CLUSTERS], launched[AS_MAX_CLUSTERS];
  unsigned no_cluster, first_task[AS_FIRST_TEN], total;
};

// the clusters' outstanding synthetic pods as one word per task: bit k = cluster k holds a pod for it (the indices are checked on the host)
COOK_KERNEL void as_outstanding_flags(AsOutOff o, unsigned n_clusters, const uint32_t* __restrict__ out_task, unsigned total,
                                      uint32_t* __restrict__ flags) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  unsigned k = 0;
  for (unsigned x = 1; x < n_clusters; ++x) k += i >= o.off[x] ? 1u : 0u;  // (offsets do not decrease: the entry's cluster)
  atomicOr(&flags[out_task[i]], 1u << k);
}

// Every job of Out chooses its cluster: the acceptable ones are those of its last checkpoint's location (none recorded: all), the choice
// is the (hash mod count)-th of them with Clojure's floor modulus.  Writes the slot's code and the block's counts per bin: kept (assigned
// and without a pod there; bin n: every such job) into cell (b, blk), assigned / outstanding into the totals.
COOK_KERNEL void as_choose_cluster(AsClusterTab tab, const uint32_t* __restrict__ task, unsigned len, const unsigned* __restrict__ n_live,
                                   const uint32_t* __restrict__ pend_ord, const uint32_t* __restrict__ ckpt, const int32_t* __restrict__ hash,
                                   const uint32_t* __restrict__ flags, unsigned nb, uint8_t* __restrict__ code_out, int* __restrict__ kept_cnt,
                                   uint8_t* __restrict__ head, AsDistOut* __restrict__ dist) {
  __shared__ unsigned s_kept[AS_BINS], s_asg[AS_BINS];
  if (threadIdx.x < AS_BINS) s_kept[threadIdx.x] = 0u, s_asg[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned n = tab.n;
  const unsigned c = blockIdx.x * AS_THREADS + threadIdx.x;
  const bool live = c < len && (!n_live || c < *n_live);
  unsigned bin = AS_DEAD;
  bool outstanding = false;
  if (live) {
    const uint32_t t = task[c];
    const uint32_t j = pend_ord[t];
    const uint32_t loc = ckpt ? ckpt[j] : 0u;
    const int32_t h = hash[j];
    uint32_t acc = 0u;
    for (unsigned k = 0; k < n; ++k) acc |= (loc == 0u || tab.location[k] == loc) ? (1u << k) : 0u;
    const int cnt = __popc(acc);
    if (cnt == 0) {
      bin = n;
    } else {
      int r = h % cnt;  // (cnt >= 1: defined for INT32_MIN too)
      if (r < 0) r += cnt;
      for (int x = 0; x < r; ++x) acc &= acc - 1u;
      bin = (unsigned)__ffs(acc) - 1u;
      outstanding = flags && ((flags[t] >> bin) & 1u);
    }
    code_out[c] = (uint8_t)(bin | (outstanding ? AS_OUTSTANDING : 0u));
  } else if (c < len) {
    code_out[c] = (uint8_t)AS_DEAD;
  }
  for (unsigned b = 0; b <= n; ++b) {
    const unsigned long long asg = __ballot(bin == b);
    const unsigned long long kept = __ballot(bin == b && !outstanding);
    if (lane_id() == 0 && asg) {
      atomicAdd(&s_asg[b], (unsigned)__popcll(asg));
      atomicAdd(&s_kept[b], (unsigned)__popcll(kept));
    }
  }
  __syncthreads();
  const unsigned b = threadIdx.x;
  if (b <= n) {
    const size_t cell = (size_t)b * nb + blockIdx.x;
    kept_cnt[cell] = (int)s_kept[b];
    head[cell] = blockIdx.x == 0 ? 1 : 0;
    if (b < n && s_asg[b]) {
      atomicAdd(&dist->assigned[b], s_asg[b]);
      if (s_asg[b] != s_kept[b]) atomicAdd(&dist->outstanding[b], s_asg[b] - s_kept[b]);
    }
  }
}

// The stable (n + 1)-way partition with the cut folded in.  incl = the segmented inclusive scan of kept_cnt over (b, blk), a segment per
// bin: a kept job's rank within its bin is the cells of its bin in front of its block, the waves of its block in front of its own, and
// the lanes of its wave in front of it — candidate order and nothing else.  It is written iff that rank is below the bin's max-launchable;
// the lists stand one after another.  The first ten jobs of bin n are reported.
COOK_KERNEL void as_partition_scatter(AsClusterTab tab, const uint32_t* __restrict__ task, unsigned len, const uint8_t* __restrict__ code_in,
                                      const int* __restrict__ kept_cnt, const SumI* __restrict__ incl, unsigned nb, uint32_t* __restrict__ out,
                                      AsDistOut* __restrict__ dist) {
  __shared__ unsigned s_base[AS_BINS], s_excl[AS_BINS], s_max[AS_BINS], s_wave[AS_THREADS / COOK_WAVE][AS_BINS];
  const unsigned n = tab.n;
  if (threadIdx.x <= n) {
    const unsigned b = threadIdx.x;
    unsigned base = 0u;
    for (unsigned k = 0; k < b && k < n; ++k) base += as_min_u((unsigned)incl[(size_t)k * nb + nb - 1].v, tab.max_launch[k]);
    const unsigned tot = (unsigned)incl[(size_t)b * nb + nb - 1].v;
    s_base[b] = base;  // (bin n: the end of the lists)
    s_max[b] = b < n ? tab.max_launch[b] : AS_FIRST_TEN;
    s_excl[b] = (unsigned)(incl[(size_t)b * nb + blockIdx.x].v - kept_cnt[(size_t)b * nb + blockIdx.x]);
    if (blockIdx.x == 0) {
      if (b < n) dist->launched[b] = as_min_u(tot, tab.max_launch[b]);
      else dist->no_cluster = tot, dist->total = base;
    }
  }
  const unsigned c = blockIdx.x * AS_THREADS + threadIdx.x;
  const unsigned code = c < len ? (unsigned)code_in[c] : AS_DEAD;
  const bool kept = code != AS_DEAD && !(code & AS_OUTSTANDING);
  const unsigned bin = code & 0x7Fu;
  const unsigned w = wave_id();
  unsigned long long mine = 0ull;
  for (unsigned b = 0; b <= n; ++b) {
    const unsigned long long in_b = __ballot(kept && bin == b);
    if (bin == b) mine = in_b;
    if (lane_id() == 0) s_wave[w][b] = (unsigned)__popcll(in_b);
  }
  __syncthreads();
  if (!kept) return;
  unsigned rank = s_excl[bin] + (unsigned)__popcll(mine & lanemask_lt());
  for (unsigned k = 0; k < w; ++k) rank += s_wave[k][bin];
  if (rank >= s_max[bin]) return;
  if (bin < n) out[s_base[bin] + rank] = task[c];
  else dist->first_task[rank] = task[c];
}
