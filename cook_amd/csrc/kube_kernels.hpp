// kube_kernels.hpp — device side of cook_kube_distribute: scheduling-capacity-constrained-job-distributor (scheduler.clj:1110-1151), the
// distributor of a Kubernetes-scheduler pool (handle-kubernetes-scheduler-pool, :1747-1810).  Integers plus the one fp64 multiply of
// rand-nth; plain C++ stores.
//
// The reference walks the jobs one by one: each job picks among the acceptable clusters that still have capacity and takes one unit of
// the cluster it picked.  The walk is sequential only where a cluster RUNS OUT: between two exhaustions the set of available clusters
// is fixed, so a job's choice depends on its own row (location, draw) and on one <= 32-bit availability mask, and its rank within its
// cluster is a count of the jobs in front of it.  One workgroup walks the jobs in tiles of KUBE_TILE; capacities, counts and the mask
// live in LDS; nothing is polled in global memory.
//
// Index spaces: k = job position (0 .. K-1: considered order); c = cluster 0 .. n-1; bin = c, or n for :no-acceptable-compute-cluster.
#pragma once
#include "common.hpp"

constexpr unsigned KUBE_MAX_CLUSTERS = 32;
constexpr unsigned KUBE_BINS = KUBE_MAX_CLUSTERS + 1;
constexpr unsigned KUBE_BIN_BITS = 6;  // a bin is 0 .. 32
static_assert(KUBE_BINS <= (1u << KUBE_BIN_BITS) && KUBE_BINS <= COOK_WAVE, "a bin fits its bits, a wave zeroes its row of counts");
constexpr int KUBE_TILE = 256;
constexpr unsigned KUBE_WAVES = KUBE_TILE / COOK_WAVE;
constexpr unsigned KUBE_NONE = 0xFFu;  // choice byte: no available cluster
constexpr unsigned KUBE_FIRST_TEN = 10;
constexpr unsigned KUBE_ERR_PASSES = 1u;  // KubeOut::err: the walk reached its pass bound

struct KubeClusterTab {  // the cluster table in the kernel arguments: scalar loads, no global load per lane
  unsigned n;
  uint32_t location[KUBE_MAX_CLUSTERS];
  uint32_t capacity[KUBE_MAX_CLUSTERS];  // cc/max-launchable clamped to [0, 2^32 - 1] (K < 2^31: the clamp changes no choice)
};
struct KubeOut {  // what the host reads back (written in full by the kernel)
  unsigned assigned[KUBE_MAX_CLUSTERS];
  unsigned no_cluster, first_task[KUBE_FIRST_TEN], launched, exhaustions, passes, err;
};

// splitmix64's output function over the state x + gamma (cookmatch.h states the constants: they are the contract)
static __host__ __device__ __forceinline__ uint64_t kube_splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static __host__ __device__ __forceinline__ double kube_seed_draw(uint64_t seed, uint64_t k) {
  return (double)(kube_splitmix64(seed + k) >> 11) * 0x1.0p-53;  // a 53-bit integer scaled by a power of two: exact, in [0, 1)
}
// rand-nth's index into m >= 1 available clusters: (int (* m u)), clamped (no u < 1 reaches the clamp, cookmatch.h)
static __device__ __forceinline__ unsigned kube_pick(unsigned m, double u) {
  const unsigned r = (unsigned)(int)((double)m * u);
  return r < m - 1u ? r : m - 1u;
}

// One workgroup of KUBE_TILE threads distributes the K jobs and writes the lists.
//   task NULL: the lists hold positions k; otherwise task[k] (a pool's cycle: the task index of considered position k).
//   j2o, summary (a pool's cycle, else NULL): j2o[k] = 0 for a job that got a cluster, -1 otherwise — the next advance reads the launched
//   jobs as the cycle's kept placements —, and the match summary of a cycle without a placement.
//   choice[k] = the job's cluster (KUBE_NONE: none); rank[k] = its rank within that cluster (within the no-cluster jobs for KUBE_NONE);
//   lists[base(c) + rank] for the jobs of cluster c, base = the exclusive sum of the final counts; *res = counts, first ten, error word.
// A pass evaluates the uncommitted lanes of the tile under the current availability mask.  A lane whose rank within its cluster (among
// the pass's lanes) equals the cluster's remaining capacity - 1 takes its last unit: the lowest such lane p is the first exhaustion.
// Lanes <= p decided under a mask that held for them: they commit.  The cluster's bit goes and the lanes behind p are evaluated again.
// Every pass retires at least one job (p is an uncommitted lane), and every pass that does not finish its tile retires a cluster:
// at most ceil(K / KUBE_TILE) + n passes.  A pass past that bound ends the kernel with KUBE_ERR_PASSES instead of spinning.
COOK_KERNEL void kube_distribute(KubeClusterTab tab, const uint32_t* __restrict__ location, const double* __restrict__ draw,
                                 unsigned long long seed, const uint32_t* __restrict__ task, unsigned K, uint8_t* __restrict__ choice,
                                 uint32_t* __restrict__ rank, uint32_t* __restrict__ lists, KubeOut* __restrict__ res,
                                 int32_t* __restrict__ j2o, unsigned* __restrict__ summary) {
  __shared__ unsigned s_cap[KUBE_BINS], s_cnt[KUBE_BINS], s_add[KUBE_BINS], s_base[KUBE_BINS], s_wave[KUBE_WAVES][KUBE_BINS];
  __shared__ unsigned s_avail, s_first, s_exh;
  const unsigned n = tab.n, tid = threadIdx.x, w = wave_id();
  if (tid <= n) {
    s_cap[tid] = tid < n ? tab.capacity[tid] : 0xFFFFFFFFu;  // (bin n never runs out)
    s_cnt[tid] = 0u;
    s_add[tid] = 0u;
  }
  if (tid == 0) {
    unsigned a = 0u;
    for (unsigned c = 0; c < n; ++c) a |= tab.capacity[c] ? (1u << c) : 0u;
    s_avail = a;
    s_first = (unsigned)KUBE_TILE;
    s_exh = 0u;
  }
  __syncthreads();
  const unsigned tiles = (K + KUBE_TILE - 1) / KUBE_TILE;
  const unsigned max_passes = tiles + n;
  unsigned passes = 0u;
  bool failed = false;
  for (unsigned t = 0; t < tiles && !failed; ++t) {
    const unsigned k = t * KUBE_TILE + tid;
    const bool live = k < K;
    uint32_t acc = 0u;
    double u = 0.0;
    if (live) {
      const uint32_t loc = location ? location[k] : 0u;
      for (unsigned c = 0; c < n; ++c) acc |= (loc == 0u || tab.location[c] == loc) ? (1u << c) : 0u;
      u = draw ? draw[k] : kube_seed_draw(seed, k);
    }
    unsigned done = 0u;  // lanes < done of this tile are committed (uniform)
    while (done < (unsigned)KUBE_TILE) {
      if (passes == max_passes) {  // (uniform: every thread leaves the walk here)
        failed = true;
        break;
      }
      ++passes;
      const bool active = live && tid >= done;
      unsigned bin = KUBE_NONE;
      if (active) {
        uint32_t av = acc & s_avail;
        const unsigned m = (unsigned)__popc(av);
        if (m == 0u) {
          bin = n;
        } else {
          const unsigned r = kube_pick(m, u);
          for (unsigned x = 0; x < r; ++x) av &= av - 1u;
          bin = (unsigned)__ffs(av) - 1u;
        }
      }
      // the wave's lanes of the same bin: KUBE_BIN_BITS ballots, one per bit of the bin, instead of one per bin
      unsigned long long mine = __ballot(active);
      for (unsigned x = 0; x < KUBE_BIN_BITS; ++x) {
        const unsigned long long bit_x = __ballot((bin >> x) & 1u);
        mine &= ((bin >> x) & 1u) ? bit_x : ~bit_x;
      }
      if (lane_id() < KUBE_BINS) s_wave[w][lane_id()] = 0u;
      wave_sync();  // (the same wave's counts come behind its zeros)
      if (active && (mine & lanemask_lt()) == 0ull) s_wave[w][bin] = (unsigned)__popcll(mine);  // lowest lane of the peer set
      __syncthreads();
      unsigned r_pass = 0u;  // rank among this pass's lanes of the same bin
      if (active) {
        r_pass = (unsigned)__popcll(mine & lanemask_lt());
        for (unsigned x = 0; x < w; ++x) r_pass += s_wave[x][bin];
        if (r_pass + 1u == s_cap[bin]) atomicMin(&s_first, tid);
      }
      __syncthreads();
      const unsigned p = s_first;  // KUBE_TILE: no exhaustion in this pass
      const bool commit = active && tid <= p;
      if (commit) {
        const unsigned rk = s_cnt[bin] + r_pass;
        choice[k] = (uint8_t)(bin < n ? bin : KUBE_NONE);
        rank[k] = rk;
        if (j2o) j2o[k] = bin < n ? 0 : -1;
        if (bin == n && rk < KUBE_FIRST_TEN) res->first_task[rk] = task ? task[k] : k;
      }
      const unsigned long long cm = mine & __ballot(commit);  // the wave's committed lanes of the same bin
      if (commit && (cm & lanemask_lt()) == 0ull) atomicAdd(&s_add[bin], (unsigned)__popcll(cm));
      __syncthreads();
      if (tid <= n) {
        const unsigned a = s_add[tid];
        s_cnt[tid] += a;
        if (tid < n) {
          const unsigned left = s_cap[tid] - a;  // (a <= cap: the lanes behind the cluster's last unit are behind p)
          s_cap[tid] = left;
          if (a && left == 0u) {
            atomicAnd(&s_avail, ~(1u << tid));
            atomicAdd(&s_exh, 1u);
          }
        }
        s_add[tid] = 0u;
      }
      if (tid == 0) s_first = (unsigned)KUBE_TILE;
      done = p < (unsigned)KUBE_TILE ? p + 1u : (unsigned)KUBE_TILE;
      __syncthreads();
    }
  }
  // ---- the lists, one after another: every thread places the positions it decided itself (its own stores) --------------------------
  if (tid == 0) {
    unsigned base = 0u;
    for (unsigned c = 0; c < n; ++c) {
      s_base[c] = base;
      base += s_cnt[c];
    }
    s_base[n] = base;
  }
  __syncthreads();
  if (!failed) {
    for (unsigned k = tid; k < K; k += KUBE_TILE) {
      const unsigned c = choice[k];
      if (c != KUBE_NONE) lists[s_base[c] + rank[k]] = task ? task[k] : k;
    }
  }
  if (tid < KUBE_MAX_CLUSTERS) res->assigned[tid] = tid < n ? s_cnt[tid] : 0u;
  if (tid == 0) {
    const unsigned none = s_cnt[n];
    res->no_cluster = none;
    for (unsigned x = none; x < KUBE_FIRST_TEN; ++x) res->first_task[x] = 0u;
    res->launched = s_base[n];
    res->exhaustions = s_exh;
    res->passes = passes;
    res->err = failed ? KUBE_ERR_PASSES : 0u;
    if (summary) summary[0] = 0u, summary[1] = 1u, summary[2] = 0u, summary[3] = 0u;  // (as a match of no jobs leaves it)
  }
}

// a pool's cycle: considered position i -> its task index and its last checkpoint's location (pos NULL: rank position i; ckpt NULL: none)
COOK_KERNEL void kube_gather(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ ranked, const uint32_t* __restrict__ j_index,
                             const uint32_t* __restrict__ ckpt, unsigned K, uint32_t* __restrict__ task, uint32_t* __restrict__ loc) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  task[i] = ranked[pos ? pos[i] : i];
  loc[i] = ckpt ? ckpt[j_index[i]] : 0u;
}
