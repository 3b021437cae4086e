// launch_res_kernels.hpp — device side of cook_match_launch_resources (cookmatch.h, "LAUNCH RESOURCES"): the assigned
// ports and the per-role takes of the KEPT placements of the last match (carry_kept: placed, offer not skipped).
//
// Index spaces: k = considered position of the last match (j2o[k] its offer, j_index[k] its row in the staged job columns);
//               p = position in the carry's stable sort of the considered positions by offer (perm[p] = k, an offer's segment
//               [seg_start[v], seg_end[v]) lists its kept tasks in considered order); v = offer row; g = a range of the rows' CSR;
//               r = resource slot; q = output port.
// The port part is data-parallel: ports per task -> an exclusive segmented sum per offer (the task's cursor c_k) and a plain one
// in considered order (port_off) -> every output port finds its range by a search over the row's range prefix sums and its place in
// the task's ascending order from the begins of the ranges its task's slice spans.  The role part is one sequential chain per
// (offer, slot): take-resources' subtractions are fp64 and not associative, so a chain walks its segment task after task, role after
// role; the chains run side by side.
#pragma once
#include "carry_kernels.hpp"

constexpr unsigned LR_MAX_RES = 2u + COOK_MAX_SCALARS;
constexpr unsigned LR_NONE = 0xFFFFFFFFu;
// the call's control block, read back by its first synchronisation
// (LR_BROKEN: lr_emit_ports met what the checks in front of it rule out; read back by the second synchronisation)
enum { LR_BAD_ROW = 0, LR_KEPT = 1, LR_OFFERS_USED = 2, LR_SHORT = 3, LR_PORTS_LO = 4, LR_PORTS_HI = 5, LR_BROKEN = 6, LR_CTL_WORDS = 8 };

struct SumU64 {  // port counts: a task asks for up to 2^31 - 1, a segment for more than 32 bits hold
  unsigned long long v;
  static __host__ __device__ __forceinline__ SumU64 zero() { return SumU64{0ull}; }
};
static __host__ __device__ __forceinline__ SumU64 combine(const SumU64& a, const SumU64& b) { return SumU64{a.v + b.v}; }
static __device__ __forceinline__ SumU64 shfl_up_v(const SumU64& x, unsigned d) {
  const unsigned lo = __shfl_up((unsigned)x.v, d, COOK_WAVE), hi = __shfl_up((unsigned)(x.v >> 32), d, COOK_WAVE);
  return SumU64{((unsigned long long)hi << 32) | (unsigned long long)lo};
}
struct LoadLrPorts {
  const uint32_t* x;
  __device__ __forceinline__ SumU64 operator()(unsigned i) const { return SumU64{(unsigned long long)x[i]}; }
};

// the role view of the offers, on the device
struct LrRows {
  unsigned n, n_roles, n_res;
  const uint32_t* range_off;
  const int32_t *range_begin, *range_end;
  const uint8_t* range_role;
  const double* avail;  // [n_res][n_roles][n]
};
// the job columns of the match behind the slots (NaN = no request)
struct LrJobs {
  const uint32_t* j_index;
  const int32_t* ports;
  const double* col[LR_MAX_RES];
};

// One wave per row: the row's ranges (0 <= begin <= end, a role below n_roles, pairwise disjoint) and amounts (finite, >= 0) are
// valid, else the row is raised in ctl[LR_BAD_ROW] (the lowest wins); range_pre[g] = the ports of the row's ranges in front of g,
// row_ports[v] = all of them; rows with a kept task are counted.
COOK_KERNEL void lr_check_rows(LrRows R, const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_end,
                               unsigned long long* __restrict__ range_pre, unsigned long long* __restrict__ row_ports,
                               unsigned* __restrict__ ctl) {
  const unsigned v = blockIdx.x, lane = threadIdx.x;
  if (v >= R.n) return;
  const unsigned lo = R.range_off[v], hi = R.range_off[v + 1];
  bool bad = false;
  for (unsigned g = lo + lane; g < hi; g += COOK_WAVE) {
    const int b = R.range_begin[g], en = R.range_end[g];
    if (b < 0 || b > en || (unsigned)R.range_role[g] >= R.n_roles) bad = true;
    for (unsigned h = lo; h < g; ++h)
      if (b <= R.range_end[h] && R.range_begin[h] <= en) bad = true;
  }
  for (unsigned x = lane; x < R.n_res * R.n_roles; x += COOK_WAVE) {
    const double a = R.avail[(size_t)x * R.n + v];
    if (!(a >= 0.0 && a < (double)INFINITY)) bad = true;
  }
  if (bad) atomicMin(&ctl[LR_BAD_ROW], v);
  if (lane == 0) {
    unsigned long long s = 0ull;
    for (unsigned g = lo; g < hi; ++g) {
      range_pre[g] = s;
      const long long len = (long long)R.range_end[g] - (long long)R.range_begin[g] + 1ll;
      s += len > 0 ? (unsigned long long)len : 0ull;
    }
    row_ports[v] = s;
    if (seg_end[v] > seg_start[v]) atomicAdd(&ctl[LR_OFFERS_USED], 1u);
  }
}

// thread i, as sorted position p = i: the ports of the task there (0 when not kept), its segment head, its requests slot by slot; as
// considered position k = i: the same ports in considered order
COOK_KERNEL void lr_gather(const uint32_t* __restrict__ perm, const uint64_t* __restrict__ okey, unsigned K, unsigned M, unsigned n_res, LrJobs J,
                           uint32_t* __restrict__ ports_p, uint8_t* __restrict__ head_p, double* __restrict__ req_p, uint32_t* __restrict__ ports_k,
                           unsigned* __restrict__ ctl) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  bool kept_k = false;
  if (i < K) {
    const unsigned k = perm[i];
    const uint64_t key = okey[k];
    const bool kept = key < (uint64_t)M;
    const unsigned jj = J.j_index ? J.j_index[k] : k;
    const int want = (kept && J.ports) ? J.ports[jj] : 0;
    ports_p[i] = want > 0 ? (uint32_t)want : 0u;
    head_p[i] = (i == 0 || okey[perm[i - 1]] != key) ? 1 : 0;
    for (unsigned r = 0; r < n_res; ++r) req_p[(size_t)r * K + i] = kept ? J.col[r][jj] : 0.0;
    kept_k = okey[i] < (uint64_t)M;
    const unsigned ji = J.j_index ? J.j_index[i] : i;
    const int wk = (kept_k && J.ports) ? J.ports[ji] : 0;
    ports_k[i] = wk > 0 ? (uint32_t)wk : 0u;
  }
  const unsigned long long b = __ballot(kept_k);
  if (lane_id() == 0 && b) atomicAdd(&ctl[LR_KEPT], (unsigned)__popcll(b));
}

// behind the two scans (inclusive): cursor[k] = the ports of the kept tasks ahead of task k on its offer; a segment that asks for more
// than its row holds raises the row; port_off[k] = the ports of the tasks in front of k, port_off[K] and ctl = all of them
COOK_KERNEL void lr_cursors(const uint32_t* __restrict__ perm, const uint64_t* __restrict__ okey, unsigned K, unsigned M,
                            const uint32_t* __restrict__ ports_p, const SumU64* __restrict__ incl_p, const uint32_t* __restrict__ ports_k,
                            const SumU64* __restrict__ incl_k, const uint32_t* __restrict__ seg_end,
                            const unsigned long long* __restrict__ row_ports, unsigned long long* __restrict__ cursor,
                            uint32_t* __restrict__ port_off, unsigned* __restrict__ ctl) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  const unsigned k = perm[i];
  const uint64_t key = okey[k];
  unsigned long long c = 0ull;
  if (key < (uint64_t)M) {
    c = incl_p[i].v - (unsigned long long)ports_p[i];
    if (i + 1u == seg_end[key] && incl_p[i].v > row_ports[key]) atomicMin(&ctl[LR_BAD_ROW], (unsigned)key);
  }
  cursor[k] = c;
  port_off[i] = (uint32_t)(incl_k[i].v - (unsigned long long)ports_k[i]);  // (truncated only where the call is refused: more than cap ports)
  if (i + 1u == K) {
    port_off[K] = (uint32_t)incl_k[i].v;
    ctl[LR_PORTS_LO] = (unsigned)incl_k[i].v, ctl[LR_PORTS_HI] = (unsigned)(incl_k[i].v >> 32);
  }
}

// take-resources: thread t = (slot r, row v) walks the row's kept tasks in considered order, role after role in take order.  take and
// short_mask are zero beforehand
COOK_KERNEL void lr_take_chains(LrRows R, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ seg_start,
                                const uint32_t* __restrict__ seg_end, unsigned K, const double* __restrict__ req_p, double* __restrict__ take,
                                uint32_t* __restrict__ short_mask) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= R.n * R.n_res) return;
  const unsigned v = t % R.n, r = t / R.n;
  const unsigned p0 = seg_start[v], p1 = seg_end[v];
  if (p0 >= p1) return;
  double av[COOK_MAX_ROLES];
#pragma unroll
  for (unsigned x = 0; x < COOK_MAX_ROLES; ++x) av[x] = x < R.n_roles ? R.avail[((size_t)r * R.n_roles + x) * R.n + v] : 0.0;
  const double* req = req_p + (size_t)r * K;
  for (unsigned p = p0; p < p1; ++p) {
    double still = req[p];
    if (still != still) continue;  // no request under this name
    double* out = take + ((size_t)perm[p] * R.n_res + r) * R.n_roles;
#pragma unroll
    for (unsigned x = 0; x < COOK_MAX_ROLES; ++x) {
      if (x >= R.n_roles) break;
      const double a = av[x];
      const double amount = still < a ? still : a;
      if (amount > 0.0) {
        still = still - amount;
        av[x] = a - amount;
        out[x] = amount;
      }
    }
    if (still != 0.0) atomicOr(&short_mask[perm[p]], 1u << r);
  }
}

COOK_KERNEL void lr_count_short(const uint32_t* __restrict__ short_mask, unsigned K, unsigned* __restrict__ ctl) {
  const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long b = __ballot(k < K && short_mask[k] != 0u);
  if (lane_id() == 0 && b) atomicAdd(&ctl[LR_SHORT], (unsigned)__popcll(b));
}

// the range of row [lo, hi) that holds the row's c-th port (c below the row's ports)
static __device__ __forceinline__ unsigned lr_range_of(const unsigned long long* __restrict__ range_pre, unsigned lo, unsigned hi, unsigned long long c) {
  unsigned a = lo, b = hi;  // the last g in [lo, hi) with range_pre[g] <= c
  while (b - a > 1u) {
    const unsigned m = a + (b - a) / 2u;
    if (range_pre[m] <= c) a = m;
    else b = m;
  }
  return a;
}

// output port q of `total`: its task (the last k with port_off[k] <= q), its number c in the row's sequence, its range, and its place in
// the task's ascending order: behind the ports that the task's slice [c0, c1) takes from ranges that begin lower (the ranges of a row
// are disjoint, so their begins order them).  The three guards keep every access in bounds whatever the inputs; the checks in front of this
// kernel rule each of them out, so one that fires is raised in ctl[LR_BROKEN] and the call fails instead of returning a port never written
COOK_KERNEL void lr_emit_ports(LrRows R, const int32_t* __restrict__ j2o, const uint32_t* __restrict__ port_off, unsigned K, unsigned total,
                               const unsigned long long* __restrict__ cursor, const unsigned long long* __restrict__ range_pre,
                               int32_t* __restrict__ port, uint8_t* __restrict__ port_role, unsigned* __restrict__ ctl) {
  const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total) return;
  unsigned a = 0u, b = K;  // the last k in [0, K) with port_off[k] <= q (a task without ports shares its offset with the next)
  while (b - a > 1u) {
    const unsigned m = a + (b - a) / 2u;
    if (port_off[m] <= q) a = m;
    else b = m;
  }
  const unsigned k = a;
  const int v = j2o[k];
  if (v < 0 || (unsigned)v >= R.n) {
    atomicOr(&ctl[LR_BROKEN], 1u);
    return;
  }
  const unsigned lo = R.range_off[v], hi = R.range_off[v + 1];
  if (lo >= hi) {
    atomicOr(&ctl[LR_BROKEN], 2u);
    return;
  }
  const unsigned long long c0 = cursor[k], c1 = c0 + (unsigned long long)(port_off[k + 1] - port_off[k]), c = c0 + (unsigned long long)(q - port_off[k]);
  const unsigned g = lr_range_of(range_pre, lo, hi, c), g0 = lr_range_of(range_pre, lo, hi, c0), g1 = lr_range_of(range_pre, lo, hi, c1 - 1ull);
  const int begin = R.range_begin[g];
  unsigned long long before = c - (range_pre[g] > c0 ? range_pre[g] : c0);
  for (unsigned h = g0; h <= g1; ++h) {
    if (R.range_begin[h] >= begin) continue;
    const unsigned long long len = (unsigned long long)((long long)R.range_end[h] - (long long)R.range_begin[h] + 1ll);
    const unsigned long long s = range_pre[h] > c0 ? range_pre[h] : c0, en = range_pre[h] + len < c1 ? range_pre[h] + len : c1;
    if (s < en) before += en - s;
  }
  const unsigned at = port_off[k] + (unsigned)before;
  if (at >= total) {
    atomicOr(&ctl[LR_BROKEN], 4u);
    return;
  }
  port[at] = begin + (int)(c - range_pre[g]);
  port_role[at] = R.range_role[g];
}
