// usage_kernels.hpp — device side of cook_usage_breakdown / cook_usage_breakdown_multi: GET /usage with its job-group breakdown
// (rest/api.clj:2894-2969 user-usage / usage / get-user-usage over tools/total-resources-of-jobs, tools.clj:294-306) from the per-user
// order the last rank run of every engine left on the device.
//
// Index spaces: A = task row of an engine's staged cook_tasks;  P = position in the CONCATENATION of the engines' per-user orders
//               (engine q owns base_q .. base_q + N_q, its part is rank_gather's s_use / s_pending / s_user, permB[P - base_q] = A);
//               S = place in the stable sort of P by (user, bucket key): the first R places are the running rows, bucket by bucket;
//               T = place in the order of the per-user total: P itself for one engine without a user map (the rank's order in place),
//                   else the stable sort of P by user alone (user, engine, task order);  b = bucket;  u = user of the call.
//
// Key of a position: user << gbits | (0 = no group, g + 1 = group g); a pending row gets the user n_users, one past the last, so that it
// sorts behind every running row and the first R places of S (and of T) are the running rows.  The ungrouped bucket of a user therefore
// stands FIRST among the user's buckets, the grouped ones follow in ascending group id.
//
// Sums: total-resources-of-jobs starts from 0.0 and adds left to right.  The segmented scans start from a bucket's (a user's) first
// value instead; the two differ only for a first value of -0.0, which the loads flag like a rounded addition.  A bucket (user) with a
// flag anywhere among its prefixes is folded again from 0.0 left to right (common.hpp "exact-sum tracking").
#pragma once
#include "common.hpp"
#include "scan.hpp"

struct UbPool {  // one engine of a call (device memory)
  unsigned base, n;          // its positions of the concatenation
  const SumU4* use;          // [n] rank_gather's rows
  const uint8_t* pending;    // [n]
  const uint32_t* s_user;    // [n] the engine's own user ids
  const uint32_t* permB;     // [n] position -> task row
  const uint32_t* map;       // engine user -> user of the call, or null = the identity
  const uint32_t* group;     // group_of_row by task row, or null = every row ungrouped
};

// the engine that owns position p: the last one whose base is <= p (an engine without rows shares its base with the next one)
static __device__ __forceinline__ unsigned ub_pool_of(const UbPool* __restrict__ pools, unsigned n_pools, unsigned p) {
  unsigned lo = 0, hi = n_pools;
  while (hi - lo > 1u) {
    const unsigned mid = (lo + hi) >> 1;
    if (pools[mid].base <= p) lo = mid; else hi = mid;
  }
  return lo;
}

static __device__ __forceinline__ SumU4 ub_value(const UbPool* __restrict__ pools, unsigned n_pools, unsigned p) {
  const UbPool& q = pools[ub_pool_of(pools, n_pools, p)];
  const unsigned l = p - q.base;
  if (q.pending[l]) return SumU4::zero();
  SumU4 x = q.use[l];
  if (__double_as_longlong(x.cpus) == LLONG_MIN || __double_as_longlong(x.mem) == LLONG_MIN || __double_as_longlong(x.gpus) == LLONG_MIN)
    x.bad = 1u;  // 0.0 + -0.0 is +0.0: the fold from 0.0 loses a leading -0.0, a scan that starts from it does not
  return x;
}

struct LoadUbRows {  // the value at place j of an order over the positions (perm null: the positions themselves)
  const UbPool* pools;
  unsigned n_pools;
  const uint32_t* perm;
  __device__ __forceinline__ SumU4 operator()(unsigned j) const { return ub_value(pools, n_pools, perm ? perm[j] : j); }
};
struct LoadUbHead {
  const uint8_t* h;
  __device__ __forceinline__ SumI operator()(unsigned j) const { return SumI{h[j] ? 1 : 0}; }
};
struct LoadUbInt {
  const int* p;
  __device__ __forceinline__ SumI operator()(unsigned j) const { return SumI{p[j]}; }
};

// ---- per position: its key; a running row whose group id is neither a group nor COOK_NONE_U32 raises *err
COOK_KERNEL void ub_keys(const UbPool* __restrict__ pools, unsigned n_pools, unsigned n_total, unsigned n_users, unsigned n_groups,
                         unsigned gbits, uint64_t* __restrict__ key, uint32_t* __restrict__ err) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_total) return;
  const UbPool& q = pools[ub_pool_of(pools, n_pools, p)];
  const unsigned l = p - q.base;
  if (q.pending[l]) {
    key[p] = (uint64_t)n_users << gbits;
    return;
  }
  unsigned u = q.s_user[l];
  if (q.map) u = q.map[u];
  unsigned g = q.group ? q.group[q.permB[l]] : COOK_NONE_U32;
  if (g != COOK_NONE_U32 && g >= n_groups) {
    *err = 1u;
    g = COOK_NONE_U32;
  }
  key[p] = ((uint64_t)u << gbits) | (g == COOK_NONE_U32 ? 0ull : (uint64_t)g + 1ull);
}

// ---- per place of S among the running rows: does a bucket start here, and which row is it (stride 2: engine index, task row)
COOK_KERNEL void ub_heads(const uint64_t* __restrict__ key, const uint32_t* __restrict__ permS, unsigned R, const UbPool* __restrict__ pools,
                          unsigned n_pools, unsigned stride, uint8_t* __restrict__ head, uint32_t* __restrict__ rows) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= R) return;
  const unsigned p = permS[j];
  head[j] = (j == 0u || key[permS[j - 1u]] != key[p]) ? 1 : 0;
  const unsigned qi = ub_pool_of(pools, n_pools, p);
  const unsigned row = pools[qi].permB[p - pools[qi].base];
  if (stride == 2u) rows[2u * (size_t)j] = qi;
  rows[(size_t)stride * j + (stride - 1u)] = row;
}

// ---- per place of T among the running rows (the sorted form): does a user start here
COOK_KERNEL void ub_user_heads(const uint64_t* __restrict__ key, const uint32_t* __restrict__ permT, unsigned R, unsigned gbits,
                               uint8_t* __restrict__ head) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= R) return;
  head[j] = (j == 0u || (key[permT[j - 1u]] >> gbits) != (key[permT[j]] >> gbits)) ? 1 : 0;
}

// ---- the users with ANY flagged prefix of their total (not only the last: an exact total does not make the prefixes before it exact)
COOK_KERNEL void ub_mark_users(const SumU4* __restrict__ preT, const uint64_t* __restrict__ key, const uint32_t* __restrict__ permT,
                               unsigned len, unsigned gbits, unsigned n_users, uint32_t* __restrict__ uflag) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= len || !preT[j].bad) return;
  const uint64_t u = key[permT ? permT[j] : j] >> gbits;
  if (u < n_users) uflag[u] = 1u;  // (a pending row carries the user n_users; its prefix is that of the running rows before it)
}

// ---- per place of S among the running rows: the bucket's flag, and at its first / last row its group, row offset and usage
COOK_KERNEL void ub_emit(const SumU4* __restrict__ preS, const uint8_t* __restrict__ head, const SumI* __restrict__ bidx,
                         const uint64_t* __restrict__ key, const uint32_t* __restrict__ permS, unsigned R, unsigned gbits,
                         uint32_t* __restrict__ bflag, uint32_t* __restrict__ bucket_group, double* __restrict__ usage,
                         uint32_t* __restrict__ row_off, uint32_t* __restrict__ counts) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= R) return;
  const unsigned b = (unsigned)bidx[j].v - 1u;
  const SumU4 t = preS[j];
  if (t.bad) bflag[b] = 1u;
  if (head[j]) {
    row_off[b] = j;
    const uint64_t gk = gbits ? key[permS[j]] & ((1ull << gbits) - 1ull) : 0ull;
    bucket_group[b] = gk ? (uint32_t)(gk - 1ull) : COOK_NONE_U32;
  }
  if (j + 1u == R || head[j + 1u]) {
    double* o = usage + (size_t)b * 4;
    o[0] = t.cpus, o[1] = t.mem, o[2] = t.gpus, o[3] = t.count;
  }
  if (j + 1u == R) {
    row_off[b + 1u] = R;
    counts[0] = b + 1u;
  }
}

// ---- a flagged bucket again, from 0.0 left to right (fractional inputs only); one thread per bucket
COOK_KERNEL void ub_fold(const UbPool* __restrict__ pools, unsigned n_pools, const uint32_t* __restrict__ permS,
                         const uint32_t* __restrict__ row_off, const uint32_t* __restrict__ bflag, const uint32_t* __restrict__ counts,
                         double* __restrict__ usage) {
  const unsigned b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= counts[0] || !bflag[b]) return;
  double c = 0.0, m = 0.0, g = 0.0;
  for (unsigned j = row_off[b]; j < row_off[b + 1u]; ++j) {
    const SumU4 x = ub_value(pools, n_pools, permS[j]);
    c += x.cpus, m += x.mem, g += x.gpus;
  }
  double* o = usage + (size_t)b * 4;
  o[0] = c, o[1] = m, o[2] = g;
}

// the first place in [0, R) of an order whose user is >= u (R: none)
static __device__ __forceinline__ unsigned ub_lower(const uint64_t* __restrict__ key, const uint32_t* __restrict__ perm, unsigned R,
                                                    unsigned gbits, uint64_t u) {
  unsigned lo = 0, hi = R;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if ((key[perm[mid]] >> gbits) < u) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// ---- per user u (and u = n_users for the end of the offsets): where its buckets start, and its total over ALL its running rows in the
// order T; a flagged user folded again from 0.0.  permT null: T is the one engine's own order, the user's part its segment.
COOK_KERNEL void ub_users(unsigned n_users, unsigned R, const uint64_t* __restrict__ key, const uint32_t* __restrict__ permS,
                          const SumI* __restrict__ bidx, unsigned gbits, const uint32_t* __restrict__ counts,
                          const SumU4* __restrict__ preT, const uint32_t* __restrict__ permT, const uint32_t* __restrict__ seg_start,
                          const uint32_t* __restrict__ seg_end, const uint32_t* __restrict__ uflag, const UbPool* __restrict__ pools,
                          unsigned n_pools, uint32_t* __restrict__ bucket_off, double* __restrict__ total) {
  const unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u > n_users) return;
  const unsigned j0 = ub_lower(key, permS, R, gbits, u);
  bucket_off[u] = j0 < R ? (unsigned)bidx[j0].v - 1u : counts[0];
  if (u == n_users) return;
  unsigned a, b;
  if (permT) {
    a = ub_lower(key, permT, R, gbits, u);
    b = ub_lower(key, permT, R, gbits, (uint64_t)u + 1ull);
  } else {
    b = seg_end[u];  // (rank_init: 0 = the user has no row in this pool)
    a = b ? seg_start[u] : 0u;
  }
  double c = 0.0, m = 0.0, g = 0.0, n = 0.0;
  if (b > a) {
    const SumU4 t = preT[b - 1u];
    c = t.cpus, m = t.mem, g = t.gpus, n = t.count;
    if (uflag[u]) {
      c = 0.0, m = 0.0, g = 0.0;
      for (unsigned j = a; j < b; ++j) {
        const SumU4 x = ub_value(pools, n_pools, permT ? permT[j] : j);
        if (x.count != 0.0) c += x.cpus, m += x.mem, g += x.gpus;  // (a pending row of the segment adds nothing, not even +0.0)
      }
    }
  }
  double* o = total + (size_t)u * 4;
  o[0] = c, o[1] = m, o[2] = g, o[3] = n;
}

// ---- a list of users: how many buckets and rows each listed user brings
COOK_KERNEL void ub_list_sizes(const uint32_t* __restrict__ users, unsigned n_list, const uint32_t* __restrict__ bucket_off,
                               const uint32_t* __restrict__ row_off, int* __restrict__ lb, int* __restrict__ lr) {
  const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_list) return;
  const unsigned u = users[k], b0 = bucket_off[u], b1 = bucket_off[u + 1u];
  lb[k] = (int)(b1 - b0);
  lr[k] = (int)(row_off[b1] - row_off[b0]);
}

// the list entry that owns output index x: the first k whose inclusive sum exceeds x
static __device__ __forceinline__ unsigned ub_owner(const SumI* __restrict__ incl, unsigned n_list, unsigned x) {
  unsigned lo = 0, hi = n_list;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if ((unsigned)incl[mid].v <= x) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

COOK_KERNEL void ub_gather_users(const uint32_t* __restrict__ users, unsigned n_list, const SumI* __restrict__ lbs,
                                 const double* __restrict__ total, uint32_t* __restrict__ o_bucket_off, double* __restrict__ o_total,
                                 uint32_t* __restrict__ o_row_off) {
  const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_list) return;
  if (k == 0u) o_bucket_off[0] = 0u, o_row_off[0] = 0u;
  o_bucket_off[k + 1u] = (unsigned)lbs[k].v;
  const double* t = total + (size_t)users[k] * 4;
  double* o = o_total + (size_t)k * 4;
  o[0] = t[0], o[1] = t[1], o[2] = t[2], o[3] = t[3];
}

COOK_KERNEL void ub_gather_buckets(const uint32_t* __restrict__ users, unsigned n_list, const SumI* __restrict__ lbs,
                                   const SumI* __restrict__ lrs, const uint32_t* __restrict__ bucket_off,
                                   const uint32_t* __restrict__ row_off, const uint32_t* __restrict__ bucket_group,
                                   const double* __restrict__ usage, unsigned n_buckets, unsigned n_rows, uint32_t* __restrict__ o_group,
                                   double* __restrict__ o_usage, uint32_t* __restrict__ o_row_off) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_buckets) return;
  const unsigned k = ub_owner(lbs, n_list, x);
  const unsigned b0 = bucket_off[users[k]];
  const unsigned b = b0 + (x - (k ? (unsigned)lbs[k - 1u].v : 0u));
  o_row_off[x] = (k ? (unsigned)lrs[k - 1u].v : 0u) + (row_off[b] - row_off[b0]);
  if (x + 1u == n_buckets) o_row_off[n_buckets] = n_rows;
  o_group[x] = bucket_group[b];
  const double* s = usage + (size_t)b * 4;
  double* o = o_usage + (size_t)x * 4;
  o[0] = s[0], o[1] = s[1], o[2] = s[2], o[3] = s[3];
}

COOK_KERNEL void ub_gather_rows(const uint32_t* __restrict__ users, unsigned n_list, const SumI* __restrict__ lrs,
                                const uint32_t* __restrict__ bucket_off, const uint32_t* __restrict__ row_off,
                                const uint32_t* __restrict__ rows, unsigned stride, unsigned n_rows, uint32_t* __restrict__ o_rows) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_rows) return;
  const unsigned k = ub_owner(lrs, n_list, x);
  const unsigned j = row_off[bucket_off[users[k]]] + (x - (k ? (unsigned)lrs[k - 1u].v : 0u));
  if (stride == 2u) o_rows[2u * (size_t)x] = rows[2u * (size_t)j];
  o_rows[(size_t)stride * x + (stride - 1u)] = rows[(size_t)stride * j + (stride - 1u)];
}
