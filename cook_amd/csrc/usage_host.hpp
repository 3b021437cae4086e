// usage_host.hpp — host orchestration of cook_usage_breakdown / cook_usage_breakdown_multi (included by engine.hip inside its anonymous
// namespace).  Both read the per-user order of the LAST rank run of every engine in place on the device (rank_gather's rows and
// segments, permB) and change nothing of the rank, considerable or match state: everything they write lives in UsageBufs.
// All launches go to the first engine's stream, after every engine's own stream has drained.  Two synchronisations: one after the
// buckets are formed, for the bad-group flag and the counts B and R (a call that fails has written nothing, and the copies to the host
// then move B entries, not the R the buffers have room for), one at the end.
//
// The order S is ONE stable LSD sort of the concatenated positions by the whole key (user digits above the group digits), not the sort
// by the group digits alone that stability would allow within one engine: `rows`, `row_off` and `bucket_off` are user-major, so a
// group-major result would have to be moved once more (a scatter of R rows and a sort of up to R bucket heads — as much traffic as the
// user digits' passes), and across several engines the input is not in user order to begin with.  The key's bits come from n_users
// and n_groups on the host, so no varying-bits pass and no read-back stand before the sort.
#pragma once
#include "usage_kernels.hpp"

struct UsageBufs {
  // as a member engine of a call
  DArr<uint32_t> map, group;
  // as the first engine of a call
  DArr<UbPool> pools;
  DArr<uint64_t> key;
  DArr<uint32_t> sa, sb, ta, tb, hist, rows, bflag, uflag, b_group, row_off, bucket_off, counts, users;
  DArr<uint8_t> head_s, head_t;
  DArr<SumU4> pre_s, pre_t;
  DArr<SumI> bidx, lbs, lrs;
  DArr<int> lb, lr;
  DArr<double> b_usage, total;
  ScanTmp<SumU4> tmp4;
  ScanTmp<SumI> tmpi;
  // a list of users: the gathered outputs
  DArr<uint32_t> o_group, o_row_off, o_rows, o_bucket_off;
  DArr<double> o_usage, o_total;
};


static unsigned ub_bit_width(unsigned v) { return v ? 32u - (unsigned)__builtin_clz(v) : 0u; }

void usage_run(cook_engine* const* es, unsigned n, const uint32_t* const* maps, unsigned n_users, const uint32_t* const* groups,
               unsigned n_groups, const uint32_t* users, unsigned n_list, cook_usage_out* out, bool multi) {
  cook_engine* e = es[0];
  const char* who = multi ? "cook_usage_breakdown_multi" : "cook_usage_breakdown";
  if (!out) e->fail(COOK_E_INVALID, std::string(who) + ": null out");
  for (unsigned i = 0; i < n; ++i)
    if (!es[i]->rank_done) e->fail(COOK_E_STATE, std::string(who) + " before cook_rank_run (or after a stage / cook_cycle_update no rank has followed)");
  if ((out->bucket_usage_is_device && !out->bucket_usage) || (out->total_is_device && !out->total))
    e->fail(COOK_E_INVALID, std::string(who) + ": *_is_device without the buffer");
  size_t n_total = 0, n_running = 0;
  bool any_group = false;
  for (unsigned i = 0; i < n; ++i) {
    const unsigned U = es[i]->U;
    if (maps && maps[i]) {
      std::vector<uint8_t> seen(n_users, 0);
      for (unsigned u = 0; u < U; ++u) {
        const uint32_t g = maps[i][u];
        if (g >= n_users || seen[g]) e->fail(COOK_E_INVALID, std::string(who) + ": user_map out of range or not one-to-one");
        seen[g] = 1;
      }
    } else if (U > n_users) {
      e->fail(COOK_E_INVALID, std::string(who) + ": an engine has more users than n_users (and no user_map)");
    }
    n_total += es[i]->N;
    n_running += es[i]->N - es[i]->n_pending;
    any_group = any_group || (groups && groups[i]);
  }
  if (n_total >= 0x7FFFFFFFull) e->fail(COOK_E_INVALID, std::string(who) + ": more than 2^31 - 2 task rows");
  for (unsigned k = 0; users && k < n_list; ++k)
    if (users[k] >= n_users) e->fail(COOK_E_INVALID, std::string(who) + ": a listed user is no user");
  const unsigned NT = (unsigned)n_total, R = (unsigned)n_running;
  const unsigned n_out = users ? n_list : n_users;
  if (!users && out->cap_rows < R) {
    out->n_buckets = R, out->n_rows = R;
    e->fail(COOK_E_INVALID, std::string(who) + ": cap_rows is less than the number of running rows");
  }
  const unsigned stride = multi ? 2u : 1u;
  for (unsigned i = 0; i < n; ++i) COOK_HIP(hipStreamSynchronize(es[i]->stream));  // (the ranks ran on the engines' own streams)
  UsageBufs& L = bufs(e->ugb);
  uint32_t B_all = 0;  // buckets of all users
  uint32_t* counts = L.counts.ensure(4);
  double* d_total = L.total.ensure((size_t)n_users * 4);
  uint32_t* d_boff = L.bucket_off.ensure((size_t)n_users + 1);
  uint32_t* d_roff = L.row_off.ensure((size_t)R + 1);
  uint32_t* d_group = L.b_group.ensure(R);
  double* d_usage = L.b_usage.ensure((size_t)R * 4);
  uint32_t* d_rows = L.rows.ensure((size_t)R * stride);
  if (R == 0) {  // (rank_run leaves the segments of an empty table as they were: nothing of them is read)
    memset_async(e, d_total, 0, (size_t)n_users * 4 * sizeof(double));
    memset_async(e, d_boff, 0, ((size_t)n_users + 1) * 4);
    memset_async(e, d_roff, 0, 4);
  } else {
    // ---- the engines of the call, their group columns and user maps
    std::vector<UbPool> hp(n);
    unsigned base = 0;
    for (unsigned i = 0; i < n; ++i) {
      cook_engine* p = es[i];
      UsageBufs& Bq = bufs(p->ugb);
      const uint32_t* dmap = (maps && maps[i] && p->U) ? (h2d(e, Bq.map, maps[i], p->U), Bq.map.ptr()) : nullptr;
      const uint32_t* dgrp = (groups && groups[i] && p->N) ? (h2d(e, Bq.group, groups[i], p->N), Bq.group.ptr()) : nullptr;
      hp[i] = UbPool{base, p->N, p->s_use.ptr(), p->s_pending.ptr(), p->s_user.ptr(), p->permB, dmap, dgrp};
      base += p->N;
    }
    h2d(e, L.pools, hp.data(), n);
    const UbPool* pools = L.pools.ptr();
    const unsigned gbits = any_group ? ub_bit_width(n_groups) : 0u, ubits = ub_bit_width(n_users);
    const unsigned kbits = gbits + ubits;
    const unsigned long long mask_all = kbits >= 64u ? ~0ull : (1ull << kbits) - 1ull;
    const unsigned long long mask_user = mask_all & ~((1ull << gbits) - 1ull);
    memset_async(e, counts, 0, 16);
    uint64_t* key = L.key.ensure(NT);
    KM<ub_keys, 256>(e, "ub_keys", div_up(NT, 256), pools, n, NT, n_users, any_group ? n_groups : 0u, gbits, key, counts + 1);
    // ---- S: the stable sort by (user, bucket key); its first R places are the running rows, bucket by bucket, each in task order
    L.sa.ensure(NT), L.sb.ensure(NT);
    const uint32_t* permS = radix_sort_masked(e, key, mask_all, nullptr, L.sa.ptr(), L.sb.ptr(), NT, &L.hist);
    if (!permS) {  // (no bit can vary: the positions themselves)
      KM<iota_u32, 256>(e, "ub_iota", div_up(NT, 256), L.sa.ptr(), NT);
      permS = L.sa.ptr();
    }
    uint8_t* head_s = L.head_s.ensure(R);
    KM<ub_heads, 256>(e, "ub_heads", div_up(R, 256), (const uint64_t*)key, permS, R, pools, n, stride, head_s, d_rows);
    SumU4* pre_s = L.pre_s.ensure(R);
    seg_scan<SumU4>(e, "ub_scan", LoadUbRows{pools, n, permS}, (const uint8_t*)head_s, R, pre_s, L.tmp4);
    SumI* bidx = L.bidx.ensure(R);
    seg_scan<SumI>(e, "ub_head_scan", LoadUbHead{head_s}, (const uint8_t*)nullptr, R, bidx, L.tmpi);
    uint32_t* bflag = L.bflag.ensure(R);
    memset_async(e, bflag, 0, (size_t)R * 4);
    KM<ub_emit, 256>(e, "ub_emit", div_up(R, 256), (const SumU4*)pre_s, (const uint8_t*)head_s, (const SumI*)bidx, (const uint64_t*)key, permS, R, gbits,
        bflag, d_group, d_usage, d_roff, counts);
    KM<ub_fold, 64>(e, "ub_fold", div_up(R, 64), pools, n, permS, (const uint32_t*)d_roff, (const uint32_t*)bflag, (const uint32_t*)counts, d_usage);
    // ---- T: the order of the per-user totals — the rank's own order in place for one engine with its own users, else by user alone
    const bool in_place = n == 1 && !hp[0].map && n_users == e->U;
    const uint32_t* permT = nullptr;
    const uint8_t* head_t = (const uint8_t*)e->head.ptr();
    unsigned len_t = NT;
    if (!in_place) {
      L.ta.ensure(NT), L.tb.ensure(NT);
      permT = radix_sort_masked(e, key, mask_user, nullptr, L.ta.ptr(), L.tb.ptr(), NT, &L.hist);
      if (!permT) {
        KM<iota_u32, 256>(e, "ub_iota", div_up(NT, 256), L.ta.ptr(), NT);
        permT = L.ta.ptr();
      }
      len_t = R;
      KM<ub_user_heads, 256>(e, "ub_user_heads", div_up(R, 256), (const uint64_t*)key, permT, R, gbits, L.head_t.ensure(R));
      head_t = L.head_t.ptr();
    }
    SumU4* pre_t = L.pre_t.ensure(len_t);
    seg_scan<SumU4>(e, "ub_total_scan", LoadUbRows{pools, n, permT}, head_t, len_t, pre_t, L.tmp4);
    uint32_t* uflag = L.uflag.ensure(n_users);
    memset_async(e, uflag, 0, (size_t)n_users * 4);
    KM<ub_mark_users, 256>(e, "ub_mark_users", div_up(len_t, 256), (const SumU4*)pre_t, (const uint64_t*)key, permT, len_t, gbits, n_users, uflag);
    KM<ub_users, 64>(e, "ub_users", div_up(n_users + 1, 64), n_users, R, (const uint64_t*)key, permS, (const SumI*)bidx, gbits, (const uint32_t*)counts,
        (const SumU4*)pre_t, permT, (const uint32_t*)e->seg_start.ptr(), (const uint32_t*)e->seg_end.ptr(), (const uint32_t*)uflag, pools, n, d_boff,
        d_total);
  }
  // ---- a list of users: what each brings, summed
  uint32_t h[4] = {0, 0, 0, 0};  // buckets of all users, bad group, then the list's buckets and rows
  const uint32_t* d_users = nullptr;
  if (users && n_list) {
    h2d(e, L.users, users, n_list);
    d_users = L.users.ptr();
    L.lb.ensure(n_list), L.lr.ensure(n_list), L.lbs.ensure(n_list), L.lrs.ensure(n_list);
    KM<ub_list_sizes, 256>(e, "ub_list_sizes", div_up(n_list, 256), d_users, n_list, (const uint32_t*)d_boff, (const uint32_t*)d_roff, L.lb.ptr(), L.lr.ptr());
    seg_scan<SumI>(e, "ub_list_scan", LoadUbInt{L.lb.ptr()}, (const uint8_t*)nullptr, n_list, L.lbs.ptr(), L.tmpi);
    seg_scan<SumI>(e, "ub_list_scan", LoadUbInt{L.lr.ptr()}, (const uint8_t*)nullptr, n_list, L.lrs.ptr(), L.tmpi);
    copy_async(e, &h[2], L.lbs.ptr() + (n_list - 1), 4, hipMemcpyDeviceToHost);
    copy_async(e, &h[3], L.lrs.ptr() + (n_list - 1), 4, hipMemcpyDeviceToHost);
  }
  if (R) copy_async(e, h, counts, 8, hipMemcpyDeviceToHost);
  sync(e);
  if (h[1]) e->fail(COOK_E_INVALID, std::string(who) + ": a running row's group id is neither below n_groups nor COOK_NONE_U32");
  B_all = h[0];
  const uint32_t Bo = users ? h[2] : B_all, Ro = users ? h[3] : R;
  if (Ro > out->cap_rows) {
    out->n_buckets = Bo, out->n_rows = Ro;
    e->fail(COOK_E_INVALID, std::string(who) + ": cap_rows is less than the rows of the listed users");
  }
  const uint32_t *s_boff = d_boff, *s_group = d_group, *s_roff = d_roff, *s_rows = d_rows;
  const double *s_usage = d_usage, *s_total = d_total;
  if (users) {
    uint32_t* ob = L.o_bucket_off.ensure((size_t)n_list + 1);
    uint32_t* orf = L.o_row_off.ensure((size_t)Bo + 1);
    double* ot = L.o_total.ensure((size_t)n_list * 4);
    uint32_t* og = L.o_group.ensure(Bo);
    double* ou = L.o_usage.ensure((size_t)Bo * 4);
    uint32_t* orw = L.o_rows.ensure((size_t)Ro * stride);
    if (n_list == 0 || Bo == 0) {
      memset_async(e, ob, 0, 4);
      memset_async(e, orf, 0, 4);
    }
    KM<ub_gather_users, 256>(e, "ub_gather_users", div_up(n_list, 256), d_users, n_list, (const SumI*)L.lbs.ptr(), (const double*)d_total, ob, ot, orf);
    KM<ub_gather_buckets, 256>(e, "ub_gather_buckets", div_up(Bo, 256), d_users, n_list, (const SumI*)L.lbs.ptr(), (const SumI*)L.lrs.ptr(),
        (const uint32_t*)d_boff, (const uint32_t*)d_roff, (const uint32_t*)d_group, (const double*)d_usage, Bo, Ro, og, ou, orf);
    KM<ub_gather_rows, 256>(e, "ub_gather_rows", div_up(Ro, 256), d_users, n_list, (const SumI*)L.lrs.ptr(), (const uint32_t*)d_boff,
        (const uint32_t*)d_roff, (const uint32_t*)d_rows, stride, Ro, orw);
    s_boff = ob, s_group = og, s_roff = orf, s_rows = orw, s_usage = ou, s_total = ot;
  }
  if (out->bucket_off) copy_async(e, out->bucket_off, s_boff, ((size_t)n_out + 1) * 4, hipMemcpyDeviceToHost);
  if (out->bucket_group) copy_async(e, out->bucket_group, s_group, (size_t)Bo * 4, hipMemcpyDeviceToHost);
  if (out->bucket_usage)
    copy_async(e, out->bucket_usage, s_usage, (size_t)Bo * 4 * sizeof(double), out->bucket_usage_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
  if (out->row_off) copy_async(e, out->row_off, s_roff, ((size_t)Bo + 1) * 4, hipMemcpyDeviceToHost);
  if (out->rows) copy_async(e, out->rows, s_rows, (size_t)Ro * stride * 4, hipMemcpyDeviceToHost);
  if (out->total)
    copy_async(e, out->total, s_total, (size_t)n_out * 4 * sizeof(double), out->total_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
  sync(e);
  out->n_buckets = Bo, out->n_rows = Ro;
}
