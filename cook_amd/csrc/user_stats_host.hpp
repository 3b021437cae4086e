// user_stats_host.hpp — host orchestration of cook_user_stats / cook_user_stats_multi (included by engine.hip inside its anonymous
// namespace).  Both read the per-user order of the LAST rank run of every engine in place on the device (rank_gather's rows and
// segments) and change nothing of the rank, considerable or match state: everything they write lives in UserStatsBufs.
// All launches go to the first engine's stream, after every engine's own stream has drained; one synchronisation at the end.
#pragma once
#include "user_stats_kernels.hpp"

struct UserStatsBufs {
  // as a member pool of a call
  DArr<SumRW> pre;
  DArr<uint32_t> map, inv;
  DArr<double> carry;
  ScanTmp<SumRW> tmp;
  // as the first engine of a call
  DArr<uint32_t> flags;
  DArr<unsigned> counts;
  DArr<double> out, res, lim[6];
  DArr<uint8_t> state, extra;
  DArr<SumRW> all_a, all_b;
  DArr<UsPool> pools;
};


void user_stats_run(cook_engine* const* es, unsigned n, const uint32_t* const* maps, unsigned n_users, const cook_user_limits* lim,
                    double* per_user, bool per_user_is_device, uint8_t* user_state, cook_user_stats_totals* totals) {
  cook_engine* e = es[0];
  for (unsigned i = 0; i < n; ++i)
    if (!es[i]->rank_done) e->fail(COOK_E_STATE, "cook_user_stats before cook_rank_run (or after a stage / cook_cycle_update no rank has followed)");
  if (per_user_is_device && !per_user) e->fail(COOK_E_INVALID, "cook_user_stats: per_user_is_device without per_user");
  if (lim) {
    if (lim->n != n_users) e->fail(COOK_E_INVALID, "cook_user_stats: limits.n is not the number of users");
    if (n_users && (!lim->share_cpus || !lim->share_mem || !lim->quota_count || !lim->quota_cpus || !lim->quota_mem || !lim->quota_gpus))
      e->fail(COOK_E_INVALID, "cook_user_stats: a limits array is NULL");
  } else if (n != 1 || (maps && maps[0]) || n_users != e->U) {
    e->fail(COOK_E_INVALID, "cook_user_stats: the staged users stand in for the limits of one engine's own users only");
  }
  for (unsigned i = 0; i < n; ++i) {
    const unsigned U = es[i]->U;
    if (maps && maps[i]) {
      std::vector<uint8_t> seen(n_users, 0);
      for (unsigned u = 0; u < U; ++u) {
        const uint32_t g = maps[i][u];
        if (g >= n_users || seen[g]) e->fail(COOK_E_INVALID, "cook_user_stats_multi: user_map out of range or not one-to-one");
        seen[g] = 1;
      }
    } else if (U > n_users) {
      e->fail(COOK_E_INVALID, "cook_user_stats_multi: an engine has more users than n_users (and no user_map)");
    }
  }
  for (unsigned i = 0; i < n; ++i) COOK_HIP(hipStreamSynchronize(es[i]->stream));  // (the ranks ran on the engines' own streams)
  UserStatsBufs& L = bufs(e->usb);
  uint32_t* flags = L.flags.ensure(n_users);
  unsigned* counts = L.counts.ensure(8);
  const unsigned nblk = std::max(1u, std::min(div_up(n_users, 256), 64u));
  KM<us_init, 256>(e, "us_init", nblk, flags, n_users, counts, nblk);
  const double *s_cpus, *s_mem, *q_count, *q_cpus, *q_mem, *q_gpus;
  const uint8_t* extra = nullptr;
  if (lim) {
    const double* src[6] = {lim->share_cpus, lim->share_mem, lim->quota_count, lim->quota_cpus, lim->quota_mem, lim->quota_gpus};
    for (int k = 0; k < 6; ++k) h2d(e, L.lim[k], src[k], n_users);
    s_cpus = L.lim[0].ptr(), s_mem = L.lim[1].ptr(), q_count = L.lim[2].ptr(), q_cpus = L.lim[3].ptr(), q_mem = L.lim[4].ptr(),
    q_gpus = L.lim[5].ptr();
    extra = h2d_opt(e, L.extra, lim->extra_quota_positive, n_users);
  } else {  // the engine's staged cook_users: the DRU divisors are the shares, the quotas as they are
    s_cpus = e->u_divc.ptr(), s_mem = e->u_divm.ptr(), q_count = e->u_qcount.ptr(), q_cpus = e->u_qcpus.ptr(), q_mem = e->u_qmem.ptr(),
    q_gpus = e->u_qgpus.ptr();
  }
  // ---- per pool: the segmented scan of running / waiting over the pool's per-user order, its rounded users, the inverse user map
  std::vector<UsPool> hp(n);
  std::vector<const uint32_t*> dmaps(n, nullptr);
  for (unsigned i = 0; i < n; ++i) {
    cook_engine* p = es[i];
    UserStatsBufs& B = bufs(p->usb);
    const unsigned N = p->N, U = p->U;
    if (maps && maps[i]) {
      h2d(e, B.map, maps[i], U);
      dmaps[i] = B.map.ptr();
    }
    B.inv.ensure(n_users);
    memset_async(e, B.inv.ptr(), 0xFF, (size_t)n_users * 4);
    KM<us_invert, 256>(e, "us_invert", div_up(U, 256), dmaps[i], U, B.inv.ptr());
    UsPool& q = hp[i];
    q = UsPool{nullptr, nullptr, nullptr, nullptr, nullptr, B.inv.ptr(), nullptr};
    if (N == 0) continue;  // (rank_run leaves the segments of an empty table as they were)
    B.pre.ensure(N);
    seg_scan<SumRW>(e, "us_task_scan", LoadTaskRW{p->s_use.ptr(), p->s_pending.ptr()}, (const uint8_t*)p->head.ptr(), N, B.pre.ptr(), B.tmp);
    KM<us_mark, 256>(e, "us_mark", div_up(N, 256), (const SumRW*)B.pre.ptr(), (const uint32_t*)p->s_user.ptr(), dmaps[i], N, flags);
    if (i > 0) B.carry.ensure((size_t)U * 4);
    q = UsPool{B.pre.ptr(), p->s_use.ptr(), p->s_pending.ptr(), p->seg_start.ptr(), p->seg_end.ptr(), B.inv.ptr(), i > 0 ? B.carry.ptr() : nullptr};
  }
  h2d(e, L.pools, hp.data(), n);
  // ---- per group user: the pools' totals in pool order; rows that rounded somewhere are folded again left to right
  double* out = per_user_is_device ? per_user : L.out.ensure((size_t)n_users * 12);
  KM<us_combine, 256>(e, "us_combine", div_up(n_users, 256), (const UsPool*)L.pools.ptr(), n, n_users, flags, out);
  for (unsigned i = 1; i < n; ++i) {
    const cook_engine* p = es[i];
    if (p->N)
      KM<us_check, 256>(e, "us_check", div_up(p->N, 256), (const SumRW*)bufs(es[i]->usb).pre.ptr(), (const uint32_t*)p->s_user.ptr(), dmaps[i],
          (const double*)bufs(es[i]->usb).carry.ptr(), p->N, flags);
  }
  KM<us_fold, 64>(e, "us_fold", div_up(n_users, 64), (const UsPool*)L.pools.ptr(), n, n_users, (const uint32_t*)flags, out);
  // ---- starved / under quota / counts, then the "all" rows
  uint8_t* state = L.state.ensure(n_users);
  KM<us_classify, 256>(e, "us_classify", div_up(n_users, 256), out, n_users, s_cpus, s_mem, q_count, q_cpus, q_mem, q_gpus, extra, state, counts);
  L.all_a.ensure(n_users);
  L.all_b.ensure(n_users);
  seg_scan<SumRW>(e, "us_all_scan", LoadUserRows{out, 0u}, (const uint8_t*)nullptr, n_users, L.all_a.ptr(), L.tmp);
  seg_scan<SumRW>(e, "us_all_scan", LoadUserRows{out, 6u}, (const uint8_t*)nullptr, n_users, L.all_b.ptr(), L.tmp);
  double* res = L.res.ensure(17);
  KM<us_finish, 256>(e, "us_finish", 1, (const SumRW*)L.all_a.ptr(), (const SumRW*)L.all_b.ptr(), (const double*)out, n_users,
      (const unsigned*)counts, res);
  double h[17];
  copy_async(e, h, res, sizeof(h), hipMemcpyDeviceToHost);
  if (per_user && !per_user_is_device) copy_async(e, per_user, out, (size_t)n_users * 12 * sizeof(double), hipMemcpyDeviceToHost);
  if (user_state) copy_async(e, user_state, state, n_users, hipMemcpyDeviceToHost);
  sync(e);
  if (totals) {
    std::memcpy(totals->all, h, 12 * sizeof(double));
    totals->total = (uint32_t)h[12], totals->starved = (uint32_t)h[13], totals->waiting_under_quota = (uint32_t)h[14],
    totals->hungry = (uint32_t)h[15], totals->satisfied = (uint32_t)h[16], totals->reserved = 0u;
  }
}
