// rank_host.hpp — host orchestration of the rank (cook_rank_*), and the segmented-scan and radix-sort drivers that it and the side
// features use.  Included by engine.hip inside its anonymous namespace, behind launch.hpp; expects rank_kernels.hpp, scan.hpp, sort.hpp and
// tile_sort.hpp.

// ---- segmented scan driver ------------------------------------------------------------------------------------
template <class T, class Load>
void seg_scan(cook_engine* e, const char* tag, Load load, const uint8_t* head, unsigned n, T* out, ScanTmp<T>& tmp) {
  if (n == 0) return;
  const unsigned nb = div_up(n, SS_TILE);
  tmp.agg.ensure(nb);
  tmp.carry.ensure(nb);
  tmp.first_head.ensure(nb);
  KM<seg_scan_local<T, Load>, SS_THREADS>(e, tag, nb, load, head, n, out, tmp.agg.ptr(), tmp.first_head.ptr());
  if (nb > 1 && nb <= (unsigned)SS_THREADS) {
    KM<seg_scan_propagate_fused<T>, SS_THREADS>(e, "seg_scan_propagate", nb, out, n, (const SegAgg<T>*)tmp.agg.ptr(), (const unsigned*)tmp.first_head.ptr());
  } else if (nb > 1) {
    KM<seg_scan_blocksums<T>, SS_THREADS>(e, "seg_scan_blocksums", 1, (const SegAgg<T>*)tmp.agg.ptr(), nb, tmp.carry.ptr());
    KM<seg_scan_propagate<T>, SS_THREADS>(e, "seg_scan_propagate", nb, out, n, (const SegAgg<T>*)tmp.carry.ptr(), (const unsigned*)tmp.first_head.ptr());
  }
}

// ---- radix sort driver: one stable pass of `perm` by the 8 key bits from `shift` up --------------------------------------
// (hist: the histogram scratch, e->hist unless a caller keeps its own)
template <int IPL>
static void radix_pass_t(cook_engine* e, const uint64_t* key, const uint32_t* in, uint32_t* out, unsigned n, unsigned shift, bool fused,
                         DArr<uint32_t>& hist) {
  const unsigned nb = div_up(n, rs_tile(IPL));
  hist.ensure((size_t)256 * nb);
  KM<radix_hist<IPL>, RS_THREADS>(e, "radix_hist", nb, key, in, n, shift, nb, fused ? 1u : 0u, hist.ptr());
  if (!fused) KM<excl_scan_u32_single, SCAN1_THREADS>(e, "radix_scan", 1, hist.ptr(), 256u * nb, (uint32_t*)nullptr);
  KM<radix_scatter<IPL>, RS_THREADS>(e, "radix_scatter", nb, key, in, out, n, shift, nb, fused ? 1u : 0u, (const uint32_t*)hist.ptr());
}
void radix_pass(cook_engine* e, const uint64_t* key, const uint32_t* in, uint32_t* out, unsigned n, unsigned shift, DArr<uint32_t>& hist) {
  if (div_up(n, rs_tile(RS_IPL_SMALL)) <= RS_FUSED_BLOCKS) radix_pass_t<RS_IPL_SMALL>(e, key, in, out, n, shift, true, hist);
  else radix_pass_t<RS_IPL_LARGE>(e, key, in, out, n, shift, div_up(n, rs_tile(RS_IPL_LARGE)) <= RS_FUSED_BLOCKS_LARGE, hist);
}
// sort by the bits of `key` selected by `mask` (bits that vary); ping-pongs between a and b; returns final buffer.  A digit starts at
// the lowest varying bit not sorted yet (bits that never vary in between cost nothing).
uint32_t* radix_sort_masked(cook_engine* e, const uint64_t* key, unsigned long long mask, const uint32_t* cur, uint32_t* a,
                            uint32_t* b, unsigned n, DArr<uint32_t>* hist = nullptr) {
  const uint32_t* in = cur;  // null: the identity (the first pass reads positions instead of a permutation)
  uint32_t* last = const_cast<uint32_t*>(cur);
  while (mask) {
    const unsigned shift = (unsigned)__builtin_ctzll(mask);
    uint32_t* out = (in == a) ? b : a;
    radix_pass(e, key, in, out, n, shift, hist ? *hist : e->hist);
    in = out;
    last = out;
    mask = shift + 8 >= 64 ? 0ull : mask & ~((1ull << (shift + 8)) - 1ull);
  }
  return last;
}

COOK_KERNEL void iota_u32(uint32_t* p, unsigned n) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = i;
}

// =================================================================================================================
// RANK
// =================================================================================================================
void rank_stage(cook_engine* e, const cook_tasks* t, const cook_users* u) {
  if (!t || !u) e->fail(COOK_E_INVALID, "cook_rank_stage: null tasks/users");
  const unsigned N = t->n, U = u->n;
  if (N && (!t->cpus || !t->mem || !t->user || !t->priority || !t->start_ms || !t->task_id || !t->job_id || !t->pending))
    e->fail(COOK_E_INVALID, "cook_rank_stage: a required task array is NULL");
  if (U == 0 && N) e->fail(COOK_E_INVALID, "cook_rank_stage: no users");
  unsigned np = 0;
  std::vector<uint32_t> pend_ord(N ? N : 1);
  for (unsigned i = 0; i < N; ++i) {
    if (t->user[i] >= U) e->fail(COOK_E_INVALID, "cook_rank_stage: user id out of range");
    pend_ord[i] = np;
    np += t->pending[i] ? 1u : 0u;
  }
  // (nothing of the previous table counts from here on: a stage that fails half-way must not leave its usage or its rank behind)
  e->rank_staged = false, e->pool_usage_known = false, e->rank_done = false;
  e->hash_set = 0;  // (cook_cycle_set_job_hashes' column is by pending ordinal: a stage drops it)
  e->N = N;
  e->U = U;
  e->n_pending = np;
  e->has_gpus = t->gpus != nullptr;
  h2d(e, e->t_cpus, t->cpus, N);
  h2d(e, e->t_mem, t->mem, N);
  if (t->gpus) h2d(e, e->t_gpus, t->gpus, N);
  h2d(e, e->t_user, t->user, N);
  h2d(e, e->t_prio, t->priority, N);
  h2d(e, e->t_start, t->start_ms, N);
  h2d(e, e->t_task, t->task_id, N);
  h2d(e, e->t_job, t->job_id, N);
  h2d(e, e->t_pending, t->pending, N);
  e->has_t_host = e->t_host_complete = t->host != nullptr;  // (cook_cycle_rebalance_stage reads it; the rank does not)
  if (t->host) h2d(e, e->t_host, t->host, N);
  h2d(e, e->pend_ord, pend_ord.data(), N);
  h2d(e, e->u_divc, u->div_cpus, U);
  h2d(e, e->u_divm, u->div_mem, U);
  h2d(e, e->u_divg, u->div_gpus, U);
  h2d(e, e->u_qcount, u->quota_count, U);
  h2d(e, e->u_qcpus, u->quota_cpus, U);
  h2d(e, e->u_qmem, u->quota_mem, U);
  h2d(e, e->u_qgpus, u->quota_gpus, U);
  sync(e);  // pend_ord is a host temporary
  e->rank_staged = true;
  e->pool_usage_known = false;
  e->rank_done = false;
}

void rank_pool_usage(cook_engine* e, cook_usage* out) {
  if (!e->rank_staged) e->fail(COOK_E_STATE, "cook_rank_pool_usage before cook_rank_stage");
  // (COOK_POOL_USAGE_MEMO=0: sum it every time — bench.py's timed cycles keep one table resident, a live cycle arrives with a new one)
  static const bool memo = [] { const char* v = std::getenv("COOK_POOL_USAGE_MEMO"); return !(v && v[0] == '0'); }();
  if (e->pool_usage_known && memo) {  // summed for this very table already (cook_rank_stage / cook_cycle_update forget it)
    *out = e->pool_usage_val;
    return;
  }
  e->pool_usage.ensure(1);
  if (e->N == 0) {
    *out = cook_usage{0, 0, 0, 0};
    return;
  }
  e->pool_usage.ensure(1 + POOL_USAGE_BLOCKS);
  e->pool_usage_bound.ensure(POOL_USAGE_BLOCKS);
  KM<pool_usage_partial, 256>(e, "pool_usage_partial", POOL_USAGE_BLOCKS, (const double*)e->t_cpus.ptr(), (const double*)e->t_mem.ptr(),
      e->has_gpus ? (const double*)e->t_gpus.ptr() : (const double*)nullptr, (const uint8_t*)e->t_pending.ptr(), e->N, e->pool_usage.ptr() + 1,
      e->pool_usage_bound.ptr(), (unsigned)POOL_USAGE_BLOCKS);
  KM<pool_usage_reduce, COOK_WAVE>(e, "pool_usage_reduce", 1, (const double*)e->t_cpus.ptr(), (const double*)e->t_mem.ptr(),
      e->has_gpus ? (const double*)e->t_gpus.ptr() : (const double*)nullptr, (const uint8_t*)e->t_pending.ptr(), e->N,
      (const SumU4*)(e->pool_usage.ptr() + 1), (const SumBound4*)e->pool_usage_bound.ptr(), (unsigned)POOL_USAGE_BLOCKS, e->pool_usage.ptr());
  SumU4 h;
  pinned_copy(e, e->h_scratch, e->pool_usage.ptr(), sizeof(SumU4), hipMemcpyDeviceToHost);
  sync(e);
  std::memcpy(&h, e->h_scratch, sizeof(SumU4));
  *out = cook_usage{h.count, h.cpus, h.mem, h.gpus};
  e->pool_usage_val = *out;
  e->pool_usage_known = true;
}

// per-user running usage [U x 3] of the pool, from the per-user order of the last rank run (rank_kernels.hpp)
void rank_user_usage(cook_engine* e, double* out, bool out_is_device) {
  if (!e->rank_done) e->fail(COOK_E_STATE, "cook_rank_user_usage before cook_rank_run");
  if (!out) e->fail(COOK_E_INVALID, "cook_rank_user_usage: null output");
  const unsigned N = e->N, U = e->U;
  if (U == 0) return;
  double* dst = out_is_device ? out : e->uu_out.ensure((size_t)U * 3);
  if (N) {
    SumU4* rp = e->uu_pre.ensure(N);
    uint32_t* bad = e->uu_bad.ensure(U);
    memset_async(e, bad, 0, (size_t)U * 4);
    seg_scan<SumU4>(e, "user_running_scan", LoadRunningU4{e->s_use.ptr(), e->s_pending.ptr()}, (const uint8_t*)e->head.ptr(), N, rp,
                    e->tmpU4);
    KM<rank_mark_inexact, 256>(e, "user_usage_mark", div_up(N, 256), (const SumU4*)rp, (const uint32_t*)e->s_user.ptr(), N, bad);
    KM<user_usage_extract, 256>(e, "user_usage_extract", div_up(U, 256), (const SumU4*)rp, (const SumU4*)e->s_use.ptr(),
        (const uint8_t*)e->s_pending.ptr(), (const uint32_t*)e->seg_start.ptr(), (const uint32_t*)e->seg_end.ptr(), (const uint32_t*)bad, U, dst);
  } else {
    memset_async(e, dst, 0, (size_t)U * 24);
  }
  if (!out_is_device) copy_async(e, out, dst, (size_t)U * 24, hipMemcpyDeviceToHost);
  sync(e);
}

// one quota filter stage over the queue (tools.clj:917-933); returns new queue length
unsigned queue_filter_quota(cook_engine* e, unsigned stage, unsigned len, const cook_usage& quota, const cook_usage& base, uint32_t*& qitem,
                            SumU4*& quse, uint32_t*& qitem_other, SumU4*& quse_other) {
  if (len == 0) return 0;
  e->qpre.ensure(len);
  e->iflag.ensure(len);
  e->scanI.ensure(len);
  LoadQueueUse ld{quse, SumU4{base.count, base.cpus, base.mem, base.gpus, 0u}};
  seg_scan<SumU4>(e, "queue_usage_scan", ld, (const uint8_t*)nullptr, len, e->qpre.ptr(), e->tmpU4);
  // [32 + 2 * stage]: a prefix rounded, [33 + 2 * stage]: the new length.  Stages 0 / 1 are rank_run's (zeroed by rank_init), stage 2 is
  // the considerable filters' (which may run without a rank before them: cleared here)
  unsigned* any_bad = e->d_counters.ptr() + 32 + 2 * stage;
  if (stage >= 2) memset_async(e, any_bad, 0, 8);
  Usage4 q{quota.count, quota.cpus, quota.mem, quota.gpus};
  KM<queue_quota_flag, 256>(e, "queue_quota_flag", div_up(len, 256), (const SumU4*)e->qpre.ptr(), len, q, e->iflag.ptr(), any_bad);
  KM<queue_quota_fix, 64>(e, "queue_quota_fix", 1, (const SumU4*)quse, len, SumU4{base.count, base.cpus, base.mem, base.gpus, 0u}, q,
      (const unsigned*)any_bad, e->iflag.ptr());
  seg_scan<SumI>(e, "queue_compact_scan", LoadI{e->iflag.ptr()}, (const uint8_t*)nullptr, len, e->scanI.ptr(), e->tmpI);
  unsigned* len_out = any_bad + 1;
  KM<queue_compact, 256>(e, "queue_compact", div_up(len, 256), (const uint32_t*)qitem, (const SumU4*)quse, (const int*)e->iflag.ptr(),
      (const SumI*)e->scanI.ptr(), len, qitem_other, quse_other, len_out);
  unsigned h[2];
  pinned_copy(e, e->h_scratch, len_out, 4, hipMemcpyDeviceToHost);
  sync(e);
  std::memcpy(h, e->h_scratch, 4);
  std::swap(qitem, qitem_other);
  std::swap(quse, quse_other);
  return h[0];
}

void rank_run(cook_engine* e) {
  if (!e->rank_staged) e->fail(COOK_E_STATE, "cook_rank_run before cook_rank_stage");
  const auto t_call = std::chrono::steady_clock::now();
  if (g_sync_trace) tl_sync_ms = 0.0, tl_syncs = 0;
  const unsigned N = e->N, U = e->U;
  e->n_ranked = 0;
  e->rank_done = false;
  e->cycle_cons_ran = false;
  e->q_valid = false;  // (the standing queue is rewritten)
  e->q_stepped = false;
  e->ranked.ensure(std::max(1u, e->n_pending));
  if (N == 0) {
    e->rank_done = true;
    return;
  }
  const unsigned gN = div_up(N, 256);
  e->d_scratch64.ensure(64);
  e->d_counters.ensure(64);
  // --- per-user order keys -------------------------------------------------------------------------------
  const bool radix_only = std::getenv("COOK_RANK_RADIX") != nullptr;  // the tie rule as radix passes (the tests run both forms)
  unsigned long long* mins = e->d_scratch64.ptr();      // [0..2]
  unsigned long long* same = e->d_scratch64.ptr() + 4;  // [4..6] bits on which all keys of a word agree
  e->seg_start.ensure(U);
  e->seg_end.ensure(U);
  e->inexact_user.ensure(U);
  TieCtl* tie_ctl0 = e->tie_ctl.ensure(1);
  bool tie_ctl_clean = true;  // until the first refinement has used it
  KM<rank_init, 256>(e, "rank_init", std::max(1u, std::min(div_up(U, 256), 64u)), e->d_scratch64.ptr(), e->d_counters.ptr(), 40u,
      e->inexact_user.ptr(), e->seg_end.ptr(), U, reinterpret_cast<unsigned*>(tie_ctl0), (unsigned)(sizeof(TieCtl) / 4), std::max(1u,
      std::min(div_up(U, 256), 64u)));
  e->w0.ensure(N);
  e->w1.ensure(N);
  e->w2.ensure(N);
  KM<rank_key_mins, 256>(e, "rank_key_mins", std::min(gN, 64u), (const int64_t*)e->t_start.ptr(), (const int64_t*)e->t_task.ptr(),
      (const int64_t*)e->t_job.ptr(), (const uint8_t*)e->t_pending.ptr(), N, mins, std::min(gN, 64u));
  KM<rank_build_keys, 256>(e, "rank_build_keys", gN, (const uint32_t*)e->t_user.ptr(), (const int32_t*)e->t_prio.ptr(),
      (const int64_t*)e->t_start.ptr(), (const int64_t*)e->t_task.ptr(), (const int64_t*)e->t_job.ptr(), (const uint8_t*)e->t_pending.ptr(), N,
      (const unsigned long long*)mins, e->w0.ptr(), e->w1.ptr(), e->w2.ptr(), same);
  readback64(e, 8);
  const unsigned long long mk0 = ~e->h_scratch[4], mk1 = ~e->h_scratch[5], mk2 = ~e->h_scratch[6];
  e->permA.ensure(N);
  e->permB2.ensure(N);
  const uint32_t* cur = nullptr;  // the identity
  cur = radix_sort_masked(e, e->w2.ptr(), mk2, cur, e->permA.ptr(), e->permB2.ptr(), N);
  cur = radix_sort_masked(e, e->w1.ptr(), mk1, cur, e->permA.ptr(), e->permB2.ptr(), N);
  cur = radix_sort_masked(e, e->w0.ptr(), mk0, cur, e->permA.ptr(), e->permB2.ptr(), N);
  if (!cur) {  // every task has the same key words
    KM<iota_u32, 256>(e, "iota", gN, e->permA.ptr(), N);
    cur = e->permA.ptr();
  }
  e->permB = const_cast<uint32_t*>(cur);
  unsigned n_kept = 0;
  unsigned long long vor = 0, vand = 0;
  unsigned* counters = e->d_counters.ptr();  // [0] n_kept [1] equal-run [2] n_tied
  // --- gather, per-user prefix sums ----------------------------------------------------------------------
  e->s_user.ensure(N);
  e->s_use.ensure(N);
  e->s_pending.ensure(N);
  e->head.ensure(N);
  e->seg_start.ensure(U);
  e->seg_end.ensure(U);
  e->pre.ensure(N);
  KM<rank_gather, 256>(e, "rank_gather", gN, (const uint32_t*)e->permB, N, (const uint32_t*)e->t_user.ptr(), (const double*)e->t_cpus.ptr(),
      (const double*)e->t_mem.ptr(), e->has_gpus ? (const double*)e->t_gpus.ptr() : (const double*)nullptr, (const uint8_t*)e->t_pending.ptr(),
      e->s_user.ptr(), e->s_use.ptr(), e->s_pending.ptr(), e->head.ptr(), e->seg_start.ptr(), e->seg_end.ptr());
  seg_scan<SumU4>(e, "user_usage_scan", LoadU4{e->s_use.ptr()}, (const uint8_t*)e->head.ptr(), N, e->pre.ptr(), e->tmpU4);
  KM<rank_mark_inexact, 256>(e, "rank_mark_inexact", gN, (const SumU4*)e->pre.ptr(), (const uint32_t*)e->s_user.ptr(), N, e->inexact_user.ptr());
  KM<rank_fix_inexact, 256>(e, "rank_fix_inexact", div_up(U, 256), (const SumU4*)e->s_use.ptr(), e->pre.ptr(), (const uint32_t*)e->seg_start.ptr(),
      (const uint32_t*)e->seg_end.ptr(), (const uint32_t*)e->inexact_user.ptr(), U);
  // --- limiter + DRU ---------------------------------------------------------------------------------------
  e->iflag.ensure(N);
  e->scanI.ensure(N);
  KM<rank_over_flag, 256>(e, "rank_over_flag", gN, (const SumU4*)e->pre.ptr(), (const uint32_t*)e->s_user.ptr(), N, (const double*)e->u_qcount.ptr(),
      (const double*)e->u_qcpus.ptr(), (const double*)e->u_qmem.ptr(), (const double*)e->u_qgpus.ptr(), e->iflag.ptr());
  seg_scan<SumI>(e, "over_quota_scan", LoadI{e->iflag.ptr()}, (const uint8_t*)e->head.ptr(), N, e->scanI.ptr(), e->tmpI);
  e->dru.ensure(N);
  e->dkey.ensure(N);
  e->keep.ensure(N);
  unsigned long long* orand = reinterpret_cast<unsigned long long*>(counters + 8);  // [0] OR of the kept keys, [1] OR of their complements
  KM<rank_score, 256>(e, "rank_score", gN, (const SumU4*)e->pre.ptr(), (const SumI*)e->scanI.ptr(), (const uint32_t*)e->s_user.ptr(), N,
      (int)e->params.max_over_quota_jobs, (int)e->params.dru_mode, (const double*)e->u_divc.ptr(), (const double*)e->u_divm.ptr(),
      (const double*)e->u_divg.ptr(), e->dru.ptr(), e->dkey.ptr(), e->keep.ptr(), counters, orand);
  pinned_copy(e, e->h_scratch, counters, 12 * 4, hipMemcpyDeviceToHost);  // the counts and, behind them, the two key words
  sync(e);
  vor = e->h_scratch[4], vand = ~e->h_scratch[5];
  unsigned hc[2];
  std::memcpy(hc, e->h_scratch, 8);
  n_kept = hc[0];
  // --- global DRU order -------------------------------------------------------------------------------------
  e->permC1.ensure(N);
  e->permC2.ensure(N);
  uint32_t* pc = nullptr;  // the identity
  if (n_kept) pc = radix_sort_masked(e, e->dkey.ptr(), vor & ~vand, pc, e->permC1.ptr(), e->permC2.ptr(), N);
  if (n_kept < N) {  // limiter dropped tasks: one extra 1-bit pass moves them behind every kept task
    e->nkkey.ensure(N);
    KM<rank_notkept_key, 256>(e, "rank_notkept_key", gN, (const uint8_t*)e->keep.ptr(), N, e->nkkey.ptr());
    pc = radix_sort_masked(e, e->nkkey.ptr(), 1ull, pc, e->permC1.ptr(), e->permC2.ptr(), N);
  }
  if (!pc) {  // all kept keys equal
    KM<iota_u32, 256>(e, "iota", gN, e->permC1.ptr(), N);
    pc = e->permC1.ptr();
  }
  e->permC = pc;
  unsigned qlen = 0;
  uint32_t* qitem = e->qitemA.ensure(std::max(1u, e->n_pending));
  uint32_t* qitem_o = e->qitemB.ensure(std::max(1u, e->n_pending));
  SumU4* quse = e->quseA.ensure(std::max(1u, e->n_pending));
  SumU4* quse_o = e->quseB.ensure(std::max(1u, e->n_pending));
  if (n_kept) {
    const unsigned gK = div_up(n_kept, 256);
    // --- tie groups + sorted-merge tie rule (prefix doubling) ------------------------------------------------
    unsigned bits = 1;
    while ((1ull << bits) <= (unsigned long long)U + N) ++bits;  // rank values <= U + N
    // composite key of a tied item = (start of its group, secondary rank), the two packed back to back: 2 * bits key bits, 36 for a
    // pool's 175k tasks = 5 radix passes (two 32-bit halves cost a pass more)
    const unsigned long long cmask = 2 * bits >= 64 ? ~0ull : (1ull << (2 * bits)) - 1ull;
    // refines `perm` (nk items of an index space with n_items items, per-user lists contiguous) in place; returns false when a
    // user has consecutive items with equal keys (the caller collapses those runs and calls again on the collapsed space)
    auto tie_refine_radix = [&](uint32_t* perm, const uint64_t* key, const uint32_t* user_of, const uint32_t* seg_first, unsigned nk,
                                unsigned n_items) -> bool {
      const unsigned gK = div_up(nk, 256);
      e->thead.ensure(nk);
      e->rank_of_item.ensure(n_items);
      e->gstart.ensure(nk);
      int* ones = e->ones_buf.ensure(nk);
      int* tied = e->tied_buf.ensure(nk);
      e->scanI.ensure(nk);
      memset_async(e, counters + 1, 0, 4);
      KM<tie_heads, 256>(e, "tie_heads", gK, (const uint32_t*)perm, key, nk, user_of, e->thead.ptr(), (uint8_t*)nullptr, ones, counters + 1);
      for (int round = 0;; ++round) {
        seg_scan<SumI>(e, "tie_group_scan", LoadI{ones}, (const uint8_t*)e->thead.ptr(), nk, e->scanI.ptr(), e->tmpI);
        memset_async(e, counters + 2, 0, 4);
        KM<tie_assign, 256>(e, "tie_assign", gK, (const uint32_t*)perm, (const uint8_t*)e->thead.ptr(), (const SumI*)e->scanI.ptr(), nk, U,
            e->rank_of_item.ptr(), e->gstart.ptr(), tied, counters + 2);
        unsigned h3[3];
        readback_counters(e, h3, 3);
        if (h3[1]) return false;
        const unsigned n_tied = h3[2];
        if (std::getenv("COOK_TIE_TRACE")) std::fprintf(stderr, "tie round %d: %u tied of %u\n", round, n_tied, nk);
        if (n_tied == 0) break;
        if (round > 31) e->fail(COOK_E_INVALID, "cook_rank: tie refinement did not converge");
        // compact tied slots, sort them by (group start, secondary), write back, split groups
        e->tpos.ensure(n_tied);
        e->titem.ensure(n_tied);
        e->ckey.ensure(n_tied);
        e->tsorted.ensure(n_tied);
        e->tsorted2.ensure(n_tied);
        seg_scan<SumI>(e, "tie_compact_scan", LoadI{tied}, (const uint8_t*)nullptr, nk, e->scanI.ptr(), e->tmpI);
        KM<tie_build, 256>(e, "tie_build", gK, (const uint32_t*)perm, (const int*)tied, (const SumI*)e->scanI.ptr(),
            (const uint32_t*)e->gstart.ptr(), nk, U, n_items, round, bits, (const uint32_t*)e->rank_of_item.ptr(), user_of, seg_first, e->tpos.ptr(),
            e->titem.ptr(), e->ckey.ptr());
        KM<iota_u32, 256>(e, "iota", div_up(n_tied, 256), e->tsorted.ptr(), n_tied);
        uint32_t* ts = radix_sort_masked(e, e->ckey.ptr(), cmask, e->tsorted.ptr(), e->tsorted.ptr(), e->tsorted2.ptr(), n_tied);
        KM<tie_writeback, 256>(e, "tie_writeback", div_up(n_tied, 256), (const uint32_t*)ts, (const uint32_t*)e->tpos.ptr(),
            (const uint32_t*)e->titem.ptr(), (const uint64_t*)e->ckey.ptr(), n_tied, perm, e->thead.ptr());
      }
      return true;
    };
    // the same refinement with the groups sorted in LDS tiles (tile_sort.hpp): two launches per doubling round, four rounds enqueued
    // per look at the counters (rounds past the last one exit at once); a tie group too long for a tile sends the call to the radix form,
    // which starts over from the keys (the order inside a group of equal keys is free when the refinement starts)
    auto tie_refine = [&](uint32_t* perm, const uint64_t* key, const uint32_t* user_of, const uint32_t* seg_first, unsigned nk,
                          unsigned n_items) -> bool {
      if (radix_only) return tie_refine_radix(perm, key, user_of, seg_first, nk, n_items);
      const unsigned gK = div_up(nk, 256);
      e->thead.ensure(nk);
      e->dhead.ensure(nk);
      e->rank_of_item.ensure(n_items);
      TieCtl* ctl = tie_ctl0;
      if (!tie_ctl_clean) memset_async(e, ctl, 0, sizeof(TieCtl));  // (rank_init cleared it for the first refinement)
      tie_ctl_clean = false;
      KM<tie_heads, 256>(e, "tie_heads", gK, (const uint32_t*)perm, key, nk, user_of, e->thead.ptr(), e->dhead.ptr(), (int*)nullptr, &ctl->equal_runs);
      constexpr int LOOK = 4;
      for (int r0 = 0; r0 < 32; r0 += LOOK) {
        for (int round = r0; round < r0 + LOOK; ++round) {
          KM<tie_rank_assign, 256>(e, "tie_rank_assign", gK, (const uint32_t*)perm, (const uint8_t*)e->thead.ptr(), nk, U, round, (const TieCtl*)ctl,
              e->rank_of_item.ptr());
          KM<tie_sort_tiles, TS_THREADS>(e, "tie_sort_tiles", div_up(nk, TS_NOMINAL), perm, e->thead.ptr(), (const uint8_t*)e->dhead.ptr(), nk, U,
              n_items, round, (const uint32_t*)e->rank_of_item.ptr(), user_of, seg_first, ctl);
        }
        TieCtl h;
        pinned_copy(e, e->h_scratch, ctl, sizeof(TieCtl), hipMemcpyDeviceToHost);
        sync(e);
        std::memcpy(&h, e->h_scratch, sizeof(TieCtl));
        if (std::getenv("COOK_TIE_TRACE"))
          for (int round = r0; round < r0 + LOOK; ++round) std::fprintf(stderr, "tie round %d: %u tied after, of %u\n", round, h.tied_after[round], nk);
        if (h.equal_runs) return false;
        if (h.overflow) return tie_refine_radix(perm, key, user_of, seg_first, nk, n_items);
        if (h.tied_after[r0 + LOOK - 1] == 0) return true;
      }
      e->fail(COOK_E_INVALID, "cook_rank: tie refinement did not converge");
      return false;
    };
    if (!tie_refine(e->permC, e->dkey.ptr(), e->s_user.ptr(), e->seg_start.ptr(), n_kept, N)) {
      // some user has a run of equal DRUs (a zero-resource task, a gpu-less task in gpu mode, a request absorbed by the sum): the
      // merge emits such a run back to back (rank_kernels.hpp, run_*), so collapse the runs, refine the heads, re-insert the rest
      int* isf = e->run_isf.ensure(N);
      int* nonf = e->run_nonf.ensure(N);
      SumI* nonf_incl = e->run_scan.ensure(N);
      KM<run_follower_flag, 256>(e, "run_follower_flag", gN, (const uint32_t*)e->s_user.ptr(), (const uint64_t*)e->dkey.ptr(),
          (const uint8_t*)e->keep.ptr(), N, isf, nonf);
      seg_scan<SumI>(e, "run_scan", LoadI{nonf}, (const uint8_t*)nullptr, N, nonf_incl, e->tmpI);
      pinned_copy(e, e->h_scratch, &nonf_incl[N - 1], 4, hipMemcpyDeviceToHost);
      sync(e);
      int n2i = 0;
      std::memcpy(&n2i, e->h_scratch, 4);
      const unsigned N2 = (unsigned)n2i, n_kept2 = n_kept - (N - N2);  // followers are kept items
      uint32_t* c_user = e->run_user.ensure(N2);
      uint64_t* c_dkey = e->run_dkey.ensure(N2);
      uint32_t* c_orig = e->run_orig.ensure(N2 + 1);
      uint32_t* c_seg = e->run_seg.ensure(U);
      uint32_t* b_to_c = e->run_b2c.ensure(N);
      KM<run_compact_items, 256>(e, "run_compact_items", gN, (const int*)nonf, (const SumI*)nonf_incl, N, (const uint32_t*)e->s_user.ptr(),
          (const uint64_t*)e->dkey.ptr(), (const uint8_t*)e->head.ptr(), c_user, c_dkey, c_orig, c_seg, b_to_c);
      KM<run_compact_sentinel, 1>(e, "run_compact_sentinel", 1, (const SumI*)nonf_incl, N, c_orig);
      int* posf = e->run_posf.ensure(n_kept);
      SumI* posf_incl = e->run_scan2.ensure(n_kept);
      KM<run_flag_positions, 256>(e, "run_flag_positions", gK, (const uint32_t*)e->permC, (const int*)isf, n_kept, posf);
      seg_scan<SumI>(e, "run_scan", LoadI{posf}, (const uint8_t*)nullptr, n_kept, posf_incl, e->tmpI);
      uint32_t* perm2 = e->run_perm.ensure(n_kept2);
      KM<run_compact_positions, 256>(e, "run_compact_positions", gK, (const uint32_t*)e->permC, (const int*)posf, (const SumI*)posf_incl, n_kept,
          (const uint32_t*)b_to_c, perm2);
      if (!tie_refine(perm2, c_dkey, c_user, c_seg, n_kept2, N2)) e->fail(COOK_E_STATE, "cook_rank: equal-DRU runs survived the collapse");
      const unsigned gK2 = div_up(n_kept2, 256);
      KM<run_count_followers, 256>(e, "run_count_followers", gK2, (const uint32_t*)perm2, (const uint32_t*)c_orig, n_kept2, posf);
      seg_scan<SumI>(e, "run_scan", LoadI{posf}, (const uint8_t*)nullptr, n_kept2, posf_incl, e->tmpI);
      KM<run_expand, 256>(e, "run_expand", gK2, (const uint32_t*)perm2, (const uint32_t*)c_orig, (const int*)posf, (const SumI*)posf_incl, n_kept2, e->permC);
    }
    // --- queue of pending jobs in rank order ---------------------------------------------------------------
    int* flag = e->iflag.ptr();
    KM<queue_flag_pending, 256>(e, "queue_flag_pending", gK, (const uint32_t*)e->permC, (const uint8_t*)e->s_pending.ptr(), n_kept, flag);
    seg_scan<SumI>(e, "queue_pending_scan", LoadI{flag}, (const uint8_t*)nullptr, n_kept, e->scanI.ptr(), e->tmpI);
    unsigned* dq = e->d_counters.ptr() + 38;  // (zeroed by rank_init)
    KM<queue_compact_pending, 256>(e, "queue_compact_pending", gK, (const uint32_t*)e->permC, (const int*)flag, (const SumI*)e->scanI.ptr(), n_kept,
        (const SumU4*)e->s_use.ptr(), qitem, quse, dq);
    pinned_copy(e, e->h_scratch, dq, 4, hipMemcpyDeviceToHost);
    sync(e);
    std::memcpy(&qlen, e->h_scratch, 4);
  }
  // --- quota filters (scheduler.clj:2134-2157) -------------------------------------------------------------
  if (qlen && e->quota.has_pool_quota) {
    cook_usage base = e->quota.pool_usage;
    if (!e->quota.pool_usage_given) rank_pool_usage(e, &base);
    qlen = queue_filter_quota(e, 0, qlen, e->quota.pool_quota, base, qitem, quse, qitem_o, quse_o);
  }
  if (qlen && e->quota.has_group_quota)
    qlen = queue_filter_quota(e, 1, qlen, e->quota.group_quota, e->quota.group_usage, qitem, quse, qitem_o, quse_o);
  // --- offensive filter (scheduler.clj:2198-2229) -----------------------------------------------------------
  const bool offensive_on = std::isfinite(e->params.offensive_max_mem_mb) || std::isfinite(e->params.offensive_max_cpus);
  if (qlen && offensive_on) {
    e->iflag.ensure(qlen);
    e->scanI.ensure(qlen);
    KM<queue_offensive_flag, 256>(e, "queue_offensive_flag", div_up(qlen, 256), (const SumU4*)quse, qlen, e->params.offensive_max_mem_mb,
        e->params.offensive_max_cpus, e->iflag.ptr());
    seg_scan<SumI>(e, "queue_compact_scan", LoadI{e->iflag.ptr()}, (const uint8_t*)nullptr, qlen, e->scanI.ptr(), e->tmpI);
    unsigned* len_out = e->d_counters.ptr() + 9;
    KM<queue_compact, 256>(e, "queue_compact", div_up(qlen, 256), (const uint32_t*)qitem, (const SumU4*)quse, (const int*)e->iflag.ptr(),
        (const SumI*)e->scanI.ptr(), qlen, qitem_o, quse_o, len_out);
    pinned_copy(e, e->h_scratch, len_out, 4, hipMemcpyDeviceToHost);
    sync(e);
    std::memcpy(&qlen, e->h_scratch, 4);
    std::swap(qitem, qitem_o);
    std::swap(quse, quse_o);
  }
  if (qlen)
    KM<queue_emit, 256>(e, "queue_emit", div_up(qlen, 256), (const uint32_t*)qitem, qlen, (const uint32_t*)e->permB, e->ranked.ptr());
  e->n_ranked = qlen;
  e->rank_done = true;
  if (g_sync_trace) {
    std::fprintf(stderr, "cook_rank_run: %u stream synchronisations, %.3f ms waiting in them, %.3f ms in the call\n", tl_syncs, tl_sync_ms,
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count());
    tl_sync_ms = 0.0, tl_syncs = 0;
  }
}

void rank_fetch(cook_engine* e, uint32_t* ranked, uint32_t* n_out, double* dru_of_task) {
  if (!e->rank_done) e->fail(COOK_E_STATE, "cook_rank_fetch before cook_rank_run");
  if (n_out) *n_out = e->n_ranked;
  if (ranked && e->n_ranked)
    copy_async(e, ranked, e->ranked.ptr(), (size_t)e->n_ranked * 4, hipMemcpyDeviceToHost);
  if (dru_of_task && e->N) {
    e->dru_out.ensure(e->N);
    KM<dru_to_task_space, 256>(e, "dru_to_task_space", div_up(e->N, 256), (const double*)e->dru.ptr(), (const uint8_t*)e->keep.ptr(),
        (const uint32_t*)e->permB, e->N, e->dru_out.ptr());
    copy_async(e, dru_of_task, e->dru_out.ptr(), (size_t)e->N * 8, hipMemcpyDeviceToHost);
  }
  sync(e);
}
