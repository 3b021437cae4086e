// rebal_resident_host.hpp — host orchestration of cook_cycle_rebalance_stage / cook_cycle_rebalance_fetch (cookmatch.h): the
// rebalancer's stage from the pool's resident cycle state.  Included by engine.hip inside its anonymous namespace, behind rebalance_host.hpp
// (RebalBufs, rebal_stage_host_tables, rebal_stage_attr_table), considerable_host.hpp (the eligible mask) and cycle_update.hpp.
// It leaves RebalBufs as cook_rebalance_stage would for the derived inputs of the header; rebalance_run and the rebal_* kernels are not
// touched.  Two parts, two stream synchronisations:
//   1. everything sized by bounds the host knows (N rows, min(max_preemption, queue length) jobs): the running rows to their slots, the
//      cut of the queue, the selected jobs, users and groups device to device, the greatest host id; then ONE read-back: R, P, H, the
//      CSR value counts, the longest cotask list, the range checks.
//   2. the tables H sizes: attribute row and spare resources per host from the offer rows (or from the caller's lists, uploaded as
//      cook_rebalance_stage does: H rows), running rows per host; then the other read-back: max_seg, spare_safe.
// No host loop over R or S, no upload that grows with R.
#pragma once
#include "rebal_resident_kernels.hpp"

struct ResidentRebalBufs {
  DArr<SumI> incl, qincl, eq_incl, nv_incl;
  DArr<uint8_t> matched, skipped;
  DArr<uint32_t> sel_task, sel_ord, run_row, out_pre;
  DArr<unsigned> host_cnt;
  DArr<RrCtl> ctl;
};

template <class T>
static void rr_d2d(cook_engine* e, DArr<T>& d, const T* src, size_t n) {
  d.ensure(n);
  copy_async(e, d.ptr(), src, n * sizeof(T), hipMemcpyDeviceToDevice);
}
static RrCtl rr_read_ctl(cook_engine* e, const RrCtl* ctl) {
  static_assert(sizeof(RrCtl) <= 64 * 8, "RrCtl is read back through h_scratch");
  pinned_copy(e, e->h_scratch, ctl, sizeof(RrCtl), hipMemcpyDeviceToHost);
  sync(e);
  RrCtl h;
  std::memcpy(&h, e->h_scratch, sizeof(h));
  return h;
}

// the staged offer rows as the attribute table (host_attrs == NULL)
static void rr_attrs_from_offers(cook_engine* e, RebalBufs& b) {
  const MatchIn& in = e->min;
  const unsigned M = e->M;
  b.has_attrs = M > 0;
  b.ha_k8s = b.ha_gpu = b.ha_disk = b.ha_attr = b.ha_loc = b.ha_start = false;
  b.n_attr = 0;
  if (!M) return;
  rr_d2d(e, b.a_host, in.o_host, M);
  if ((b.ha_k8s = in.o_k8s != nullptr)) rr_d2d(e, b.a_k8s, in.o_k8s, M);
  if ((b.ha_gpu = in.o_gpu_model != nullptr)) {
    b.a_gpu_slots = in.gpu_slots;
    rr_d2d(e, b.a_gpu_model, in.o_gpu_model, (size_t)M * in.gpu_slots);
    rr_d2d(e, b.a_gpu_count, in.o_gpu_count, (size_t)M * in.gpu_slots);
  }
  if ((b.ha_disk = in.o_disk_type != nullptr && in.o_disk_space != nullptr)) {
    b.a_disk_slots = in.disk_slots;
    rr_d2d(e, b.a_disk_type, in.o_disk_type, (size_t)M * in.disk_slots);
    rr_d2d(e, b.a_disk_space, in.o_disk_space, (size_t)M * in.disk_slots);
  }
  if ((b.ha_attr = in.o_attr != nullptr && in.n_attr > 0)) {
    b.n_attr = in.n_attr;
    rr_d2d(e, b.a_attr, in.o_attr, (size_t)M * in.n_attr);
  }
  if ((b.ha_loc = in.o_location != nullptr)) rr_d2d(e, b.a_location, in.o_location, M);
  if ((b.ha_start = in.o_host_start != nullptr)) rr_d2d(e, b.a_host_start, in.o_host_start, M);
}

void rebal_resident_stage(cook_engine* e, const cook_cycle_rebalance* req) {
  const char* who = "cook_cycle_rebalance_stage";
  if (!req) e->fail(COOK_E_INVALID, std::string(who) + ": null request");
  // ---- everything that can refuse, before anything changes -----------------------------------------------------------------------------
  if (!e->cycle_staged) e->fail(COOK_E_STATE, std::string(who) + " before cook_cycle_stage");
  if (!e->rank_done) e->fail(COOK_E_STATE, std::string(who) + " before a rank (or after a stage / cook_cycle_update no rank has followed)");
  if (e->q_stepped)
    e->fail(COOK_E_STATE, std::string(who) + " after a queue cycle: the task table no longer lists what runs (cook_cycle_update and a rank cycle first)");
  if (!e->has_t_host) e->fail(COOK_E_STATE, std::string(who) + ": the staged tasks carry no host column (cook_cycle_stage with cook_tasks.host)");
  if (!e->t_host_complete)
    e->fail(COOK_E_STATE, std::string(who) + ": a cook_cycle_update added running rows without host (restage with cook_cycle_stage and cook_tasks.host)");
  if (e->placement.state == cook_engine::Placement::ROUNDS || e->placement.state == cook_engine::Placement::WALK)
    e->fail(COOK_E_STATE, std::string(who) + " while a placement is set up and has not run (cook_cycle_match_multi first)");
  if (req->skip_matched > 1u || req->reserved != 0u) e->fail(COOK_E_INVALID, std::string(who) + ": skip_matched is 0 or 1, reserved is 0");
  if (req->offer_skipped && !req->skip_matched) e->fail(COOK_E_INVALID, std::string(who) + ": offer_skipped without skip_matched");
  const cook_host_spare* spare = req->spare;
  const cook_offers* attrs = req->host_attrs;
  const MatchIn& in = e->min;
  if ((!spare || !attrs) && in.host_dup)
    e->fail(COOK_E_INVALID, std::string(who) + ": two staged offers share a host: pass spare and host_attrs");
  if (spare && spare->n && (!spare->host || !spare->cpus || !spare->mem)) e->fail(COOK_E_INVALID, std::string(who) + ": spare needs host, cpus and mem");
  if (attrs && attrs->n && !attrs->host) e->fail(COOK_E_INVALID, std::string(who) + ": host_attrs needs host");
  if (attrs && attrs->gpu_model && !attrs->gpu_count) e->fail(COOK_E_INVALID, "cook_rebalance: host_attrs gpu_model without gpu_count");
  if (attrs && (attrs->gpu_slots > COOK_MAX_RES_SLOTS || attrs->disk_slots > COOK_MAX_RES_SLOTS))
    e->fail(COOK_E_INVALID, "cook_rebalance: host_attrs slots > COOK_MAX_RES_SLOTS");
  unsigned maxh1 = 0;  // greatest host id + 1 of the caller's lists (H rows)
  if (spare)
    for (unsigned i = 0; i < spare->n; ++i) maxh1 = std::max(maxh1, spare->host[i] + 1u);
  if (attrs)
    for (unsigned i = 0; i < attrs->n; ++i) maxh1 = std::max(maxh1, attrs->host[i] + 1u);

  RebalBufs& b = bufs(e->rb);
  ResidentRebalBufs& r = bufs(e->rrb);
  const unsigned N = e->N, U = e->U, G = e->G, M = e->M, nq = e->n_ranked;
  const unsigned cap = req->params.max_preemption > 0 ? std::min<unsigned>((unsigned)req->params.max_preemption, nq) : 0u;
  b.staged = b.done = b.resident = false;
  b.rp = req->params;
  b.U = U, b.G = G;
  b.has_cached = false;
  RrCtl* ctl = r.ctl.ensure(1);
  memset_async(e, ctl, 0, sizeof(RrCtl));
  // ---- the running rows -> slots [0, R): one scan over the pending flags, one gather ------------------------------------------------------
  const size_t S_hi = (size_t)N + cap;
  b.cpus.ensure(S_hi), b.mem.ensure(S_hi), b.gpus.ensure(S_hi), b.user.ensure(S_hi), b.prio.ensure(S_hi), b.start.ensure(S_hi);
  b.task.ensure(S_hi), b.job.ensure(S_hi), b.pending.ensure(S_hi), b.host.ensure(N);
  if (N) {
    SumI* incl = r.incl.ensure(N);
    seg_scan<SumI>(e, "rr_running_scan", LoadRunningFlag{e->t_pending.ptr()}, (const uint8_t*)nullptr, N, incl, e->tmpI);
    RrColSet cs{};
    auto col = [&](const void* src, void* dst, unsigned esize) { cs.c[cs.n_cols++] = RrCol{src, dst, esize, 0u}; };
    col(e->t_cpus.ptr(), b.cpus.ptr(), 8), col(e->t_mem.ptr(), b.mem.ptr(), 8);
    col(e->has_gpus ? e->t_gpus.ptr() : nullptr, b.gpus.ptr(), 8);
    col(e->t_user.ptr(), b.user.ptr(), 4), col(e->t_prio.ptr(), b.prio.ptr(), 4), col(e->t_start.ptr(), b.start.ptr(), 8);
    col(e->t_task.ptr(), b.task.ptr(), 8), col(e->t_job.ptr(), b.job.ptr(), 8);
    KL("rr_gather_running", rr_gather_running, div_up(N, 256), 256, cs, (const uint8_t*)e->t_pending.ptr(), (const SumI*)incl,
       (const uint32_t*)e->t_host.ptr(), N, b.host.ptr(), r.run_row.ensure(N), b.pending.ptr(), ctl);
  }
  // ---- the queue -> the selected jobs: a scan over a mask and a cut, then one gather ----------------------------------------------------
  r.sel_task.ensure(cap), r.sel_ord.ensure(cap);
  b.j_cpus.ensure(cap), b.j_mem.ensure(cap), b.j_user.ensure(cap);
  if (cap) {
    const uint8_t* elig = (e->cb && e->cb->cycle_on && e->cb->has_elig_by_pending) ? (const uint8_t*)e->cb->elig_by_pending.ptr() : nullptr;
    const uint8_t* matched = nullptr;
    const unsigned k = e->cycle_considered;
    if (req->skip_matched && e->q_valid && e->match_ran() && k) {  // (no placement since the rank: nothing is matched)
      uint8_t* m = r.matched.ensure(nq);
      memset_async(e, m, 0, nq);
      const uint8_t* skipped = (req->offer_skipped && M) ? h2d_opt(e, r.skipped, req->offer_skipped, M) : nullptr;
      KM<rr_mark_matched, 256>(e, "rr_mark_matched", div_up(k, 256), e->q_last_pos, (const int32_t*)e->m_j2o.ptr(), k, nq, skipped, m);
      matched = m;
    }
    const uint32_t *ranked = e->ranked.ptr(), *pend_ord = e->pend_ord.ptr();
    SumI* qincl = r.qincl.ensure(nq);
    seg_scan<SumI>(e, "rr_queue_scan", LoadQueueKeep{ranked, pend_ord, elig, matched}, (const uint8_t*)nullptr, nq, qincl, e->tmpI);
    KM<rr_select, 256>(e, "rr_select", div_up(nq, 256), ranked, pend_ord, elig, matched, (const SumI*)qincl, nq, cap, r.sel_task.ptr(), r.sel_ord.ptr(), ctl);
    RrJobsArgs a{};
    auto jcol = [&](const void* src, void* dst, unsigned esize) { a.js.c[a.js.n_cols++] = RrCol{src, dst, esize, 0u}; };
    jcol(in.j_cpus, b.j_cpus.ptr(), 8), jcol(in.j_mem, b.j_mem.ptr(), 8);
    if (in.j_gpus) jcol(in.j_gpus, b.j_gpus.ensure(cap), 8);
    if (in.j_gpu_model) jcol(in.j_gpu_model, b.j_gpu_model.ensure(cap), 4);
    if (in.j_group && G) jcol(in.j_group, b.j_group.ensure(cap), 4);
    if (in.j_ckpt) jcol(in.j_ckpt, b.j_ckpt.ensure(cap), 4);
    if (in.j_est_end) jcol(in.j_est_end, b.j_est_end.ensure(cap), 8);
    if (in.j_disk_req && in.j_disk_type) jcol(in.j_disk_req, b.j_disk_req.ensure(cap), 8), jcol(in.j_disk_type, b.j_disk_type.ensure(cap), 4);
    a.sel_task = r.sel_task.ptr(), a.sel_ord = r.sel_ord.ptr(), a.ctl = ctl;
    a.t_user = e->t_user.ptr(), a.t_prio = e->t_prio.ptr(), a.t_job = e->t_job.ptr();
    a.j_cpus = in.j_cpus, a.j_mem = in.j_mem, a.j_gpus = in.j_gpus;
    a.j_user = e->has_j_user ? (const uint32_t*)e->j_user.ptr() : nullptr, a.j_group = G ? in.j_group : nullptr;
    a.U = U, a.G = G;
    a.s_cpus = b.cpus.ptr(), a.s_mem = b.mem.ptr(), a.s_gpus = b.gpus.ptr(), a.s_user = b.user.ptr(), a.s_prio = b.prio.ptr();
    a.s_start = b.start.ptr(), a.s_task = b.task.ptr(), a.s_job = b.job.ptr(), a.s_pending = b.pending.ptr(), a.o_user = b.j_user.ptr();
    if (in.j_eq_off) {  // (the values are bounded by what the resident column can hold)
      const size_t vals = std::max<size_t>(1, e->j_eq_key.b.cap / 4);
      a.eq_off = in.j_eq_off, a.eq_key = in.j_eq_key, a.eq_val = in.j_eq_val;
      a.o_eq_off = b.j_eq_off.ensure((size_t)cap + 1), a.o_eq_key = b.j_eq_key.ensure(vals), a.o_eq_val = b.j_eq_val.ensure(vals);
      SumI* li = r.eq_incl.ensure(cap);
      seg_scan<SumI>(e, "rr_csr_scan", LoadSelCsrLen{in.j_eq_off, r.sel_ord.ptr(), ctl}, (const uint8_t*)nullptr, cap, li, e->tmpI);
      a.eq_incl = li;
    }
    if (in.j_novel_off) {
      const size_t vals = std::max<size_t>(1, e->j_novel_host.b.cap / 4);
      a.nv_off = in.j_novel_off, a.nv_host = in.j_novel_host;
      a.o_nv_off = b.j_novel_off.ensure((size_t)cap + 1), a.o_nv_host = b.j_novel_host.ensure(vals);
      SumI* li = r.nv_incl.ensure(cap);
      seg_scan<SumI>(e, "rr_csr_scan", LoadSelCsrLen{in.j_novel_off, r.sel_ord.ptr(), ctl}, (const uint8_t*)nullptr, cap, li, e->tmpI);
      a.nv_incl = li;
    }
    KL("rr_gather_jobs", rr_gather_jobs, div_up(cap, 256), 256, a, cap);
  }
  // ---- users and groups, device to device; the greatest host id -----------------------------------------------------------------------
  rr_d2d(e, b.divc, (const double*)e->u_divc.ptr(), U), rr_d2d(e, b.divm, (const double*)e->u_divm.ptr(), U);
  rr_d2d(e, b.divg, (const double*)e->u_divg.ptr(), U), rr_d2d(e, b.qcount, (const double*)e->u_qcount.ptr(), U);
  rr_d2d(e, b.qcpus, (const double*)e->u_qcpus.ptr(), U), rr_d2d(e, b.qmem, (const double*)e->u_qmem.ptr(), U);
  rr_d2d(e, b.qgpus, (const double*)e->u_qgpus.ptr(), U);
  b.hg_run = false;
  if (G) {
    rr_d2d(e, b.g_type, in.g_type, G), rr_d2d(e, b.g_attr_key, in.g_attr_key, G), rr_d2d(e, b.g_min, in.g_min, G);
    if ((b.hg_run = in.g_run_off != nullptr)) {
      const unsigned total = e->cf_group_run_total;
      rr_d2d(e, b.g_run_off, in.g_run_off, (size_t)G + 1);
      rr_d2d(e, b.g_run_host, in.g_run_host, std::max(1u, total));
      if (total) KM<rr_max_host, 256>(e, "rr_max_host", div_up(total, 256), in.g_run_host, total, ctl);
      KM<rr_max_run, 256>(e, "rr_max_run", div_up(G, 256), in.g_run_off, G, ctl);
    }
  }
  const bool from_offers = (!spare || !attrs) && M;
  if (from_offers) KM<rr_max_host, 256>(e, "rr_max_host", div_up(M, 256), in.o_host, M, ctl);
  const RrCtl h1 = rr_read_ctl(e, ctl);  // ---- the first look at the device: H sizes what follows ------------------------------------
  if (h1.bad & RR_BAD_USER) e->fail(COOK_E_INVALID, "cook_rebalance: user id out of range");
  if (h1.bad & RR_BAD_GROUP) e->fail(COOK_E_INVALID, "cook_rebalance: group id out of range");
  const unsigned R = h1.R, P = h1.P, S = R + P, H = std::max(maxh1, h1.maxh1);
  b.R = R, b.P = P, b.S = S, b.H = H;
  b.co_cap = S + h1.max_run + 1;
  b.hj_gpus = in.j_gpus != nullptr, b.hj_gpu_model = in.j_gpu_model != nullptr, b.hj_group = in.j_group != nullptr && G > 0;
  b.hj_eq = in.j_eq_off != nullptr && P > 0, b.hj_novel = in.j_novel_off != nullptr && P > 0;
  b.hj_ckpt = in.j_ckpt != nullptr, b.hj_est = in.j_est_end != nullptr, b.hj_disk = in.j_disk_req != nullptr && in.j_disk_type != nullptr;
  // ---- the tables H sizes ----------------------------------------------------------------------------------------------------------------
  RebalHostTmp tmp;
  rebal_stage_host_tables(e, b, H, spare, attrs, tmp);  // (the caller's lists; the parts that come from the offers stay empty here)
  if (attrs) rebal_stage_attr_table(e, b, attrs);
  else rr_attrs_from_offers(e, b);
  if (from_offers && H)
    KM<rr_scatter_offers, 256>(e, "rr_scatter_offers", div_up(M, 256), in.o_host, in.o_cpus, in.o_mem, in.o_gpu_count, in.gpu_slots, M, H,
        attrs ? 0u : 1u, spare ? 0u : 1u, b.row_of_host.ptr(), b.spare0_c.ptr(), b.spare0_m.ptr(), b.spare0_g.ptr(), b.has_spare0.ptr(), ctl);
  if (R && H) {  // running rows on the fullest host: decides whether rebal_decide_big is ever needed
    unsigned* cnt = r.host_cnt.ensure(H);
    memset_async(e, cnt, 0, (size_t)H * 4);
    KM<rr_host_count, 256>(e, "rr_host_count", div_up(R, 256), (const uint32_t*)b.host.ptr(), R, H, cnt);
    KM<rr_host_fullest, 256>(e, "rr_host_fullest", div_up(H, 256), (const unsigned*)cnt, H, ctl);
  }
  const RrCtl h2 = rr_read_ctl(e, ctl);  // ---- the second: max_seg, spare_safe (and the host temporaries above are free) ------------------
  b.max_seg = h2.max_seg;
  if (h2.spare_unsafe) b.spare_safe = false;
  b.staged = b.resident = true;
}

void rebal_resident_fetch(cook_engine* e, cook_preemption* decisions, uint32_t* n_decisions, uint32_t* preempted_task_idx, uint32_t* n_preempted,
                          double* pending_dru, uint32_t* selected_task_idx, uint32_t* selected_pending_ord, uint32_t* n_selected) {
  if (!e->rb || !e->rrb || !e->rb->resident) e->fail(COOK_E_STATE, "cook_cycle_rebalance_fetch: the last stage was not cook_cycle_rebalance_stage");
  RebalBufs& b = *e->rb;
  ResidentRebalBufs& r = *e->rrb;
  if (!b.done) e->fail(COOK_E_STATE, "cook_cycle_rebalance_fetch before cook_rebalance_run");
  const unsigned nd = b.last.nd, np = b.last.np, P = b.P;
  if (n_decisions) *n_decisions = nd;
  if (n_preempted) *n_preempted = np;
  if (n_selected) *n_selected = P;
  if (decisions && nd) copy_async(e, decisions, b.decisions.ptr(), (size_t)nd * sizeof(cook_preemption), hipMemcpyDeviceToHost);
  if (preempted_task_idx && np) {
    uint32_t* out = r.out_pre.ensure(np);
    KM<rr_translate, 256>(e, "rr_translate", div_up(np, 256), (const uint32_t*)b.preempted.ptr(), np, (const uint32_t*)r.run_row.ptr(), b.R, out);
    copy_async(e, preempted_task_idx, out, (size_t)np * 4, hipMemcpyDeviceToHost);
  }
  if (pending_dru && P) copy_async(e, pending_dru, b.pending_dru.ptr(), (size_t)P * 8, hipMemcpyDeviceToHost);
  if (selected_task_idx && P) copy_async(e, selected_task_idx, r.sel_task.ptr(), (size_t)P * 4, hipMemcpyDeviceToHost);
  if (selected_pending_ord && P) copy_async(e, selected_pending_ord, r.sel_ord.ptr(), (size_t)P * 4, hipMemcpyDeviceToHost);
  sync(e);
}
