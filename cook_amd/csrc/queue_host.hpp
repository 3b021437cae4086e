// queue_host.hpp — host orchestration of the queue cycles' advance (included by engine.hip inside its anonymous namespace).
// The standing queue is e->ranked[0 .. e->n_ranked): a rank writes it, a queue cycle removes the last cycle's jobs from it in place.
// The advance enqueues everything over the OLD queue length (mark, scan, compact, the group fold, then the uploads of the step's offers
// and groups, which the stream orders behind the kernels that still read the old offers) and reads two words back — the number of
// jobs removed and of cotasks folded in — in ONE synchronisation; the new queue length is the only value the host needs before it
// sizes the considerable filters' launches.  A carry (carry_host.hpp) is enqueued in the same place, over the same old rows.
// A release (release_host.hpp) is enqueued behind the carry and the fold, also when there is nothing to advance over; its counters ride
// in the same synchronisation.  A host churn (churn_host.hpp) is enqueued behind the release; its counter rides there too.  The host
// reservations (reserve_host.hpp) are enqueued behind the churn: they touch neither the queue nor the offers, and their two counters
// ride there as well.  The launch-rate limiters (limiter_host.hpp) spend the last cycle's kept placements behind the reservations; their two
// counters ride there too.  The pod delta and the offer rebuild of a pool whose offers are built from its pods (podtable_host.hpp) are enqueued
// behind all of these, which read the old rows; the rebuilt offer count rides in the same synchronisation.
#pragma once
#include "queue_kernels.hpp"

struct QueueBufs {
  DArr<int> removed;
  DArr<SumI> scan, gscan;
  DArr<uint32_t> ranked_tmp, g_off[2], g_host[2], g_attr[2];
  DArr<unsigned> add_cnt, cursor, counters;  // counters: [0] jobs removed, [1] cotasks folded in, then the release's (REL_CNT_*)
  DArr<uint8_t> skipped;
  unsigned cur = 0;  // which of g_*[2] holds the groups' current cotask table (when e->q_groups_own)
};


// a rank puts the groups' cotasks back to the staged table (the queue cycles' folds live in QueueBufs)
void queue_reset_groups(cook_engine* e) {
  if (!e->q_groups_own) return;
  e->min.g_run_off = e->q_sg_off, e->min.g_run_host = e->q_sg_host, e->min.g_run_attr = e->q_sg_attr;
  e->cf_group_run_total = e->q_sg_total;
  e->q_groups_own = false;
}

// everything that can refuse a step, before anything changes
void queue_check_step(cook_engine* e, const QueueArgs& q) {
  const cook_queue_step* s = q.step;
  if (!e->cycle_staged || !e->q_valid || !e->rank_done || !e->match_ran())
    e->fail(COOK_E_STATE, "cook_cycle_run_queue needs a completed cycle (cook_cycle_run, cook_cycle_run_rank* + cook_cycle_match_multi or a queue "
                          "cycle) with no cook_cycle_stage / cook_cycle_update / cook_rank* / cook_considerable / cook_match_stage since");
  carry_check(e, q);
  release_check(e, q);
  churn_check(e, q);
  reserve_check(e, q);
  limiter_check(e, q);
  podq_check(e, q);
  if (!s) return;
  if (s->remove_mode > 1u) e->fail(COOK_E_INVALID, "cook_queue_step.remove_mode: 0 = the kept matches, 1 = every considered job");
  if (s->offer_skipped && s->n_offer_skipped != e->M)
    e->fail(COOK_E_INVALID, "cook_queue_step: offer_skipped has one entry per offer of the LAST cycle (n_offer_skipped differs from that count)");
  if (const cook_offers* o = s->offers) {
    if (o->n && (!o->cpus || !o->mem || !o->host)) e->fail(COOK_E_INVALID, "cook_queue_step: offers need cpus, mem and host");
    if (o->gpu_slots > COOK_MAX_RES_SLOTS || o->disk_slots > COOK_MAX_RES_SLOTS) e->fail(COOK_E_INVALID, "cook_queue_step: offers' slots > COOK_MAX_RES_SLOTS");
    if (o->gpu_model && !o->gpu_count) e->fail(COOK_E_INVALID, "cook_queue_step: offers' gpu_model without gpu_count");
    if (o->scalars && o->n_scalars > COOK_MAX_SCALARS) e->fail(COOK_E_INVALID, "cook_queue_step: more than COOK_MAX_SCALARS named scalars");
    match_check_offer_count(e, o->n);
  }
  if (const cook_groups* g = s->groups) {
    const unsigned G = e->G;
    if (g->n != G) e->fail(COOK_E_INVALID, "cook_queue_step: groups->n differs from the staged groups");
    if (G && (!g->type || !g->attr_key || !g->minimum || !g->run_off)) e->fail(COOK_E_INVALID, "cook_queue_step: groups need type, attr_key, minimum, run_off");
    for (unsigned x = 0; x < G; ++x)
      if (g->type[x] != e->h_g_type[x] || g->attr_key[x] != e->h_g_key[x] || g->minimum[x] != e->h_g_min[x])
        e->fail(COOK_E_INVALID, "cook_queue_step: type / attr_key / minimum of the groups must equal the staged ones");
    if (G && g->run_off[0] != 0u) e->fail(COOK_E_INVALID, "cook_queue_step: groups->run_off must start at 0");
    for (unsigned x = 0; x < G; ++x)
      if (g->run_off[x + 1] < g->run_off[x]) e->fail(COOK_E_INVALID, "cook_queue_step: groups->run_off decreases");
    if (G && g->run_off[G] && (!g->run_host || !g->run_attr)) e->fail(COOK_E_INVALID, "cook_queue_step: groups need run_host and run_attr");
  }
}

// steps 1-3 of a queue cycle (cookmatch.h): the last cycle's jobs leave the queue, their cotasks join the groups, fresh offers
void queue_advance(cook_engine* e, const QueueArgs& q) {
  queue_check_step(e, q);
  const cook_queue_step* s = q.step;
  const cook_queue_carry* c = q.carry;
  const cook_finished* f = q.finished;
  const auto t_call = std::chrono::steady_clock::now();
  e->q_stepped = true;
  e->q_valid = false;  // from here on the queue is being edited: a call that fails below leaves no standing queue (cycle_take_part sets it again)
  QueueBufs& b = bufs(e->qb);
  MatchIn& in = e->min;
  const unsigned n = e->n_ranked, k = e->cycle_considered, G = e->G, M_old = e->M;
  const bool fold = G && k && in.j_group && !(s && s->groups) && !e->kube_last;  // (a Kubernetes cycle's launched jobs have no host yet)
  unsigned* cnt = b.counters.ensure(REL_CNT_WORDS);
  const bool advance = k && n, release = release_active(f), churn = churn_active(q.hosts), reserve = reserve_active(q.reservations),
             spend = limiter_spend_due(e, advance ? k : 0u);
  bool carried = false;
  const uint8_t* skipped = nullptr;  // the step's offer_skipped on the device (the advance's kernels and the reservations' release read it)
  if (advance || release || churn || reserve || spend) memset_async(e, cnt, 0, REL_CNT_WORDS * 4);
  if (advance) {
    int* removed = b.removed.ensure(n);
    memset_async(e, removed, 0, (size_t)n * 4);
    unsigned* add_cnt = b.add_cnt.ensure(std::max(1u, G));
    unsigned* cursor = b.cursor.ensure(std::max(1u, G));
    if (fold) memset_async(e, add_cnt, 0, (size_t)G * 4), memset_async(e, cursor, 0, (size_t)G * 4);
    // (behind a Kubernetes cycle job_to_offer is 0 / -1 = launched / not, no offer index: offer_skipped says nothing about those jobs and is not read)
    skipped = (s && s->offer_skipped && M_old && !e->kube_last) ? h2d_opt(e, b.skipped, s->offer_skipped, M_old) : nullptr;
    const int32_t* j2o = e->m_j2o.ptr();
    const uint32_t* j_index = e->j_index.ptr();
    KM<q_mark_removed, 256>(e, "q_mark_removed", div_up(k, 256), e->q_last_pos, j2o, k, n, skipped, (unsigned)((s && s->remove_mode == 1u) || e->kube_last), j_index,
        in.j_group, G, (unsigned)fold, removed, add_cnt, cnt);
    if (c) carried = carry_enqueue(e, c, skipped, k);  // (the carried offer columns are the staged ones from here: the fold below reads hosts and attributes, which stay)
    // ---- the queue: stable compaction, back into the resident buffer ----------------------------------------------------------------
    b.scan.ensure(n);
    uint32_t* tmp = b.ranked_tmp.ensure(n);
    seg_scan<SumI>(e, "q_queue_scan", LoadUnmatched{removed}, (const uint8_t*)nullptr, n, b.scan.ptr(), e->tmpI);
    KM<q_compact_ranked, 256>(e, "q_compact_ranked", div_up(n, 256), (const int*)removed, (const SumI*)b.scan.ptr(), n, (const uint32_t*)e->ranked.ptr(), tmp);
    copy_async(e, e->ranked.ptr(), tmp, (size_t)n * 4, hipMemcpyDeviceToDevice);  // (entries past the new length are never read)
    // ---- the groups: the kept matches' cotasks into a new CSR (the old one, staged or folded, stays as it is) --------------------------
    if (fold) {
      const unsigned n_old = e->cf_group_run_total;
      const unsigned nx = b.cur ^ (e->q_groups_own ? 1u : 0u);  // (the table in use may be g_*[cur])
      uint32_t* n_off = b.g_off[nx].ensure(G + 1);
      uint32_t* n_host = b.g_host[nx].ensure(std::max(1u, n_old + k));
      uint32_t* n_attr = b.g_attr[nx].ensure(std::max(1u, n_old + k));
      b.gscan.ensure(G);
      seg_scan<SumI>(e, "q_group_scan", LoadGroupRows{in.g_run_off, add_cnt}, (const uint8_t*)nullptr, G, b.gscan.ptr(), e->tmpI);
      KM<q_fold_offsets, 256>(e, "q_fold_offsets", div_up(G, 256), (const SumI*)b.gscan.ptr(), G, n_off);
      if (n_old && in.g_run_off)
        KM<q_fold_copy_old, 256>(e, "q_fold_copy_old", div_up(n_old, 256), in.g_run_off, in.g_run_host, in.g_run_attr, G, n_old, (const uint32_t*)n_off, n_host, n_attr);
      KM<q_fold_append, 256>(e, "q_fold_append", div_up(k, 256), j2o, k, skipped, j_index, in.j_group, G, in.g_run_off, (const uint32_t*)n_off, cursor,
          in.o_host, in.o_attr, in.n_attr, in.g_attr_key, n_host, n_attr);
      b.cur = nx;
      groups_install(e, n_off, n_host, n_attr);
    }
    pinned_copy(e, e->h_scratch + Q_H_ADVANCE, cnt, 8, hipMemcpyDeviceToHost);
  }
  // ---- the release: behind the carry and the fold, whether or not the last cycle considered anything ------------------------------------
  // (the host-id -> row table of this advance, host_rows: the release or, without one, the churn builds it and the other finds it built.
  //  Between the two e->M, cf_max_host and min.o_host do not change — the release's carry_stage_cols stages other columns — so one
  //  table serves both)
  if (e->cyb) e->cyb->h2row_built = false;
  if (f || e->rlb) release_enqueue(e, f, cnt, carried, (advance && fold) ? k : 0u);
  if (carry_release_offers(q)) e->o_run_cols_made = true;
  // ---- the host churn: behind the release (all of the above index the OLD rows), in front of the considerable filters ------------------
  if (q.hosts || e->chb) churn_enqueue(e, q.hosts, cnt);
  // ---- the host reservations: the last cycle's kept matches release theirs, a rebalancer's list replaces the map ----------------------------
  if (q.reservations || e->rvb) reserve_enqueue(e, q.reservations, cnt, skipped, advance ? k : 0u);
  // ---- the launch-rate limiters: the last cycle's kept placements spend their tokens, in front of the considerable filters --------------------
  limiter_enqueue(e, cnt, skipped, advance ? k : 0u);
  // ---- the pod delta and the offer rebuild (cook_cycle_run_queue_pods*): behind everything above, which reads the OLD rows -----------------------
  if (q.pods_on) podq_enqueue(e, q);
  if (release || churn || reserve || spend) pinned_copy(e, e->h_scratch + REL_H_CNT, cnt, REL_CNT_WORDS * 4, hipMemcpyDeviceToHost);
  // ---- the step's groups and offers (behind the kernels above on the stream: the fold read the OLD offers) ------------------------------
  if (s && s->groups && G) {
    const cook_groups* g = s->groups;
    const unsigned nx = b.cur ^ (e->q_groups_own ? 1u : 0u);
    const unsigned nr = g->run_off[G];
    const uint32_t* n_off = h2d_opt(e, b.g_off[nx], g->run_off, G + 1);
    b.g_host[nx].ensure(std::max(1u, nr)), b.g_attr[nx].ensure(std::max(1u, nr));
    if (nr) copy_async(e, b.g_host[nx].ptr(), g->run_host, (size_t)nr * 4, hipMemcpyHostToDevice);
    if (nr) copy_async(e, b.g_attr[nx].ptr(), g->run_attr, (size_t)nr * 4, hipMemcpyHostToDevice);
    groups_install(e, n_off, b.g_host[nx].ptr(), b.g_attr[nx].ptr());
    b.cur = nx;
    e->cf_group_run_total = nr;
  }
  if (s && s->offers) match_stage_offers(e, s->offers, false);
  if (e->chb) e->chb->info.n_offers = e->M;  // (the rows behind the advance, whoever set them)
  carry_tokens(e, c);
  if (advance || release || churn || reserve || spend || q.pods_on || (s && (s->groups || s->offers)) || (c && c->tokens_left)) sync(e);  // (the host arrays of the step are read until here)
  if (q.pods_on) podq_finish(e, q);  // (the rebuilt rows are the staged offers from here)
  if (c) carry_finish(e);
  if (advance) {
    unsigned h[2] = {0, 0};
    std::memcpy(h, e->h_scratch + Q_H_ADVANCE, 8);
    e->n_ranked = n - h[0];
    if (fold) e->cf_group_run_total += h[1];
  }
  if (release || churn || reserve || spend) {
    unsigned h[REL_CNT_WORDS];
    std::memcpy(h, e->h_scratch + REL_H_CNT, sizeof(h));
    release_finish(e, h);
    churn_finish(e, h);
    reserve_finish(e, h);
    limiter_finish(e, h);
  }
  e->q_advance_us = (uint32_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_call).count();
}
