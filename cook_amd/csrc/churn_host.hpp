// churn_host.hpp — host orchestration of the host churn (cook_cycle_run_queue_hosts*, cook_cycle_fetch_offers, cookmatch.h; DESIGN.md
// §21).  Included by engine.hip inside its anonymous namespace, behind release_host.hpp (carry_host.hpp's host-indexed table and SegSort, the
// counters' read-back); queue_host.hpp calls churn_check from queue_check_step and churn_enqueue / churn_finish from queue_advance.  Everything
// is enqueued on the advance's stream behind the carry, the groups' fold and the release, which still index the OLD rows; the one
// counter the host reads back rides in the advance's one synchronisation.  The host knows the new row count before the first launch
// from its mirror of the staged host ids (cook_engine::o_hosts), so no launch waits for a read-back.  No column is named here: the
// refusal "a column the staged offers lack", the joining rows' upload, the new table's columns and the fetch each walk offer_columns
// (offer_table.hpp), which also says which columns every table has and which a carry makes.
#pragma once
#include "churn_kernels.hpp"

struct ChurnBufs {
  DArr<uint32_t> leave, before;  // the lists on the device
  OfferStore join;               // ... and the joining rows' columns
  // the churn's own full column sets, written in turns: a churn reads the staged table (which may be the other set, or partly the
  // carry's) and writes the set the last match cannot have read
  OfferStore set[2];
  unsigned cur = 0;
  DArr<uint32_t> src;
  DArr<uint8_t> keep;
  DArr<uint64_t> akey;
  SegSort a;
  DArr<SumI> scan;
  ChurnGather h_args{};  // (read by the upload until the advance's synchronisation)
  DArr<ChurnGather> d_args;
  cook_churn_info info{};  // of the last queue cycle
  bool pending = false;    // this advance reads the churn's counter back
  // what churn_check worked out from the mirror, for the churn_enqueue of the same step
  unsigned plan_left = 0, plan_new = 0;
};

// this step carries into or releases into the staged offers: run_cpus / run_mem / run_count / num_tasks / ports exist from here on
static bool carry_release_offers(const QueueArgs& q) {
  return (q.carry && q.carry->offers) || (release_active(q.finished) && q.finished->offers);
}
static bool churn_active(const cook_host_churn* h) { return h && (h->n_leave || (h->join && h->join->n)); }

// named scalar columns the staged offers have
static unsigned churn_staged_scalars(const MatchIn& in) {
  unsigned n = 0;
  while (n < (unsigned)COOK_MAX_SCALARS && in.o_scal[n]) ++n;
  return n;
}

// what can refuse a churn, before anything changes (queue_check_step)
void churn_check(cook_engine* e, const QueueArgs& q) {
  const cook_host_churn* h = q.hosts;
  if (!churn_active(h)) return;
  const cook_queue_step* s = q.step;
  const MatchIn& in = e->min;
  if (s && s->offers) e->fail(COOK_E_INVALID, "cook_host_churn edits the STAGED offers; step->offers replaces them (one or the other)");
  if (in.host_dup) e->fail(COOK_E_INVALID, "cook_host_churn: two staged offers are on one host");
  if (!e->o_hosts_known)
    e->fail(COOK_E_STATE, "cook_host_churn: the staged offers were built on the device (cook_cycle_stage_built_offers): build them again from the nodes");
  if (h->n_leave && !h->leave_host) e->fail(COOK_E_INVALID, "cook_host_churn: n_leave without leave_host");
  const cook_offers* j = h->join;
  const unsigned nj = j ? j->n : 0u, M_old = e->M;
  const std::vector<uint32_t>& staged = e->o_hosts;  // ascending
  if (staged.size() != M_old) e->fail(COOK_E_STATE, "cook_host_churn: the engine's record of the staged hosts is out of step with the staged offers");
  auto is_staged = [&](uint32_t x) { return std::binary_search(staged.begin(), staged.end(), x); };
  std::vector<uint32_t> lv(h->leave_host, h->leave_host + h->n_leave);
  std::sort(lv.begin(), lv.end());
  if (std::adjacent_find(lv.begin(), lv.end()) != lv.end()) e->fail(COOK_E_INVALID, "cook_host_churn: a host twice in leave_host");
  unsigned left = 0;
  for (uint32_t x : lv) left += is_staged(x) ? 1u : 0u;
  if (nj) {
    if (!j->cpus || !j->mem || !j->host) e->fail(COOK_E_INVALID, "cook_host_churn: join needs cpus, mem and host");
    if (j->gpu_model && !j->gpu_count) e->fail(COOK_E_INVALID, "cook_host_churn: join has gpu_model without gpu_count");
    if (j->disk_type && !j->disk_space) e->fail(COOK_E_INVALID, "cook_host_churn: join has disk_type without disk_space");
    // (the five columns a carry or a release brings into existence count as present from the first such step on this table on, this
    //  very advance included, whether or not it had anything to carry or to release: absent, they read as 0 for every row, and the
    //  gather writes them out when the joining rows bring values)
    const bool made = e->o_run_cols_made || carry_release_offers(q);
    const OfferCols<false> staged = offer_cols_of(in);
    bool lacks = false;
    offer_columns([&](const auto& col) {
      if ((col.flags & OFFER_REQUIRED) || col.sub) return;  // (the named scalars are one pointer, judged by the first; their count is compared below)
      lacks |= j->*col.pub && !col.col(staged) && !((col.flags & OFFER_MADE) && made);
    });
    if (lacks) e->fail(COOK_E_INVALID, "cook_host_churn: join carries a column the staged offers lack");
    auto slots = [](uint32_t x) { return x ? x : 1u; };
    if ((j->gpu_model || j->gpu_count) && slots(j->gpu_slots) != in.gpu_slots) e->fail(COOK_E_INVALID, "cook_host_churn: join->gpu_slots differs from the staged offers'");
    if ((j->disk_type || j->disk_space) && slots(j->disk_slots) != in.disk_slots) e->fail(COOK_E_INVALID, "cook_host_churn: join->disk_slots differs from the staged offers'");
    if (j->attr && j->n_attr_keys != in.n_attr) e->fail(COOK_E_INVALID, "cook_host_churn: join->n_attr_keys differs from the staged offers'");
    if (j->scalars && j->n_scalars != churn_staged_scalars(in)) e->fail(COOK_E_INVALID, "cook_host_churn: join->n_scalars differs from the staged offers'");
    std::vector<uint32_t> jh(j->host, j->host + nj);
    std::sort(jh.begin(), jh.end());
    if (std::adjacent_find(jh.begin(), jh.end()) != jh.end()) e->fail(COOK_E_INVALID, "cook_host_churn: a host twice in join");
    for (uint32_t x : jh)
      if (is_staged(x) && !std::binary_search(lv.begin(), lv.end(), x))
        e->fail(COOK_E_INVALID, "cook_host_churn: a joining host is already staged and does not leave in this call");
    if (h->join_before)
      for (unsigned i = 0; i < nj; ++i)
        if (h->join_before[i] != COOK_NONE_U32 && !is_staged(h->join_before[i]))
          e->fail(COOK_E_INVALID, "cook_host_churn: join_before names a host that has no row in the staged offers");
  }
  const unsigned M_new = M_old - left + nj;
  match_check_offer_count(e, M_new);
  ChurnBufs& b = bufs(e->chb);
  b.plan_left = left, b.plan_new = M_new;
}

// Inside queue_advance, behind the release (so: over the table the NEXT match would have read), also when the last cycle considered
// nothing.  cnt: QueueBufs::counters, zero on the stream.
void churn_enqueue(cook_engine* e, const cook_host_churn* h, unsigned* cnt) {
  ChurnBufs& b = bufs(e->chb);
  b.info = cook_churn_info{0u, 0u, 0u, e->M};
  b.pending = false;
  if (!churn_active(h)) return;
  MatchIn& in = e->min;
  const cook_offers* j = h->join;
  const unsigned M_old = e->M, n_leave = h->n_leave, nj = j ? j->n : 0u, M_new = b.plan_new;
  const OfferDims d = offer_dims(in);
  // ---- the lists (read until the advance's synchronisation) ----------------------------------------------------------------------------
  const uint32_t* leave = h2d_opt(e, b.leave, h->leave_host, n_leave);
  const uint32_t* before = nj ? h2d_opt(e, b.before, h->join_before, nj) : nullptr;
  OfferCols<false> jc{};
  if (nj)
    offer_columns([&](const auto& col) {
      const size_t width = d.width(col.kind);
      col.col(jc) = width ? h2d_opt(e, col.col(b.join), col.of(*j), nj * width) : nullptr;
    });
  // ---- rows of the leaving hosts and of the anchors --------------------------------------------------------------------------------------
  unsigned n_hosts = 0;
  const uint32_t* h2row = M_old ? host_rows(e, n_hosts) : nullptr;  // (null: churn_row_of looks through o_host; built by this advance's release: found)
  uint8_t* keep = b.keep.ensure(M_old);
  memset_async(e, keep, 1, M_old);
  uint64_t* akey = b.akey.ensure(nj);
  KM<churn_mark, 256>(e, "churn_mark", div_up(std::max(n_leave, nj), 256), leave, n_leave, before, nj, h2row, n_hosts, in.o_host, M_old, keep, akey, cnt);
  // ---- the joins by anchor in list order, ONE scan, the source map -----------------------------------------------------------------------
  const uint32_t* perm = nj ? b.a.carry_segments(e, akey, nj, M_old + 1u) : nullptr;
  const LoadChurnRows rows{keep, nj ? (const uint32_t*)b.a.start.ptr() : nullptr, nj ? (const uint32_t*)b.a.end.ptr() : nullptr, M_old};
  SumI* incl = b.scan.ensure(M_old + 1u);
  seg_scan<SumI>(e, "churn_scan", rows, (const uint8_t*)nullptr, M_old + 1u, incl, e->tmpI);
  uint32_t* src = b.src.ensure(M_new);
  memset_async(e, src, 0xFF, (size_t)M_new * 4);
  KM<churn_source, 256>(e, "churn_source", div_up(std::max(M_old, nj), 256), rows, (const SumI*)incl, perm, (const uint64_t*)akey, nj, M_new, src);
  // ---- ONE gather of every column into the set the staged table is not -------------------------------------------------------------------
  ChurnGather& g = b.h_args;
  g = ChurnGather{};
  g.old = offer_cols_of(in), g.join = jc;
  g.M_old = M_old, g.n_join = nj, g.M_new = M_new, g.dims = d;
  // the new table has the columns the old one has, and of the columns a carry makes also those only the joining rows bring values for
  g.out = b.set[b.cur ^ 1u].ensure(d, M_new, [&](const auto& col) {
    return (col.flags & OFFER_REQUIRED) || col.col(g.old) || ((col.flags & OFFER_MADE) && col.col(jc));
  });
  const ChurnGather* d_args = h2d_opt(e, b.d_args, (const ChurnGather*)&g, 1);
  KM<churn_gather, 256>(e, "churn_gather", div_up(M_new, 256), d_args, (const uint32_t*)src);
  b.cur ^= 1u;
  offer_cols_stage(in, g.out, d, M_new);
  e->M = M_new;
  // ---- the mirror: host_dup stays 0, and the greatest host id stays exact (the class-ordered walk's and the release's tables) --------------
  std::vector<uint32_t>& staged = e->o_hosts;
  for (unsigned t = 0; t < n_leave; ++t) {
    auto it = std::lower_bound(staged.begin(), staged.end(), h->leave_host[t]);
    if (it != staged.end() && *it == h->leave_host[t]) staged.erase(it);
  }
  for (unsigned i = 0; i < nj; ++i) staged.insert(std::lower_bound(staged.begin(), staged.end(), j->host[i]), j->host[i]);
  e->cf_max_host = staged.empty() ? 0xFFFFFFFFu : staged.back();
  b.info = cook_churn_info{b.plan_left, 0u, nj, M_new};
  b.pending = true;
}

// behind the advance's synchronisation; h: the advance's counters
void churn_finish(cook_engine* e, const unsigned* h) {
  if (!e->chb || !e->chb->pending) return;
  e->chb->pending = false;
  e->chb->info.leave_missing = h[CHURN_CNT_MISSING];
}

// cook_cycle_fetch_offers: the staged offer table as the next match will read it, in one synchronisation
void churn_fetch_offers(cook_engine* e, cook_offer_rows* out) {
  if (!out) e->fail(COOK_E_INVALID, "cook_cycle_fetch_offers: null out");
  if (!e->match_staged) e->fail(COOK_E_STATE, "cook_cycle_fetch_offers before offers were staged");
  const MatchIn& in = e->min;
  const OfferCols<false> staged = offer_cols_of(in);
  OfferDims d = offer_dims(in);
  if (!staged.attr) d.n_attr = 0;
  const unsigned n = e->M;
  out->n = n, out->gpu_slots = d.gpu_slots, out->disk_slots = d.disk_slots, out->n_attr_keys = d.n_attr, out->n_scalars = churn_staged_scalars(in);
  if (out->cap < n) e->fail(COOK_E_INVALID, "cook_cycle_fetch_offers: cap is smaller than the staged offers' row count (see n)");
  bool copied = false;
  offer_columns([&](const auto& col) {
    auto* dst = col.of(*out);
    const size_t cells = (size_t)n * d.width(col.kind);
    if (!dst || !cells) return;
    if (const auto* src = col.col(staged)) {
      copy_async(e, dst, src, cells * sizeof(*dst), hipMemcpyDeviceToHost);
      copied = true;
    } else {
      std::fill(dst, dst + cells, col.none);  // what a NULL column means
    }
  });
  if (copied) sync(e);
}
