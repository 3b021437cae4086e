// podtable_host.hpp — host orchestration of the resident pod table (cook_offers_stage_pod_ids, cook_offers_update, cook_offers_fetch_pods,
// cook_cycle_set_built_offers and the pod part of cook_cycle_run_queue_pods*, cookmatch.h).  Included by engine.hip inside
// its anonymous namespace, behind offers_host.hpp (OfferBufs: the staged node and pod columns, offers_enqueue / offers_finish,
// built_offers_cols) and limiter_host.hpp (QueueArgs); queue_host.hpp calls podq_check from queue_check_step and podq_enqueue /
// podq_finish from queue_advance.  A delta is checked completely on the host — against the engine's bitmap of the live ids and the
// column sets of the staged tables — before anything changes (podtable_plan), so the new row count is known before the first launch and
// nothing waits for a read-back; podtable_apply only enqueues.  The pod columns are gathered into second buffers that are swapped in (a
// grow-only buffer that grows forgets what it held); the node rows are scattered in place.
#pragma once
#include "podtable_kernels.hpp"

struct PodTableBufs {
  // identity
  bool ids = false;
  unsigned id_cap = 0;
  DArr<uint32_t> p_id, id2row;
  std::vector<uint64_t> live;  // bit id: the id has a row
  // the delta on the device (read until the call's / the advance's synchronisation)
  DArr<uint32_t> remove_id, add_id, node_row, a_node, a_gpu_model, a_disk_type, v_host, v_gpu_model, v_disk_type, v_attr;
  DArr<double> a_cpus, a_mem, a_disk, v_cpus, v_mem, v_disk;
  DArr<int32_t> a_gpus, v_gpus;
  DArr<uint8_t> a_flags, v_flags;
  // work, and the pod columns' second buffers (PodColSet order)
  DArr<uint8_t> keep;
  DArr<SumI> scan;
  DBuf alt[POD_MAX_COLS];
  cook_pod_delta_info info{};
  // what podtable_plan worked out for the podtable_apply of the same call
  unsigned plan_removed = 0, plan_missing = 0;
  bool live_test(uint32_t id) const { return (live[id >> 6] >> (id & 63u)) & 1ull; }
  void live_set(uint32_t id, bool on) {
    if (on) live[id >> 6] |= 1ull << (id & 63u);
    else live[id >> 6] &= ~(1ull << (id & 63u));
  }
  void drop_ids() { ids = false, id_cap = 0, live.clear(); }
};

static unsigned long long pod_bits64(double v) {
  unsigned long long b;
  std::memcpy(&b, &v, 8);
  return b;
}
static bool sorted_has_dup(std::vector<uint32_t>& v) {
  std::sort(v.begin(), v.end());
  return std::adjacent_find(v.begin(), v.end()) != v.end();
}

// cook_offers_stage_pod_ids
void podtable_stage_ids(cook_engine* e, const uint32_t* pod_id, uint32_t n, uint32_t id_cap) {
  if (!e->ofb || !e->ofb->staged) e->fail(COOK_E_STATE, "cook_offers_stage_pod_ids before cook_offers_stage");
  OfferBufs& b = *e->ofb;
  PodTableBufs& t = bufs(e->ptb);
  t.drop_ids();
  if (n != b.Np) e->fail(COOK_E_INVALID, "cook_offers_stage_pod_ids: n differs from the staged pods' row count");
  if (n && !pod_id) e->fail(COOK_E_INVALID, "cook_offers_stage_pod_ids: null pod_id");
  std::vector<uint64_t> live((size_t)id_cap / 64 + 1, 0ull);
  for (unsigned i = 0; i < n; ++i) {
    const uint32_t id = pod_id[i];
    if (id >= id_cap) e->fail(COOK_E_INVALID, "cook_offers_stage_pod_ids: an id at or above id_cap");
    if ((live[id >> 6] >> (id & 63u)) & 1ull) e->fail(COOK_E_INVALID, "cook_offers_stage_pod_ids: an id twice");
    live[id >> 6] |= 1ull << (id & 63u);
  }
  h2d(e, t.p_id, pod_id, n);
  uint32_t* id2row = t.id2row.ensure(std::max(1u, id_cap));
  memset_async(e, id2row, 0xFF, (size_t)std::max(1u, id_cap) * 4);
  KM<pod_id_scatter, 256>(e, "pod_id_scatter", div_up(n, 256), (const uint32_t*)t.p_id.ptr(), n, id_cap, id2row);
  sync(e);
  t.live = std::move(live);
  t.id_cap = id_cap;
  t.ids = true;
  t.info = cook_pod_delta_info{0u, 0u, 0u, 0u, n, b.done ? b.n_offers : 0u};
}

// everything that can refuse a delta, before anything changes; leaves the counts for podtable_apply
void podtable_plan(cook_engine* e, const cook_pod_delta* d) {
  if (!d) e->fail(COOK_E_INVALID, "cook_offers_update: null delta");
  if (!e->ofb || !e->ofb->staged || !e->ptb || !e->ptb->ids)
    e->fail(COOK_E_STATE, "cook_offers_update needs cook_offers_stage and cook_offers_stage_pod_ids before it");
  const OfferBufs& b = *e->ofb;
  PodTableBufs& t = *e->ptb;
  const cook_pods* a = d->add;
  const unsigned n_add = a ? a->n : 0u;
  if (d->n_remove && !d->remove_id) e->fail(COOK_E_INVALID, "cook_offers_update: n_remove without remove_id");
  if (n_add && (!a->node || !a->cpus || !a->mem || !d->add_id)) e->fail(COOK_E_INVALID, "cook_offers_update: add needs node, cpus, mem and add_id");
  // ---- the ids ------------------------------------------------------------------------------------------------------------------------
  std::vector<uint32_t> rm(d->remove_id, d->remove_id + d->n_remove);
  for (uint32_t id : rm)
    if (id >= t.id_cap) e->fail(COOK_E_INVALID, "cook_offers_update: a remove_id at or above id_cap");
  if (sorted_has_dup(rm)) e->fail(COOK_E_INVALID, "cook_offers_update: an id twice in remove_id");
  unsigned removed = 0;
  for (uint32_t id : rm) removed += t.live_test(id) ? 1u : 0u;
  std::vector<uint32_t> ad(n_add ? d->add_id : nullptr, n_add ? d->add_id + n_add : nullptr);
  for (uint32_t id : ad) {
    if (id >= t.id_cap) e->fail(COOK_E_INVALID, "cook_offers_update: an add_id at or above id_cap");
    if (t.live_test(id) && !std::binary_search(rm.begin(), rm.end(), id))
      e->fail(COOK_E_INVALID, "cook_offers_update: an added id is live and does not leave in this call");
  }
  if (sorted_has_dup(ad)) e->fail(COOK_E_INVALID, "cook_offers_update: an id twice in add_id");
  // ---- the columns ----------------------------------------------------------------------------------------------------------------------
  if (n_add && ((a->gpus && !b.pd.gpus) || (a->gpu_model && !b.pd.gpu_model) || (a->disk && !b.pd.disk) || (a->disk_type && !b.pd.disk_type) ||
                (a->flags && !b.pd.flags)))
    e->fail(COOK_E_INVALID, "cook_offers_update: add carries a column the staged pods lack (stage again with cook_offers_stage)");
  // ---- the node rows ----------------------------------------------------------------------------------------------------------------------
  const cook_nodes* v = d->node_values;
  if (d->n_node_rows) {
    if (!d->node_row || !v) e->fail(COOK_E_INVALID, "cook_offers_update: n_node_rows without node_row / node_values");
    if (v->n != d->n_node_rows) e->fail(COOK_E_INVALID, "cook_offers_update: node_values->n differs from n_node_rows");
    if (!v->cpus || !v->mem) e->fail(COOK_E_INVALID, "cook_offers_update: node_values needs cpus and mem");
    std::vector<uint32_t> rows(d->node_row, d->node_row + d->n_node_rows);
    for (uint32_t r : rows)
      if (r >= b.Nn) e->fail(COOK_E_INVALID, "cook_offers_update: node_row out of range");
    if (sorted_has_dup(rows)) e->fail(COOK_E_INVALID, "cook_offers_update: a row twice in node_row");
    if ((v->host && !b.d_host) || (v->gpus && !b.nd.gpus) || (v->gpu_model && !b.nd.gpu_model) || (v->disk && !b.nd.disk) ||
        (v->disk_type && !b.nd.disk_type) || (v->flags && !b.nd.flags) || (v->attr && !b.n_attr))
      e->fail(COOK_E_INVALID, "cook_offers_update: node_values carries a column the staged nodes lack (stage again with cook_offers_stage)");
    if (v->attr && v->n_attr_keys != b.n_attr) e->fail(COOK_E_INVALID, "cook_offers_update: node_values->n_attr_keys differs from the staged nodes'");
  }
  t.plan_removed = removed, t.plan_missing = d->n_remove - removed;
}

// the planned delta, enqueued: no synchronisation, no read-back (the lists and the joining rows are read until the caller's next one)
void podtable_apply(cook_engine* e, const cook_pod_delta* d) {
  OfferBufs& b = *e->ofb;
  PodTableBufs& t = *e->ptb;
  const cook_pods* a = d->add;
  const unsigned n_old = b.Np, n_add = a ? a->n : 0u, n_keep = n_old - t.plan_removed, n_new = n_keep + n_add;
  uint32_t* id2row = t.id2row.ptr();
  if (d->n_remove || n_add) {
    // ---- which rows stay, and where they go -----------------------------------------------------------------------------------------
    uint8_t* keep = t.keep.ensure(n_old);
    SumI* incl = t.scan.ensure(n_old);
    if (n_old) memset_async(e, keep, 1, n_old);
    if (d->n_remove) {
      const uint32_t* rem = h2d_opt(e, t.remove_id, d->remove_id, d->n_remove);
      KM<pod_mark, 256>(e, "pod_mark", div_up(d->n_remove, 256), rem, d->n_remove, t.id_cap, id2row, n_old, keep);
    }
    if (n_old) seg_scan<SumI>(e, "pod_scan", LoadPodKeep{keep}, (const uint8_t*)nullptr, n_old, incl, e->tmpI);
    // ---- every column the table has, into its second buffer ---------------------------------------------------------------------------
    PodColSet cs{};
    std::vector<std::pair<DBuf*, DBuf*>> swaps;
    auto col = [&](auto& resident, bool has, const auto* given, auto& up, unsigned long long dflt) {
      if (!has) return;
      using T = std::remove_reference_t<decltype(*resident.ptr())>;
      DBuf& alt = t.alt[cs.n_cols];
      alt.ensure(std::max<size_t>(1, n_new) * sizeof(T));
      const void* add = (n_add && given) ? (const void*)h2d_opt(e, up, given, n_add) : nullptr;
      cs.c[cs.n_cols++] = PodCol{resident.ptr(), alt.p, add, dflt, (unsigned)sizeof(T), 1u};
      swaps.push_back({&resident.b, &alt});
    };
    col(b.p_node, true, a ? a->node : nullptr, t.a_node, 0xFFFFFFFFull);
    col(b.p_cpus, true, a ? a->cpus : nullptr, t.a_cpus, 0ull);
    col(b.p_mem, true, a ? a->mem : nullptr, t.a_mem, 0ull);
    col(b.p_gpus, b.pd.gpus != nullptr, a ? a->gpus : nullptr, t.a_gpus, 0ull);
    col(b.p_gpu_model, b.pd.gpu_model != nullptr, a ? a->gpu_model : nullptr, t.a_gpu_model, 0ull);
    col(b.p_disk, b.pd.disk != nullptr, a ? a->disk : nullptr, t.a_disk, pod_bits64(-1.0));  // (absent)
    col(b.p_disk_type, b.pd.disk_type != nullptr, a ? a->disk_type : nullptr, t.a_disk_type, 0ull);
    col(b.p_flags, b.pd.flags != nullptr, a ? a->flags : nullptr, t.a_flags, 0ull);
    col(t.p_id, true, n_add ? d->add_id : nullptr, t.add_id, 0xFFFFFFFFull);
    KM<pod_gather, 256>(e, "pod_gather", div_up(n_old, 256), cs, (const uint8_t*)keep, (const SumI*)incl, n_old, n_new);
    KM<pod_append, 256>(e, "pod_append", div_up(n_add, 256), cs, n_keep, n_add, n_new);
    for (auto& s : swaps) std::swap(s.first->p, s.second->p), std::swap(s.first->cap, s.second->cap);
    b.Np = n_new;
    b.pd = PodCols{b.p_node.ptr(), b.p_cpus.ptr(), b.p_mem.ptr(), b.pd.gpus ? b.p_gpus.ptr() : nullptr, b.pd.gpu_model ? b.p_gpu_model.ptr() : nullptr,
                   b.pd.disk ? b.p_disk.ptr() : nullptr, b.pd.disk_type ? b.p_disk_type.ptr() : nullptr, b.pd.flags ? b.p_flags.ptr() : nullptr, n_new};
    KM<pod_id_scatter, 256>(e, "pod_id_scatter", div_up(n_new, 256), (const uint32_t*)t.p_id.ptr(), n_new, t.id_cap, id2row);
    for (unsigned i = 0; i < d->n_remove; ++i) t.live_set(d->remove_id[i], false);
    for (unsigned i = 0; i < n_add; ++i) t.live_set(d->add_id[i], true);
  }
  // ---- the node rows, in place ------------------------------------------------------------------------------------------------------------
  if (const unsigned nr = d->n_node_rows) {
    const cook_nodes* v = d->node_values;
    PodColSet cs{};
    auto col = [&](auto& resident, bool has, const auto* given, auto& up, unsigned long long dflt, unsigned width, bool keep_if_null = false) {
      if (!has || (keep_if_null && !given)) return;
      using T = std::remove_reference_t<decltype(*resident.ptr())>;
      const void* add = given ? (const void*)h2d_opt(e, up, given, (size_t)nr * width) : nullptr;
      cs.c[cs.n_cols++] = PodCol{nullptr, resident.ptr(), add, dflt, (unsigned)sizeof(T), width};
    };
    col(b.n_host, b.d_host != nullptr, v->host, t.v_host, 0ull, 1u, true);
    col(b.n_cpus, true, v->cpus, t.v_cpus, 0ull, 1u);
    col(b.n_mem, true, v->mem, t.v_mem, 0ull, 1u);
    col(b.n_gpus, b.nd.gpus != nullptr, v->gpus, t.v_gpus, 0ull, 1u);
    col(b.n_gpu_model, b.nd.gpu_model != nullptr, v->gpu_model, t.v_gpu_model, 0ull, 1u);
    col(b.n_disk, b.nd.disk != nullptr, v->disk, t.v_disk, pod_bits64(-1.0), 1u);
    col(b.n_disk_type, b.nd.disk_type != nullptr, v->disk_type, t.v_disk_type, 0ull, 1u);
    col(b.n_flags, b.nd.flags != nullptr, v->flags, t.v_flags, 0ull, 1u);
    col(b.n_attr_tab, b.d_attr != nullptr, v->attr, t.v_attr, 0ull, b.n_attr);
    if (v->host && b.max_host != 0xFFFFFFFFu) b.max_host = std::max(b.max_host, *std::max_element(v->host, v->host + nr));
    const uint32_t* rows = h2d_opt(e, t.node_row, d->node_row, nr);
    KM<pod_node_scatter, 256>(e, "pod_node_scatter", div_up(nr, 256), cs, rows, nr, b.Nn);
  }
  t.info = cook_pod_delta_info{t.plan_removed, t.plan_missing, n_add, d->n_node_rows, b.Np, b.done ? b.n_offers : 0u};
}

// cook_offers_update
void podtable_update(cook_engine* e, const cook_pod_delta* d) {
  podtable_plan(e, d);
  podtable_apply(e, d);
  sync(e);  // (the caller's lists are read until here)
}

// cook_offers_update_info
void podtable_info(cook_engine* e, cook_pod_delta_info* out) {
  if (!out) e->fail(COOK_E_INVALID, "cook_offers_update_info: null out");
  const OfferBufs* b = e->ofb.get();
  *out = e->ptb ? e->ptb->info : cook_pod_delta_info{};
  out->n_pods = (b && b->staged) ? b->Np : 0u;
  out->n_offers = (b && b->done) ? b->n_offers : 0u;
}

// cook_offers_fetch_pods
void podtable_fetch(cook_engine* e, cook_pod_rows* out) {
  if (!out) e->fail(COOK_E_INVALID, "cook_offers_fetch_pods: null out");
  if (!e->ofb || !e->ofb->staged) e->fail(COOK_E_STATE, "cook_offers_fetch_pods before cook_offers_stage");
  const OfferBufs& b = *e->ofb;
  const unsigned n = b.Np;
  out->n = n;
  if (out->cap < n) e->fail(COOK_E_INVALID, "cook_offers_fetch_pods: cap is smaller than the pod table's row count (see n)");
  bool copied = false;
  auto col = [&](auto* dst, const auto* src, auto none) {
    if (!dst || !n) return;
    if (src) {
      copy_async(e, dst, src, (size_t)n * sizeof(*dst), hipMemcpyDeviceToHost);
      copied = true;
    } else {
      std::fill(dst, dst + n, none);
    }
  };
  col(out->node, b.pd.node, (uint32_t)COOK_NONE_U32);
  col(out->cpus, b.pd.cpus, 0.0);
  col(out->mem, b.pd.mem, 0.0);
  col(out->gpus, b.pd.gpus, (int32_t)0);
  col(out->gpu_model, b.pd.gpu_model, (uint32_t)0);
  col(out->disk, b.pd.disk, -1.0);
  col(out->disk_type, b.pd.disk_type, (uint32_t)0);
  col(out->flags, b.pd.flags, (uint8_t)0);
  col(out->id, (e->ptb && e->ptb->ids) ? (const uint32_t*)e->ptb->p_id.ptr() : (const uint32_t*)nullptr, (uint32_t)COOK_NONE_U32);
  if (copied) sync(e);
}

// cook_cycle_set_built_offers: the rows of the last cook_offers_run as the staged offers of the cycle, in place
void podq_set_built_offers(cook_engine* e, int with_task_limits) {
  if (!e->cycle_staged) e->fail(COOK_E_STATE, "cook_cycle_set_built_offers before cook_cycle_stage");
  if (!e->ofb || !e->ofb->done) e->fail(COOK_E_STATE, "cook_cycle_set_built_offers before cook_offers_run");
  match_check_offer_count(e, e->ofb->n_offers);
  const cook_offers o = built_offers_view(e, with_task_limits);
  e->placement_drop();  // (a set-up points at the rows that were staged)
  e->q_valid = false;   // (the last cycle's job_to_offer indexes them: no queue cycle behind this)
  match_stage_offers(e, &o, true);
  if (o.n) e->cf_max_host = e->ofb->max_host;  // (one row per node: no two on one host, and none above the nodes' greatest)
  sync(e);
}

// ---- the pod part of a queue cycle (cook_cycle_run_queue_pods*) -------------------------------------------------------------------------------
constexpr unsigned PODQ_H_OFFERS = 24;  // where the rebuilt offer count lands in h_scratch (64-bit words), behind the release's pool
static_assert(PODQ_H_OFFERS >= REL_H_POOL + 4 && PODQ_H_OFFERS < 64, "the rebuild's read-back lies behind the release's in h_scratch");

// what can refuse the pod part of a step, before anything changes (queue_check_step)
void podq_check(cook_engine* e, const QueueArgs& q) {
  if (!q.pods_on) return;
  if (q.step && q.step->offers) e->fail(COOK_E_INVALID, "cook_cycle_run_queue_pods: the offers come from the pods; step->offers replaces them (one or the other)");
  if (q.carry && q.carry->offers) e->fail(COOK_E_INVALID, "cook_cycle_run_queue_pods: carry->offers: a launched pod is a row of pods->add, not a smaller lease");
  if (q.finished && q.finished->offers) e->fail(COOK_E_INVALID, "cook_cycle_run_queue_pods: finished->offers: a finished task's pod is in pods->remove_id");
  if (!e->offers_built || !e->ofb || !e->ofb->staged)
    e->fail(COOK_E_STATE, "cook_cycle_run_queue_pods: the staged offers were not built on this engine (cook_cycle_stage_built_offers / cook_cycle_set_built_offers)");
  match_check_offer_count(e, e->ofb->Nn);
  if (q.pods) podtable_plan(e, q.pods);
}

// Inside queue_advance, behind everything that reads the OLD rows (the advance's kernels, the carry, the fold, the release, the
// reservations, the limiters' spend): the delta, the rebuild, the constant columns.  One stream: the rebuild overwrites the rows the
// last match read only when every reader enqueued above has run.
void podq_enqueue(cook_engine* e, const QueueArgs& q) {
  OfferBufs& b = *e->ofb;
  if (q.pods) podtable_apply(e, q.pods);
  else if (e->ptb) e->ptb->info = cook_pod_delta_info{0u, 0u, 0u, 0u, b.Np, 0u};
  offers_enqueue(e, b, PODQ_H_OFFERS);
  (void)built_offers_cols(e, b, 0u, b.Nn, 1);
}
// behind the advance's synchronisation: the count, and the rebuilt rows as the staged offers
void podq_finish(cook_engine* e, const QueueArgs& q) {
  OfferBufs& b = *e->ofb;
  offers_finish(e, b, PODQ_H_OFFERS);
  const cook_offers o = built_offers_cols(e, b, b.n_offers, 0u, q.with_task_limits);
  match_stage_offers(e, &o, true);
  if (o.n) e->cf_max_host = b.max_host;  // (one row per node: no two on one host, and none above the nodes' greatest)
  if (e->ptb) e->ptb->info.n_offers = b.n_offers;
  if (e->chb) e->chb->info.n_offers = e->M;  // (cook_cycle_churn_info: the rows behind the advance, whoever set them)
}
