// autoscale_host.hpp — host orchestration of cook_cycle_autoscale (included by engine.hip inside its anonymous namespace).
// Reads the pool's last cycle in place on the device (the ranked queue, the considered rank positions, job_to_offer, the staged user
// state) and changes none of it: everything it writes lives in AutoscaleBufs, the filters run on AutoscaleBufs::w.
// Synchronisations: one to read m back (N depends on it and sizes the filters' queue), those of cons_run_device, one for the result.
#pragma once
#include "autoscale_kernels.hpp"

struct AutoscaleBufs {
  ConsWork w;  // cons_run_device's work set for the post-match queue
  DArr<int> matched, keep;
  DArr<SumI> scan;
  DArr<double> a_cpus, a_mem, a_gpus;
  DArr<uint32_t> a_user, a_rpos, exclude, task, out;
  DArr<uint8_t> skipped, excluded;
  DArr<unsigned> counters;  // [0] m, [1] |Out|
  // cook_cycle_autoscale_clusters: the tasks' outstanding-pod bits, Out's codes, the per-block counts per bin and their scan, the launch lists
  DArr<uint32_t> c_flags, c_out_task, c_launch;
  DArr<uint8_t> c_code, c_head;
  DArr<int> c_kept;
  DArr<SumI> c_scan;
  DArr<AsDistOut> c_dist;
};

// what cook_cycle_autoscale_clusters adds to the call: the cluster table and where its results go
struct AsClusterReq {
  const cook_autoscale_clusters* cl;
  uint32_t* cluster_off;
  cook_autoscale_cluster_info* cinfo;
  cook_autoscale_no_cluster* none;
};
constexpr unsigned AS_DIST_WORDS = sizeof(AsDistOut) / 4, AS_DIST_AT = 2;  // the read-back's place in h_scratch, behind |Out| (128 words in all)
static_assert(AS_DIST_AT + AS_DIST_WORDS <= 128 && AS_MAX_CLUSTERS == COOK_MAX_CLUSTERS, "the distribution's counts ride in h_scratch");

// max-launchable (compute_cluster.clj:642-644) in int64; a difference that leaves int64 saturates
static int64_t as_max_launchable(const cook_autoscale_clusters* cl, unsigned k) {
  auto diff = [](int64_t a, int64_t b) {
    int64_t r;
    if (__builtin_sub_overflow(a, b, &r)) r = b < 0 ? INT64_MAX : INT64_MIN;
    return r;
  };
  return std::min({diff(cl->max_pods_outstanding[k], cl->num_synthetic_pods[k]), diff(cl->max_total_nodes[k], cl->total_nodes[k]),
                   diff(cl->max_total_pods[k], cl->total_pods[k])});
}
// everything the host can know about the request, in front of the first launch
static void as_check_clusters(cook_engine* e, const AsClusterReq& r) {
  const cook_autoscale_clusters* cl = r.cl;
  if (!cl) e->fail(COOK_E_INVALID, "cook_cycle_autoscale_clusters: null clusters");
  if (cl->n < 1 || cl->n > COOK_MAX_CLUSTERS) e->fail(COOK_E_INVALID, "cook_cycle_autoscale_clusters: 1 <= clusters->n <= COOK_MAX_CLUSTERS");
  if (!cl->location || !cl->max_pods_outstanding || !cl->num_synthetic_pods || !cl->max_total_nodes || !cl->total_nodes || !cl->max_total_pods ||
      !cl->total_pods)
    e->fail(COOK_E_INVALID, "cook_cycle_autoscale_clusters: a column of clusters is NULL");
  if (!r.cluster_off || !r.cinfo) e->fail(COOK_E_INVALID, "cook_cycle_autoscale_clusters: null cluster_off / cluster_info");
  if (cl->out_off) {
    if (cl->out_off[0] != 0) e->fail(COOK_E_INVALID, "cook_cycle_autoscale_clusters: out_off must start at 0");
    for (unsigned k = 0; k < cl->n; ++k)
      if (cl->out_off[k + 1] < cl->out_off[k]) e->fail(COOK_E_INVALID, "cook_cycle_autoscale_clusters: out_off decreases");
    if (cl->out_off[cl->n] && !cl->out_task) e->fail(COOK_E_INVALID, "cook_cycle_autoscale_clusters: out_off without out_task");
    for (uint32_t x = 0; x < cl->out_off[cl->n]; ++x)
      if (cl->out_task[x] >= e->N) e->fail(COOK_E_INVALID, "cook_cycle_autoscale_clusters: outstanding task index out of range");
  }
  if (e->hash_set != e->n_pending)
    e->fail(COOK_E_STATE, "cook_cycle_autoscale_clusters: cook_cycle_set_job_hashes has not set every pending row's hash");
}

// the engine-owned (hash uuid) column by pending ordinal (cookmatch.h)
void cycle_set_job_hashes(cook_engine* e, const int32_t* hash, uint32_t first, uint32_t n) {
  if (!e->cycle_staged) e->fail(COOK_E_STATE, "cook_cycle_set_job_hashes before cook_cycle_stage");
  if (n && !hash) e->fail(COOK_E_INVALID, "cook_cycle_set_job_hashes: null hash");
  if (first > e->n_pending || n > e->n_pending - first) e->fail(COOK_E_INVALID, "cook_cycle_set_job_hashes: rows past the pending count");
  if (first > e->hash_set) e->fail(COOK_E_INVALID, "cook_cycle_set_job_hashes: rows in front of `first` are not set (a gap)");
  if (!n) return;
  if (!e->hash_set) e->j_hash.ensure(e->n_pending);  // (a set prefix lives in a buffer that holds every pending row: a stage or an update sized it)
  copy_async(e, e->j_hash.ptr() + first, hash, (size_t)n * 4, hipMemcpyHostToDevice);
  sync(e);
  e->hash_set = std::max(e->hash_set, first + n);
}

void cycle_autoscale(cook_engine* e, const cook_autoscale_params* p, uint32_t* task_idx, uint32_t cap, cook_autoscale_info* info,
                     const AsClusterReq* req = nullptr) {
  if (!p) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: null params");
  if (!e->cycle_cons_ran || !e->rank_done || !e->match_ran() || !e->cb || e->kube_last)
    e->fail(COOK_E_STATE, "cook_cycle_autoscale needs the last cook_cycle_run (or cook_cycle_run_rank + cook_cycle_match_multi) to have run the "
                          "considerable filters, with no stage / cook_cycle_update / cook_considerable since");
  if (!std::isfinite(p->scale_factor)) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: scale_factor is not finite");
  if (p->max_jobs > (uint32_t)INT32_MAX) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: max_jobs > INT32_MAX");
  if (p->n_exclude && !p->exclude_task) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: n_exclude without exclude_task");
  for (uint32_t x = 0; x < p->n_exclude; ++x)
    if (p->exclude_task[x] >= e->N) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: exclude_task index out of range");
  if (cap && !task_idx) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: null task_idx");
  if (req) as_check_clusters(e, *req);
  const ConsBufs& c = *e->cb;
  AutoscaleBufs& b = bufs(e->asb);
  const unsigned n = e->n_ranked, k = e->cycle_considered;
  // ---- the kept matches and Q' (remove-matched-jobs-from-pending-jobs, scheduler.clj:790-795) ------------------------------------------
  unsigned* cnt = b.counters.ensure(2);
  int* matched = b.matched.ensure(n);
  memset_async(e, cnt, 0, 8);
  if (n) memset_async(e, matched, 0, (size_t)n * 4);
  const uint8_t* skipped = p->offer_skipped && e->M ? h2d_opt(e, b.skipped, p->offer_skipped, e->M) : nullptr;
  KM<as_mark_matched, 256>(e, "as_mark_matched", div_up(k, 256), (const uint32_t*)c.result, (const int32_t*)e->m_j2o.ptr(), k, skipped, matched, cnt);
  pinned_copy(e, e->h_scratch, cnt, 4, hipMemcpyDeviceToHost);
  sync(e);
  unsigned m = 0;
  std::memcpy(&m, e->h_scratch, 4);
  const unsigned u = k - m, nq = n - m;
  // ---- N (:1288-1306): max(u, int(min(fraction * scale, 1) * max-jobs)), fraction = (float u) / k ---------------------------------------
  const double fraction = k ? (double)(float)u / (double)k : 0.0;
  const double scaled = std::min(fraction * p->scale_factor, 1.0) * (double)p->max_jobs;
  const unsigned N = std::max<unsigned>(u, scaled > 0.0 ? (unsigned)scaled : 0u);
  // ---- A: the first N jobs of Q' that pass filter-pending-jobs-for-quota under the staged state, fresh rate-limit counters (:1307-1318);
  //      no eligible mask (job-allowed-to-start? and the launch plugin are the considerable path's only, :747-748) -------------------------
  unsigned n_cand = 0;
  if (nq) {
    b.a_cpus.ensure(nq), b.a_mem.ensure(nq), b.a_gpus.ensure(nq), b.a_user.ensure(nq), b.a_rpos.ensure(nq);
    b.scan.ensure(n);
    seg_scan<SumI>(e, "as_queue_scan", LoadUnmatched{matched}, (const uint8_t*)nullptr, n, b.scan.ptr(), e->tmpI);
    KM<as_compact_queue, 256>(e, "as_compact_queue", div_up(n, 256), (const int*)matched, (const SumI*)b.scan.ptr(), n, (const double*)c.q_cpus.ptr(),
        (const double*)c.q_mem.ptr(), (const double*)c.q_gpus.ptr(), (const uint32_t*)c.q_user.ptr(), b.a_cpus.ptr(), b.a_mem.ptr(), b.a_gpus.ptr(),
        b.a_user.ptr(), b.a_rpos.ptr());
    cons_run_device(e, c, b.w, nq, b.a_cpus.ptr(), b.a_mem.ptr(), b.a_gpus.ptr(), b.a_user.ptr(), nullptr, N, LIM_READ);
    n_cand = b.w.n_result;
  }
  // ---- Out: A without the host's excluded tasks, after the take (:1319) ------------------------------------------------------------------
  unsigned n_out = n_cand;
  const uint32_t* out = b.task.ensure(n_cand);
  const bool excl = p->n_exclude && n_cand;
  if (excl) {
    uint8_t* flags = b.excluded.ensure(e->N);
    memset_async(e, flags, 0, e->N);
    h2d(e, b.exclude, p->exclude_task, p->n_exclude);
    KM<as_exclude_flags, 256>(e, "as_exclude_flags", div_up(p->n_exclude, 256), (const uint32_t*)b.exclude.ptr(), (unsigned)p->n_exclude, flags);
    b.keep.ensure(n_cand);
    KM<as_candidate_tasks, 256>(e, "as_candidate_tasks", div_up(n_cand, 256), (const uint32_t*)b.w.result, n_cand, (const uint32_t*)b.a_rpos.ptr(),
        (const uint32_t*)e->ranked.ptr(), (const uint8_t*)flags, b.task.ptr(), b.keep.ptr());
    b.scan.ensure(n_cand);
    seg_scan<SumI>(e, "as_out_scan", LoadI{b.keep.ptr()}, (const uint8_t*)nullptr, n_cand, b.scan.ptr(), e->tmpI);
    KM<as_compact_out, 256>(e, "as_compact_out", div_up(n_cand, 256), (const uint32_t*)b.task.ptr(), (const int*)b.keep.ptr(), (const SumI*)b.scan.ptr(),
        n_cand, b.out.ensure(n_cand), cnt + 1);
    out = b.out.ptr();
    pinned_copy(e, e->h_scratch, cnt + 1, 4, hipMemcpyDeviceToHost);
  } else if (n_cand) {
    KM<as_candidate_tasks, 256>(e, "as_candidate_tasks", div_up(n_cand, 256), (const uint32_t*)b.w.result, n_cand, (const uint32_t*)b.a_rpos.ptr(),
        (const uint32_t*)e->ranked.ptr(), (const uint8_t*)nullptr, b.task.ptr(), (int*)nullptr);
  }
  // ---- the clusters' launch lists (cook_cycle_autoscale_clusters): behind Out on the stream, in the place of Out in the read-back ---------
  const unsigned n_cl = req ? req->cl->n : 0u;
  AsClusterTab tab{};
  if (req) {
    tab.n = n_cl;
    for (unsigned x = 0; x < n_cl; ++x) {
      const int64_t ml = as_max_launchable(req->cl, x);
      tab.location[x] = req->cl->location[x];
      tab.max_launch[x] = ml <= 0 ? 0u : (uint32_t)std::min<int64_t>(ml, 0xFFFFFFFFll);
    }
  }
  if (req && n_cand) {
    const cook_autoscale_clusters* cl = req->cl;
    AsDistOut* dist = b.c_dist.ensure(1);
    memset_async(e, dist, 0, sizeof(AsDistOut));
    const unsigned n_outst = cl->out_off ? cl->out_off[n_cl] : 0u;
    const uint32_t* flags = nullptr;
    if (n_outst) {
      AsOutOff off{};
      for (unsigned x = 0; x <= n_cl; ++x) off.off[x] = cl->out_off[x];
      uint32_t* f = b.c_flags.ensure(e->N);
      memset_async(e, f, 0, (size_t)e->N * 4);
      h2d(e, b.c_out_task, cl->out_task, n_outst);
      KM<as_outstanding_flags, 256>(e, "as_outstanding_flags", div_up(n_outst, 256), off, n_cl, (const uint32_t*)b.c_out_task.ptr(), n_outst, f);
      flags = f;
    }
    const unsigned nb = div_up(n_cand, AS_THREADS);
    const size_t cells = (size_t)(n_cl + 1) * nb;
    b.c_code.ensure(n_cand), b.c_kept.ensure(cells), b.c_head.ensure(cells), b.c_scan.ensure(cells), b.c_launch.ensure(n_cand);
    KM<as_choose_cluster, AS_THREADS>(e, "as_choose_cluster", nb, tab, out, n_cand, excl ? (const unsigned*)(cnt + 1) : (const unsigned*)nullptr,
        (const uint32_t*)e->pend_ord.ptr(), e->min.j_ckpt ? (const uint32_t*)e->j_ckpt.ptr() : (const uint32_t*)nullptr,
        (const int32_t*)e->j_hash.ptr(), flags, nb, b.c_code.ptr(), b.c_kept.ptr(), b.c_head.ptr(), dist);
    seg_scan<SumI>(e, "as_bin_scan", LoadI{b.c_kept.ptr()}, (const uint8_t*)b.c_head.ptr(), (unsigned)cells, b.c_scan.ptr(), e->tmpI);
    KM<as_partition_scatter, AS_THREADS>(e, "as_partition_scatter", nb, tab, out, n_cand, (const uint8_t*)b.c_code.ptr(), (const int*)b.c_kept.ptr(),
        (const SumI*)b.c_scan.ptr(), nb, b.c_launch.ptr(), dist);
    pinned_copy(e, (uint32_t*)e->h_scratch + AS_DIST_AT, dist, sizeof(AsDistOut), hipMemcpyDeviceToHost);
    out = b.c_launch.ptr();
  }
  // |Out| <= |A|: the first min(|A|, cap) entries come back with |Out| in one synchronisation (the launch lists are no longer than Out)
  const unsigned n_copy = std::min(n_cand, cap);
  if (n_copy) copy_async(e, task_idx, out, (size_t)n_copy * 4, hipMemcpyDeviceToHost);
  if (excl || n_copy || (req && n_cand)) sync(e);
  if (excl) std::memcpy(&n_out, e->h_scratch, 4);
  if (info) {
    info->considered = k, info->matched = m, info->unmatched = u, info->scaled = N, info->autoscalable = n_cand, info->n_out = n_out;
    info->fraction_unmatched = fraction;
  }
  if (!req) {
    if (n_out > cap) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: more jobs than cap");
    return;
  }
  AsDistOut h{};
  if (n_cand) std::memcpy(&h, (const uint32_t*)e->h_scratch + AS_DIST_AT, sizeof(AsDistOut));
  req->cluster_off[0] = 0;
  for (unsigned x = 0; x < n_cl; ++x) {
    req->cinfo[x] = cook_autoscale_cluster_info{h.assigned[x], h.outstanding[x], as_max_launchable(req->cl, x), h.launched[x], 0u};
    req->cluster_off[x + 1] = req->cluster_off[x] + h.launched[x];
  }
  if (req->none) {
    *req->none = cook_autoscale_no_cluster{};
    req->none->no_cluster = h.no_cluster;
    req->none->n_first = std::min(h.no_cluster, AS_FIRST_TEN);
    for (unsigned x = 0; x < req->none->n_first; ++x) req->none->first_task[x] = h.first_task[x];
  }
  if (h.total != req->cluster_off[n_cl]) e->fail(COOK_E_STATE, "cook_cycle_autoscale_clusters: the launch lists' lengths do not add up");
  if (h.total > cap) e->fail(COOK_E_INVALID, "cook_cycle_autoscale_clusters: more jobs than cap");
}
