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
};


void cycle_autoscale(cook_engine* e, const cook_autoscale_params* p, uint32_t* task_idx, uint32_t cap, cook_autoscale_info* info) {
  if (!p) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: null params");
  if (!e->cycle_cons_ran || !e->rank_done || !e->match_ran() || !e->cb)
    e->fail(COOK_E_STATE, "cook_cycle_autoscale needs the last cook_cycle_run (or cook_cycle_run_rank + cook_cycle_match_multi) to have run the "
                          "considerable filters, with no stage / cook_cycle_update / cook_considerable since");
  if (!std::isfinite(p->scale_factor)) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: scale_factor is not finite");
  if (p->max_jobs > (uint32_t)INT32_MAX) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: max_jobs > INT32_MAX");
  if (p->n_exclude && !p->exclude_task) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: n_exclude without exclude_task");
  for (uint32_t x = 0; x < p->n_exclude; ++x)
    if (p->exclude_task[x] >= e->N) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: exclude_task index out of range");
  if (cap && !task_idx) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: null task_idx");
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
  // |Out| <= |A|: the first min(|A|, cap) entries come back with |Out| in one synchronisation
  const unsigned n_copy = std::min(n_cand, cap);
  if (n_copy) copy_async(e, task_idx, out, (size_t)n_copy * 4, hipMemcpyDeviceToHost);
  if (excl || n_copy) sync(e);
  if (excl) std::memcpy(&n_out, e->h_scratch, 4);
  if (info) {
    info->considered = k, info->matched = m, info->unmatched = u, info->scaled = N, info->autoscalable = n_cand, info->n_out = n_out;
    info->fraction_unmatched = fraction;
  }
  if (n_out > cap) e->fail(COOK_E_INVALID, "cook_cycle_autoscale: more jobs than cap");
}
