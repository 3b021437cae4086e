// unscheduled_host.hpp — host orchestration of cook_unscheduled (included by engine.hip inside its anonymous namespace).  It reads the
// per-user order of the LAST rank run in place on the device (rank_gather's rows and segments, permB) and the staged users, and changes
// nothing of the rank, considerable or match state: everything it writes lives in UnschedBufs.
// All launches go to the engine's stream after it has drained; one synchronisation at the end.
#pragma once
#include "unscheduled_kernels.hpp"

struct UnschedBufs {
  DArr<SumUL> pre;
  ScanTmp<SumUL> tmp;
  DArr<uint8_t> window;
  DArr<uint32_t> rows, pos, flags, list_len, ahead, reasons, queue_pos;
  DArr<double> run, total, lim[7];
};


void unscheduled_run(cook_engine* e, const cook_unsched_limits* lim, const uint8_t* in_window, const uint32_t* rows, uint32_t n_rows,
                     uint32_t* reasons, uint32_t* queue_pos, double* total, bool total_is_device, uint32_t* ahead, uint32_t* list_len) {
  if (!e->rank_done) e->fail(COOK_E_STATE, "cook_unscheduled before cook_rank_run (or after a stage / cook_cycle_update no rank has followed)");
  const unsigned N = e->N, U = e->U;
  if (total_is_device && !total) e->fail(COOK_E_INVALID, "cook_unscheduled: total_is_device without total");
  if (lim) {
    if (lim->n != U) e->fail(COOK_E_INVALID, "cook_unscheduled: limits.n is not the number of users");
    if (U && (!lim->quota_count || !lim->quota_cpus || !lim->quota_mem || !lim->quota_gpus || !lim->share_cpus || !lim->share_mem || !lim->share_gpus))
      e->fail(COOK_E_INVALID, "cook_unscheduled: a limits array is NULL");
  }
  if (!rows && n_rows != 0 && n_rows != N) e->fail(COOK_E_INVALID, "cook_unscheduled: n_rows without rows is not the number of staged tasks");
  const unsigned n_out = rows ? n_rows : N;
  for (unsigned i = 0; rows && i < n_rows; ++i)
    if (rows[i] >= N) e->fail(COOK_E_INVALID, "cook_unscheduled: a row is not a row of the staged tasks");
  COOK_HIP(hipStreamSynchronize(e->stream));
  UnschedBufs& B = bufs(e->unb);
  UnLimits L;
  if (lim) {
    const double* src[7] = {lim->quota_count, lim->quota_cpus, lim->quota_mem, lim->quota_gpus, lim->share_cpus, lim->share_mem, lim->share_gpus};
    for (int k = 0; k < 7; ++k) h2d(e, B.lim[k], src[k], U);
    L = UnLimits{B.lim[0].ptr(), B.lim[1].ptr(), B.lim[2].ptr(), B.lim[3].ptr(), B.lim[4].ptr(), B.lim[5].ptr(), B.lim[6].ptr()};
  } else {  // the engine's staged cook_users: the DRU divisors are the shares, the quotas as they are
    L = UnLimits{e->u_qcount.ptr(), e->u_qcpus.ptr(), e->u_qmem.ptr(), e->u_qgpus.ptr(), e->u_divc.ptr(), e->u_divm.ptr(), e->u_divg.ptr()};
  }
  uint32_t* d_flags = B.flags.ensure(U);
  uint32_t* d_len = B.list_len.ensure(U);
  uint32_t* d_ahead = B.ahead.ensure((size_t)U * COOK_UNSCHED_AHEAD);
  double* d_run = B.run.ensure((size_t)U * 4);
  const unsigned nblk = std::max(1u, std::min(div_up(U * COOK_UNSCHED_AHEAD, 256), 256u));
  KM<un_init, 256>(e, "un_init", nblk, d_flags, d_len, d_ahead, U, nblk);
  const uint32_t* permB = e->permB;
  const uint8_t* d_window = nullptr;
  const SumUL* pre = nullptr;
  if (N) {  // (rank_run leaves the segments of an empty table as they were: nothing of them is read then)
    d_window = h2d_opt(e, B.window, in_window, N);
    B.pre.ensure(N);
    seg_scan<SumUL>(e, "un_scan", LoadUnsched{e->s_use.ptr(), e->s_pending.ptr(), permB, d_window}, (const uint8_t*)e->head.ptr(), N, B.pre.ptr(),
                    B.tmp);
    pre = B.pre.ptr();
    KM<un_lists, 256>(e, "un_lists", div_up(N, 256), pre, (const uint32_t*)e->s_user.ptr(), (const uint8_t*)e->s_pending.ptr(), permB, d_window,
        (const uint32_t*)e->seg_end.ptr(), N, d_flags, d_len, d_ahead);
  }
  KM<un_user_sums, 64>(e, "un_user_sums", div_up(U, 64), pre, (const SumU4*)e->s_use.ptr(), (const uint8_t*)e->s_pending.ptr(),
      (const uint32_t*)e->seg_start.ptr(), N ? (const uint32_t*)e->seg_end.ptr() : (const uint32_t*)nullptr, (const uint32_t*)d_flags, U, d_run);
  const uint32_t *d_rows = nullptr, *d_pos = nullptr;
  if (rows && n_out) {
    B.pos.ensure(N);
    KM<un_invert, 256>(e, "un_invert", div_up(N, 256), permB, N, B.pos.ptr());
    h2d(e, B.rows, rows, n_out);
    d_rows = B.rows.ptr(), d_pos = B.pos.ptr();
  }
  uint32_t* d_reasons = B.reasons.ensure(n_out);
  uint32_t* d_qpos = B.queue_pos.ensure(n_out);
  double* d_total = total_is_device ? total : B.total.ensure((size_t)n_out * 4);
  KM<un_classify, 256>(e, "un_classify", div_up(n_out, 256), pre, (const SumU4*)e->s_use.ptr(), (const uint8_t*)e->s_pending.ptr(),
      (const uint32_t*)e->s_user.ptr(), permB, d_window, d_rows, d_pos, n_out, (const double*)d_run, (const uint32_t*)d_len, L, d_reasons, d_qpos,
      d_total);
  if (reasons) copy_async(e, reasons, d_reasons, (size_t)n_out * 4, hipMemcpyDeviceToHost);
  if (queue_pos) copy_async(e, queue_pos, d_qpos, (size_t)n_out * 4, hipMemcpyDeviceToHost);
  if (total && !total_is_device) copy_async(e, total, d_total, (size_t)n_out * 4 * sizeof(double), hipMemcpyDeviceToHost);
  if (ahead) copy_async(e, ahead, d_ahead, (size_t)U * COOK_UNSCHED_AHEAD * 4, hipMemcpyDeviceToHost);
  if (list_len) copy_async(e, list_len, d_len, (size_t)U * 4, hipMemcpyDeviceToHost);
  sync(e);
}
