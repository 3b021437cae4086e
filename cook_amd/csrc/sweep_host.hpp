// sweep_host.hpp — host orchestration of cook_sweep_running (included by engine.hip inside its anonymous namespace).
// Stateless: the call uploads its own tables into SweepBufs and touches no rank, considerable, match, offers or rebalance state (the
// radix sort gets a histogram buffer of its own too).  Synchronisations: one to read the three list lengths (the last entry of the
// reason bits' scan) and the error words, one for the result.
#pragma once
#include "sweep_kernels.hpp"

struct SweepBufs {
  DArr<int64_t> start, max_rt, s_start, s_end;
  DArr<uint8_t> unknown, cancelled, type, reason;
  DArr<uint32_t> group, job_count, off, permA, permB, hist, out;
  DArr<double> quantile, multiplier, thr;
  DArr<int> gsel;
  DArr<uint64_t> key;
  DArr<SumI3> scan;
  ScanTmp<SumI3> tmp;
  DArr<unsigned> ctl;
};


void sweep_running(cook_engine* e, const cook_running_set* tasks, const cook_straggler_groups* groups, const cook_sweep_params* p,
                   uint8_t* reason, uint32_t* idx, uint32_t cap, double* group_threshold_s, cook_sweep_info* info) {
  // ---- arguments ---------------------------------------------------------------------------------------------------------------
  if (!tasks || !p) e->fail(COOK_E_INVALID, "cook_sweep_running: null tasks or params");
  const unsigned what = p->what;
  if (what & ~7u) e->fail(COOK_E_INVALID, "cook_sweep_running: unknown bits in what");
  const unsigned n = tasks->n;
  if (n > (unsigned)INT32_MAX) e->fail(COOK_E_INVALID, "cook_sweep_running: n > INT32_MAX");
  if (n && (what & 3u) && !tasks->start_ms) e->fail(COOK_E_INVALID, "cook_sweep_running: start_ms is needed for lingering and stragglers");
  if ((what & 1u) && (p->default_timeout_ms < 0 || p->max_timeout_ms < 0)) e->fail(COOK_E_INVALID, "cook_sweep_running: negative timeout");
  if (cap && !idx) e->fail(COOK_E_INVALID, "cook_sweep_running: null idx");
  const bool strag = (what & 2u) != 0;
  if (strag && !groups) e->fail(COOK_E_INVALID, "cook_sweep_running: stragglers need the groups");
  const unsigned G = strag ? groups->n : 0u;
  unsigned NS = 0;
  if (G) {
    if (!groups->type || !groups->quantile || !groups->multiplier || !groups->job_count || !groups->succ_off)
      e->fail(COOK_E_INVALID, "cook_sweep_running: the groups need type, quantile, multiplier, job_count and succ_off");
    if (groups->succ_off[0] != 0u) e->fail(COOK_E_INVALID, "cook_sweep_running: succ_off[0] != 0");
    NS = groups->succ_off[G];
    if (NS > (unsigned)INT32_MAX) e->fail(COOK_E_INVALID, "cook_sweep_running: more than INT32_MAX successful instances");
    if (NS && (!groups->succ_start_ms || !groups->succ_end_ms)) e->fail(COOK_E_INVALID, "cook_sweep_running: succ_start_ms / succ_end_ms missing");
  }
  SweepBufs& b = bufs(e->swb);
  unsigned* ctl = b.ctl.ensure(SW_CTL_WORDS);
  memset_async(e, ctl, 0, SW_CTL_WORDS * 4);
  memset_async(e, ctl + SW_BAD_ROW, 0xFF, 8);  // SW_BAD_ROW, SW_BAD_SUCC = COOK_NONE_U32
  static_assert(SW_BAD_SUCC == SW_BAD_ROW + 1, "the two minima are adjacent");
  const SweepTimes t{p->now_ms, p->default_timeout_ms, p->max_timeout_ms};
  // ---- uploads: only the columns of the killers that run -------------------------------------------------------------------------
  const int64_t* d_start = n && (what & 3u) ? (h2d(e, b.start, tasks->start_ms, n), b.start.ptr()) : nullptr;
  const int64_t* d_maxrt = n && (what & 1u) ? h2d_opt(e, b.max_rt, tasks->max_runtime_ms, n) : nullptr;
  const uint8_t* d_unknown = n && strag ? h2d_opt(e, b.unknown, tasks->unknown, n) : nullptr;
  const uint32_t* d_group = n && strag ? h2d_opt(e, b.group, tasks->group, n) : nullptr;
  const uint8_t* d_cancelled = n && (what & 4u) ? h2d_opt(e, b.cancelled, tasks->cancelled, n) : nullptr;
  int* gsel = b.gsel.ensure(G);
  double* thr = b.thr.ensure(G);
  // ---- straggler groups: readiness, the sorted s of the ready ones, thresholds (find-stragglers, group.clj:17-44) -------------------
  if (G) {
    h2d(e, b.type, groups->type, G);
    h2d(e, b.quantile, groups->quantile, G);
    h2d(e, b.multiplier, groups->multiplier, G);
    h2d(e, b.job_count, groups->job_count, G);
    h2d(e, b.off, groups->succ_off, (size_t)G + 1);
    KM<sw_groups, 256>(e, "sweep_groups", div_up(G, 256), (const uint8_t*)b.type.ptr(), (const double*)b.quantile.ptr(),
                       (const double*)b.multiplier.ptr(), (const uint32_t*)b.job_count.ptr(), (const uint32_t*)b.off.ptr(), G, NS, gsel, thr, ctl);
    if (NS) {
      h2d(e, b.s_start, groups->succ_start_ms, NS);
      h2d(e, b.s_end, groups->succ_end_ms, NS);
      uint64_t* key = b.key.ensure(NS);
      KM<sw_keys, 256>(e, "sweep_keys", div_up(NS, 256), (const uint32_t*)b.off.ptr(), G, NS, (const int64_t*)b.s_start.ptr(),
                       (const int64_t*)b.s_end.ptr(), p->now_ms, (const int*)gsel, key, ctl);
      // (g, s) keys: the 31 bits of s and as many group bits as G - 1 has.  Which of them vary is not read back (it would cost a third
      // synchronisation); digits of the mask's gap cost nothing all the same.
      const unsigned gbits = G > 1 ? 64u - (unsigned)__builtin_clzll((unsigned long long)(G - 1)) : 0u;
      const unsigned long long mask = ((1ull << SW_S_BITS) - 1ull) | (((1ull << gbits) - 1ull) << SW_S_BITS);
      const uint32_t* perm = radix_sort_masked(e, key, mask, nullptr, b.permA.ensure(NS), b.permB.ensure(NS), NS, &b.hist);
      KM<sw_select, 256>(e, "sweep_select", div_up(G, 256), (const int*)gsel, (const uint32_t*)b.off.ptr(), perm, (const uint64_t*)key,
                         (const double*)b.multiplier.ptr(), G, thr);
    }
  }
  // ---- the three killers per row ---------------------------------------------------------------------------------------------------
  uint8_t* d_reason = b.reason.ensure(n);
  KM<sw_rows, 256>(e, "sweep_rows", div_up(n, 256), d_start, d_unknown, d_maxrt, d_cancelled, d_group, n, what, t, (const int*)gsel,
                   (const double*)thr, G, d_reason, ctl);
  SumI3* incl = b.scan.ensure(n);
  seg_scan<SumI3>(e, "sweep_scan", LoadReason3{d_reason}, (const uint8_t*)nullptr, n, incl, b.tmp);
  pinned_copy(e, e->h_scratch, ctl, SW_CTL_WORDS * 4, hipMemcpyDeviceToHost);
  if (n) pinned_copy(e, e->h_scratch + 2, incl + (n - 1), sizeof(SumI3), hipMemcpyDeviceToHost);
  sync(e);
  unsigned c[SW_CTL_WORDS];
  SumI3 len = SumI3::zero();
  std::memcpy(c, e->h_scratch, sizeof(c));
  if (n) std::memcpy(&len, e->h_scratch + 2, sizeof(len));
  const unsigned L = (unsigned)len.v[0], S = (unsigned)len.v[1], Cn = (unsigned)len.v[2];
  const unsigned bad = c[SW_BAD_ROW] != COOK_NONE_U32 ? c[SW_BAD_ROW] : c[SW_BAD_SUCC] != COOK_NONE_U32 ? n + c[SW_BAD_SUCC] : COOK_NONE_U32;
  if (info) *info = cook_sweep_info{L, S, Cn, c[SW_READY], bad};
  if (c[SW_ERR] & SW_ERR_OFF) e->fail(COOK_E_INVALID, "cook_sweep_running: succ_off decreases");
  if (c[SW_ERR] & SW_ERR_GROUP)
    e->fail(COOK_E_INVALID, "cook_sweep_running: a group of type > 1, or of type 1 with quantile outside (0, 1), multiplier <= 1 or not "
                            "finite, or job_count > INT32_MAX");
  if (c[SW_BAD_ROW] != COOK_NONE_U32)
    e->fail(COOK_E_INVALID, "cook_sweep_running: running row " + std::to_string(c[SW_BAD_ROW]) +
                                ": group index out of range, or no start time / an interval outside 0 .. INT32_MAX s in a ready group");
  if (c[SW_BAD_SUCC] != COOK_NONE_U32)
    e->fail(COOK_E_INVALID, "cook_sweep_running: successful instance " + std::to_string(c[SW_BAD_SUCC]) +
                                " of a ready group: no start time, or an interval outside 0 .. INT32_MAX s");
  const uint64_t total = (uint64_t)L + S + Cn;
  if (total > cap) e->fail(COOK_E_INVALID, "cook_sweep_running: the lists hold more than cap entries");
  // ---- lingering ++ stragglers ++ cancelled ------------------------------------------------------------------------------------------
  if (total) {
    KM<sw_scatter, 256>(e, "sweep_scatter", div_up(n, 256), (const uint8_t*)d_reason, (const SumI3*)incl, n, L, L + S, b.out.ensure(total));
    copy_async(e, idx, b.out.ptr(), (size_t)total * 4, hipMemcpyDeviceToHost);
  }
  if (reason && n) copy_async(e, reason, d_reason, n, hipMemcpyDeviceToHost);
  if (group_threshold_s && G) copy_async(e, group_threshold_s, thr, (size_t)G * 8, hipMemcpyDeviceToHost);
  if (group_threshold_s && groups && !strag)  // (the straggler killer does not run: no group is evaluated)
    for (unsigned g = 0; g < groups->n; ++g) group_threshold_s[g] = __builtin_nan("");
  sync(e);
}
