// launch_res_host.hpp — host orchestration of cook_match_launch_resources (cookmatch.h, "LAUNCH RESOURCES").  Included by
// engine.hip inside its anonymous namespace, behind carry_host.hpp, whose key / sort / bounds step (carry_keys, SegSort) it reuses as it
// is.  It reads the result of the LAST match in place on the device, as explain_host.hpp does (job_to_offer, the staged job columns
// through the match's j_index), and writes only LaunchBufs and the caller's memory.  Two synchronisations: everything but the ports'
// expansion runs in front of the first, which brings the control block (the lowest bad row, the totals) — a call that fails has written
// nothing; the expansion (sized by the total just read), the copies and the second follow.
#pragma once
#include "launch_res_kernels.hpp"

struct LaunchBufs {
  DArr<uint64_t> okey;
  SegSort seg;
  DArr<uint8_t> skipped, range_role, head_p, port_role;
  DArr<uint32_t> range_off, ports_p, ports_k, port_off, short_mask;
  DArr<int32_t> range_begin, range_end, port;
  DArr<double> avail, req_p, take;
  DArr<unsigned long long> range_pre, row_ports, cursor;
  DArr<SumU64> incl_p, incl_k;
  DArr<unsigned> ctl;
  ScanTmp<SumU64> tmp;
};

void launch_resources(cook_engine* e, const cook_launch_offers* o, cook_launch_out* out, cook_launch_info* info) {
  const char* who = "cook_match_launch_resources";
  if (!info) e->fail(COOK_E_INVALID, std::string(who) + ": null info");
  *info = cook_launch_info{};
  info->bad_row = COOK_NONE_U32;
  if (!o || !out) e->fail(COOK_E_INVALID, std::string(who) + ": null offers / out");
  if (!e->match_ran() || !e->last_in_valid)
    e->fail(COOK_E_STATE, std::string(who) + " before a match ran (or behind a Kubernetes-scheduler cycle: no placement ran)");
  const MatchIn in = e->last_in;
  const unsigned K = in.K, M = in.M;
  if (o->n != M) e->fail(COOK_E_INVALID, std::string(who) + ": offers->n is not the offer count of the last match");
  if (o->n_roles < 1u || o->n_roles > (unsigned)COOK_MAX_ROLES) e->fail(COOK_E_INVALID, std::string(who) + ": n_roles is 1 .. COOK_MAX_ROLES");
  if (o->n_res < 1u || o->n_res > LR_MAX_RES) e->fail(COOK_E_INVALID, std::string(who) + ": n_res is 1 .. 2 + COOK_MAX_SCALARS");
  if (!o->range_off || !o->res_source || (M && !o->avail)) e->fail(COOK_E_INVALID, std::string(who) + ": null range_off / res_source / avail");
  if (!out->port_off || (K && (!out->take || !out->short_mask)) || (out->cap && (!out->port || !out->port_role)))
    e->fail(COOK_E_INVALID, std::string(who) + ": a null output array");
  const unsigned n_roles = o->n_roles, n_res = o->n_res;
  LrJobs J{};
  J.j_index = in.j_index, J.ports = in.j_ports;
  for (unsigned r = 0; r < n_res; ++r) {
    const uint32_t s = o->res_source[r];
    if (s == (uint32_t)COOK_LAUNCH_CPUS) J.col[r] = in.j_cpus;
    else if (s == (uint32_t)COOK_LAUNCH_MEM) J.col[r] = in.j_mem;
    else if (s - (uint32_t)COOK_LAUNCH_SCALAR0 < in.n_scal && s >= (uint32_t)COOK_LAUNCH_SCALAR0) J.col[r] = in.j_scal[s - COOK_LAUNCH_SCALAR0];
    else e->fail(COOK_E_INVALID, std::string(who) + ": a res_source names no column, or a scalar the match did not have");
  }
  if (o->range_off[0] != 0u) e->fail(COOK_E_INVALID, std::string(who) + ": range_off does not start at 0");
  for (unsigned v = 0; v < M; ++v)
    if (o->range_off[v + 1] < o->range_off[v]) e->fail(COOK_E_INVALID, std::string(who) + ": range_off decreases");
  const unsigned NR = o->range_off[M];
  if (NR && (!o->range_begin || !o->range_end || !o->range_role)) e->fail(COOK_E_INVALID, std::string(who) + ": null range arrays");

  // ---- every buffer before the first launch
  LaunchBufs& b = bufs(e->lrb);
  unsigned* ctl = b.ctl.ensure(LR_CTL_WORDS);
  uint64_t* okey = b.okey.ensure(K);
  b.ports_p.ensure(K), b.ports_k.ensure(K), b.head_p.ensure(K), b.incl_p.ensure(K), b.incl_k.ensure(K), b.cursor.ensure(K);
  b.req_p.ensure((size_t)K * n_res);
  uint32_t* port_off = b.port_off.ensure((size_t)K + 1);
  double* take = b.take.ensure((size_t)K * n_res * n_roles);
  uint32_t* short_mask = b.short_mask.ensure(K);
  b.range_pre.ensure(NR), b.row_ports.ensure(M);
  b.range_off.ensure((size_t)M + 1), b.range_begin.ensure(NR), b.range_end.ensure(NR), b.range_role.ensure(NR);
  b.avail.ensure((size_t)n_res * n_roles * M);
  b.seg.permA.ensure(K), b.seg.permB.ensure(K), b.seg.start.ensure(M), b.seg.end.ensure(M);

  // ---- the role view, the keys, the segments
  h2d(e, b.range_off, o->range_off, (size_t)M + 1);
  h2d(e, b.range_begin, o->range_begin, NR);
  h2d(e, b.range_end, o->range_end, NR);
  h2d(e, b.range_role, o->range_role, NR);
  h2d(e, b.avail, o->avail, (size_t)n_res * n_roles * M);
  const uint8_t* skipped = (M && K) ? h2d_opt(e, b.skipped, o->offer_skipped, M) : nullptr;
  const LrRows R{M, n_roles, n_res, b.range_off.ptr(), b.range_begin.ptr(), b.range_end.ptr(), b.range_role.ptr(), b.avail.ptr()};
  memset_async(e, ctl, 0, LR_CTL_WORDS * 4);
  memset_async(e, ctl + LR_BAD_ROW, 0xFF, 4);
  memset_async(e, port_off, 0, ((size_t)K + 1) * 4);
  memset_async(e, take, 0, (size_t)K * n_res * n_roles * sizeof(double));
  memset_async(e, short_mask, 0, (size_t)K * 4);
  const int32_t* j2o = e->m_j2o.ptr();
  const unsigned gK = div_up(K, 256);
  KM<carry_keys, 256>(e, "carry_keys", gK, j2o, K, skipped, (const uint32_t*)in.j_index, (const uint32_t*)nullptr, M, 0u, okey, (uint64_t*)nullptr);
  const uint32_t* perm = b.seg.carry_segments(e, okey, K, M);
  const uint32_t *seg_start = b.seg.start.ptr(), *seg_end = b.seg.end.ptr();
  KM<lr_check_rows, COOK_WAVE>(e, "lr_check_rows", M, R, seg_start, seg_end, b.range_pre.ptr(), b.row_ports.ptr(), ctl);
  // ---- ports per task, the cursors, the offsets
  KM<lr_gather, 256>(e, "lr_gather", gK, perm, (const uint64_t*)okey, K, M, n_res, J, b.ports_p.ptr(), b.head_p.ptr(), b.req_p.ptr(), b.ports_k.ptr(), ctl);
  seg_scan<SumU64>(e, "lr_cursor_scan", LoadLrPorts{b.ports_p.ptr()}, (const uint8_t*)b.head_p.ptr(), K, b.incl_p.ptr(), b.tmp);
  seg_scan<SumU64>(e, "lr_offset_scan", LoadLrPorts{b.ports_k.ptr()}, (const uint8_t*)nullptr, K, b.incl_k.ptr(), b.tmp);
  KM<lr_cursors, 256>(e, "lr_cursors", gK, perm, (const uint64_t*)okey, K, M, (const uint32_t*)b.ports_p.ptr(), (const SumU64*)b.incl_p.ptr(),
      (const uint32_t*)b.ports_k.ptr(), (const SumU64*)b.incl_k.ptr(), seg_end, (const unsigned long long*)b.row_ports.ptr(), b.cursor.ptr(), port_off, ctl);
  // ---- the takes: a chain per (offer, slot)
  if (K) {
    KM<lr_take_chains, 64>(e, "lr_take_chains", div_up(M * n_res, 64), R, perm, seg_start, seg_end, K, (const double*)b.req_p.ptr(), take, short_mask);
    KM<lr_count_short, 256>(e, "lr_count_short", gK, (const uint32_t*)short_mask, K, ctl);
  }
  pinned_copy(e, e->h_scratch, ctl, LR_CTL_WORDS * 4, hipMemcpyDeviceToHost);
  sync(e);
  unsigned h[LR_CTL_WORDS];
  std::memcpy(h, e->h_scratch, sizeof(h));
  if (h[LR_BAD_ROW] != LR_NONE) {
    info->bad_row = h[LR_BAD_ROW];
    e->fail(COOK_E_INVALID, std::string(who) + ": row " + std::to_string(h[LR_BAD_ROW]) +
                                ": ranges that overlap or are not 0 <= begin <= end, a role out of range, an amount that is not finite and >= 0, "
                                "or kept tasks that ask for more ports than the ranges hold");
  }
  const unsigned long long total64 = ((unsigned long long)h[LR_PORTS_HI] << 32) | (unsigned long long)h[LR_PORTS_LO];
  info->kept = h[LR_KEPT], info->offers_used = h[LR_OFFERS_USED], info->short_tasks = h[LR_SHORT];
  info->ports = total64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)total64;
  if (total64 > (unsigned long long)out->cap) e->fail(COOK_E_INVALID, std::string(who) + ": out->cap is less than the ports of the kept tasks (info->ports)");
  const unsigned total = (unsigned)total64;
  // ---- the ports, each at its place; the copies
  if (total) {
    int32_t* port = b.port.ensure(total);
    uint8_t* port_role = b.port_role.ensure(total);
    KM<lr_emit_ports, 256>(e, "lr_emit_ports", div_up(total, 256), R, j2o, (const uint32_t*)port_off, K, total, (const unsigned long long*)b.cursor.ptr(),
        (const unsigned long long*)b.range_pre.ptr(), port, port_role, ctl);
    pinned_copy(e, e->h_scratch, ctl + LR_BROKEN, 4, hipMemcpyDeviceToHost);
    copy_async(e, out->port, port, (size_t)total * 4, hipMemcpyDeviceToHost);
    copy_async(e, out->port_role, port_role, (size_t)total, hipMemcpyDeviceToHost);
  }
  copy_async(e, out->port_off, port_off, ((size_t)K + 1) * 4, hipMemcpyDeviceToHost);
  copy_async(e, out->take, take, (size_t)K * n_res * n_roles * sizeof(double), hipMemcpyDeviceToHost);
  copy_async(e, out->short_mask, short_mask, (size_t)K * 4, hipMemcpyDeviceToHost);
  sync(e);
  unsigned broken = 0;
  if (total) std::memcpy(&broken, e->h_scratch, 4);
  if (broken)  // (the outputs have been copied by now: the one failure of this call that is not all-or-nothing, and none an input can cause)
    e->fail(COOK_E_STATE, std::string(who) + ": internal inconsistency while the ports were written (" + std::to_string(broken) + "); the outputs are not valid");
}
