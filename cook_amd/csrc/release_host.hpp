// release_host.hpp — host orchestration of the release (cook_cycle_run_queue_release*, cookmatch.h).  Included by
// engine.hip inside its anonymous namespace, behind carry_host.hpp (SegSort, host_rows, CarryBufs' column sets); queue_host.hpp calls
// release_check from queue_check_step and release_enqueue / release_finish from queue_advance.  Everything is enqueued on the advance's
// stream behind the carry and the groups' fold; what the host reads back — three counters behind the advance's two, and the pool's four
// sums — rides in the advance's one synchronisation.
#pragma once
#include <cmath>

#include "release_kernels.hpp"

struct ReleaseBufs {
  // the list on the device
  DArr<uint32_t> host, user, group, gpu_model, disk_type;
  DArr<double> cpus, mem, gpus, disk_req, scal[3];
  DArr<int32_t> ports;
  DArr<uint64_t> okey, ukey, gkey;
  SegSort o, u, g;
  DArr<double> pool;  // {count, cpus, mem, gpus} of all entries
  // the groups' table behind a release, two of them: a release reads the table in use (staged, folded, or the other one of these) and
  // writes the one the last match cannot have read
  DArr<uint8_t> claimed;
  DArr<SumI> scan;
  DArr<uint32_t> t_off[2], t_host[2], t_attr[2];
  unsigned tcur = 0;
  cook_release_info info{};    // of the last queue cycle
  bool pending = false;        // this advance reads the release's counters back
  bool pool_pending = false;   // ... and the pool's sums
  unsigned n_row_entries = 0;  // entries the device looked a row up for / a cotask (the host counts them: the list is short)
  unsigned n_group_entries = 0;
};

// the read-back slots of carry_host.hpp, now that every size is known
static_assert(Q_H_ADVANCE + 1 <= Q_H_CARRY_POOL && Q_H_CARRY_POOL + 4 <= REL_H_CNT && REL_H_CNT + (REL_CNT_WORDS + 1) / 2 <= REL_H_POOL && REL_H_POOL + 4 <= 64,
              "the queue advance's read-backs overlap in h_scratch");

static bool release_active(const cook_finished* f) { return f && f->n && (f->offers || f->usage || f->groups); }

// what can refuse a release, before anything changes (queue_check_step)
void release_check(cook_engine* e, const QueueArgs& q) {
  const cook_queue_step* s = q.step;
  const cook_finished* f = q.finished;
  if (!f) return;
  if (f->offers > 1u || f->usage > 1u || f->groups > 1u) e->fail(COOK_E_INVALID, "cook_finished: offers / usage / groups are 0 or 1");
  if (!release_active(f)) return;
  if (f->offers && s && s->offers)
    e->fail(COOK_E_INVALID, "cook_finished: offers = 1 releases into the STAGED offers; step->offers replaces them (one or the other)");
  if (f->groups && s && s->groups)
    e->fail(COOK_E_INVALID, "cook_finished: groups = 1 releases from the groups' table on the device; step->groups replaces it (one or the other)");
  if (f->offers && e->min.host_dup) e->fail(COOK_E_INVALID, "cook_finished: offers = 1, but two staged offers are on one host");
  if (!f->host || !f->cpus || !f->mem) e->fail(COOK_E_INVALID, "cook_finished needs host, cpus and mem");
  if (f->scalars && f->n_scalars > COOK_MAX_SCALARS) e->fail(COOK_E_INVALID, "cook_finished: more than COOK_MAX_SCALARS named scalars");
  const bool staged = e->cb && e->cb->cycle_on && e->cb->users_staged;
  if (f->usage && !staged) e->fail(COOK_E_STATE, "cook_finished: usage = 1 needs a user state staged by cook_cycle_set_considerable");
  if (f->usage && !f->user) e->fail(COOK_E_INVALID, "cook_finished: usage = 1 needs user");
  const unsigned n = f->n, U = f->usage ? e->cb->U : 0u, G = e->G;
  auto amount = [&](double x) { return x >= 0.0 && std::isfinite(x); };  // (false for NaN)
  for (unsigned t = 0; t < n; ++t) {
    if (!amount(f->cpus[t]) || !amount(f->mem[t]) || (f->gpus && !amount(f->gpus[t])))
      e->fail(COOK_E_INVALID, "cook_finished: cpus / mem / gpus must be finite and not negative");
    if (f->disk_request && !std::isfinite(f->disk_request[t])) e->fail(COOK_E_INVALID, "cook_finished: disk_request must be finite");
    if (f->usage && f->user[t] >= U) e->fail(COOK_E_INVALID, "cook_finished: user id out of range");
    if (f->group && f->group[t] != COOK_NONE_U32 && f->group[t] >= G) e->fail(COOK_E_INVALID, "cook_finished: group id out of range");
  }
  if (f->scalars)
    for (size_t x = 0; x < (size_t)f->n_scalars * n; ++x) {
      const double r = f->scalars[x];
      if (r == r && !amount(r)) e->fail(COOK_E_INVALID, "cook_finished: a named scalar must be NaN (none) or finite and not negative");
    }
}

// Inside queue_advance, behind the carry and the groups' fold (so: over the columns and the table the NEXT match reads), also when the
// last cycle considered nothing.  cnt: QueueBufs::counters, REL_CNT_WORDS words, zero on the stream; carried: the carry of this advance
// has just written a fresh set of offer columns (min.o_* point at it); fold_rows: an upper bound of the rows this advance's fold
// appended to the groups' table (the exact count is only on the device until the synchronisation).
void release_enqueue(cook_engine* e, const cook_finished* f, unsigned* cnt, bool carried, unsigned fold_rows) {
  ReleaseBufs& b = bufs(e->rlb);
  b.info = cook_release_info{};
  b.pending = b.pool_pending = false;
  b.n_row_entries = b.n_group_entries = 0;
  if (!release_active(f)) return;
  MatchIn& in = e->min;
  const unsigned n = f->n, M = e->M, G = e->G;
  const bool offers = f->offers && M, usage = f->usage && e->cb->U;
  const unsigned U = usage ? e->cb->U : 0u;
  unsigned n_ge = 0;
  if (f->groups && f->group)
    for (unsigned t = 0; t < n; ++t) n_ge += f->group[t] != COOK_NONE_U32 ? 1u : 0u;
  const unsigned rows_max = e->cf_group_run_total + fold_rows;
  const bool groups = n_ge && G && in.g_run_off && in.g_run_host && rows_max;
  if (f->offers && !offers) b.info.without_row = n;   // no staged offers: no entry has a row
  if (n_ge && !groups) b.info.cotasks_missing = n_ge;  // no running cotasks at all: every entry misses
  if (!offers && !usage && !groups) return;
  b.pending = true;
  b.n_row_entries = offers ? n : 0u;
  b.n_group_entries = groups ? n_ge : 0u;
  // ---- the list (read until the advance's synchronisation) -----------------------------------------------------------------------------
  ReleaseList l{};
  l.host = h2d_opt(e, b.host, f->host, n);
  l.cpus = h2d_opt(e, b.cpus, f->cpus, n), l.mem = h2d_opt(e, b.mem, f->mem, n);
  if (offers || usage) l.gpus = h2d_opt(e, b.gpus, f->gpus, n);
  if (usage) l.user = h2d_opt(e, b.user, f->user, n);
  if (groups) l.group = h2d_opt(e, b.group, f->group, n);
  if (offers) {
    l.ports = h2d_opt(e, b.ports, f->ports, n);
    l.gpu_model = h2d_opt(e, b.gpu_model, f->gpu_model, n);
    l.disk_req = h2d_opt(e, b.disk_req, f->disk_request, n);
    l.disk_type = h2d_opt(e, b.disk_type, f->disk_type, n);
    for (unsigned s = 0; s < 3u; ++s)
      l.scal[s] = (f->scalars && s < f->n_scalars) ? h2d_opt(e, b.scal[s], f->scalars + (size_t)s * n, n) : nullptr;
  }
  const CarryJobs rows = l.rows();
  // ---- keys ---------------------------------------------------------------------------------------------------------------------------
  unsigned n_hosts = 0;
  const uint32_t* h2row = offers ? host_rows(e, n_hosts) : nullptr;  // (null: release_keys looks the host up in o_host)
  uint64_t* okey = offers ? b.okey.ensure(n) : nullptr;
  uint64_t* ukey = usage ? b.ukey.ensure(n) : nullptr;
  uint64_t* gkey = groups ? b.gkey.ensure(n) : nullptr;
  KM<release_keys, 256>(e, "release_keys", div_up(n, 256), l, n, h2row, n_hosts, in.o_host, offers ? M : 0u, U, groups ? G : 0u, okey, ukey, gkey, cnt);
  // ---- offers -------------------------------------------------------------------------------------------------------------------------
  if (offers) {
    const uint32_t* perm = b.o.carry_segments(e, okey, n, M);
    CarryBufs& cy = bufs(e->cyb);
    // behind a carry of this advance: its fresh set, in place (one wave owns one row); else a fresh set of its own, every row written
    CarryOfferIn ci;
    CarryOfferCols co;
    const OfferCols<true> out = carry_offer_cols(in, M, cy.cols[carried ? cy.cur : (cy.cur ^ 1u)], ci, co);
    KM<fold_offers<true>, FOLD_OT>(e, "release_fold_offers", M, perm, (const uint32_t*)b.o.start.ptr(), (const uint32_t*)b.o.end.ptr(), M,
        carried ? 0u : 1u, rows, ci, co, cnt + REL_CNT_CLAMPED);
    if (!carried) cy.cur ^= 1u;
    offer_cols_stage(in, out, offer_dims(in), M, true);
  }
  // ---- the users and the pool ----------------------------------------------------------------------------------------------------------
  if (usage) {
    ConsBufs& cb = *e->cb;
    const uint32_t* perm = b.u.carry_segments(e, ukey, n, U);
    KM<fold_users<true, RowsSorted>, FOLD_UT>(e, "release_fold_users", U, RowsSorted{perm, rows}, (const uint32_t*)b.u.start.ptr(),
        (const uint32_t*)b.u.end.ptr(), U, cb.ucount.ptr(), cb.ucpus.ptr(), cb.umem.ptr(), cb.ugpus.ptr(), (int64_t*)nullptr);
    if (cb.pool_usage_given) {
      KM<fold_pool<true, RowsSorted>, FOLD_UT>(e, "release_fold_pool", 1, RowsSorted{nullptr, rows}, n, b.pool.ensure(4));
      pinned_copy(e, e->h_scratch + REL_H_POOL, b.pool.ptr(), 32, hipMemcpyDeviceToHost);
      b.pool_pending = true;
    }
  }
  // ---- the groups: mark, scan, compact into a table the last match did not read ----------------------------------------------------------
  if (groups) {
    const uint32_t* perm = b.g.carry_segments(e, gkey, n, G);
    uint8_t* claimed = b.claimed.ensure(rows_max);
    memset_async(e, claimed, 0, rows_max);
    KM<release_group_mark, COOK_WAVE>(e, "release_group_mark", G, perm, (const uint32_t*)b.g.start.ptr(), (const uint32_t*)b.g.end.ptr(), G, l.host,
        in.g_run_off, in.g_run_host, rows_max, claimed, cnt);
    const unsigned nx = b.tcur ^ 1u;  // (the table in use, and the one the last match read, may be t_*[tcur]; never t_*[tcur ^ 1])
    uint32_t* n_off = b.t_off[nx].ensure(G + 1);
    uint32_t* n_host = b.t_host[nx].ensure(rows_max);
    uint32_t* n_attr = b.t_attr[nx].ensure(rows_max);
    SumI* incl = b.scan.ensure(rows_max);
    const uint32_t* n_rows = in.g_run_off + G;
    seg_scan<SumI>(e, "release_group_scan", LoadUnclaimed{claimed, n_rows}, (const uint8_t*)nullptr, rows_max, incl, e->tmpI);
    KM<release_group_offsets, 256>(e, "release_group_offsets", div_up(G + 1, 256), (const SumI*)incl, in.g_run_off, G, n_off);
    KM<release_group_compact, 256>(e, "release_group_compact", div_up(rows_max, 256), (const uint8_t*)claimed, (const SumI*)incl, n_rows, rows_max,
        in.g_run_host, in.g_run_attr, n_host, n_attr);
    b.tcur = nx;
    groups_install(e, n_off, n_host, n_attr);
  }
}

// behind the advance's synchronisation (and behind carry_finish: the pool usage grows by the carry first); h: the advance's counters
void release_finish(cook_engine* e, const unsigned* h) {
  if (!e->rlb || !e->rlb->pending) return;
  ReleaseBufs& b = *e->rlb;
  b.pending = false;
  if (b.n_row_entries) {
    b.info.without_row = h[REL_CNT_NO_ROW];
    b.info.with_row = b.n_row_entries - b.info.without_row;
    b.info.counts_clamped = h[REL_CNT_CLAMPED];
  }
  if (b.n_group_entries) {
    b.info.cotasks_missing = h[REL_CNT_MISSING];
    b.info.cotasks_removed = b.n_group_entries - b.info.cotasks_missing;
    e->cf_group_run_total -= b.info.cotasks_removed;
  }
  if (b.pool_pending) {
    b.pool_pending = false;
    double s[4];
    std::memcpy(s, e->h_scratch + REL_H_POOL, 32);
    cook_usage& p = e->cb->pool_usage;
    p.count = p.count - s[0], p.cpus = p.cpus - s[1], p.mem = p.mem - s[2], p.gpus = p.gpus - s[3];
  }
}
