// reserve_host.hpp — host orchestration of the rebalancer's host reservations (cook_cycle_set_reservations,
// cook_cycle_run_queue_reserve*, cook_cycle_fetch_reservations, cookmatch.h).  Included by engine.hip inside its
// anonymous namespace, behind churn_host.hpp; queue_host.hpp calls reserve_check from queue_check_step and reserve_enqueue /
// reserve_finish from queue_advance.  The state is the reference's atom per engine: a reservation list, an engine-owned
// j_reserved_host column over the staged pending rows, a bitmap rebuilt from the live list, a byte per pending row (`launched`).
// The column and the bitmap are what a match reads, so there are two sets of them: cook_cycle_set_reservations, which may be called
// between a match and the cook_match_explain / cook_match_metrics that describe it, writes the set the last match did NOT read
// (a copy of the column first) and leaves the other as it is until the next match.  A queue step edits the current set in place: its
// own match follows in the same call (or, set up only, answers COOK_E_STATE to explain and metrics until it has run).  Everything is enqueued on the advance's stream; the two counters the host reads back ride in the advance's one
// synchronisation (this file synchronises only in cook_cycle_set_reservations and the fetch, which are calls of their own).  All
// launches are sized on the host: it knows the list's length and its greatest host id, not which entries are alive.
#pragma once
#include "reserve_kernels.hpp"

struct ReserveBufs {
  struct List {
    DArr<uint32_t> job, host;
    DArr<uint8_t> live;
  } list;                  // (one set: the retire, the upload and the install are ordered on the stream)
  DArr<int32_t> col[2];    // [pending rows] reserved host of a pending row, -1: none; col[cs] is the current one
  DArr<uint32_t> bits[2];  // the bitmap that goes with col[s]
  unsigned cs = 0;
  DArr<uint8_t> launched;  // [pending rows]
  DArr<unsigned> counters;  // cook_cycle_set_reservations' own (a queue cycle's ride in QueueBufs::counters)
  bool own = false;        // MatchIn reads the engine's map, not the staged reserved_hosts / reserved_host
  unsigned n_list = 0, n_words = 0, alive = 0;
  // what was staged (cook_cycle_stage, cook_match_stage*, cook_cycle_update), to put back when the map is dropped
  const uint32_t* s_bits = nullptr;
  unsigned s_words = 0;
  const int32_t* s_col = nullptr;
  cook_reserve_info info{};  // of the last call that could change the map
  bool pending = false, pending_replace = false;
  unsigned pending_n = 0;
};

static bool reserve_active(const cook_reservations* r) { return r && (r->release_matched || r->replace); }

// cook_cycle_stage, cook_match_stage* and cook_cycle_update shift the pending rows: the engine's map and `launched` go, the match reads
// what was staged again.  Called in front of them (cook_cycle_update reads and re-points MatchIn.j_reserved_host).
void reserve_drop(cook_engine* e) {
  if (!e->rvb) return;
  ReserveBufs& b = *e->rvb;
  if (b.own) {
    MatchIn& in = e->min;
    in.reserved_bits = b.s_bits, in.reserved_words = b.s_words, in.j_reserved_host = b.s_col;
  }
  b.own = b.pending = false;
  b.n_list = b.alive = b.n_words = 0;
  b.info = cook_reserve_info{};
}

// cook_cycle_update: MatchIn shows the staged pointers while the update runs; dropped behind it, put back when it is refused
struct ReserveSuspend {
  cook_engine* e;
  bool held = false;
  const uint32_t* bits = nullptr;
  unsigned words = 0;
  const int32_t* col = nullptr;
  explicit ReserveSuspend(cook_engine* e_) : e(e_) {
    if (!e->rvb || !e->rvb->own) return;
    MatchIn& in = e->min;
    held = true, bits = in.reserved_bits, words = in.reserved_words, col = in.j_reserved_host;
    in.reserved_bits = e->rvb->s_bits, in.reserved_words = e->rvb->s_words, in.j_reserved_host = e->rvb->s_col;
  }
  void drop() {
    if (held) e->rvb->own = false;  // (MatchIn holds what the update left there)
    held = false;
    reserve_drop(e);
  }
  ~ReserveSuspend() {
    if (!held) return;
    MatchIn& in = e->min;
    in.reserved_bits = bits, in.reserved_words = words, in.j_reserved_host = col;
  }
};

// what can refuse a list, before anything changes (point 4 of the header's block)
void reserve_check_list(cook_engine* e, const cook_reservations* r, const char* who) {
  if (!r) return;
  if (r->release_matched > 1u || r->replace > 1u) e->fail(COOK_E_INVALID, std::string(who) + ": cook_reservations.release_matched / replace are 0 or 1");
  if (!r->replace || !r->n) return;
  if (!r->pending || !r->host) e->fail(COOK_E_INVALID, std::string(who) + ": cook_reservations.n without pending / host");
  std::vector<uint32_t> rows;
  rows.reserve(r->n);
  for (unsigned i = 0; i < r->n; ++i) {
    if (r->host[i] > 0x7FFFFFFFu) e->fail(COOK_E_INVALID, std::string(who) + ": cook_reservations.host above 2^31 - 1 (the reserved_host column is int32)");
    if (r->pending[i] == COOK_NONE_U32) continue;
    if (r->pending[i] >= e->n_pending) e->fail(COOK_E_INVALID, std::string(who) + ": cook_reservations.pending is not a staged pending row");
    rows.push_back(r->pending[i]);
  }
  std::sort(rows.begin(), rows.end());
  if (std::adjacent_find(rows.begin(), rows.end()) != rows.end()) e->fail(COOK_E_INVALID, std::string(who) + ": a pending row twice in cook_reservations");
}
void reserve_check(cook_engine* e, const QueueArgs& q) {
  const cook_reservations* r = q.reservations;
  reserve_check_list(e, r, "cook_cycle_run_queue_reserve");
  if (reserve_active(r) && !r->replace && !(e->rvb && e->rvb->own))
    e->fail(COOK_E_STATE, "cook_cycle_run_queue_reserve: release_matched without a map of the engine's own (cook_cycle_set_reservations, or replace = 1, "
                          "first: the staged bitmap does not say which job a host belongs to)");
}

// Enqueues the release (k > 0: over the last cycle's considered jobs; skipped: the step's offer_skipped on the device, or null) and the
// replacement, then the bitmap.  cnt: REL_CNT_WORDS words, zero on the stream.  keep_last: the column and the bitmap the last match
// read stay as they are (cook_cycle_set_reservations); else the current set is edited in place (a queue step: its match follows).
void reserve_enqueue(cook_engine* e, const cook_reservations* r, unsigned* cnt, const uint8_t* skipped, unsigned k, bool keep_last = false) {
  ReserveBufs& b = bufs(e->rvb);
  b.pending = false;
  b.info = cook_reserve_info{0u, 0u, 0u, b.own ? b.alive : 0u};
  if (!reserve_active(r)) return;
  MatchIn& in = e->min;
  const unsigned n_rows = e->n_pending;
  auto read_by_last = [&](unsigned s) {  // the inputs of the last match that ran (cook_match_explain, cook_match_metrics) point into set s
    const MatchIn& li = e->last_in;
    return e->match_ran() && e->last_in_valid &&
           ((b.col[s].ptr() && li.j_reserved_host == b.col[s].ptr()) || (b.bits[s].ptr() && li.reserved_bits == b.bits[s].ptr()));
  };
  const unsigned t = (keep_last && read_by_last(b.cs)) ? b.cs ^ 1u : b.cs;  // (one match reads one set: the other is free)
  if (!b.own) {  // (only with replace = 1: reserve_check) the atom begins empty
    b.s_bits = in.reserved_bits, b.s_words = in.reserved_words, b.s_col = in.j_reserved_host;
    memset_async(e, b.col[t].ensure(n_rows), 0xFF, (size_t)n_rows * 4);
    memset_async(e, b.launched.ensure(n_rows), 0, n_rows);
    b.n_list = b.alive = 0;
  } else if (t != b.cs) {
    copy_async(e, b.col[t].ensure(n_rows), b.col[b.cs].ptr(), (size_t)n_rows * 4, hipMemcpyDeviceToDevice);
  }
  b.cs = t;
  int32_t* col = b.col[t].ptr();
  uint8_t* launched = b.launched.ptr();
  if (r->release_matched && k)
    KM<resv_release, 256>(e, "resv_release", div_up(k, 256), (const int32_t*)e->m_j2o.ptr(), k, skipped, (const uint32_t*)e->j_index.ptr(), n_rows, col,
        launched, cnt);
  if (r->replace) {
    ReserveBufs::List& w = b.list;
    if (b.n_list) KM<resv_retire, 256>(e, "resv_retire", div_up(b.n_list, 256), (const uint32_t*)w.job.ptr(), b.n_list, n_rows, col);
    const unsigned n = r->n;
    w.live.ensure(n);  // (a list that outgrows its buffers: DBuf drains the stream before it frees, the retire has run by then)
    if (n) {
      h2d(e, w.job, r->pending, n), h2d(e, w.host, r->host, n);  // (behind the retire on the stream; read until the advance's synchronisation)
      KM<resv_install, 256>(e, "resv_install", div_up(n, 256), (const uint32_t*)w.job.ptr(), (const uint32_t*)w.host.ptr(), n, n_rows,
          (const uint8_t*)launched, col, cnt);
    }
    memset_async(e, launched, 0, n_rows);
    b.n_list = n;
    b.n_words = n ? *std::max_element(r->host, r->host + n) / 32u + 1u : 0u;
  }
  if (b.n_list) {
    ReserveBufs::List& w = b.list;
    uint32_t* bits = b.bits[t].ensure(b.n_words);
    memset_async(e, bits, 0, (size_t)b.n_words * 4);
    KM<resv_bits, 256>(e, "resv_bits", div_up(b.n_list, 256), (const uint32_t*)w.job.ptr(), (const uint32_t*)w.host.ptr(), b.n_list, n_rows,
        (const int32_t*)col, b.n_words, bits, w.live.ptr());
  }
  b.own = true;
  in.j_reserved_host = col;
  in.reserved_bits = b.n_list ? b.bits[t].ptr() : nullptr;  // (reserve_finish: null again when nothing is alive)
  in.reserved_words = b.n_words;
  b.pending = true, b.pending_replace = r->replace != 0u, b.pending_n = r->replace ? r->n : 0u;
}

// behind the synchronisation; h: the counters
void reserve_finish(cook_engine* e, const unsigned* h) {
  if (!e->rvb || !e->rvb->pending) return;
  ReserveBufs& b = *e->rvb;
  b.pending = false;
  const unsigned released = h[RESV_CNT_RELEASED], dropped = h[RESV_CNT_DROPPED];
  if (b.pending_replace)
    b.alive = b.pending_n - dropped;
  else
    b.alive -= std::min(b.alive, released);
  b.info = cook_reserve_info{released, b.pending_replace ? b.pending_n - dropped : 0u, dropped, b.alive};
  if (!b.alive) e->min.reserved_bits = nullptr, e->min.reserved_words = 0;  // the class-ordered walk is eligible again
}

// cook_cycle_set_reservations: reserve-hosts! on its own, for the next RANK cycle; touches none of q_valid / rank_done / the placement,
// and what the last match read stays as it was (keep_last).  A placement that is set up and has not run was packed with the old map:
// refused until cook_cycle_match_multi has run it.
void reserve_set(cook_engine* e, const cook_reservations* r) {
  if (!e->cycle_staged) e->fail(COOK_E_STATE, "cook_cycle_set_reservations before cook_cycle_stage");
  if (e->placement.state == cook_engine::Placement::ROUNDS || e->placement.state == cook_engine::Placement::WALK)
    e->fail(COOK_E_STATE, "cook_cycle_set_reservations while a placement is set up and has not run (cook_cycle_match_multi first): it was set up with the map as it stands");
  cook_reservations rr{0u, 1u, 0u, nullptr, nullptr};
  if (r && r->replace) rr.n = r->n, rr.pending = r->pending, rr.host = r->host;
  if (r) {
    cook_reservations chk = *r;
    chk.release_matched = 0u;  // (ignored here, whatever it holds)
    reserve_check_list(e, &chk, "cook_cycle_set_reservations");
    if (!r->replace) {  // the list is ignored and nothing changes: a map the engine holds stays, without one the staged reservations stay
      if (e->rvb) e->rvb->info = cook_reserve_info{0u, 0u, 0u, e->rvb->own ? e->rvb->alive : 0u};
      return;
    }
  }
  unsigned* cnt = bufs(e->rvb).counters.ensure(REL_CNT_WORDS);
  memset_async(e, cnt, 0, REL_CNT_WORDS * 4);
  reserve_enqueue(e, &rr, cnt, nullptr, 0u, /*keep_last=*/true);
  pinned_copy(e, e->h_scratch + REL_H_CNT, cnt, REL_CNT_WORDS * 4, hipMemcpyDeviceToHost);
  sync(e);
  unsigned h[REL_CNT_WORDS];
  std::memcpy(h, e->h_scratch + REL_H_CNT, sizeof(h));
  reserve_finish(e, h);
}

// cook_cycle_fetch_reservations: the live entries in list order, in one synchronisation
void reserve_fetch(cook_engine* e, uint32_t* pending, uint32_t* host, uint32_t cap, uint32_t* n_out) {
  if (!n_out) e->fail(COOK_E_INVALID, "cook_cycle_fetch_reservations: null n_out");
  *n_out = 0;
  if (!e->rvb || !e->rvb->own || !e->rvb->n_list) return;
  ReserveBufs& b = *e->rvb;
  *n_out = b.alive;
  if (cap < b.alive) e->fail(COOK_E_INVALID, "cook_cycle_fetch_reservations: cap is smaller than the live reservations (see n_out)");
  if (!b.alive || (!pending && !host)) return;
  const unsigned n = b.n_list;
  std::vector<uint32_t> hj(n), hh(n);
  std::vector<uint8_t> hl(n);
  ReserveBufs::List& w = b.list;
  copy_async(e, hj.data(), w.job.ptr(), (size_t)n * 4, hipMemcpyDeviceToHost);
  copy_async(e, hh.data(), w.host.ptr(), (size_t)n * 4, hipMemcpyDeviceToHost);
  copy_async(e, hl.data(), w.live.ptr(), n, hipMemcpyDeviceToHost);
  sync(e);
  unsigned m = 0;
  for (unsigned x = 0; x < n && m < cap; ++x)
    if (hl[x]) {
      if (pending) pending[m] = hj[x];
      if (host) host[m] = hh[x];
      ++m;
    }
  *n_out = m;
}
