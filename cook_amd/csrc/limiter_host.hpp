// limiter_host.hpp — host orchestration of the launch-rate limiters kept across match cycles (cook_cycle_set_limiters,
// cook_cycle_set_clock, cook_cycle_limiters_spend, cook_cycle_fetch_limiters, cookmatch.h).  Included by engine.hip inside
// its anonymous namespace, behind carry_host.hpp (QueueArgs) and in front of queue_host.hpp, which calls limiter_check from
// queue_check_step and limiter_enqueue / limiter_finish from queue_advance; considerable_host.hpp, cycle_host.hpp and carry_host.hpp
// call the functions engine.hip declares ahead of them (limiter_view, limiter_commit_earn, limiter_filter_finish,
// limiter_check_user_state, limiter_new_cycle, limiter_own).
// The state is four columns over the staged users.  A cycle touches it in at most three launches of per-user work: the spend of the
// last cycle's kept placements inside the advance (lim_count_kept, lim_spend), and the commit of the earn behind the rate-limit stage
// (lim_commit_earn); the stage itself computes earn(now) on the fly.  What the host uploads per cycle is cook_clock, which stays on
// the host: both times travel as kernel arguments.  This file synchronises only in the calls of its own (set, explicit spend, fetch):
// a cycle's counters ride in the advance's and the filter's read-backs.
#pragma once
#include "limiter_kernels.hpp"

struct LimiterBufs {
  DArr<double> rate;
  DArr<int64_t> bucket, tokens, last;
  struct {  // a list on its way in (cook_cycle_set_limiters)
    DArr<uint32_t> user;
    DArr<double> per_minute;
    DArr<int64_t> bucket, tokens, last;
  } in;
  DArr<unsigned> kept;      // [users] kept placements of the cycle being spent; zero between two spends
  DArr<unsigned> counters;  // cook_cycle_limiters_spend's own (a queue cycle's ride in QueueBufs::counters)
  DArr<uint8_t> skipped;    // ... and its offer_skipped
  std::vector<double> h_rate;  // the host's copy of rate (it only changes in cook_cycle_set_limiters): time-until of the fetch
  bool own = false;         // the considerable filters read these columns, not the staged tokens_left
  unsigned U = 0;
  bool has_clock = false;   // cook_cycle_set_clock, until a cycle's filters consume it
  cook_clock clock{};
  bool cycle_spent = false;  // the last cycle's kept placements have spent their tokens (or there is nothing to spend)
  bool spend_pending = false;
  cook_limiter_info info{};
};

static bool limiter_own(const cook_engine* e) { return e->lmb && e->lmb->own; }

// cook_cycle_stage restages the users: the limiters go, the filters read the staged tokens_left again
void limiter_drop(cook_engine* e) {
  if (!e->lmb) return;
  LimiterBufs& b = *e->lmb;
  b.own = b.has_clock = b.cycle_spent = b.spend_pending = false;
  b.U = 0;
  b.info = cook_limiter_info{};
}

// cons_stage_users: while limiters are held, the tokens are the engine's and the users are the ones they were installed for
static void limiter_check_user_state(cook_engine* e, const cook_user_state* us) {
  if (!limiter_own(e)) return;
  if (us->tokens_left)
    e->fail(COOK_E_INVALID, "cook_user_state.tokens_left while the engine holds limiters (cook_cycle_set_limiters): the tokens are the engine's; "
                            "cook_cycle_set_limiters(NULL) drops them");
  if (us->n != e->lmb->U) e->fail(COOK_E_INVALID, "cook_user_state.n differs from the users the engine's limiters were installed for");
}

// every cycle, rank cycle or queue cycle, makes placements that have not spent yet
static void limiter_new_cycle(cook_engine* e) {
  if (!e->lmb) return;
  LimiterBufs& b = *e->lmb;
  if (!b.cycle_spent) b.info.spent_users = 0u, b.info.spent = 0;  // (nothing spent in front of this cycle: a rank cycle, or nothing was kept)
  b.cycle_spent = false;
}

// what the rate-limit stage reads.  cycle: a cycle's filters, which consume the staged clock; else the tokens as they stand
static LimView limiter_view(cook_engine* e, unsigned U, bool cycle) {
  if (!e->lmb) return LimView{};
  LimiterBufs& b = *e->lmb;
  const bool clock = cycle && b.has_clock;
  const int64_t now = b.clock.now_ms;
  if (cycle) b.has_clock = false, b.info.earned = 0u;
  if (!b.own) return LimView{};
  if (U != b.U) e->fail(COOK_E_STATE, "the staged user state has another user count than the engine's limiters");
  return LimView{b.rate.ptr(), b.bucket.ptr(), b.tokens.ptr(), b.last.ptr(), now, clock ? 1 : 0};
}
// behind cons_rate_limit; fcnt: the filter's counters (LIM_F_*), zero on the stream
static void limiter_commit_earn(cook_engine* e, const LimView& v, unsigned U, const uint32_t* passed, const uint32_t* rate_limited, unsigned* fcnt) {
  LimiterBufs& b = *e->lmb;
  KM<lim_commit_earn, 256>(e, "lim_commit_earn", div_up(U, 256), passed, rate_limited, U, v.rate, v.bucket, b.tokens.ptr(), b.last.ptr(), v.now, v.clock, fcnt);
}
// behind the filter's synchronisation; h: the words read back from d_counters + LIM_F_LEN
static void limiter_filter_finish(cook_engine* e, const unsigned* h) {
  e->lmb->info.earned = h[LIM_F_EARNED - LIM_F_LEN], e->lmb->info.in_debt = h[LIM_F_DEBT - LIM_F_LEN];
}

// what can refuse a step, before anything changes (queue_check_step)
void limiter_check(cook_engine* e, const QueueArgs& q) {
  if (limiter_own(e) && q.carry && q.carry->tokens_left)
    e->fail(COOK_E_INVALID, "cook_queue_carry.tokens_left while the engine holds limiters (cook_cycle_set_limiters): the tokens are the engine's");
}
// the last cycle's k considered jobs still have to spend
static bool limiter_spend_due(const cook_engine* e, unsigned k) { return limiter_own(e) && !e->lmb->cycle_spent && k; }

// spend-tokens over the last cycle's kept placements: e->m_j2o, e->j_index, `skipped` that cycle's offer_skipped on the device or null.
// cnt: REL_CNT_WORDS words, zero on the stream
static void limiter_spend_launch(cook_engine* e, unsigned* cnt, const uint8_t* skipped, unsigned k, int64_t spend_ms, bool clock) {
  LimiterBufs& b = *e->lmb;
  KM<lim_count_kept, 256>(e, "lim_count_kept", div_up(k, 256), (const int32_t*)e->m_j2o.ptr(), k, skipped, (const uint32_t*)e->j_index.ptr(),
      (const uint32_t*)e->j_user.ptr(), e->n_pending, b.U, b.kept.ptr());
  KM<lim_spend, 256>(e, "lim_spend", div_up(b.U, 256), b.kept.ptr(), b.U, (const double*)b.rate.ptr(), (const int64_t*)b.bucket.ptr(), b.tokens.ptr(),
      b.last.ptr(), spend_ms, clock ? 1 : 0, cnt);
  b.cycle_spent = true;
  b.spend_pending = true;
}
// inside queue_advance, behind the reservations, in front of the considerable filters: the spend of the cycle that this advance takes
// out of the queue, at the staged clock's spend_ms (without a clock nobody earns, the tokens still go)
void limiter_enqueue(cook_engine* e, unsigned* cnt, const uint8_t* skipped, unsigned k) {
  if (!limiter_own(e)) return;
  LimiterBufs& b = *e->lmb;
  if (!b.cycle_spent) b.info.spent_users = 0u, b.info.spent = 0;  // (else cook_cycle_limiters_spend's counts stand)
  if (limiter_spend_due(e, k)) limiter_spend_launch(e, cnt, skipped, k, b.clock.spend_ms, b.has_clock);
}
// behind the synchronisation; h: the counters
void limiter_finish(cook_engine* e, const unsigned* h) {
  if (!e->lmb || !e->lmb->spend_pending) return;
  LimiterBufs& b = *e->lmb;
  b.spend_pending = false;
  b.info.spent_users = h[LIM_CNT_USERS], b.info.spent = (int64_t)h[LIM_CNT_SPENT];
}

// cook_cycle_limiters_spend: the spend of a cycle that no queue advance follows (the last queue cycle in front of a rank trigger)
void limiter_spend(cook_engine* e, const uint8_t* offer_skipped, uint32_t n_offer_skipped, int64_t spend_ms) {
  if (!e->cycle_staged) e->fail(COOK_E_STATE, "cook_cycle_limiters_spend before cook_cycle_stage");
  if (!limiter_own(e)) e->fail(COOK_E_STATE, "cook_cycle_limiters_spend without limiters (cook_cycle_set_limiters first)");
  if (!e->q_valid || !e->rank_done || !e->match_ran())
    e->fail(COOK_E_STATE, "cook_cycle_limiters_spend needs a completed cycle with no cook_cycle_stage / cook_cycle_update / cook_rank* / cook_considerable / "
                          "cook_match_stage since");
  LimiterBufs& b = *e->lmb;
  if (b.cycle_spent) e->fail(COOK_E_STATE, "cook_cycle_limiters_spend: the last cycle's placements have spent already");
  if (offer_skipped && n_offer_skipped != e->M)
    e->fail(COOK_E_INVALID, "cook_cycle_limiters_spend: offer_skipped has one entry per offer of the LAST cycle (n_offer_skipped differs from that count)");
  if (spend_ms > (int64_t)LIM_PRODUCT_MAX || spend_ms < -(int64_t)LIM_PRODUCT_MAX) e->fail(COOK_E_INVALID, "cook_cycle_limiters_spend: |spend_ms| above 2^62");
  const unsigned k = e->cycle_considered;
  b.info.spent_users = 0u, b.info.spent = 0;
  b.cycle_spent = true;
  if (!k) return;
  unsigned* cnt = b.counters.ensure(REL_CNT_WORDS);
  memset_async(e, cnt, 0, REL_CNT_WORDS * 4);
  const uint8_t* skipped = (offer_skipped && e->M && !e->kube_last) ? h2d_opt(e, b.skipped, offer_skipped, e->M) : nullptr;  // (a Kubernetes cycle has no offer indices)
  limiter_spend_launch(e, cnt, skipped, k, spend_ms, true);
  pinned_copy(e, e->h_scratch + REL_H_CNT, cnt, REL_CNT_WORDS * 4, hipMemcpyDeviceToHost);
  sync(e);
  unsigned h[REL_CNT_WORDS];
  std::memcpy(h, e->h_scratch + REL_H_CNT, sizeof(h));
  limiter_finish(e, h);
}

// cook_cycle_set_limiters: the whole table (user NULL, or a first list that names every user), or a listed replacement (the host's
// flush! after a quota edit).  Everything that can refuse runs before anything changes
void limiter_set(cook_engine* e, const cook_limiters* l) {
  if (!e->cycle_staged) e->fail(COOK_E_STATE, "cook_cycle_set_limiters before cook_cycle_stage");
  if (e->placement.state == cook_engine::Placement::ROUNDS || e->placement.state == cook_engine::Placement::WALK)
    e->fail(COOK_E_STATE, "cook_cycle_set_limiters while a placement is set up and has not run (cook_cycle_match_multi first): its jobs passed the filters "
                          "under the limiters as they stand");
  if (!l) {
    limiter_drop(e);
    return;
  }
  const bool staged = e->cb && e->cb->cycle_on && e->cb->users_staged;
  const unsigned U = limiter_own(e) ? e->lmb->U : (staged ? e->cb->U : e->U);
  const unsigned n = l->n;
  if (!e->has_j_user) e->fail(COOK_E_INVALID, "cook_cycle_set_limiters needs pending_jobs->user");
  if (!l->user && n != U) e->fail(COOK_E_INVALID, "cook_limiters.n differs from the staged users (user NULL: entry i is user i)");
  if (!limiter_own(e) && n != U) e->fail(COOK_E_INVALID, "cook_limiters: the first call must cover every staged user");
  if (n && (!l->per_minute || !l->bucket || !l->tokens || !l->last_update_ms)) e->fail(COOK_E_INVALID, "cook_limiters: per_minute, bucket, tokens and last_update_ms are required");
  constexpr int64_t TOK_MAX = (int64_t)1 << 53, T_MAX = (int64_t)1 << 62;
  std::vector<uint8_t> seen(l->user ? U : 0u, 0);
  for (unsigned x = 0; x < n; ++x) {
    if (l->user) {
      if (l->user[x] >= U) e->fail(COOK_E_INVALID, "cook_limiters.user: not a staged user");
      if (seen[l->user[x]]) e->fail(COOK_E_INVALID, "cook_limiters.user: a user twice");
      seen[l->user[x]] = 1;
    }
    if (!(l->per_minute[x] > 0.0) || !std::isfinite(l->per_minute[x])) e->fail(COOK_E_INVALID, "cook_limiters.per_minute must be finite and above 0");
    if (l->bucket[x] < 0 || l->bucket[x] > TOK_MAX) e->fail(COOK_E_INVALID, "cook_limiters.bucket outside 0 .. 2^53");
    if (l->tokens[x] < -TOK_MAX || l->tokens[x] > TOK_MAX) e->fail(COOK_E_INVALID, "cook_limiters.tokens outside -2^53 .. 2^53");
    if (l->last_update_ms[x] < -T_MAX || l->last_update_ms[x] > T_MAX) e->fail(COOK_E_INVALID, "cook_limiters.last_update_ms outside -2^62 .. 2^62");
  }
  LimiterBufs& b = bufs(e->lmb);
  if (!b.own) {
    b.rate.ensure(std::max(1u, U)), b.bucket.ensure(std::max(1u, U)), b.tokens.ensure(std::max(1u, U)), b.last.ensure(std::max(1u, U));
    memset_async(e, b.kept.ensure(std::max(1u, U)), 0, (size_t)std::max(1u, U) * 4);
    b.h_rate.assign(U, 0.0);
    b.U = U;
    b.cycle_spent = true;  // (the host's counts are current: they know the launches of the cycle in front of the install)
    b.info = cook_limiter_info{};
  }
  if (n) {
    const uint32_t* user = h2d_opt(e, b.in.user, l->user, n);
    h2d(e, b.in.per_minute, l->per_minute, n), h2d(e, b.in.bucket, l->bucket, n), h2d(e, b.in.tokens, l->tokens, n), h2d(e, b.in.last, l->last_update_ms, n);
    KM<lim_install, 256>(e, "lim_install", div_up(n, 256), user, (const double*)b.in.per_minute.ptr(), (const int64_t*)b.in.bucket.ptr(),
        (const int64_t*)b.in.tokens.ptr(), (const int64_t*)b.in.last.ptr(), n, U, b.rate.ptr(), b.bucket.ptr(), b.tokens.ptr(), b.last.ptr());
    for (unsigned x = 0; x < n; ++x) b.h_rate[l->user ? l->user[x] : x] = l->per_minute[x] / 60000.0;
  }
  sync(e);  // (the caller's arrays are read until here)
  b.own = true;
}

// cook_cycle_set_clock: host-only state
void limiter_set_clock(cook_engine* e, const cook_clock* c) {
  LimiterBufs& b = bufs(e->lmb);
  if (!c) {
    b.has_clock = false;
    return;
  }
  constexpr int64_t T_MAX = (int64_t)1 << 62;
  if (c->now_ms < -T_MAX || c->now_ms > T_MAX || c->spend_ms < -T_MAX || c->spend_ms > T_MAX) e->fail(COOK_E_INVALID, "cook_clock: a time outside -2^62 .. 2^62");
  b.clock = *c;
  b.has_clock = true;
}

// time-until-out-of-debt-millis! without the earn
static int64_t limiter_time_until(int64_t tokens, double rate) {
  double q = std::ceil((double)(-tokens) / rate);
  if (!(q > 0.0)) return 0;
  return q > LIM_PRODUCT_MAX ? (int64_t)LIM_PRODUCT_MAX : (int64_t)q;
}
// cook_cycle_fetch_limiters: one synchronisation, no state changes
void limiter_fetch(cook_engine* e, int64_t* tokens, int64_t* last_update_ms, int64_t* time_until_ms) {
  if (!limiter_own(e)) e->fail(COOK_E_STATE, "cook_cycle_fetch_limiters without limiters (cook_cycle_set_limiters first)");
  LimiterBufs& b = *e->lmb;
  const unsigned U = b.U;
  if (!U || (!tokens && !last_update_ms && !time_until_ms)) return;
  std::vector<int64_t> tk(tokens ? 0u : U);
  int64_t* t = tokens ? tokens : tk.data();
  if (tokens || time_until_ms) copy_async(e, t, b.tokens.ptr(), (size_t)U * 8, hipMemcpyDeviceToHost);
  if (last_update_ms) copy_async(e, last_update_ms, b.last.ptr(), (size_t)U * 8, hipMemcpyDeviceToHost);
  sync(e);
  if (time_until_ms)
    for (unsigned u = 0; u < U; ++u) time_until_ms[u] = limiter_time_until(t[u], b.h_rate[u]);
}
// cook_cycle_fetch_rate_limit: the rate-limit stage's per-user counts of the last cycle that ran the filters
void limiter_fetch_counts(cook_engine* e, uint32_t* rate_limited, uint32_t* passed) {
  if (!e->cycle_cons_ran || !e->cb) e->fail(COOK_E_STATE, "cook_cycle_fetch_rate_limit: the last cycle did not run the considerable filters");
  const ConsBufs& c = *e->cb;
  if (!c.U || (!rate_limited && !passed)) return;
  if (rate_limited) copy_async(e, rate_limited, c.rate_limited.ptr(), (size_t)c.U * 4, hipMemcpyDeviceToHost);
  if (passed) copy_async(e, passed, c.passed.ptr(), (size_t)c.U * 4, hipMemcpyDeviceToHost);
  sync(e);
}
