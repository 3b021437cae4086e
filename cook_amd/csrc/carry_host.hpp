// carry_host.hpp — host orchestration of the carry (cook_cycle_run_queue_carry*, cookmatch.h), and in front of it what
// the carry, the release, the churn and the advance share: QueueArgs, the read-back slots, groups_install, SegSort, host_rows.  Included by engine.hip inside
// its anonymous namespace, behind offer_table.hpp (the offer columns a fold reads and writes), match_host.hpp (MatchIn's staging), considerable_host.hpp (ConsBufs) and rank_host.hpp
// (radix_sort_masked); queue_host.hpp calls carry_check from queue_check_step and carry_enqueue / carry_finish from queue_advance.
// Everything is enqueued on the advance's stream over the OLD offers and the OLD considered rows; the only thing the host reads back,
// the pool's four sums, rides in the advance's one synchronisation.
#pragma once
#include "carry_kernels.hpp"
#include "release_kernels.hpp"  // (release_host_rows, for host_rows below)

// what a queue cycle's entry point was given (carry, finished, hosts, reservations: null = none)
struct QueueArgs {
  const cook_queue_step* step;
  const cook_queue_carry* carry;
  const cook_finished* finished;
  const cook_host_churn* hosts;
  const cook_reservations* reservations;
  // cook_cycle_run_queue_pods* (podtable_host.hpp): the offers are rebuilt from the resident pod table inside the advance
  const cook_pod_delta* pods = nullptr;
  bool pods_on = false;
  int with_task_limits = 0;
};

// where a queue cycle's advance lands its read-backs in h_scratch, in 64-bit words: the advance's two counters (1 word), the carry's
// pool (4 doubles), the release's counters (REL_CNT_WORDS of 4 bytes) and its pool (4 doubles)
constexpr unsigned Q_H_ADVANCE = 0, Q_H_CARRY_POOL = 1, REL_H_CNT = 8, REL_H_POOL = 16;  // (release_host.hpp asserts that they do not overlap)

// a queue cycle's table of the groups' cotasks takes the place of the one in use; the staged one is kept for the next rank
void groups_install(cook_engine* e, const uint32_t* off, const uint32_t* host, const uint32_t* attr) {
  MatchIn& in = e->min;
  if (!e->q_groups_own) {
    e->q_sg_off = in.g_run_off, e->q_sg_host = in.g_run_host, e->q_sg_attr = in.g_run_attr, e->q_sg_total = e->cf_group_run_total;
    e->q_groups_own = true;
  }
  in.g_run_off = off, in.g_run_host = host, in.g_run_attr = attr;
}

static unsigned long long carry_key_mask(unsigned max_key) {
  unsigned long long m = 0;
  for (unsigned long long x = max_key; x; x >>= 1) m = (m << 1) | 1ull;
  return m;
}
// the positions [0, k) of a key column, stably sorted by key (-> the permutation), and the segments [start[x], end[x]) of the keys below n_seg
struct SegSort {
  DArr<uint32_t> permA, permB, start, end;
  const uint32_t* carry_segments(cook_engine* e, const uint64_t* key, unsigned k, unsigned n_seg) {
    permA.ensure(k), permB.ensure(k);
    start.ensure(n_seg), end.ensure(n_seg);
    memset_async(e, start.ptr(), 0, (size_t)n_seg * 4);
    memset_async(e, end.ptr(), 0, (size_t)n_seg * 4);
    KM<iota_u32, 256>(e, "iota", div_up(k, 256), permA.ptr(), k);
    const uint32_t* perm = radix_sort_masked(e, key, carry_key_mask(n_seg), permA.ptr(), permA.ptr(), permB.ptr(), k);
    KM<carry_seg_bounds, 256>(e, "carry_seg_bounds", div_up(k, 256), perm, key, k, n_seg, start.ptr(), end.ptr());
    return perm;
  }
};
struct CarryBufs {
  DArr<uint64_t> okey, ukey;
  SegSort o, u;
  DArr<double> pool;  // {count, cpus, mem, gpus} of all kept jobs
  // the engine's own copy of the offer columns a fold changes (OFFER_FOLDED); two sets: a carry reads the staged columns (which may be
  // the other set) and writes a fresh one, so the last match's inputs (cook_match_explain) stay as they were
  OfferStore cols[2];
  unsigned cur = 0;
  bool pool_pending = false;  // this advance reads the pool's sums back
  DArr<uint32_t> h2row;       // host id -> row of the staged offers (host_rows)
  bool h2row_built = false;   // ... as THIS advance built it (queue_advance clears the mark)
};

// host id -> row of the staged offers, for the release and the churn of one advance: the table and its entries, or null and 0 where the
// greatest host id is not known (offers built on the device) or far above the row count — the callers' kernels then look a host up in
// o_host itself.  The first caller of an advance builds the table, the second finds it built.
static const uint32_t* host_rows(cook_engine* e, unsigned& n_hosts) {
  const unsigned M = e->M;
  n_hosts = 0;
  if (e->cf_max_host == 0xFFFFFFFFu || (size_t)e->cf_max_host > 8u * (size_t)M + 65536u) return nullptr;
  CarryBufs& b = bufs(e->cyb);
  n_hosts = e->cf_max_host + 1u;
  uint32_t* t = b.h2row.ensure(n_hosts);
  if (!b.h2row_built) {
    memset_async(e, t, 0xFF, (size_t)n_hosts * 4);
    KM<release_host_rows, 256>(e, "release_host_rows", div_up(M, 256), e->min.o_host, M, n_hosts, t);
    b.h2row_built = true;
  }
  return t;
}

// what can refuse a carry, before anything changes (queue_check_step)
void carry_check(cook_engine* e, const QueueArgs& q) {
  const cook_queue_step* s = q.step;
  const cook_queue_carry* c = q.carry;
  if (!c) return;
  if (c->offers > 1u || c->usage > 1u) e->fail(COOK_E_INVALID, "cook_queue_carry: offers / usage are 0 or 1");
  if (c->offers && s && s->offers)
    e->fail(COOK_E_INVALID, "cook_queue_carry: offers = 1 carries the placements into the STAGED offers; step->offers replaces them (one or the other)");
  const bool staged = e->cb && e->cb->cycle_on && e->cb->users_staged;
  if ((c->usage || c->tokens_left) && !staged)
    e->fail(COOK_E_STATE, "cook_queue_carry: usage / tokens_left need a user state staged by cook_cycle_set_considerable");
  if (c->tokens_left && !e->cb->has_tokens)
    e->fail(COOK_E_INVALID, "cook_queue_carry: tokens_left given, but the staged user state has no launch-rate limiter");
  if (c->usage && !e->has_j_user) e->fail(COOK_E_INVALID, "cook_queue_carry: usage = 1 needs pending_jobs->user");
}

// a fold of the offers: `ci` the staged offer columns, `co` the set w of the engine's own, with room for the columns a fold writes: cpus,
// mem and the columns a fold makes whatever is staged; of the others (named scalars, the maps' amounts) those the staged table has.
// -> the written set: the staged offers from here on (offer_cols_stage, only_held: hosts, attributes and limits are the same rows, so
// host_dup and the greatest host id stay valid; every match packs its offers afresh, so nothing else is cached per offer table)
static OfferCols<true> carry_offer_cols(const MatchIn& in, unsigned M, OfferStore& w, CarryOfferIn& ci, CarryOfferCols& co) {
  const OfferDims d = offer_dims(in);
  const OfferCols<false> staged = offer_cols_of(in);
  const OfferCols<true> out = w.ensure(d, M, [&](const auto& col) {
    return (col.flags & OFFER_FOLDED) && ((col.flags & (OFFER_REQUIRED | OFFER_MADE)) || col.col(staged));
  });
  ci = fold_offer_in(staged, d), co = fold_offer_cols(out);
  return out;
}

// Inside queue_advance, behind q_mark_removed: k > 0 considered jobs of the last cycle, their job_to_offer in e->m_j2o, their rows
// through e->j_index, `skipped` the step's offer_skipped on the device (or null).  -> the staged offers are a fresh set of columns
// written by this call (what a release behind it may update in place).
bool carry_enqueue(cook_engine* e, const cook_queue_carry* c, const uint8_t* skipped, unsigned k) {
  CarryBufs& b = bufs(e->cyb);
  b.pool_pending = false;
  if (!c || !(c->offers || c->usage) || !k) return false;
  MatchIn& in = e->min;
  const unsigned M = e->M;
  const int32_t* j2o = e->m_j2o.ptr();
  CarryJobs j{};
  j.j_index = e->j_index.ptr();
  j.cpus = in.j_cpus, j.mem = in.j_mem, j.gpus = in.j_gpus, j.disk_req = in.j_disk_req;
  j.gpu_model = in.j_gpu_model, j.disk_type = in.j_disk_type, j.ports = in.j_ports;
  for (unsigned s = 0; s < 3u; ++s) j.scal[s] = s < in.n_scal ? in.j_scal[s] : nullptr;
  const bool offers = c->offers && M, usage = c->usage && e->cb->U;
  const unsigned U = usage ? e->cb->U : 0u;
  uint64_t* okey = offers ? b.okey.ensure(k) : nullptr;
  uint64_t* ukey = usage ? b.ukey.ensure(k) : nullptr;
  if (!okey && !ukey) return false;
  KM<carry_keys, 256>(e, "carry_keys", div_up(k, 256), j2o, k, skipped, (const uint32_t*)j.j_index, (const uint32_t*)e->j_user.ptr(), M, U, okey, ukey);
  if (offers) {
    const uint32_t* perm = b.o.carry_segments(e, okey, k, M);
    CarryOfferIn ci;
    CarryOfferCols co;
    const OfferCols<true> out = carry_offer_cols(in, M, b.cols[b.cur ^ 1u], ci, co);
    KM<fold_offers<false>, FOLD_OT>(e, "carry_fold_offers", M, perm, (const uint32_t*)b.o.start.ptr(), (const uint32_t*)b.o.end.ptr(), M, 1u, j, ci, co,
        (unsigned*)nullptr);
    b.cur ^= 1u;
    offer_cols_stage(in, out, offer_dims(in), M, true);
  }
  if (usage) {
    ConsBufs& cb = *e->cb;
    const uint32_t* perm = b.u.carry_segments(e, ukey, k, U);
    int64_t* spend = (cb.has_tokens && !c->tokens_left && !limiter_own(e)) ? cb.tokens.ptr() : nullptr;  // (limiters of the engine's own spend in limiter_enqueue)
    KM<fold_users<false, RowsSorted>, FOLD_UT>(e, "carry_fold_users", U, RowsSorted{perm, j}, (const uint32_t*)b.u.start.ptr(),
        (const uint32_t*)b.u.end.ptr(), U, cb.ucount.ptr(), cb.ucpus.ptr(), cb.umem.ptr(), cb.ugpus.ptr(), spend);
    if (cb.pool_usage_given) {
      KM<fold_pool<false, RowsKept>, FOLD_UT>(e, "carry_fold_pool", 1, RowsKept{j2o, skipped, j}, k, b.pool.ensure(4));
      pinned_copy(e, e->h_scratch + Q_H_CARRY_POOL, b.pool.ptr(), 32, hipMemcpyDeviceToHost);
      b.pool_pending = true;
    }
  }
  return offers;
}
// the host's refill of the tokens (behind the spend on the stream; read until the advance's synchronisation)
void carry_tokens(cook_engine* e, const cook_queue_carry* c) {
  if (!c || !c->tokens_left) return;
  ConsBufs& cb = *e->cb;
  h2d(e, cb.tokens, c->tokens_left, cb.U);
}
// behind the advance's synchronisation
void carry_finish(cook_engine* e) {
  if (!e->cyb || !e->cyb->pool_pending) return;
  e->cyb->pool_pending = false;
  double h[4];
  std::memcpy(h, e->h_scratch + Q_H_CARRY_POOL, 32);
  cook_usage& p = e->cb->pool_usage;
  p.count = p.count + h[0], p.cpus = p.cpus + h[1], p.mem = p.mem + h[2], p.gpus = p.gpus + h[3];
}
