// cycle_host.hpp — a match cycle's part in front of the placement (a fresh rank, or a queue step's advance; the considerable filters; the
// take of K jobs) and the one body of the four single-pool cycle entry points.  Included by engine.hip inside its anonymous namespace, LAST:
// behind rank_host.hpp, match_host.hpp, considerable_host.hpp (ConsBufs, cons_run_device) and queue_host.hpp (queue_reset_groups, queue_advance).

COOK_KERNEL void cycle_job_index(const uint32_t* __restrict__ ranked, const uint32_t* __restrict__ pend_ord, unsigned k, uint32_t* __restrict__ j_index) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k) j_index[i] = pend_ord[ranked[i]];
}

// (considerable filters) -> take K over the standing queue -> the job index array of the match; returns K
static unsigned cycle_take_part(cook_engine* e, uint32_t num_considerable) {
  e->q_last_pos = nullptr;
  limiter_new_cycle(e);  // (the placements this cycle makes have not spent their tokens)
  unsigned K = std::min<unsigned>(num_considerable, e->n_ranked);  // (take num-considerable), scheduler.clj:751
  if (e->cb && e->cb->cycle_on) {  // pending-jobs->considerable-jobs between rank and match (scheduler.clj:729-762)
    ConsBufs& c = *e->cb;
    if (!e->has_j_user) e->fail(COOK_E_INVALID, "cook_cycle_run: the considerable filters need pending_jobs->user");
    const unsigned n = e->n_ranked;
    c.q_cpus.ensure(n), c.q_mem.ensure(n), c.q_gpus.ensure(n), c.q_user.ensure(n), c.q_elig.ensure(n);
    if (n)
      KM<cons_gather_queue, 256>(e, "cons_gather_queue", div_up(n, 256), (const uint32_t*)e->ranked.ptr(), (const uint32_t*)e->pend_ord.ptr(), n,
          e->min.j_cpus, e->min.j_mem, e->min.j_gpus, (const uint32_t*)e->j_user.ptr(),
          c.has_elig_by_pending ? (const uint8_t*)c.elig_by_pending.ptr() : (const uint8_t*)nullptr, c.q_cpus.ptr(), c.q_mem.ptr(), c.q_gpus.ptr(),
          c.q_user.ptr(), c.q_elig.ptr());
    cons_run_device(e, c, c, n, c.q_cpus.ptr(), c.q_mem.ptr(), c.q_gpus.ptr(), c.q_user.ptr(), c.q_elig.ptr(), num_considerable, LIM_CYCLE);
    K = c.n_result;
    e->cycle_cons_ran = true;
    e->q_last_pos = c.result;
    e->j_index.ensure(K);
    if (K)
      KM<cons_job_index, 256>(e, "cons_job_index", div_up(K, 256), (const uint32_t*)c.result, (const uint32_t*)e->ranked.ptr(),
          (const uint32_t*)e->pend_ord.ptr(), K, e->j_index.ptr());
  } else {
    e->j_index.ensure(K);
    if (K)
      KM<cycle_job_index, 256>(e, "cycle_job_index", div_up(K, 256), (const uint32_t*)e->ranked.ptr(), (const uint32_t*)e->pend_ord.ptr(), K, e->j_index.ptr());
  }
  e->q_valid = true;
  return K;
}
// rank -> cycle_take_part.  Any rank resets the standing queue to the fresh order and the groups' cotasks to the staged table
static unsigned cycle_rank_part(cook_engine* e, uint32_t num_considerable) {
  if (!e->cycle_staged) e->fail(COOK_E_STATE, "cook_cycle_run before cook_cycle_stage");
  queue_reset_groups(e);
  if (recording()) {  // (a pool batch times its joint sequence of launches itself)
    rank_run(e);
  } else {
    StageTimer tr(e, 0, &e->rank_ms);
    rank_run(e);
    tr.stop();
  }
  return cycle_take_part(e, num_considerable);
}
// a queue cycle's part in front of the placement: advance -> cycle_take_part, no rank
static unsigned cycle_queue_part(cook_engine* e, const QueueArgs& q, uint32_t num_considerable) {
  if (recording()) {
    queue_advance(e, q);
    return cycle_take_part(e, num_considerable);
  }
  StageTimer tr(e, 0, &e->rank_ms);
  queue_advance(e, q);
  const unsigned K = cycle_take_part(e, num_considerable);
  tr.stop();
  return K;
}

// the match of a cycle's K considered jobs; defer: set up only, the rounds run in cook_cycle_match_multi
static void cycle_match(cook_engine* e, unsigned K, bool defer) { match_run_device(e, K, K ? e->j_index.ptr() : nullptr, defer); }

// One pool's cycle behind its C entry point: `front` is cycle_rank_part or cycle_queue_part and returns K.  A match that runs here is timed
// as the match stage; a deferred one is timed by cook_cycle_match_multi, which runs it.
template <class Front>
int cycle_run_one(cook_engine* e, Front&& front, bool defer) {
  return guarded(e, [&] {
    const unsigned K = front();
    if (defer) {
      cycle_match(e, K, true);
    } else {
      StageTimer tm(e, 2, &e->match_ms);
      cycle_match(e, K, false);
      tm.stop();
    }
    prof_collect(e);
  });
}
