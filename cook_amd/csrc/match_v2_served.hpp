// match_v2_served.hpp — served walkers: a persistent walker workgroup per pool (match_walkers) beside serve launches (match_serve_eval,
// match_serve_merge, match_serve_latch), with their control blocks.  Last part of match_v2.hpp: needs PoolCtx (match_v2_multi.hpp) and, through
// it, the three blocks of a round.
#pragma once

// ---- served walkers: the pools of a rank DECOUPLED -------------------------------------------------------------------------------
// The lockstep launches above make every pool of a chain wait for the slowest walk of the round and for the evaluation of all its
// neighbours.  Here every pool has ONE persistent walker workgroup — match_walkers, one launch per match of the whole rank, on a
// stream of its own — that runs resolve_round after resolve_round; between two rounds it posts "my next window wants evaluating"
// (ServeSlot::req) and waits for "lists ready" (ServeSlot::ready).  A second stream carries SERVE ITERATIONS — match_serve_eval +
// match_serve_merge, the same evaluation and merge as above — for whichever pools had a request open when the iteration was put
// together (the LATCH: taken by the last workgroup of the previous iteration's merge, so that every workgroup of an iteration
// agrees on the pools it serves).  That workgroup also publishes the iteration's results and then WAITS (bounded) for the next
// request, so the chain of serve launches is paced by the walkers: two streams per GPU, whatever the number of pools.
//
// Hand-offs (MI355X_MICROARCH.md, inter-workgroup visibility): walker -> server: plain stores, agent_release(), relaxed agent store
// of req; the latch reads req with agent loads and the NEXT launch's kernel-start acquire makes the walker's stores visible to its
// workgroups on every XCD.  server -> walker: every merge workgroup releases before it takes its arrival ticket, the last arriver
// stores ready, the walker polls it, acquires once, and reads with plain loads.  Every wait is bounded: a walker that is not served
// within `spin_ticks` raises ServeCtl::error and leaves, the pool's state is consistent (the last finished round), and the host
// finishes the match with lockstep launches.
//
// STEPPING form (spin_ticks == 0; the SIMT emulator of the test suite, which runs one launch at a time, and COOK_SERVE_STEP=1 on the
// GPU): nothing waits — a walker that finds its window not served yet returns, and the host alternates walker launches, latch
// launches and serve iterations.  Same kernels, same words, same results.
struct alignas(128) ServeSlot {  // per pool; the walker's words and the server's on lines of their own
  unsigned req;   // [walker -> server] windows asked for so far (the first one by the host: 1)
  unsigned done;  // [walker -> server] 1 = every job of the pool is resolved, 2 = the walker gave up (ServeCtl::error)
  // the walker's own account (100 MHz ticks; COOK_SERVE_TRACE=1 prints it): from posting a request to seeing its lists, and from the end
  // of a round to the posting of the next request (drain, barrier, L2 write-back)
  unsigned long long wait_ticks, post_ticks;
  unsigned waits, pad0[25];
  unsigned ready;  // [server -> walker] windows served so far
  unsigned claim;  // [server <-> server] the last request of this pool that a server has taken (dynamic assignment: whichever latch sees a
                   // request first takes it with a compare-and-swap from req - 1 to req)
  unsigned pad1[30];
};
constexpr unsigned MV_SERVE_MAX = 16;  // pools per served call
// What ONE serve iteration works on: the pools that had a request open when the iteration was put together, the request numbers it
// serves, and the arrival count that completes its merge.  Two of them, used in turn (iteration `it` reads latch[it & 1], its last
// merge workgroup writes latch[(it + 1) & 1]): workgroups of an iteration that START late — behind the latch, which happens when another
// server's evaluation holds the chip's wave slots — still find the iteration's own list.  (With one list a late workgroup read the NEXT
// iteration's pools, merged windows nobody had evaluated into lists a walker was reading, and took an arrival ticket it was not counted
// for: profiles/r05i_probe.txt.)
struct ServeLatch {
  unsigned n;
  unsigned ticket_target;  // cumulative: the arrival counter is never reset
  unsigned pool[MV_SERVE_MAX], seq[MV_SERVE_MAX];
};
// one per SERVER (a stream of serve iterations): it serves the pools first, first + stride, ... (n_pools of them).  On cache lines of
// its own, the arrival counter on another.
struct alignas(256) ServeCtl {
  unsigned n_pools, pool_first, pool_stride;
  unsigned claim_max;     // > 0: DYNAMIC assignment — this server looks at every pool of the call (first 0, stride 1) and takes up to claim_max
                          // open requests per iteration, first come first served among the servers (ServeSlot::claim); 0: its own pools only
  unsigned dbg_fence;     // (diagnostics, COOK_SERVE_FENCE=1) every hand-off with full agent-scope fences by every workgroup
  unsigned dbg_delay[3];  // (diagnostics) 100 MHz ticks to wait [0] before publishing, [1] between seeing ready and the acquire, [2] behind the acquire
  ServeLatch latch[2];
  unsigned served[MV_SERVE_MAX];  // = ServeSlot::ready of every pool (the latch's own copy)
  unsigned all_done;              // no walker is left
  unsigned error;                 // a walker gave up
  unsigned iterations, empty_iterations, pools_served;  // statistics
  unsigned long long wait_ticks;  // 100 MHz ticks the latch spent waiting for a request
  unsigned long long formed_tick, busy_ticks;  // when the running iteration's list was put together; ticks from there to the publishing of its results (iterations with work)
  alignas(128) unsigned ticket;   // arrivals of merge workgroups so far (agent-scope atomics only; zeroed by the host)
};
struct alignas(128) ServeHost {  // page-locked host memory, written by the latch with system-scope stores, polled by the host
  unsigned iter_done;  // serve iterations finished
  unsigned all_done, error, pad;
};

// the latch of iteration `it` (one wave): publish what the iteration served, then put the next iteration together
static __device__ __forceinline__ void serve_latch(ServeCtl* sc, ServeSlot* slots, ServeHost* host, unsigned long long poll_ticks, unsigned it) {
  const unsigned lane = lane_id();
  const ServeLatch& cur = sc->latch[it & 1u];
  ServeLatch& nxt = sc->latch[(it + 1u) & 1u];
  const unsigned n = wave_uniform_u32(sc->n_pools), nl = wave_uniform_u32(cur.n);
  const unsigned my_pool = wave_uniform_u32(sc->pool_first) + lane * wave_uniform_u32(sc->pool_stride);  // lane = the server's lane-th pool
  unsigned mine = lane < n ? sc->served[lane] : 0u;  // (the previous latch's values)
  for (unsigned x = 0; x < nl; ++x) {                  // ... brought up to date from the iteration that just ran, without a trip through memory
    const unsigned p = wave_uniform_u32(cur.pool[x]), q = wave_uniform_u32(cur.seq[x]);
    if (my_pool == p) mine = q;
  }
  if (lane < n) sc->served[lane] = mine;
  if (sc->dbg_delay[0] != 0u) {
    const unsigned long long d0 = cook_ticks();
    while (cook_ticks() - d0 < sc->dbg_delay[0]) SPIN_PAUSE_FAR();
  }
  if (lane < nl) st_agent(&slots[cur.pool[lane]].ready, cur.seq[lane]);
  const unsigned long long t0 = cook_ticks();
  if (lane == 0 && nl != 0u && sc->formed_tick != 0ull) sc->busy_ticks += t0 - sc->formed_tick;
  unsigned rq = 0, dn = 0;
  unsigned long long pend, alive;
  const unsigned claim_max = wave_uniform_u32(sc->claim_max);
  for (;;) {
    unsigned cl = mine;
    if (lane < n) {
      rq = ld_agent(&slots[my_pool].req);
      dn = ld_agent(&slots[my_pool].done);
      if (claim_max != 0u) cl = ld_agent(&slots[my_pool].claim);
    }
    alive = __ballot(lane < n && dn == 0u);
    pend = __ballot(lane < n && dn == 0u && rq != cl);
    if (claim_max != 0u && pend != 0ull) {  // dynamic: take what nobody has taken yet, at most claim_max of them (the others are some other server's)
      const bool mine_to_try = ((pend >> lane) & 1ull) != 0ull && (unsigned)__popcll(pend & ((1ull << lane) - 1ull)) < claim_max;
      bool won = false;
      if (mine_to_try) won = atomicCAS(&slots[my_pool].claim, cl, rq) == cl;
      pend = __ballot(won);
    }
    if (pend != 0ull || alive == 0ull || poll_ticks == 0ull || cook_ticks() - t0 > poll_ticks) break;
    SPIN_PAUSE_FAR();
  }
  const unsigned long long waited = cook_ticks() - t0;
  if ((pend >> lane) & 1ull) {
    const unsigned x = (unsigned)__popcll(pend & ((1ull << lane) - 1ull));
    nxt.pool[x] = my_pool;
    nxt.seq[x] = rq;
  }
  if (lane == 0) {
    const unsigned np = (unsigned)__popcll(pend);
    nxt.n = np;
    nxt.ticket_target = cur.ticket_target + np * (unsigned)MV_MERGE_BLOCKS;
    sc->iterations += 1u;
    sc->empty_iterations += nl == 0u ? 1u : 0u;
    sc->pools_served += nl;
    sc->wait_ticks += waited;
    sc->formed_tick = cook_ticks();
    const unsigned err = ld_agent(&sc->error);
    if (alive == 0ull) sc->all_done = 1u;
    if (alive == 0ull) st_system(&host->all_done, 1u);
    if (err != 0u) st_system(&host->error, err);
    st_system(&host->iter_done, sc->iterations);
  }
}
// (stepping form) behind a walker launch: the latch of iteration `it` once more — it publishes the same numbers again and now finds the
// requests the walkers have just posted
__global__ void __launch_bounds__(COOK_WAVE) match_serve_latch(ServeCtl* sc, ServeSlot* slots, ServeHost* host, unsigned it) {
  serve_latch(sc, slots, host, 0ull, it);
}
template <bool GE>
__global__ void __launch_bounds__(COOK_WAVE* MV_EW) COOK_EVAL_OCCUPANCY match_serve_eval(const PoolCtx* __restrict__ ctx, const ServeCtl* __restrict__ sc, unsigned it) {
  __shared__ __attribute__((aligned(16))) char lds[sizeof(EvalLds<GE>)];
  const ServeLatch& cur = sc->latch[it & 1u];
  if (blockIdx.z >= cur.n) return;
  const PoolCtx& c = ctx[cur.pool[blockIdx.z]];
  if (blockIdx.x >= c.vb.C) return;
  const bool dbg = sc->dbg_fence != 0u;
  if (dbg) {
    agent_acquire();
    __syncthreads();
  }
  eval_block<GE>(lds, c.in, c.st, c.vb, c.vb.ctl->head, c.vb.ctl->wcur, blockIdx.x, blockIdx.y, gridDim.y);
  if (dbg) {
    drain_stores();
    agent_release();
  }
}
template <bool GE>
__global__ void __launch_bounds__(COOK_WAVE* MV_MW) match_serve_merge(const PoolCtx* __restrict__ ctx, ServeCtl* sc, ServeSlot* slots, ServeHost* host,
                                                                      unsigned long long poll_ticks, unsigned it) {
  __shared__ unsigned s_last;
  const ServeLatch& cur = sc->latch[it & 1u];  // (stable for the whole launch: the latch writes the OTHER one)
  const unsigned nl = cur.n;
  if (nl == 0u ? (blockIdx.x | blockIdx.z) != 0u : blockIdx.z >= nl) return;  // (an empty iteration: block 0 is the latch)
  if (nl != 0u) {
    const PoolCtx& c = ctx[cur.pool[blockIdx.z]];
    if (sc->dbg_fence != 0u) {
      agent_acquire();
      __syncthreads();
    }
    merge_block<GE>(c.in, c.vb);
    if (sc->dbg_fence != 0u) {
      drain_stores();
      agent_release();
    }
  }
  drain_stores();  // (every wave: its list entries are in the L2 before thread 0 writes the L2 back)
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned last = 1u;
    if (nl != 0u) {
      agent_release();  // this workgroup's lists are in memory before its arrival counts
      last = atomicAdd(&sc->ticket, 1u) + 1u == cur.ticket_target ? 1u : 0u;
    }
    s_last = last;
  }
  __syncthreads();
  if (s_last == 0u || threadIdx.x >= (unsigned)COOK_WAVE) return;
  serve_latch(sc, slots, host, poll_ticks, it);
}

struct WalkCtx {  // what resolve_round needs of a pool (MatchIn through vb.in_dev): small enough for MV_WALK_PACK of them in the kernel arguments
  MatchState st;
  V2Buf vb;
};
constexpr int MV_WALK_PACK = 8;
template <int N>
struct WalkPack {
  WalkCtx c[N];
};
// one walker workgroup's life: rounds until the pool is placed (or, stepping form, until a window is not served yet)
template <bool GE>
static __device__ __forceinline__ void walk_pool(char* lds, int& s_go, const MatchState& st, const V2Buf& vb, ServeSlot* slot, ServeCtl* sc,
                                                 unsigned long long spin_ticks) {
  const unsigned K = vb.in_dev->K;
  for (;;) {
    if (threadIdx.x == 0) {
      int go = 0;
      const unsigned want = ld_agent(&slot->req);  // (this workgroup's own word, or the host's first request)
      if (ld_agent(&slot->done) == 0u) {
        const unsigned long long t0 = cook_ticks();
        for (;;) {
          if (ld_agent(&slot->ready) == want) {
            go = 1;
            break;
          }
          if (spin_ticks == 0ull) break;  // stepping form: come back when served
          if (ld_agent(&sc->error) != 0u || cook_ticks() - t0 > spin_ticks) {
            st_agent(&sc->error, 1u);
            st_agent(&slot->done, 2u);
            break;
          }
          SPIN_PAUSE_FAR();
        }
        if (go == 1) {
          slot->wait_ticks += cook_ticks() - t0;
          slot->waits += 1u;
          if (sc->dbg_delay[1] != 0u) {
            const unsigned long long d0 = cook_ticks();
            while (cook_ticks() - d0 < sc->dbg_delay[1]) SPIN_PAUSE_FAR();
          }
          agent_acquire();  // ONE acquire for the workgroup: the merged lists, colbits, group rows
          if (sc->dbg_delay[2] != 0u) {
            const unsigned long long d0 = cook_ticks();
            while (cook_ticks() - d0 < sc->dbg_delay[2]) SPIN_PAUSE_FAR();
          }
        }
      }
      s_go = go;
    }
    EMU_SITE("walker: served?");
    __syncthreads();
    if (s_go != 1) return;
    if (sc->dbg_fence != 0u) {
      agent_acquire();
      __syncthreads();
    }
    resolve_round<GE>(lds, st, vb);
    const unsigned long long t_round_end = cook_ticks();
    EMU_SITE("walker: round done");
    drain_stores();   // (every wave: see drain_stores)
    if (sc->dbg_fence != 0u) agent_release();
    __syncthreads();  // the walk is over (the helper waves wait here), every store of the round has been acknowledged
    if (threadIdx.x == 0) {
      const unsigned head = vb.ctl->head;  // (written by this thread, resolve_finish)
      agent_release();  // offer state, results, group chains, the control block: in memory before the request is
      if (head >= K) {
        st_agent(&slot->done, 1u);
        s_go = 0;
      } else {
        slot->post_ticks += cook_ticks() - t_round_end;
        st_agent(&slot->req, ld_agent(&slot->req) + 1u);
      }
    }
    __syncthreads();
    if (s_go != 1) return;
  }
}
template <bool GE, int N>
__global__ void __launch_bounds__(MV_RTHREADS) match_walkers_pack(const WalkPack<N> p, ServeSlot* slots, ServeCtl* sc, unsigned long long spin_ticks) {
  __shared__ __attribute__((aligned(16))) char lds[MV_RLDS_BYTES];
  __shared__ int s_go;
  const WalkCtx& c = p.c[blockIdx.x];
  walk_pool<GE>(lds, s_go, c.st, c.vb, &slots[blockIdx.x], sc, spin_ticks);
}
template <bool GE>
__global__ void __launch_bounds__(MV_RTHREADS) match_walkers(const PoolCtx* __restrict__ ctx, ServeSlot* slots, ServeCtl* sc, unsigned long long spin_ticks) {
  __shared__ __attribute__((aligned(16))) char lds[MV_RLDS_BYTES];
  __shared__ int s_go;
  const PoolCtx& c = ctx[blockIdx.x];
  walk_pool<GE>(lds, s_go, c.st, c.vb, &slots[blockIdx.x], sc, spin_ticks);
}
