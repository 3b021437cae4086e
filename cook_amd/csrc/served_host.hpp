// served_host.hpp — the pools of a device placed by served walkers (match_v2_served.hpp): the other form of cook_cycle_match_multi.
// Included by engine.hip inside its anonymous namespace, behind match_host.hpp (pools_set_up, pools_gather, pools_read_ctl,
// match_finish_rounds — which completes a pool's placement —, pack_args).

// COOK_MATCH_SERVED=0: cook_cycle_match_multi always runs its pools in lockstep launches (match_rounds_multi); default: served walkers
static bool served_enabled() {
  const char* s = std::getenv("COOK_MATCH_SERVED");
  return !(s && std::atoi(s) == 0);
}
// the stepping form (nothing waits on the device; the host alternates walker launches, latches and serve iterations): always in the
// emulated build, whose launches run one after the other; COOK_SERVE_STEP=1 forces it on the GPU (A/B, debugging)
static bool served_stepping() {
#ifdef __HIP_EMU__
  return true;
#else
  const char* s = std::getenv("COOK_SERVE_STEP");
  return s && std::atoi(s) != 0;
#endif
}
static unsigned long long env_ticks(const char* name, double dflt_us) {
  const char* s = std::getenv(name);
  const double us = s ? std::atof(s) : dflt_us;
  return (unsigned long long)(std::max(0.0, us) * 100.0);  // 100 MHz
}

// The placements of n engines (pools of one rank, same device) by persistent walkers — one workgroup per pool, ONE launch — beside
// serve iterations (evaluation + merge for the pools that asked) on a second stream: match_v2_served.hpp.  -> false: the
// served match gave up (a walker was not served in time); the pools are in a consistent state and the caller finishes them in lockstep.
bool match_rounds_served(cook_engine** es, unsigned n) {
  cook_engine* lead = es[0];
  cook_engine* e = lead;  // KL / KLS time and launch on the lead engine
  const std::vector<cook_engine*> live = pools_set_up(es, n, cook_engine::Placement::ROUNDS);
  const unsigned L = (unsigned)live.size();
  lead->served = cook_engine::ServedStats{};
  if (L == 0) return true;
  if (L > MV_SERVE_MAX) return false;
  constexpr unsigned MAXS = cook_engine::kMaxServers;
  if (!lead->s_walk) {
    // The walkers' stream must never share a HARDWARE queue with a serve stream: a serve launch queued behind the persistent walker
    // launch would wait for walkers that wait for it (seen with eight serve streams on GPU_MAX_HW_QUEUES=8: every cycle ran into the
    // walkers' time-out).  HIP hands streams of different priorities queues of different pools, so the walkers get the only
    // high-priority stream of the process; the serve streams are ordinary ones (two of them on one queue would only take turns).
    int prio_least = 0, prio_greatest = 0;
    COOK_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    COOK_HIP(hipStreamCreateWithPriority(&lead->s_walk, hipStreamNonBlocking, prio_greatest));
    COOK_HIP(hipHostMalloc((void**)&lead->h_serve, MAXS * sizeof(ServeHost), hipHostMallocDefault));
  }
  // SERVERS: streams of serve iterations, each for its own share of the pools (pool x -> server x mod S).  An iteration is a chain of
  // latency-bound launches that leaves most of the chip idle (a window of 300 jobs is 980 waves for 4 096 slots), so two or three of
  // them side by side serve the walkers sooner than one; the walkers' launch makes S + 1 streams.
  unsigned S = 3;  // (eight pools on MI355X: 1 / 2 / 3 / 4 servers 56.6 / 53.7 / 52.7 / 57.3 ms: walkers + three servers are the four streams the part runs at full speed)
  if (const char* ev = std::getenv("COOK_SERVE_STREAMS")) S = (unsigned)std::max(1, std::atoi(ev));
  S = std::min(std::min(S, MAXS), L);
  for (unsigned sv = 0; sv < S; ++sv)
    if (!lead->s_serve[sv]) COOK_HIP(hipStreamCreateWithFlags(&lead->s_serve[sv], hipStreamNonBlocking));
  const PoolsOfLaunch g = pools_gather(lead, live);
  const std::vector<PoolCtx>& hctx = g.hctx;
  PoolCtx* dctx = lead->w_pctx.ensure(L);
  ServeSlot* slots = lead->w_slots.ensure(L);
  ServeCtl* sctl = lead->w_sctl.ensure(MAXS);
  std::vector<ServeSlot> hslots(L);
  for (unsigned x = 0; x < L; ++x) {
    std::memset((void*)&hslots[x], 0, sizeof(ServeSlot));
    hslots[x].req = 1u;  // the first window of every pool: asked for here
    hslots[x].claim = 1u;  // ... and given to a server here (the first iterations' lists below)
  }
  // DYNAMIC assignment (default; COOK_SERVE_DYNAMIC=0: pool x belongs to server x mod S for the whole call): every server looks at every pool and
  // takes the open requests it sees first — a walker's request no longer queues behind its neighbours' on ONE server while another polls an empty list
  // (measured: 133 us from request to lists on the servers with three pools, 107-123 on the one with two: profiles/r05zz_serve_trace.txt)
  const bool dynamic = !(std::getenv("COOK_SERVE_DYNAMIC") && std::atoi(std::getenv("COOK_SERVE_DYNAMIC")) == 0);
  const unsigned claim_max = std::max(1u, div_up(L, S));
  std::vector<ServeCtl> hs(S);
  unsigned zmax = 1;
  for (unsigned sv = 0; sv < S; ++sv) {
    std::memset(&hs[sv], 0, sizeof(ServeCtl));
    hs[sv].pool_first = sv;
    hs[sv].pool_stride = S;
    hs[sv].dbg_fence = std::getenv("COOK_SERVE_FENCE") && std::atoi(std::getenv("COOK_SERVE_FENCE")) ? 1u : 0u;
    unsigned cnt = 0;
    for (unsigned x = sv; x < L; x += S) hs[sv].latch[0].pool[cnt] = x, hs[sv].latch[0].seq[cnt] = 1u, ++cnt;
    hs[sv].n_pools = hs[sv].latch[0].n = cnt;
    hs[sv].latch[0].ticket_target = cnt * (unsigned)MV_MERGE_BLOCKS;
    if (dynamic) hs[sv].n_pools = L, hs[sv].pool_first = 0u, hs[sv].pool_stride = 1u, hs[sv].claim_max = claim_max;
    hs[sv].dbg_delay[0] = (unsigned)env_ticks("COOK_SERVE_DELAY_PUBLISH_US", 0.0);
    hs[sv].dbg_delay[1] = (unsigned)env_ticks("COOK_SERVE_DELAY_ACQ_US", 0.0);
    hs[sv].dbg_delay[2] = (unsigned)env_ticks("COOK_SERVE_DELAY_READ_US", 0.0);
    zmax = std::max(zmax, cnt);
  }
  if (dynamic) zmax = std::max(zmax, std::min(L, claim_max));
  ServeHost* hh = lead->h_serve;
  std::memset(hh, 0, MAXS * sizeof(ServeHost));
  hipStream_t s0 = lead->s_serve[0];
  COOK_HIP(hipMemcpyAsync(dctx, hctx.data(), L * sizeof(PoolCtx), hipMemcpyHostToDevice, s0));
  COOK_HIP(hipMemcpyAsync(slots, hslots.data(), L * sizeof(ServeSlot), hipMemcpyHostToDevice, s0));
  COOK_HIP(hipMemcpyAsync(sctl, hs.data(), S * sizeof(ServeCtl), hipMemcpyHostToDevice, s0));
  COOK_HIP(hipStreamSynchronize(s0));  // (pageable sources; and the walkers must find their slots initialised)
  WalkPack<MV_WALK_PACK> wp{};
  const bool packed = L <= (unsigned)MV_WALK_PACK && pack_args();
  for (unsigned x = 0; x < (unsigned)MV_WALK_PACK; ++x) {
    wp.c[x].st = hctx[x < L ? x : 0].st;
    wp.c[x].vb = hctx[x < L ? x : 0].vb;
  }
  const bool stepping = served_stepping();
  const bool one_stream = std::getenv("COOK_SERVE_ONE_STREAM") && std::atoi(std::getenv("COOK_SERVE_ONE_STREAM"));  // (diagnostics: the servers' iterations all on one stream)
  const unsigned long long spin = stepping ? 0ull : env_ticks("COOK_SERVE_WALK_TIMEOUT_US", 2.5e5);  // a walker not served for 250 ms gives up (a cycle is 50)
  const unsigned long long poll = stepping ? 0ull : env_ticks("COOK_SERVE_POLL_US", 40.0);          // the latch waits that long for a request
  std::vector<unsigned> launched(S, 0u);  // serve iterations launched, per server
  auto walkers = [&](auto ge_tag) {
    constexpr bool GE = decltype(ge_tag)::value;
    if (packed) KLS("match_walkers", lead->s_walk, (match_walkers_pack<GE, MV_WALK_PACK>), L, MV_RTHREADS, wp, slots, sctl, spin);
    else KLS("match_walkers", lead->s_walk, match_walkers<GE>, L, MV_RTHREADS, (const PoolCtx*)dctx, slots, sctl, spin);
  };
  auto serve = [&](auto ge_tag, unsigned sv) {
    constexpr bool GE = decltype(ge_tag)::value;
    hipStream_t st_ = lead->s_serve[one_stream ? 0u : sv];
    const unsigned it = launched[sv];  // the iteration's number picks its latch list (ServeLatch)
    KLS("match_serve_eval", st_, match_serve_eval<GE>, dim3(g.cmax, MV_JG, zmax), COOK_WAVE * MV_EW, (const PoolCtx*)dctx, (const ServeCtl*)(sctl + sv), it);
    KLS("match_serve_merge", st_, match_serve_merge<GE>, dim3(MV_MERGE_BLOCKS, 1, zmax), COOK_WAVE * MV_MW, (const PoolCtx*)dctx, sctl + sv, slots, hh + sv, poll, it);
    ++launched[sv];
  };
  auto launch_walkers = [&] { g.any_ge ? walkers(std::true_type{}) : walkers(std::false_type{}); };
  auto launch_serve = [&](unsigned sv) { g.any_ge ? serve(std::true_type{}, sv) : serve(std::false_type{}, sv); };
  volatile ServeHost* vh = hh;
  auto all_done = [&] {
    for (unsigned sv = 0; sv < S; ++sv)
      if (!vh[sv].all_done) return false;
    return true;
  };
  auto any_error = [&] {
    for (unsigned sv = 0; sv < S; ++sv)
      if (vh[sv].error) return true;
    return false;
  };
  auto sync_servers = [&] {
    for (unsigned sv = 0; sv < S; ++sv) COOK_HIP(hipStreamSynchronize(lead->s_serve[sv]));
  };
  bool stuck = false;
  if (stepping) {
    unsigned guard = 0;
    for (;;) {
      // (one phase at a time, on the GPU too: the latch launch publishes nothing and expects to find every open request unlatched)
      for (unsigned sv = 0; sv < S; ++sv) launch_serve(sv);  // evaluates what the latch put together (first: every pool's first window), publishes
      sync_servers();
      launch_walkers();   // every pool walks the windows it has been served, asks for the next, returns
      COOK_HIP(hipStreamSynchronize(lead->s_walk));
      for (unsigned sv = 0; sv < S; ++sv) KLS("match_serve_latch", lead->s_serve[sv], match_serve_latch, 1, COOK_WAVE, sctl + sv, slots, hh + sv, launched[sv] - 1u);
      sync_servers();
      if (all_done() || any_error()) break;
      if (++guard > 4000000u) lead->fail(COOK_E_STATE, "cook_cycle_match_multi: served placement made no progress");
    }
  } else {
    launch_walkers();
    // serve iterations, a few ahead of the device: each ends with the latch waiting (bounded) for the next request, so every server's chain
    // is paced by its walkers; iter_done / all_done arrive in page-locked memory
    constexpr unsigned DEPTH = 3;
    const auto t_begin = std::chrono::steady_clock::now();
    unsigned long long spins = 0;
    while (!all_done() && !any_error()) {
      bool any = false;
      for (unsigned sv = 0; sv < S; ++sv) {
        if (vh[sv].all_done || launched[sv] - vh[sv].iter_done >= DEPTH) continue;
        launch_serve(sv);
        any = true;
      }
      if (!any && (++spins & 0xFFFFull) == 0ull && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count() > 30.0) {
        stuck = true;  // (the walkers give up on their own after COOK_SERVE_WALK_TIMEOUT_US without being served)
        break;
      }
    }
    sync_servers();
    COOK_HIP(hipStreamSynchronize(lead->s_walk));
    if (stuck) lead->fail(COOK_E_STATE, "cook_cycle_match_multi: the serve launches stopped finishing");
  }
  // what the pools reached
  std::vector<WinCtl> hc;
  COOK_HIP(hipMemcpyAsync(hs.data(), sctl, S * sizeof(ServeCtl), hipMemcpyDeviceToHost, s0));
  static const bool serve_trace = std::getenv("COOK_SERVE_TRACE") != nullptr;
  if (serve_trace) COOK_HIP(hipMemcpyAsync(hslots.data(), slots, L * sizeof(ServeSlot), hipMemcpyDeviceToHost, s0));
  pools_read_ctl(lead, hctx, hc, s0);  // (synchronises s0: the two copies above have arrived too)
  if (serve_trace) {  // the walkers' and the servers' own accounts of the call (100 MHz ticks -> microseconds)
    for (unsigned x = 0; x < L; ++x)
      std::fprintf(stderr, "SERVETRACE pool %u: %u windows waited for, %.1f us each from request to lists, %.1f us from the end of a round to its request\n", x,
                   hslots[x].waits, hslots[x].waits ? hslots[x].wait_ticks / 100.0 / hslots[x].waits : 0.0,
                   hslots[x].waits ? hslots[x].post_ticks / 100.0 / hslots[x].waits : 0.0);
    for (unsigned sv = 0; sv < S; ++sv) {
      const unsigned work = hs[sv].iterations - hs[sv].empty_iterations;
      std::fprintf(stderr, "SERVETRACE server %u: %u iterations with work (%u pool windows), %.1f us each from its list to its results; %u empty iterations, %.1f ms waiting for requests\n",
                   sv, work, hs[sv].pools_served, work ? hs[sv].busy_ticks / 100.0 / work : 0.0, hs[sv].empty_iterations, hs[sv].wait_ticks / 1.0e5);
    }
  }
  bool complete = true;
  for (unsigned x = 0; x < L; ++x) {
    live[x]->placement.c0 = hc[x];  // (where a lockstep continuation would start)
    complete = complete && hc[x].head >= live[x]->placement.k;
  }
  lead->served.mode = stepping ? 2u : 1u;
  lead->served.pools = L;
  lead->served.servers = S;
  for (unsigned sv = 0; sv < S; ++sv) {
    lead->served.iterations += hs[sv].iterations;
    lead->served.empty_iterations += hs[sv].empty_iterations;
    lead->served.pools_served += hs[sv].pools_served;
    lead->served.latch_wait_ms += (double)hs[sv].wait_ticks / 1.0e5;
  }
  if (!complete) {
    lead->served.fell_back = 1;
    return false;
  }
  for (unsigned x = 0; x < L; ++x) match_finish_rounds(live[x], hctx[x].st, hctx[x].vb, hc[x], s0);
  return true;
}
