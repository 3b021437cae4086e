// classfit_host.hpp — host orchestration of the class-ordered best fit (classfit.hpp): when it is taken, its set-up, its launch.  Included by
// engine.hip inside its anonymous namespace, behind launch.hpp and g_engines_on_device; match_host.hpp attempts it for one pool,
// cook_cycle_match_multi runs the walks that are set up (cook_engine::Placement) for a device's pools in one launch.

// ---- class-ordered best fit (classfit.hpp): set-up, eligibility, launch --------------------------------------------------------------------
// match_algo 3 asks for the class-ordered best fit.  match_algo 0 (the engine's choice) takes it when six or more engines share the device: its walks need no
// evaluation launches, so eight pools cost what one costs (measured on MI355X, profiles/r06*: eight C4 pools 48.5 against 49.8 ms as served walkers, K = 1000 4.95
// against 5.11 ms), while a pool that has the GPU (nearly) to itself is faster in window rounds (one C4 pool 38.3 against 44.5 ms).  Measured per pool count (profiles/r06n_pools_5_6_7.txt,
// C4 pools, served walkers against class-ordered): 5 pools 45.4 / 46.1 ms, 6 pools 49.0 / 46.5, 7 pools 50.9 / 46.6, 8 pools 49.9 / 47.1: the rule turns at six.  COOK_CLASSFIT=1 / 0 forces / forbids
// it for match_algo 0.  (A plain function, not a namespace-scope lambda initialiser: hipcc gave the second such initialiser the body of the first)
static int classfit_env() {
  static const int v = [] {
    const char* s = std::getenv("COOK_CLASSFIT");
    return s && (s[0] == '0' || s[0] == '1') ? s[0] - '0' : -1;
  }();
  return v;
}
static bool classfit_by_default(const cook_engine* e) {
  const int f = classfit_env();
  if (f >= 0) return f == 1;
  return g_engines_on_device[e->device & 63].load() >= 6;
}
static size_t cf_lds_bytes_host(unsigned NP, unsigned M, bool eq, unsigned G, unsigned S) {  // the layout of cf_walk_pool (classfit_walk.hpp)
  size_t n = sizeof(CfFixed) + (size_t)NP * 10u;
  n = (n + 7u) & ~(size_t)7u;
  if (eq) n += (size_t)M * 8u;
  n += ((size_t)G + 1u) * 2u + (size_t)G * 2u + (size_t)S * 2u;
  return n + 64u;
}
// the three set-up kernels of a call and the look at what they found -> true: the call can be placed by cf_walk (ctx filled in)
bool cf_setup(cook_engine* e, const MatchIn& in, const MatchIn* in_dev, const MatchState& st, const JobRec* jr, const JobCons* jcons, const OfferA* oa, const OfferB* ob,
              CfPoolCtx& ctx) {
  const unsigned K = in.K, M = in.M, G = in.G;
  e->cf_inelig = 0x10000u;
  if (K == 0 || M == 0 || M > CF_SORT_N || G > CF_MAXG || in.good_enough < 1.0 || in.has_x || in.reserved_bits || in.host_dup) return false;
  if (e->cf_max_host == 0xFFFFFFFFu || (size_t)e->cf_max_host > 8u * (size_t)M + 65536u) return false;
  CfBuf b{};
  b.ctl = e->cf_ctl.ensure(1);
  b.jr = jr, b.jcons = jcons, b.oa = oa, b.ob = ob;
  b.attr8 = e->cf_attr8.ensure(M);
  b.max_host = e->cf_max_host;
  b.h2o = e->cf_h2o.ensure((size_t)b.max_host + 1u);
  b.pos_fc = e->cf_pos[0].ensure(M), b.pos_fm = e->cf_pos[1].ensure(M), b.pos_cid = e->cf_pos[2].ensure(M);
  b.scr_fc = e->cf_scr[0].ensure(M), b.scr_fm = e->cf_scr[1].ensure(M), b.scr_cid = e->cf_scr[2].ensure(M);
  b.jobs = e->cf_jobs.ensure(K);
  b.gcount = e->cf_gcount.ensure(std::max(1u, G));
  b.gmem = e->cf_gmem.ensure((size_t)std::max(1u, G) * CF_GMEM);
  static_assert(sizeof(CfCtl) % 4 == 0, "cf_init clears the control block word by word");
  KM<cf_init, 256>(e, "cf_init", std::min(div_up(b.max_host + 1u, 1024u), 512u), b, b.max_host + 1u, std::max(1u, G));
  KM<cf_scan, 256>(e, "cf_scan", div_up(std::max(K, M), 256), in_dev, b, K, M);
  KM<cf_prepare, 1024>(e, "cf_prepare", 1u, in_dev, b, st.jmin, K, M, G, in.host_dup, in.reserved_bits ? 1u : 0u);
  KM<cf_pack_jobs, 256>(e, "cf_pack_jobs", div_up(K, 256), in_dev, b, K);
  static_assert(offsetof(CfCtl, t) <= 512, "the control block's head is read back through the 512-byte scratch");
  pinned_copy(e, e->h_scratch, b.ctl, offsetof(CfCtl, t), hipMemcpyDeviceToHost);
  sync(e);
  CfCtl hc;
  std::memcpy((void*)&hc, e->h_scratch, offsetof(CfCtl, t));
  e->cf_inelig = hc.inelig;
  if (hc.inelig) return false;
  const unsigned NP = (M + 63u) & ~63u;
  const unsigned S = hc.any_group ? e->cf_group_run_total + hc.n_grouped : 0u;
  if (cf_lds_bytes_host(NP, M, hc.any_eq != 0u, hc.any_group ? G : 0u, S) > CF_LDS_BYTES || S > 60000u) {
    e->cf_inelig = CF_X_SHAPE;
    return false;
  }
  ctx.in = in_dev;
  ctx.st = st;
  ctx.b = b;
  return true;
}
// -DCF_PROF (scripts/sessions/gpu_walkprof.sh): the walk's own cycle counts of a pool, to stderr
static void cf_prof_print(const uint32_t* q) {
#ifdef CF_PROF
  std::fprintf(stderr, "CFPROF (x16 shader cycles) decider: slow steps %u (candidates %u evaluation %u commit %u) plain steps %u in %u walk-total %u | class wave 1: poll %u answer %u answers %u idle %u idles %u | class wave 2: poll %u answer %u answers %u idle %u idles %u | walk ticks(100MHz) %u | batch boundaries: decider %u, batches without a walked job %u\n", q[27], q[24], q[25], q[26], q[28], q[29], q[31], q[32], q[33], q[35], q[36], q[37], q[40], q[41], q[43], q[44], q[45], q[CFS_TICKS_WALK], q[30], q[38]);
  std::fprintf(stderr, "CFPROF plain steps %u, C++ steps %u; steps that left the plain form: gpu kind %u, novel hosts %u, group %u, answer missing after the re-reads %u, guard band %u, epoch end %u\n", q[46], q[47], q[34] & 65535u, q[34] >> 16, q[39] & 65535u, q[39] >> 16, q[42] & 65535u, q[42] >> 16);
#else
  (void)q;
#endif
}
// cf_walk for the given engines (pools of one device, each with a walk set up) on `stream`, their group chains, the books of each
void cf_run(cook_engine* lead, cook_engine* const* es, unsigned n, hipStream_t stream) {
  cook_engine* e = lead;
  for (unsigned i0 = 0; i0 < n; i0 += (unsigned)CF_PACK) {
    const unsigned c = std::min<unsigned>(CF_PACK, n - i0);
    CfPack pk{};
    for (unsigned x = 0; x < (unsigned)CF_PACK; ++x) pk.c[x] = es[i0 + (x < c ? x : 0u)]->placement.walk;
    KLS("cf_walk", stream, cf_walk, c, CF_THREADS, pk);
  }
  for (unsigned i = 0; i < n; ++i) {
    const CfPoolCtx& c = es[i]->placement.walk;
    const unsigned G = es[i]->last_in.G;
    if (G) KLS("cf_group_chains", stream, cf_group_chains, div_up(G, 256), 256, c.b, c.st, G);
  }
  constexpr size_t SLOT = 16 + 48 * 4;  // a pool's summary words and statistics
  if (!lead->h_cf) COOK_HIP(hipHostMalloc((void**)&lead->h_cf, 64 * SLOT, hipHostMallocDefault));  // (at most 64 pools: pools_set_up, match_host.hpp)
  for (unsigned i = 0; i < n; ++i) {
    char* slot = lead->h_cf + i * SLOT;
    COOK_HIP(hipMemcpyAsync(slot, es[i]->placement.walk.st.summary, 16, hipMemcpyDeviceToHost, stream));
    COOK_HIP(hipMemcpyAsync(slot + 16, es[i]->placement.walk.b.ctl->stats, 48 * 4, hipMemcpyDeviceToHost, stream));
  }
  COOK_HIP(hipStreamSynchronize(stream));
  for (unsigned i = 0; i < n; ++i) {
    cook_engine* x = es[i];
    const unsigned* sum = (const unsigned*)(lead->h_cf + i * SLOT);
    if (sum[3] == 0xDEADu) lead->fail(COOK_E_STATE, "cf_walk: the pool's tables do not fit the workgroup's LDS (the host's check let it through)");
    std::memcpy(x->cf_stats, lead->h_cf + i * SLOT + 16, 48 * 4);
    cf_prof_print(x->cf_stats);
    WinCtl c{};
    c.matched = sum[0], c.head_matched = sum[1], c.rounds = sum[2], c.head = x->last_in.K, c.visited_sum = x->cf_stats[CFS_WALKED];
    c.t_seq = x->cf_stats[CFS_TICKS_TOTAL], c.t_setup = x->cf_stats[CFS_TICKS_PROLOGUE];
    x->placement_complete(3, c);
  }
}
