// match_host.hpp — host orchestration of the match (cook_match_*, and the match of a cycle): staging of jobs, offers and groups; one pool's
// placement in named pieces (match_run_device); the pools of a device in lockstep rounds (match_rounds_multi).  Included by engine.hip
// inside its anonymous namespace, behind launch.hpp, classfit_host.hpp (cf_setup, cf_run) and g_engines_on_device; expects match_kernels.hpp
// and match_v2.hpp.  served_host.hpp and the side features use its staging and pools_set_up / pools_gather / pools_read_ctl /
// match_finish_rounds / pack_args.  Where a pool's match is, is ONE member of the engine (cook_engine::Placement): match_defer and
// match_try_classfit enter a set-up; the ways out are placement_drop (match_run_device, match_stage_inputs, cycle_update, a
// cook_cycle_match_multi that failed after its first launch) and placement_complete (match_finish_rounds, cf_run, the sweep and K = 0).

// The placement walk keeps one LDS byte per offer of the pool.  A pool in a lockstep chain runs the good-enough flavour of the kernels
// whenever ANY pool of its chain has good-enough < 1 (match_rounds_multi), so the table must leave room for segments in both.
// the spreaders (cook_params.fitness 3..5) are placed by the serial sweep whatever match_algo says (match_run_device)
static bool fitness_is_spreader(const cook_engine* e) { return e->params.fitness >= COOK_FITNESS_CPU_MEM_SPREADER; }
void match_check_offer_count(cook_engine* e, unsigned M) {
  if (e->params.match_algo == 1 || fitness_is_spreader(e)) return;  // (the one-job-at-a-time sweep has no such table)
  if (std::min(resolve_wseg<true>(M), resolve_wseg<false>(M)) < MV_WSEG_MIN)
    e->fail(COOK_E_INVALID, "cook_match: too many offers in one pool for the placement walk's offer table (about 150 000)");
}
// entries per host of a k8s "gpus" / "disk" map column pair (cookmatch.h cook_offers.gpu_slots): 0 means 1
unsigned res_slots(cook_engine* e, uint32_t slots, const char* what) {
  if (slots > COOK_MAX_RES_SLOTS) e->fail(COOK_E_INVALID, std::string(what) + " > COOK_MAX_RES_SLOTS");
  return slots ? slots : 1u;
}

// =================================================================================================================
// MATCH
// =================================================================================================================
// What the host keeps of a freshly staged offer table's host column, for both staging routes (match_stage_offers, cycle_update.hpp's
// offers_block_commit): two offers on one host?, the greatest host id (the class-ordered walk's and the release's host tables are sized
// by it), and the ascending mirror a host churn is checked against.  on_host false: the column is on the device, nothing is known
void offers_note_hosts(cook_engine* e, const uint32_t* host, unsigned M, bool on_host) {
  e->min.host_dup = 0;
  e->cf_max_host = 0xFFFFFFFFu;
  e->o_hosts.clear();
  e->o_run_cols_made = false;
  e->o_hosts_known = on_host;
  e->offers_built = !on_host;
  if (!on_host || !M) return;
  std::vector<uint32_t> hs(host, host + M);
  std::sort(hs.begin(), hs.end());
  e->min.host_dup = std::adjacent_find(hs.begin(), hs.end()) != hs.end() ? 1u : 0u;
  e->cf_max_host = hs.back();
  e->o_hosts = std::move(hs);
}

// the offer columns of a staged match (cook_match_stage / cook_cycle_stage; cook_cycle_update's come in one block: cycle_update.hpp): every
// column of offer_columns, a device pointer used in place, a host column uploaded into the engine's OfferStore
void match_stage_offers(cook_engine* e, const cook_offers* o, bool offers_dev) {
  MatchIn& in = e->min;
  const unsigned M = o->n;
  if (M && (!o->cpus || !o->mem || !o->host)) e->fail(COOK_E_INVALID, "cook_match_stage: offers need cpus, mem and host");
  OfferDims d{};
  d.gpu_slots = res_slots(e, o->gpu_slots, "cook_match_stage: gpu_slots");
  d.disk_slots = res_slots(e, o->disk_slots, "cook_match_stage: disk_slots");
  d.n_attr = o->attr ? o->n_attr_keys : 0;
  if (o->gpu_model && !o->gpu_count) e->fail(COOK_E_INVALID, "cook_match_stage: gpu_model without gpu_count");
  // ports / named scalars of the leases (offer.clj:57-73); jobs' names beyond the offers' columns find a total of 0
  if (o->scalars && o->n_scalars > COOK_MAX_SCALARS) e->fail(COOK_E_INVALID, "cook_match_stage: more than COOK_MAX_SCALARS named scalars");
  OfferCols<false> c{};
  offer_columns([&](const auto& col) {
    const auto* given = col.of(*o);
    col.col(c) = offers_dev ? given : h2d_opt(e, col.col(e->offers), given, (size_t)M * d.width(col.kind));
  });
  offer_cols_stage(in, c, d, M);
  e->M = M;
  offers_note_hosts(e, o->host, M, !offers_dev);  // (offers built on the device are one per node: no two on one host)
}
void match_stage_offers(cook_engine* e, const cook_offers* o) {
  match_stage_offers(e, o, false);
  sync(e);
}

// offers_dev: the pointers of `o` are DEVICE columns (the rows of cook_offers_run): used in place, nothing is copied
void match_stage_inputs(cook_engine* e, const cook_jobs* j, const cook_offers* o, const cook_groups* g,
                        const uint32_t* reserved_hosts, uint32_t n_reserved, bool offers_dev = false) {
  if (!j || !o) e->fail(COOK_E_INVALID, "cook_match_stage: null jobs/offers");
  e->cycle_cons_ran = false;
  const unsigned K = j->n, M = o->n, G = g ? g->n : 0;
  if (K && (!j->cpus || !j->mem)) e->fail(COOK_E_INVALID, "cook_match_stage: jobs need cpus and mem");
  if (M && (!o->cpus || !o->mem || !o->host)) e->fail(COOK_E_INVALID, "cook_match_stage: offers need cpus, mem and host");
  if (j->group && !g) {
    for (unsigned k = 0; k < K; ++k)
      if (j->group[k] != COOK_NONE_U32) e->fail(COOK_E_INVALID, "cook_match_stage: job has a group but no groups table given");
  }
  if (j->group && g)
    for (unsigned k = 0; k < K; ++k)
      if (j->group[k] != COOK_NONE_U32 && j->group[k] >= G) e->fail(COOK_E_INVALID, "cook_match_stage: group id out of range");
  // a pool beyond the walk's owner table is refused HERE, with the other checks on the inputs and under the params in force NOW: behind a
  // refused cook_match_stage the last match and its inputs are whole and can still be fetched (cook_cycle_stage has restaged the rank's
  // inputs by then, as for its other checks).  match_run_device asks again, since cook_engine_set_params may come in between: a pool staged
  // under the serial sweep (no such table) and run under the window rounds is refused only there, the last match's state already reset; one
  // staged under the window rounds is refused here even if the sweep was meant to run it — set the params first
  if (K) match_check_offer_count(e, M);
  e->placement_drop();  // (the columns below may move: a set-up would point at freed ones)
  reserve_drop(e);      // (the engine's own reservation map and `launched` go with the rows they index)
  MatchIn& in = e->min;
  std::memset(&in, 0, sizeof(in));
  in.K = K;
  in.M = M;
  in.G = G;
  e->Kjobs = K;
  e->cf_group_run_total = 0;
  e->q_valid = false, e->q_groups_own = false;
  e->h_g_type.clear(), e->h_g_key.clear(), e->h_g_min.clear();
  if (G && g->type && g->attr_key && g->minimum)
    e->h_g_type.assign(g->type, g->type + G), e->h_g_key.assign(g->attr_key, g->attr_key + G), e->h_g_min.assign(g->minimum, g->minimum + G);
  in.j_cpus = h2d_opt(e, e->j_cpus, j->cpus, K);
  in.j_mem = h2d_opt(e, e->j_mem, j->mem, K);
  in.j_gpus = h2d_opt(e, e->j_gpus, j->gpus, K);
  in.j_gpu_model = h2d_opt(e, e->j_gpu_model, j->gpu_model, K);
  e->has_j_user = h2d_opt(e, e->j_user, j->user, K) != nullptr;
  in.j_group = h2d_opt(e, e->j_group, j->group, K);
  if (j->eq_off) {
    in.j_eq_off = h2d_opt(e, e->j_eq_off, j->eq_off, K + 1);
    const unsigned ne = K ? j->eq_off[K] : 0;
    in.j_eq_key = h2d_opt(e, e->j_eq_key, j->eq_key, std::max(1u, ne));
    in.j_eq_val = h2d_opt(e, e->j_eq_val, j->eq_val, std::max(1u, ne));
  }
  if (j->novel_off) {
    in.j_novel_off = h2d_opt(e, e->j_novel_off, j->novel_off, K + 1);
    const unsigned nn = K ? j->novel_off[K] : 0;
    in.j_novel_host = h2d_opt(e, e->j_novel_host, j->novel_host, std::max(1u, nn));
  }
  in.j_reserved_host = h2d_opt(e, e->j_reserved_host, j->reserved_host, K);
  in.j_ckpt = h2d_opt(e, e->j_ckpt, j->ckpt_location, K);
  in.j_est_end = h2d_opt(e, e->j_est_end, j->est_end_ms, K);
  in.j_disk_req = h2d_opt(e, e->j_disk_req, j->disk_request, K);
  in.j_disk_type = h2d_opt(e, e->j_disk_type, j->disk_type, K);
  if (in.j_disk_req && !in.j_disk_type) e->fail(COOK_E_INVALID, "cook_match_stage: disk_request without disk_type");
  // ports / named scalar requests (scheduler.clj:466, 177-189): has_x = some job asks for any
  if (j->scalars && j->n_scalars > COOK_MAX_SCALARS) e->fail(COOK_E_INVALID, "cook_match_stage: more than COOK_MAX_SCALARS named scalars");
  unsigned has_x = 0;
  in.j_ports = h2d_opt(e, e->j_ports, j->ports, K);
  if (j->ports)
    for (unsigned k = 0; k < K; ++k) {
      if (j->ports[k] < 0) e->fail(COOK_E_INVALID, "cook_match_stage: negative port count");
      has_x |= j->ports[k] > 0;
    }
  const unsigned n_scal = j->scalars ? j->n_scalars : 0u;
  for (unsigned sc = 0; sc < n_scal; ++sc) {
    const double* col = j->scalars + (size_t)sc * K;
    in.j_scal[sc] = h2d_opt(e, e->j_scal[sc], col, K);
    for (unsigned k = 0; k < K && !has_x; ++k) has_x = col[k] == col[k];
  }
  match_stage_offers(e, o, offers_dev);
  in.n_scal = n_scal;
  in.has_x = has_x;
  e->groups_simple = true;
  for (unsigned x = 0; x < G; ++x)
    if (g->type && g->type[x] >= 2) e->groups_simple = false;
  if (G) {
    in.g_type = h2d_opt(e, e->g_type, g->type, G);
    in.g_attr_key = h2d_opt(e, e->g_attr_key, g->attr_key, G);
    in.g_min = h2d_opt(e, e->g_min, g->minimum, G);
    if (!in.g_type || !in.g_attr_key || !in.g_min) e->fail(COOK_E_INVALID, "cook_match_stage: groups need type, attr_key, minimum");
    e->cf_group_run_total = g->run_off ? g->run_off[G] : 0u;
    if (g->run_off) {
      in.g_run_off = h2d_opt(e, e->g_run_off, g->run_off, G + 1);
      const unsigned nr = g->run_off[G];
      in.g_run_host = h2d_opt(e, e->g_run_host, g->run_host, std::max(1u, nr));
      in.g_run_attr = h2d_opt(e, e->g_run_attr, g->run_attr, std::max(1u, nr));
    }
  }
  std::vector<uint32_t> bits;
  if (n_reserved) {
    uint32_t mx = 0;
    for (unsigned i = 0; i < n_reserved; ++i) mx = std::max(mx, reserved_hosts[i]);
    bits.assign(mx / 32 + 1, 0u);
    for (unsigned i = 0; i < n_reserved; ++i) bits[reserved_hosts[i] >> 5] |= 1u << (reserved_hosts[i] & 31);
    in.reserved_bits = h2d_opt(e, e->reserved_bits, bits.data(), bits.size());
    in.reserved_words = (unsigned)bits.size();
  }
  in.good_enough = e->params.good_enough_fitness;
  in.host_lifetime_mins = e->params.host_lifetime_mins;
  in.fitness = (unsigned)e->params.fitness;
  sync(e);  // `bits` is a host temporary
  e->K = K;
  e->M = M;
  e->G = G;
  e->match_staged = true;
}

// the state a match call starts from, in ONE launch (nine memsets before round 5: each is a launch, and the set-up of a pool's match sits
// in the chain of small launches a cycle begins with): nothing assigned, no job placed, jmin = {max, max, 0, 0}
COOK_KERNEL void match_init_state_kernel(MatchState st, unsigned long long* __restrict__ jmin, unsigned K, unsigned M, unsigned G, unsigned nblk) {
  const unsigned stride = nblk * blockDim.x;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
    st.ac[i] = 0.0, st.am[i] = 0.0, st.acount[i] = 0;
    if (st.xports) {
      st.xports[i] = 0;
      for (unsigned s = 0; s < (unsigned)COOK_MAX_SCALARS; ++s) st.xscal[(size_t)s * M + i] = 0.0;
    }
  }
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < G; i += stride) st.group_last[i] = -1;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < K; i += stride) st.job_prev[i] = -1, st.job_to_offer[i] = -1;
  if (blockIdx.x == 0 && threadIdx.x < 4) {
    st.summary[threadIdx.x] = 0u;
    jmin[threadIdx.x] = threadIdx.x < 2 ? 0x7F7F7F7F7F7F7F7Full : 0ull;  // [0..1] > every finite double's bit pattern; [2] a job with a
                                                                             // negative / non-finite request was seen
  }
}
void match_init_state(cook_engine* e, const MatchState& st, unsigned K, unsigned M, unsigned G) {
  const unsigned n = std::max(std::max(K, M), std::max(G, 1u));
  KM<match_init_state_kernel, 256>(e, "match_init_state", std::min(div_up(n, 256), 512u), st, e->m_jmin.ptr(), K, M, G, std::min(div_up(n, 256), 512u));
}

// rounds launched between two looks at the pools' progress.  The estimate comes from the rate of the last batch; when the cluster
// fills up in the middle of a batch the rest of the queue settles thousands of jobs per round and what is left of the batch are
// launches that exit at once (145 of a chain's 520 rounds at a cap of 256): cheap each, not free together.
static unsigned batch_cap() {
  static const unsigned cap = [] {
    const char* s = std::getenv("COOK_BATCH_CAP");
    const long v = s ? std::atol(s) : 0;
    return (unsigned)(v >= 2 ? v : 64);  // (256 / 96 / 48 / 24: eight pools 82.7 / 81.9 / 82.0 / 82.8 ms, one pool 57.5 / 57.1 / 56.9 / 56.6)
  }();
  return cap;
}
// the rounds a pool still needs at the jobs-per-round of its last batch (prev: its control block at the look before)
static double rounds_left(unsigned K, const WinCtl& now, const WinCtl& prev) {
  const double per_round = (double)(now.head - prev.head) / std::max(1u, now.rounds - prev.rounds);
  return (K - now.head) / std::max(1.0, per_round);
}
// the next batch, from the worst such estimate over the pools of the launch (over-launching is cheap: finished rounds exit at once)
static unsigned next_batch(double est) { return (unsigned)std::min((double)batch_cap(), std::max(2.0, est * 1.05 + 2.0)); }
// COOK_PACK_ARGS=0: the multi-pool launches read their contexts from memory even when they would fit the kernel arguments (A/B switch)
static bool pack_args() {
  static const bool on = [] {
    const char* s = std::getenv("COOK_PACK_ARGS");
    return !(s && std::atoi(s) == 0);
  }();
  return on;
}
// one round of launches on the engine's stream, for ONE pool: GE = the call runs with good-enough-fitness < 1 (the resolve kernel whose
// fast path knows the rule)
template <bool GE>
static void launch_round(cook_engine* e, const MatchIn& in, const MatchState& st, const V2Buf& vb) {
  KL("match_eval2", match_eval2<GE>, dim3(vb.C, MV_JG), COOK_WAVE * MV_EW, in, st, vb);
  KL("match_merge2", match_merge2<GE>, MV_MERGE_BLOCKS, COOK_WAVE * MV_MW, in, vb);
  KL("match_resolve2", match_resolve2<GE>, 1, MV_RTHREADS, st, vb);
}

// after the last round: statistics, the optional per-round log, the summary words of cook_*_fetch; the pool's placement is complete
void match_finish_rounds(cook_engine* e, const MatchState& st, const V2Buf& vb, const WinCtl& hc, hipStream_t stream) {
  const char* rlog_path = std::getenv("COOK_ROUND_LOG");
  if (rlog_path && vb.round_log) {
    std::vector<RoundLog> h(std::min(hc.rounds, MV_ROUND_LOG_CAP));
    if (!h.empty()) COOK_HIP(hipMemcpy(h.data(), vb.round_log, h.size() * sizeof(RoundLog), hipMemcpyDeviceToHost));
    // one file per engine when the path ends in '@' (several pools in one process): "<path minus @>.<engine number>"
    static std::atomic<unsigned> g_rlog_seq{0};
    std::string path = rlog_path;
    if (!path.empty() && path.back() == '@') {
      if (e->rlog_id == 0) e->rlog_id = ++g_rlog_seq;
      path = path.substr(0, path.size() - 1) + "." + std::to_string(e->rlog_id);
    }
    if (FILE* f = std::fopen(path.c_str(), "w")) {
      std::fprintf(f, "head,wcur,resolved,n_list,touched,stop,matched,setup_us,seq_us,segments,h_cinfo,h_state,h_alive,h_col\n");
      for (auto& r : h)
        std::fprintf(f, "%u,%u,%u,%u,%u,%u,%u,%.2f,%.2f,%u,%08x,%08x,%08x,%08x\n", r.head, r.wcur, r.resolved, r.n_list, r.touched, r.stop, r.matched,
                     r.setup_ticks / 100.0, r.seq_ticks / 100.0, r.segments, r.h_cinfo, r.h_state, r.h_alive, r.h_col);
      std::fclose(f);
    }
  }
#ifdef COOK_WALK_PROF
  {
    static const char* cat[8] = {"shortcut", "touched_wins", "new_lane", "unmatched", "grouped", "exact", "touched_wins_by_good_enough", "fast_turn_that_left_the_loop"};
    std::fprintf(stderr, "WALKPROF rounds=%u", hc.rounds);
    for (int i = 0; i < 8; ++i)
      std::fprintf(stderr, " %s:n=%u,cyc/job=%.0f", cat[i], hc.prof_cnt[i], hc.prof_cnt[i] ? (double)hc.prof_cyc[i] / hc.prof_cnt[i] : 0.0);
    std::fprintf(stderr, "\n");
  }
#endif
  unsigned sum[4] = {hc.matched, (hc.matched == 0 || hc.head_matched) ? 1u : 0u, hc.rounds, 0u};
  std::memcpy(e->h_scratch, sum, 16);
  COOK_HIP(hipMemcpyAsync(st.summary, e->h_scratch, 16, hipMemcpyHostToDevice, stream));
  COOK_HIP(hipStreamSynchronize(stream));
  e->placement_complete(0, hc);
}

// ---- one pool's match, in named pieces (match_run_device below puts them together) ------------------------------------------------------
// the state a match starts from: nothing assigned, no job placed
static MatchState match_state_setup(cook_engine* e, const MatchIn& in) {
  const unsigned K = in.K, M = in.M, G = in.G;
  MatchState st;
  st.ac = e->m_ac.ensure(M);
  st.am = e->m_am.ensure(M);
  st.acount = e->m_acount.ensure(M);
  st.group_last = e->m_group_last.ensure(G);
  st.job_prev = e->m_job_prev.ensure(K);
  st.job_to_offer = e->m_j2o.ensure(K);
  st.fail_code = e->m_fail.ensure(K);
  st.summary = e->m_summary.ensure(4);
  st.alive = e->m_alive.ensure((M + 63u) / 64u + 1u);
  st.jmin = (const double*)e->m_jmin.ensure(4);
  st.xports = in.has_x ? e->m_xports.ensure(M) : nullptr;
  st.xscal = in.has_x ? e->m_xscal.ensure((size_t)M * COOK_MAX_SCALARS) : nullptr;
  match_init_state(e, st, K, M, G);
  st.cutoff = 0x7FFFFFFF;
  return st;
}
// the window rounds' buffers (match_v2.hpp), the call's MatchIn on the device, the packed offers and jobs; K > 0
static V2Buf match_v2_setup(cook_engine* e, const MatchIn& in, const MatchState& st, bool ge) {
  const unsigned K = in.K, M = in.M;
  V2Buf vb;
  const char* rlog_path = std::getenv("COOK_ROUND_LOG");  // diagnostics: one CSV line per round of the last match
  vb.round_log = rlog_path ? e->w_rlog.ensure(MV_ROUND_LOG_CAP) : nullptr;
  const unsigned C = div_up(M ? M : 1u, MV_OCB);
  vb.C = C;
  OfferA* oa = e->v_oa.ensure(M);
  OfferB* ob = e->v_ob.ensure(M);
  JobRec* jr = e->v_jr.ensure(K);
  vb.oa = oa;
  vb.ob = ob;
  vb.ow = e->v_ow.ensure(std::max(1u, M));
  vb.jr = jr;
  JobCons* jcons = e->v_jcons.ensure(K);
  vb.jcons = jcons;
  // sized for a LONG window (MV_WLONG jobs, match_v2.hpp) and the eval grid's largest offer split: 128 / 160 bytes per (job, offer chunk)
  vb.prec = e->v_prec.ensure((size_t)MV_WLONG * C * (sizeof(ChunkRecT<true>) > sizeof(ChunkRecT<false>) ? sizeof(ChunkRecT<true>) : sizeof(ChunkRecT<false>)));  // (a split window holds at most MV_WEVAL / split jobs)
  vb.colbits = e->v_colbits.ensure((size_t)(M ? M : 1u) * MV_JGL);
  vb.cand_fit = e->v_cand_fit.ensure((size_t)MV_WLONG * MV_LM_MAX);
  vb.cand_idx = e->v_cand_idx.ensure((size_t)MV_WLONG * MV_LM_MAX);
  vb.ge_idx = e->v_ge_idx.ensure((size_t)MV_WLONG * MV_LG_MAX);
  vb.cinfo = e->v_cinfo.ensure((size_t)MV_WLONG * 4);
  vb.jfh = e->v_jfh.ensure((size_t)MV_WLONG * (MV_FH + 2));
  vb.ctl = e->w_ctl.ensure(1);
  {  // idle rows of the eval grid take a share of the offers (eval_split) when the pool has the GPU to itself; measured on
     // MI355X: one C4 pool 66.3 -> 64.7 ms with splits up to 4, eight pools on the GPU 103 -> 113 ms (twice the chunk lists to merge,
     // more blocks than fit beside the other chains)
    const int sharing = std::max(1, g_engines_on_device[e->device & 63].load());
    vb.split_max = sharing == 1 ? (unsigned)MV_SPLIT_MAX : (sharing <= 4 ? 2u : 1u);  // (2 / 4 pools on the GPU: 69.4 -> 67.5, 72.9 -> 72.0 ms with 2)
    if (const char* ev = std::getenv("COOK_EVAL_SPLIT")) vb.split_max = (unsigned)std::max(1, std::min(MV_SPLIT_MAX, std::atoi(ev)));
    if (ge) vb.split_max = 1u;  // (the good-enough bits of a chunk are laid out for whole wave batches: match_v2.hpp ChunkRecT::gm)
  }
  {
    MatchIn* din = e->v_in.ensure(1);
    MatchIn* hin = (MatchIn*)e->h_inbuf;
    *hin = in;
    pinned_copy(e, din, hin, sizeof(MatchIn), hipMemcpyHostToDevice);
    vb.in_dev = din;
    e->v_in_is_last = std::memcmp(&in, &e->last_in, sizeof(MatchIn)) == 0;  // (cook_match_metrics reads it in place)
  }
  if (M) KM<match_pack_offers, 256>(e, "match_pack_offers", div_up(M, 256), (const MatchIn*)vb.in_dev, oa, ob, vb.ow);
  KM<match_pack_jobs, 256>(e, "match_pack_jobs", div_up(K, 256), (const MatchIn*)vb.in_dev, jr, jcons);
  KM<match_job_minima, 256>(e, "match_job_minima", std::min(div_up(K, 256), 256u), (const JobRec*)jr, K, e->m_jmin.ptr(), std::min(div_up(K, 256), 256u));
  if (M) KM<match_init_alive, 256>(e, "match_init_alive", div_up(M, 256), (const OfferA*)oa, M, st.jmin, st.alive);
  return vb;
}
// the control block the rounds start from: the first window, how it grows, how long it may get
static WinCtl first_window(const cook_engine* e, unsigned K) {
  WinCtl c0;
  std::memset(&c0, 0, sizeof(c0));
  // the first window: a call of few jobs (config.clj:113 ships fenzo-max-jobs-considered 1000) in one go — a round that stops early costs it
  // little —, a long queue with a short one (the window then follows what the rounds resolve)
  // (up to two windows' worth: the default 1000 is forty jobs more than one evaluation covers)
  c0.wcur = K <= 2u * (unsigned)MV_WEVAL ? std::max(std::min<unsigned>(K, MV_WEVAL), 1u) : std::min<unsigned>(MV_WEVAL, 128u);
  {
    // window growth: with several pools on one GPU the eval phase is compute-bound (evaluate few jobs twice); a pool
    // that has the GPU to itself is bound by the chain of rounds (prefer fewer, larger rounds)
    const int sharing = std::max(1, g_engines_on_device[e->device & 63].load());
    c0.wgrow_pct = sharing >= 4 ? 150u : 200u;
    if (const char* ev = std::getenv("COOK_WGROW_PCT")) c0.wgrow_pct = (unsigned)std::max(100, std::atoi(ev));
  }
  c0.wlong_cap = (unsigned)MV_WLONG;
  if (const char* ev = std::getenv("COOK_WLONG")) c0.wlong_cap = std::atoi(ev) ? (unsigned)MV_WLONG : (unsigned)MV_WEVAL;
  return c0;
}
// class-ordered best fit when the call's numbers and constraints allow it (classfit_host.hpp) -> true: the match is placed, or (defer) set up
// for cook_cycle_match_multi, which runs the walks of a device's pools in one launch
static bool match_try_classfit(cook_engine* e, const MatchIn& in, const MatchState& st, const V2Buf& vb, bool defer) {
  if (in.fitness != 0u) {  // its class order IS cpuMemBinPacker's: refused from the params alone, before any of its set-up launches
    e->cf_inelig = CF_X_FITNESS;
    return false;
  }
  if (!cf_setup(e, in, (const MatchIn*)vb.in_dev, st, vb.jr, vb.jcons, vb.oa, vb.ob, e->placement.walk)) return false;
  e->cycle_considered = in.K;
  e->placement.state = cook_engine::Placement::WALK;
  if (defer) return true;
  cook_engine* one[1] = {e};
  cf_run(e, one, 1, e->stream);
  return true;
}
// set up only: cook_cycle_match_multi runs the rounds of several pools together
static void match_defer(cook_engine* e, const MatchIn& in, const MatchState& st, const V2Buf& vb, const WinCtl& c0, bool ge) {
  sync(e);
  cook_engine::Placement& p = e->placement;
  p.rounds.in = in, p.rounds.st = st, p.rounds.vb = vb;
  p.c0 = c0, p.k = in.K, p.ge = ge;
  p.state = cook_engine::Placement::ROUNDS;
  e->cycle_considered = in.K;
}

// -DCOOK_EVAL_TRACE (timing-study build, scripts/eval_trace.py): the waves' phase stamps of the evaluation of round COOK_EVAL_TRACE_ROUND, to
// stderr.  Without the definition the four calls in match_run_rounds are empty.
#ifdef COOK_EVAL_TRACE
struct EvalTrace {
  const int round = std::getenv("COOK_EVAL_TRACE_ROUND") ? std::atoi(std::getenv("COOK_EVAL_TRACE_ROUND")) : -1;
  const unsigned blocks;  // of the evaluation's grid
  const size_t words;
  DArr<unsigned long long> d;
  explicit EvalTrace(V2Buf& vb) : blocks(vb.C * (unsigned)MV_JG), words((size_t)blocks * 3 + (size_t)blocks * 32) { vb.eval_trace = nullptr; }
  bool on() const { return round >= 0; }  // (then one round per look: the round whose stamps are wanted is found by its number)
  void arm(cook_engine* e, V2Buf& vb, const WinCtl& hc) {  // before a round's launches
    vb.eval_trace = nullptr;
    if (!on() || (int)hc.rounds != round) return;
    vb.eval_trace = d.ensure(words);
    memset_async(e, vb.eval_trace, 0, words * 8);
  }
  void dump(const V2Buf& vb, const WinCtl& hc) const {  // behind them
    if (!vb.eval_trace) return;
    std::vector<unsigned long long> h(words);
    COOK_HIP(hipMemcpy(h.data(), vb.eval_trace, words * 8, hipMemcpyDeviceToHost));
    double ph[5] = {0, 0, 0, 0, 0}, tot = 0, kmin = 1e30, kmax = 0;
    unsigned nw = 0, nb = 0;
    unsigned long long k0 = ~0ull, k1 = 0;
    for (unsigned blk = 0; blk < blocks; ++blk) {
      const unsigned long long a = h[blk * 3], b2 = h[blk * 3 + 1];
      if (!a || !b2) continue;
      k0 = std::min(k0, a), k1 = std::max(k1, b2);
      kmin = std::min(kmin, (double)(b2 - a)), kmax = std::max(kmax, (double)(b2 - a));
      ++nb;
    }
    for (size_t t = 0; t < (size_t)blocks * 4; ++t) {
      const unsigned long long* w8 = &h[(size_t)blocks * 3 + t * 8];
      if (!w8[0] || !w8[4]) continue;
      for (int x = 0; x < 4; ++x) ph[x] += (double)(w8[x + 1] - w8[x]);
      if (w8[5]) ph[4] += (double)(w8[5] - w8[4]);
      tot += (double)((w8[5] ? w8[5] : w8[4]) - w8[0]);
      ++nw;
    }
    std::fprintf(stderr, "EVALTRACE round %d head %u wcur %u: %u blocks over %.2f us (block %.2f..%.2f us); %u waves, mean us: lane setup %.2f, stage offers %.2f, "
                         "constraint pass %.2f, fitness pass %.2f, epilogue (wave 0; /4 waves) %.2f, wave total %.2f\n",
                 round, hc.head, hc.wcur, nb, (k1 - k0) / 100.0, kmin / 100.0, kmax / 100.0, nw, ph[0] / nw / 100.0, ph[1] / nw / 100.0, ph[2] / nw / 100.0,
                 ph[3] / nw / 100.0, ph[4] / nw / 100.0, tot / nw / 100.0);
  }
};
#else
struct EvalTrace {
  explicit EvalTrace(V2Buf&) {}
  bool on() const { return false; }
  void arm(cook_engine*, V2Buf&, const WinCtl&) {}
  void dump(const V2Buf&, const WinCtl&) const {}
};
#endif

// the window rounds of one pool (eval -> merge -> resolve, match_v2.hpp) in batches, a look at the pool's control block between two
static void match_run_rounds(cook_engine* e, const MatchIn& in, const MatchState& st, V2Buf vb, WinCtl hc, bool ge) {
  const unsigned K = in.K;
  EvalTrace trace(vb);
  unsigned batch = trace.on() ? 1 : 8;
  unsigned guard = 0;
  while (hc.head < K) {
    for (unsigned r = 0; r < batch; ++r) {
      trace.arm(e, vb, hc);
      if (ge) launch_round<true>(e, in, st, vb);
      else launch_round<false>(e, in, st, vb);
      trace.dump(vb, hc);
    }
    copy_async(e, e->h_scratch, vb.ctl, sizeof(WinCtl), hipMemcpyDeviceToHost);
    sync(e);
    const WinCtl prev = hc;
    std::memcpy(&hc, e->h_scratch, sizeof(WinCtl));
    if (hc.head >= K) break;
    batch = trace.on() ? 1 : next_batch(rounds_left(K, hc, prev));
    if (++guard > 4u * K + 64u) e->fail(COOK_E_STATE, "cook_match: window placement made no progress");
  }
  match_finish_rounds(e, st, vb, hc, e->stream);
}

// One pool's match of the first K staged jobs (j_index: which, null: 0 .. K - 1).  defer: set up only, cook_cycle_match_multi places it
// with the other pools of the device.
void match_run_device(cook_engine* e, unsigned K, const uint32_t* j_index, bool defer = false) {
  e->placement_drop();  // (whatever was set up and not run: this match takes its state and its buffers)
  e->kube_last = false;
  MatchIn in = e->min;
  in.K = K;
  in.j_index = j_index;
  in.good_enough = e->params.good_enough_fitness;
  in.host_lifetime_mins = e->params.host_lifetime_mins;
  in.fitness = (unsigned)e->params.fitness;
  e->last_in = in;
  e->last_in_valid = true;
  e->v_in_is_last = false;
  const MatchState st = match_state_setup(e, in);
  e->cf_inelig = 0;  // (stats word 38 speaks of THIS match: set below or by match_try_classfit where the class-ordered form was asked for and refused)
  const int algo = e->params.match_algo;
  if (!(algo == 0 || algo == 1 || algo == 2 || algo == 3))
    e->fail(COOK_E_INVALID, "cook_params.match_algo: 0 = engine default (window rounds; class-ordered best fit where the call allows it when six or more engines share the device), 1 = serial sweep, 2 = window rounds, 3 = class-ordered best fit where the call allows it, else window rounds");
  // A spreader's fitness FALLS on the offer a job lands on, so the window rounds' rule "a touched offer that is still feasible beats every
  // untouched offer behind it" is false for it: such a pool is placed by the sweep, as match_algo 1
  const bool spread = fitness_is_spreader(e);
  WinCtl no_rounds{};  // the counts of a match without rounds: the sweep keeps none, K = 0 has none
  no_rounds.head = K;
  if (spread && algo != 1) {
    ++e->spread_serial_calls;
    if (algo == 3 || (algo == 0 && classfit_by_default(e))) e->cf_inelig = CF_X_FITNESS;
  }
  if (algo == 1 || spread) {  // one-job-at-a-time sweep by a single workgroup (reference implementation of the chain)
    constexpr int SERIAL_THREADS = COOK_SHAPE(1024, 256);
    auto k_match = match_serial<SERIAL_THREADS>;
    KL("match_serial", k_match, 1, SERIAL_THREADS, in, st);
    e->placement_complete(1, no_rounds);
  } else if (K > 0) {  // window rounds (only they, and the class-ordered walk, run several pools in one launch: defer)
    match_check_offer_count(e, in.M);
    const bool ge = in.good_enough < 1.0;
    const V2Buf vb = match_v2_setup(e, in, st, ge);
    if ((algo == 3 || (algo == 0 && classfit_by_default(e))) && match_try_classfit(e, in, st, vb, defer)) return;
    const WinCtl c0 = first_window(e, K);
    std::memcpy(e->h_scratch, &c0, sizeof(c0));
    pinned_copy(e, vb.ctl, e->h_scratch, sizeof(WinCtl), hipMemcpyHostToDevice);
    if (defer) return match_defer(e, in, st, vb, c0, ge);
    match_run_rounds(e, in, st, vb, c0, ge);
  } else {
    unsigned sum[4] = {0u, 1u, 0u, 0u};
    std::memcpy(e->h_scratch, sum, 16);
    copy_async(e, st.summary, e->h_scratch, 16, hipMemcpyHostToDevice);
    sync(e);
    e->placement_complete(0, no_rounds);  // (window rounds, none of them)
  }
  e->cycle_considered = K;
}

// The engines of one cook_cycle_match_multi call, checked BEFORE its first launch (a refusal leaves every engine as it was): all on the lead's device,
// each with a match set up or finished (what cook_cycle_run_rank leaves), at most 64 of either form (the slots of the lead's page-locked blocks h_multi, h_cf)
void pools_check(cook_engine* const* es, unsigned n) {
  cook_engine* lead = es[0];
  unsigned rounds = 0, walks = 0;
  for (unsigned i = 0; i < n; ++i) {
    if (!es[i] || es[i]->device != lead->device) lead->fail(COOK_E_INVALID, "cook_cycle_match_multi: engines must share one device");
    const auto st = es[i]->placement.state;
    if (st == cook_engine::Placement::NONE) lead->fail(COOK_E_STATE, "cook_cycle_match_multi before cook_cycle_run_rank");
    rounds += st == cook_engine::Placement::ROUNDS, walks += st == cook_engine::Placement::WALK;
  }
  if (rounds > 64 || walks > 64) lead->fail(COOK_E_INVALID, "cook_cycle_match_multi: at most 64 pools per call");
}
// -> those of them whose match is in `state` (ROUNDS: window rounds set up, WALK: a class-ordered walk set up), in the call's order
std::vector<cook_engine*> pools_set_up(cook_engine* const* es, unsigned n, cook_engine::Placement::State state) {
  std::vector<cook_engine*> live;
  for (unsigned i = 0; i < n; ++i)
    if (es[i]->placement.state == state) live.push_back(es[i]);
  return live;
}

// What a launch for several pools needs of them: the contexts in the launch's order, the widest eval grid, and whether some pool runs with good-enough-fitness
// below 1: the GE launches for the whole chain then (a pool at 1.0 in it is placed by best fit all the same, from the GE shape's shorter best-fit lists)
struct PoolsOfLaunch { std::vector<PoolCtx> hctx; unsigned cmax = 1; bool any_ge = false; };
static PoolsOfLaunch pools_gather(cook_engine* lead, const std::vector<cook_engine*>& live) {
  if (!lead->h_multi) COOK_HIP(hipHostMalloc((void**)&lead->h_multi, 64 * sizeof(WinCtl), hipHostMallocDefault));
  PoolsOfLaunch g;
  for (const cook_engine* e : live) {
    g.hctx.push_back(e->placement.rounds);
    g.cmax = std::max(g.cmax, e->placement.rounds.vb.C);
    g.any_ge = g.any_ge || e->placement.ge;
  }
  return g;
}
// the pools' control blocks as the device has them now, read back on `stream` (which it synchronises) -> hc
static void pools_read_ctl(cook_engine* lead, const std::vector<PoolCtx>& hctx, std::vector<WinCtl>& hc, hipStream_t stream) {
  const unsigned L = (unsigned)hctx.size();
  for (unsigned x = 0; x < L; ++x) COOK_HIP(hipMemcpyAsync(&lead->h_multi[x], hctx[x].vb.ctl, sizeof(WinCtl), hipMemcpyDeviceToHost, stream));
  COOK_HIP(hipStreamSynchronize(stream));
  hc.assign(lead->h_multi, lead->h_multi + L);
}

// The placements of n engines (pools of one rank, same device) in lockstep rounds on the lead engine's stream.
void match_rounds_multi(cook_engine** es, unsigned n) {
  cook_engine* lead = es[0];
  const std::vector<cook_engine*> live = pools_set_up(es, n, cook_engine::Placement::ROUNDS);
  const unsigned L = (unsigned)live.size();
  if (L == 0) return;
  const PoolsOfLaunch g = pools_gather(lead, live);
  const std::vector<PoolCtx>& hctx = g.hctx;
  std::vector<WinCtl> hc(L);
  for (unsigned x = 0; x < L; ++x) hc[x] = live[x]->placement.c0;
  PoolCtx* dctx = lead->w_pctx.ensure(L);
  COOK_HIP(hipMemcpyAsync(dctx, hctx.data(), L * sizeof(PoolCtx), hipMemcpyHostToDevice, lead->stream));
  COOK_HIP(hipStreamSynchronize(lead->stream));  // hctx is pageable
  cook_engine* e = lead;                         // KL times / launches on the lead engine
  unsigned batch = 8, guard = 0;
  auto all_done = [&] {
    for (unsigned x = 0; x < L; ++x)
      if (hc[x].head < live[x]->placement.k) return false;
    return true;
  };
  // up to MV_PACK pools: their contexts travel in the kernel arguments (match_v2.hpp: PoolPack)
  const bool packed = L <= (unsigned)MV_PACK && pack_args();
  PoolPack<2> pk2{};
  PoolPack<MV_PACK> pk4{};
  for (unsigned x = 0; x < (unsigned)MV_PACK; ++x) {
    if (x < 2) pk2.c[x] = hctx[x < L ? x : 0];
    pk4.c[x] = hctx[x < L ? x : 0];
  }
  auto round = [&](auto ge_tag) {
    constexpr bool GE = decltype(ge_tag)::value;
    auto launch3 = [&](auto eval, auto merge, auto resolve, const auto& arg) {
      KL("match_eval2", eval, dim3(g.cmax, MV_JG, L), COOK_WAVE * MV_EW, arg);
      KL("match_merge2", merge, dim3(MV_MERGE_BLOCKS, 1, L), COOK_WAVE * MV_MW, arg);
      KL("match_resolve2", resolve, dim3(1, 1, L), MV_RTHREADS, arg);
    };
    if (packed && L <= 2u) launch3(match_eval2_pack<GE, 2>, match_merge2_pack<GE, 2>, match_resolve2_pack<GE, 2>, pk2);
    else if (packed) launch3(match_eval2_pack<GE, MV_PACK>, match_merge2_pack<GE, MV_PACK>, match_resolve2_pack<GE, MV_PACK>, pk4);
    else launch3(match_eval2_multi<GE>, match_merge2_multi<GE>, match_resolve2_multi<GE>, (const PoolCtx*)dctx);
  };
  while (!all_done()) {
    for (unsigned r = 0; r < batch; ++r) {
      if (g.any_ge) round(std::true_type{});
      else round(std::false_type{});
    }
    const std::vector<WinCtl> prev = hc;
    pools_read_ctl(lead, hctx, hc, lead->stream);
    double est = 0;
    for (unsigned x = 0; x < L; ++x) {
      const unsigned K = live[x]->placement.k;
      if (hc[x].head < K) est = std::max(est, rounds_left(K, hc[x], prev[x]));
    }
    batch = next_batch(est);
    if (++guard > 1000000u) lead->fail(COOK_E_STATE, "cook_cycle_match_multi: placement made no progress");
  }
  for (unsigned x = 0; x < L; ++x) match_finish_rounds(live[x], hctx[x].st, hctx[x].vb, hc[x], lead->stream);
}

void match_fetch(cook_engine* e, unsigned K, int32_t* job_to_offer, uint32_t* fail_code, uint8_t* head_matched) {
  if (!e->match_ran()) e->fail(COOK_E_STATE, "cook_match_fetch before cook_match_run");
  if (job_to_offer && K) copy_async(e, job_to_offer, e->m_j2o.ptr(), (size_t)K * 4, hipMemcpyDeviceToHost);
  if (fail_code && K) copy_async(e, fail_code, e->m_fail.ptr(), (size_t)K * 4, hipMemcpyDeviceToHost);
  copy_async(e, e->h_scratch, e->m_summary.ptr(), 16, hipMemcpyDeviceToHost);
  sync(e);
  unsigned s[4];
  std::memcpy(s, e->h_scratch, 16);
  if (head_matched) *head_matched = (uint8_t)s[1];
}
