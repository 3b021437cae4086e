// match_v2_resolve.hpp — the walk of a window in rank order: JobL and the walk's LDS layout, the round's set-up, the segments, the end of a
// round, resolve_round and match_resolve2, with the COOK_L_* / WALK_* macros the walk is written in.  Part of match_v2.hpp: needs
// match_v2_shapes.hpp, and match_v2_eval.hpp for the constraint checks a touched offer is evaluated again with.
#pragma once

// ---- resolve -----------------------------------------------------------------------------------------------------------------
struct JobL {  // a job of the window as the walk reads it (one 32-byte LDS record)
  double c, m;
  unsigned info;  // bits 0-7 ncand, 8-15 nge, 16 gpu job, 17 member of a constrained group, 18-19 group type
  unsigned group;
  unsigned short f1, f2, f4;  // saturated counts of offers failing on resources / constraints / zero fitness under S
  unsigned short b;           // window position of the job (the record itself sits at its WALK position)
};
constexpr unsigned JL_GPU = 1u << 16, JL_GROUPED = 1u << 17, JL_HASGROUP = 1u << 20;  // (bits 18-19: group type)
constexpr unsigned JL_XRES = 1u << 28;    // asks for ports / named scalars: general path only
constexpr unsigned JL_TRUNC = 1u << 29;   // the merged list may not hold every feasible offer (cinfo bit 16)
constexpr unsigned JL_GTRUNC = 1u << 30;  // the good-enough list may not hold every offer above the threshold (cinfo bit 17)
// "entries may exist beyond the job's list" / "the list holds every feasible offer" inside the walk (cinfo_u: the walk's local)
#define COOK_L_TRUNC() ((cinfo_u & JL_TRUNC) != 0u)
#define COOK_L_COMPLETE() ((cinfo_u & JL_TRUNC) == 0u)
constexpr unsigned JL_GSLOT_SHIFT = 21, JL_GSLOT_NONE = 0x7Fu;  // bits 21-27: the job's row of ResolveFixed::gfh, or none
constexpr int MV_GMAX = 64;  // group members per segment whose hosts-to-avoid are staged for the walk's fast path
// Offers a round may touch beyond its 64 lanes: when every lane is taken, a lane whose offer is DEAD — it cannot take even the smallest
// job of the call any more, so no later job can go there — is given to the next offer (the dead offer's state is written back at once,
// its byte in the owner table says "dead": list entries that name it are skipped like touched offers that do not fit).  On the
// benchmark's pools 40-50 of the 64 lanes are dead when the 65th offer is asked for (best fit fills offers to the brim).
// List entries per job whose OfferW line and colbits word the STAGING of a segment touches, so that the walk's open_lane finds them in
// the L2 of the XCD the workgroup runs on (they were last written / read by evaluation blocks all over the chip): 70 % of the offers a
// walk opens are among the first four entries of the job's list, 80 % among the first eight (emulator, C4 pool).  Costs the walking
// wave nothing: the other waves of the workgroup issue the loads while they stage.
#ifndef COOK_MV_PF
#define COOK_MV_PF 8
#endif
constexpr int MV_PF = COOK_MV_PF;
constexpr unsigned MV_RETIRE_CAP = 192;
constexpr unsigned MV_TMAX = (unsigned)MV_T + MV_RETIRE_CAP;  // offers one round can touch at most
constexpr unsigned OWNER_UNTOUCHED = 0xFFu, OWNER_NONE = 0xFEu, OWNER_DEAD = 0xFDu;  // values of the owner table / of JobRegs::owner beside lane numbers

// (WALK_STAT: platform.hpp — counters of the emulated build's design studies, nothing on the GPU)

// The resolve workgroup's LDS: this fixed part, then — sized at run time from the number of offers (resolve_wseg) — the segment's
// job records, candidate lists and results BY WALK POSITION, and the owner table: one byte per OFFER of the pool, the lane that
// owns it in this round, 0xFF = untouched.
struct ResolveFixed {
  unsigned long long visit[MV_JGL];  // bit b of the window: the walk has to visit job b (the others are settled in parallel)
  unsigned vbase[MV_JGL + 1];        // walk position of the first visited job of each 64-job group
  // members of unique (or unconstrained) host-placement groups among the segment's jobs: the hosts their cotasks occupied when the
  // round began (running ++ placed by earlier rounds; 0xFFFFFFFF = unused) and the group's last placed job then
  unsigned gfh[MV_GMAX][MV_FH];
  int glast[MV_GMAX];
  unsigned n_gslots;
  unsigned dbg_h[4];                // (round log only) checksums of the round's inputs, see RoundLog
  int cmd;                          // the walker's word to the other waves: 1 = stage the next segment, 0 = the round is over
  unsigned seg_lo;                  // first walk position of the segment being staged
  int sink[COOK_WAVE];              // where lanes 1..63 put their copy of a result the walk stores (see store_result)
  unsigned char sinkb[COOK_WAVE];
  // what a lane WITHOUT a list entry loads instead of one (the walk's loads are select-on-the-address, never a branch on the lane)
  double fit_none;                  // -1
  int off_none;                     // -1
  unsigned char owner_none[4];      // 0xFE = "no entry"
  // ports / named scalars assigned on a touched offer when the round began, by owner lane: saved by the first job of the round
  // that moves them (the failure summary of an unmatched job compares against the round's snapshot)
  double x0s[MV_T][3];
  int x0p[MV_T];
  unsigned char x0set[MV_T];
  // the state of a touched offer as the round began, by owner lane (the failure summary of an unmatched job swaps each touched offer's
  // verdict under the snapshot for its current one)
  double ac0[MV_T], am0[MV_T];
  int acount0[MV_T];
};
constexpr unsigned MV_RLDS_BYTES = 160u * 1024u - 2048u;  // the workgroup's static LDS array (the CU has 160 KB)
template <bool GE>
constexpr unsigned resolve_job_bytes() {  // LDS per staged job: record, best-fit entries (fitness + offer), good-enough entries, result, failure code
  return (unsigned)sizeof(JobL) + 12u * (unsigned)VShape<GE>::LM + 4u * (unsigned)VShape<GE>::LG + 4u + 1u;
}
constexpr unsigned resolve_fixed_bytes() { return ((unsigned)sizeof(ResolveFixed) + 15u) / 16u * 16u + 128u; }  // (+ alignment slack of the carved arrays)
// jobs per segment for a pool of M offers (0 = the owner table alone does not fit: the host refuses such a pool)
template <bool GE>
static __host__ __device__ __forceinline__ unsigned resolve_wseg(unsigned M) {
  const unsigned owner = (M + 16u) / 16u * 16u;
  if (resolve_fixed_bytes() + owner >= MV_RLDS_BYTES) return 0u;
  const unsigned w = (MV_RLDS_BYTES - resolve_fixed_bytes() - owner) / resolve_job_bytes<GE>();
  return w < (unsigned)MV_WSEG ? w : (unsigned)MV_WSEG;
}
constexpr unsigned MV_WSEG_MIN = 16;  // pools whose owner table leaves less than that per segment are refused (about 150 000 offers)

// The run-time part of the resolve workgroup's LDS, carved behind ResolveFixed (resolve_wseg sizes it)
template <bool GE>
struct SegLds {
  JobL* job;             // [wseg] the segment's jobs, in rank order (walk position - seg_lo; JobL::b = window position)
  double* efit;          // [wseg][LM] fitness under S of the candidate entries, by walk position
  int* eoff;             // [wseg][LM] offer of the entry, -1 = none
  int* goff;             // [wseg][LG] (GE) good-enough entries: offer, -1 = none
  int* j2o;              // [wseg] results of the walk BY WALK POSITION, flushed to HBM once per segment: a global store inside the
                         //        walk would stall later s_waitcnt vmcnt(0) on its acknowledgement
  unsigned char* fail;   // [wseg] failure codes, by walk position
  unsigned char* owner;  // [M] owner lane of an offer, OWNER_UNTOUCHED / OWNER_DEAD
  unsigned wseg;
  __device__ __forceinline__ SegLds(char* lds, unsigned M) {
    constexpr int LM = VShape<GE>::LM, LG = VShape<GE>::LG;
    wseg = resolve_wseg<GE>(M);
    char* carve = lds + ((sizeof(ResolveFixed) + 15u) / 16u * 16u);
    job = reinterpret_cast<JobL*>(carve);
    carve += (size_t)wseg * sizeof(JobL);
    efit = reinterpret_cast<double*>(carve);
    carve += (size_t)wseg * LM * 8u;
    eoff = reinterpret_cast<int*>(carve);
    carve += (size_t)wseg * LM * 4u;
    goff = reinterpret_cast<int*>(carve);
    carve += (size_t)wseg * LG * 4u;
    j2o = reinterpret_cast<int*>(carve);
    carve += (size_t)wseg * 4u;
    fail = reinterpret_cast<unsigned char*>(carve);
    carve += ((size_t)wseg + 15u) / 16u * 16u;
    owner = reinterpret_cast<unsigned char*>(carve);
  }
};

// ---- once per round (all threads): the owner table, the jobs the walk can skip ---------------------------------------------------
// A job without any feasible offer under S stays unmatched whatever the jobs before it do (placements only take capacity away;
// constrained groups excepted), and its failure summary cannot change when every class it reports is backed by more offers than the
// round can touch (t_max): such jobs are settled here, in parallel, and the walk skips them.  -> the number of jobs the walk must visit
// (L.visit: their bits by window position, L.vbase: walk position of the first visited job of each 64-job group).
template <bool GE>
static __device__ __forceinline__ unsigned resolve_settle(ResolveFixed& L, const SegLds<GE>& S, const MatchState& st, const V2Buf& vb, unsigned head,
                                                          unsigned nwin, unsigned M, unsigned t_max) {
  const unsigned tid = threadIdx.x, NT = blockDim.x;
  for (unsigned x = tid; x < (M + 3u) / 4u; x += NT) reinterpret_cast<unsigned*>(S.owner)[x] = 0xFFFFFFFFu;
  if (tid < MV_JGL) L.visit[tid] = 0ull;
  if (tid < (unsigned)MV_T) L.x0set[tid] = 0;
  if (tid == 0) {
    L.fit_none = -1.0;
    L.off_none = -1;
    L.owner_none[0] = L.owner_none[1] = L.owner_none[2] = L.owner_none[3] = (unsigned char)OWNER_NONE;
    L.cmd = 0;
    L.n_gslots = 0;
    L.dbg_h[0] = L.dbg_h[1] = L.dbg_h[2] = L.dbg_h[3] = 0u;
  }
  __syncthreads();
  if (vb.round_log) {  // diagnostics: what this round was given
    const unsigned ngrp = (nwin + COOK_WAVE - 1) / COOK_WAVE;
    unsigned hs = 0, ha = 0, hc = 0;
    for (unsigned v = tid; v < M; v += NT) {
      const unsigned long long a = (unsigned long long)__double_as_longlong(st.ac[v]), m2 = (unsigned long long)__double_as_longlong(st.am[v]);
      hs += (unsigned)(a >> 20) * (v + 1u) + (unsigned)(m2 >> 20) * (v + 7u) + (unsigned)st.acount[v] * 131u;
      for (unsigned g = 0; g < ngrp; ++g) {
        const unsigned long long w = vb.colbits[(size_t)v * MV_JGL + g];
        hc += ((unsigned)w ^ (unsigned)(w >> 32)) * (v * 31u + g + 1u);
      }
    }
    for (unsigned w2 = tid; w2 < (M + 63u) / 64u; w2 += NT) {
      const unsigned long long w = st.alive[w2];
      ha += ((unsigned)w ^ (unsigned)(w >> 32)) * (w2 + 1u);
    }
    atomicAdd(&L.dbg_h[1], hs);
    atomicAdd(&L.dbg_h[2], ha);
    atomicAdd(&L.dbg_h[3], hc);
  }
  for (unsigned b = tid; b < nwin; b += NT) {
    const unsigned flags = vb.jr[head + b].flags;
    const unsigned info = vb.cinfo[(size_t)b * 4 + 0];
    const unsigned c1 = vb.cinfo[(size_t)b * 4 + 1], c2 = vb.cinfo[(size_t)b * 4 + 2], c4 = vb.cinfo[(size_t)b * 4 + 3];
    if (vb.round_log) atomicAdd(&L.dbg_h[0], (info * 31u + c1 * 7u + c2 * 3u + c4) * (b + 1u));
    // members of balanced / attribute-equals groups excepted: a cotask's placement can make an offer FEASIBLE for them; a unique
    // group only ever takes hosts away (constraints.clj:586-598), like a resource
    const bool opens = (flags & JF_GROUPED) != 0 && ((flags >> 8) & 3u) != 1u;
    const bool trivial = (info & 0xFFFFu) == 0u && !opens && c1 > 0u && (c2 == 0u || c2 > t_max) && (c4 == 0u || c4 > t_max);
    if (trivial) {
      // final whatever this round does, also for a job behind the point where the round stops: job_to_offer keeps the -1 it was
      // initialised with; should the job still be unresolved next round, its summary is simply rewritten under the newer snapshot
      if (st.fail_code) st.fail_code[head + b] = 1u | (c2 ? 2u : 0u) | (c4 ? 4u : 0u);
    } else {
      atomicOr(&L.visit[b >> 6], 1ull << (b & 63u));
    }
  }
  __syncthreads();
  if (tid <= (unsigned)MV_JGL) {  // every thread sums its own prefix ([MV_JGL] = the total)
    unsigned acc = 0;
    for (unsigned g = 0; g < tid; ++g) acc += (unsigned)__popcll(L.visit[g]);  // (groups beyond the window hold no bits)
    L.vbase[tid] = acc;
  }
  __syncthreads();
  return wave_uniform_u32(L.vbase[MV_JGL]);
}

// ---- the segment [lo, lo + n) of walk positions -> LDS, by walk position (all threads; L.n_gslots = 0 and a barrier behind it are
// ---- the caller's) -> n ------------------------------------------------------------------------------------------------------
template <bool GE>
static __device__ __forceinline__ unsigned resolve_stage_segment(ResolveFixed& L, const SegLds<GE>& S, const V2Buf& vb, unsigned head, unsigned nwin,
                                                                 unsigned n_list, unsigned lo, double good_enough) {
  constexpr int LM = VShape<GE>::LM, LG = VShape<GE>::LG;
  const unsigned tid = threadIdx.x, NT = blockDim.x;
  const bool use_ge = GE && good_enough < 1.0;
  const unsigned ngrp = (nwin + COOK_WAVE - 1) / COOK_WAVE;
  const unsigned hi = lo + S.wseg < n_list ? lo + S.wseg : n_list;
  // the job groups of the window that hold walk positions of the segment
  unsigned g0 = 0;
  while (g0 + 1 < ngrp && L.vbase[g0 + 1] <= lo) ++g0;
  // pass 1, thread = window position: the records of the visited jobs, compacted to walk positions
  for (unsigned b = g0 * COOK_WAVE + tid; b < nwin && L.vbase[b >> 6] < hi; b += NT) {
    const unsigned long long vw = L.visit[b >> 6];
    if (!((vw >> (b & 63u)) & 1ull)) continue;
    const unsigned i = L.vbase[b >> 6] + (unsigned)__popcll(vw & ((1ull << (b & 63u)) - 1ull));
    if (i < lo || i >= hi) continue;
    const unsigned x = i - lo;
    const unsigned info = vb.cinfo[(size_t)b * 4 + 0];
    const unsigned c1 = vb.cinfo[(size_t)b * 4 + 1], c2 = vb.cinfo[(size_t)b * 4 + 2], c4 = vb.cinfo[(size_t)b * 4 + 3];
    const JobRec j = vb.jr[head + b];
    S.fail[x] = 0;  // a visited job that gets matched leaves it at that
    JobL r;
    r.c = j.c;
    r.m = j.m;
    const bool grouped = (j.flags & JF_GROUPED) != 0;
    r.info = (info & 0xFFFFu) | (j.g > 0 ? JL_GPU : 0u) | (grouped ? JL_GROUPED : 0u) | (((j.flags >> 8) & 3u) << 18) |
             (j.group != 0xFFFFFFFFu ? JL_HASGROUP : 0u) | ((j.flags & JF_XRES) ? JL_XRES : 0u) |
             ((info & (1u << 16)) ? JL_TRUNC : 0u) | ((info & (1u << 17)) ? JL_GTRUNC : 0u);
    // a member of a unique (type 1) or unconstrained (type 0) group: stage what the walk's fast path needs — the hosts to avoid
    // as the round begins and the group's last placed job (for the chain link) — so that it never has to go to HBM for them
    unsigned gslot = JL_GSLOT_NONE;
    const unsigned gt = (j.flags >> 8) & 3u;
    if (j.group != 0xFFFFFFFFu && gt <= 1u && (GE || !(good_enough < 1.0)) && vb.in_dev->host_dup == 0u && !(j.flags & JF_XRES)) {
      const unsigned* row = vb.jfh + (size_t)b * (MV_FH + 2);  // gathered by the evaluation of this round
      const int nfh = (int)row[MV_FH];
      if (gt == 0u || (nfh >= 0 && nfh <= MV_FH)) {
        const unsigned gs = atomicAdd(&L.n_gslots, 1u);
        if (gs < (unsigned)MV_GMAX) {
#pragma unroll
          for (int y = 0; y < MV_FH; ++y) L.gfh[gs][y] = gt == 1u ? row[y] : 0xFFFFFFFFu;
          L.glast[gs] = (int)row[MV_FH + 1];
          gslot = gs;
        }
      }
    }
    r.info |= gslot << JL_GSLOT_SHIFT;
    r.group = j.group;
    r.f1 = (unsigned short)(c1 < 0xFFFFu ? c1 : 0xFFFFu);
    r.f2 = (unsigned short)(c2 < 0xFFFFu ? c2 : 0xFFFFu);
    r.f4 = (unsigned short)(c4 < 0xFFFFu ? c4 : 0xFFFFu);
    r.b = (unsigned short)b;
    S.job[x] = r;
  }
  __syncthreads();
  // pass 2, thread = list entry: the candidate lists by walk position.  The loads do not wait for the job's counts (the arrays are
  // sized for every entry of every job of a window: entries beyond a list hold stale values, replaced by "none" behind the load)
  const unsigned n = hi - lo;
#pragma unroll 4
  for (unsigned e = tid; e < n * (unsigned)LM; e += NT) {
    const unsigned x = e / (unsigned)LM, q = e % (unsigned)LM;
    const JobL* jl = &S.job[x];
    const unsigned b = jl->b, nl = jl->info & 0xFFu;
    const int o = vb.cand_idx[(size_t)b * LM + q];
    const double f = vb.cand_fit[(size_t)b * LM + q];
    S.efit[e] = q < nl ? f : -1.0;
    S.eoff[e] = q < nl ? o : -1;
  }
  if constexpr (LG > 0) {
#pragma unroll 4
    for (unsigned e = tid; e < n * (unsigned)LG; e += NT) {
      const unsigned x = e / (unsigned)LG, q = e % (unsigned)LG;
      const JobL* jl = &S.job[x];
      const unsigned b = jl->b, ngl = (jl->info >> 8) & 0xFFu;
      const int o = vb.ge_idx[(size_t)b * LG + q];
      S.goff[e] = (use_ge && q < ngl) ? o : -1;
    }
  }
  __syncthreads();
  return n;
}

// (MV_PF) the waves that do not walk touch what opening the first entries of the segment's lists would read — behind the staging's
// last barrier, i.e. while wave 0 already walks
template <bool GE>
static __device__ __forceinline__ void resolve_prefetch_segment(const SegLds<GE>& S, const V2Buf& vb, unsigned n) {
  constexpr int LM = VShape<GE>::LM;
  const unsigned tid = threadIdx.x, NT = blockDim.x;
  unsigned pf_sink = 0u;
  for (unsigned e = tid - COOK_WAVE; e < n * (unsigned)MV_PF; e += NT - COOK_WAVE) {
    const unsigned x = e / (unsigned)MV_PF, q = e % (unsigned)MV_PF;
    const int o = S.eoff[(size_t)x * LM + q];
    if (o < 0) continue;
    PREFETCH_WORD(pf_sink, &vb.ow[(unsigned)o]);
    PREFETCH_WORD(pf_sink, &vb.colbits[(size_t)(unsigned)o * MV_JGL + ((unsigned)S.job[x].b >> 6)]);
  }
  PREFETCH_DRAIN(pf_sink);
}

// ---- the end of a round (lane 0 of the walking wave): statistics, the window of the next round, the control block back to HBM -----
static __device__ __forceinline__ void resolve_finish(WinCtl& ctl, const V2Buf& vb, unsigned head, unsigned nwin, unsigned resolved, unsigned stop,
                                                      unsigned matched, unsigned head_matched, unsigned touched, unsigned n_list,
                                                      unsigned n_segments, unsigned n_trunc, unsigned long long t_stage, unsigned long long t_all,
                                                      const unsigned* dbg_h) {
  ctl.head = head + resolved;
  ctl.rounds += 1;
  ctl.matched += matched;
  ctl.head_matched = head_matched;
  ctl.touched_sum += touched;
  ctl.visited_sum += n_list;
  ctl.segments += n_segments;
  ctl.t_setup += t_stage;
  ctl.t_seq += t_all - t_stage;
  ctl.trunc_lists += n_trunc;
  if (vb.round_log && ctl.rounds <= MV_ROUND_LOG_CAP) {
    RoundLog r;
    r.head = head, r.wcur = ctl.wcur, r.resolved = resolved, r.n_list = n_list, r.touched = touched, r.stop = stop, r.matched = matched;
    r.setup_ticks = (unsigned)t_stage, r.seq_ticks = (unsigned)(t_all - t_stage), r.segments = n_segments;
    r.h_cinfo = dbg_h[0], r.h_state = dbg_h[1], r.h_alive = dbg_h[2], r.h_col = dbg_h[3];
    vb.round_log[ctl.rounds - 1] = r;
  }
  if (stop == 1) ctl.stop_list += 1;
  if (stop == 2 || stop == 5) ctl.stop_full += 1;
  if (stop == 3) ctl.stop_group += 1;
  if (stop == 0) ctl.stop_window += 1;
  // adapt the window: a multiple of what a round resolves (more = fewer rounds, less = fewer jobs evaluated twice)
  unsigned wn = stop == 0 ? ctl.wcur * 2 : (unsigned)(((unsigned long long)resolved * ctl.wgrow_pct + 99ull) / 100ull);
  if (wn < 64) wn = 64;
  // past MV_WEVAL only while next to nothing of a window has to be walked (see MV_WLONG), and never beyond what this launch
  // sequence sized its buffers and grids for
  unsigned cap = (unsigned)MV_WEVAL;
  if (stop == 0 && nwin >= (unsigned)MV_WEVAL && n_list * 8u <= nwin) cap = ctl.wlong_cap > cap ? ctl.wlong_cap : cap;
  if (wn > cap) wn = cap;
  ctl.wcur = wn;
  ctl.no_retire = touched < (unsigned)MV_T * 3u / 4u ? 1u : 0u;
  *vb.ctl = ctl;
}

// One round of the window walk by ONE workgroup of MV_RTHREADS threads (all of them must call it): resolve_settle, then per segment
// resolve_stage_segment (all threads) / resolve_prefetch_segment (the waves that do not walk) and the walk below (wave 0),
// resolve_finish at the end.
//
// The walk is one dependent chain run by a single wave.  What it costs per job is the number of INSTRUCTIONS on the job's path — a
// wave issues one every fourth cycle or so: 945 cycles for the ~200 instructions of a job that goes to an offer touched before
// (-DCOOK_WALK_PROF) — not the latencies of scripts/ubench_wave.hip one by one (dependent LDS read 60-68 cycles,
// compiler-form DPP reduction 166, ballot -> ffs -> readlane 62): those are hidden behind the issue of the rest.  The loop is
// organised as (1) a look-ahead of ONE job over walk records that are laid out by WALK position (no dependent address chain: record
// and list entries of job i+1 are loaded while job i is decided, the owner look-up of its entries at the end of job i's turn), the
// fast loop unrolled by two over two register sets so that the look-ahead costs no register rotation; (2) a FAST PATH for the
// common job — no constrained group, finite positive fitness values — that orders the touched offers by an fp32 image of the
// approximate fitness (one hand-placed DPP reduction, gpu_prims.hpp), written without a branch on the lane number (stores, loads and
// bookings are selects: see store_result / open_lane / take_job for what such a branch does to the whole loop), and falls back to
// (3) the GENERAL PATH below it whenever the order is not certain at fp32 resolution (two touched offers within 2^-20, touched and
// untouched best within 2^-38), the job is unmatched, or anything unusual is involved.  Both paths produce the same decision; only
// the general path knows every rule.
template <bool GE>  // GE: the launch was made for good-enough-fitness < 1 (list shape VShape<true>; the fast path knows the "first offer above the threshold" rule)
static __device__ void resolve_round(char* lds, MatchState st, const V2Buf& vb) {
  constexpr int LM = VShape<GE>::LM, LG = VShape<GE>::LG;
  constexpr bool GEF = GE;
  ResolveFixed& L = *reinterpret_cast<ResolveFixed*>(lds);
  auto& s_gfh = L.gfh;
  auto& s_glast = L.glast;
  unsigned& s_ngslots = L.n_gslots;
  const unsigned tid = threadIdx.x, lane = lane_id();
  WinCtl ctl = *vb.ctl;
  // (the launch's scalars through scalar registers, explicitly: in the multi-pool kernels `vb` and `st` are read from a context record
  //  in memory, their pointers are generic pointers to the compiler, and whatever is loaded through a generic pointer counts as a
  //  per-lane value — the walk loop built on them would run under execution masks with its counters in vector registers)
  ctl.head = wave_uniform_u32(ctl.head);
  ctl.wcur = wave_uniform_u32(ctl.wcur);
  const unsigned head = ctl.head;
  const unsigned K = wave_uniform_u32(vb.in_dev->K);
  if (head >= K) return;
  const unsigned M = wave_uniform_u32(vb.in_dev->M);
  const unsigned long long tk0 = cook_ticks();
  const unsigned wend = (head + ctl.wcur < K) ? head + ctl.wcur : K;
  const unsigned nwin = wend - head;
  const double good_enough = wave_uniform_f64(vb.in_dev->good_enough);
  const bool use_ge = GE && good_enough < 1.0;
  const unsigned fit_mode = wave_uniform_u32(vb.in_dev->fitness);  // 0 cpuMemBinPacker, 1 / 2 the one-resource packers (fitness_of)
  const uint32_t* const j_index = wave_uniform_ptr(vb.in_dev->j_index);
  // dead lanes are given away (MV_RETIRE_CAP) unless jobs of the call move ports / named scalars (their per-lane snapshots would go with the lane)
  // ... and unless the previous round used few of its lanes: a round that may touch MV_TMAX offers must WALK every unmatched job whose
  // failure classes are backed by no more offers than that, and once the cluster is full (rounds that touch a handful of offers, windows
  // of thousands of jobs settled in parallel) those would be most of the queue
  const bool can_retire = wave_uniform_u32(vb.in_dev->has_x) == 0u && wave_uniform_u32(ctl.no_retire) == 0u;
  const unsigned t_max = can_retire ? MV_TMAX : (unsigned)MV_T;  // offers this round can touch at most
  const double jmin_c = wave_uniform_f64(st.jmin[0]), jmin_m = wave_uniform_f64(st.jmin[1]);
  // the run-time part of the LDS
  const SegLds<GE> S(lds, M);
  JobL* const s_job = S.job;
  double* const s_efit = S.efit;
  int* const s_eoff = S.eoff;
  int* const s_goff = S.goff;
  int* const s_j2o = S.j2o;
  unsigned char* const s_fail = S.fail;
  unsigned char* const s_owner = S.owner;
  // ---- once per round (all threads): what the walk can skip, the owner table -------------------------------------------------------
  const unsigned n_list = resolve_settle<GE>(L, S, st, vb, head, nwin, M, t_max);  // jobs the walk has to visit
  auto stage_segment = [&](unsigned lo) -> unsigned { return resolve_stage_segment<GE>(L, S, vb, head, nwin, n_list, lo, good_enough); };
  auto prefetch_segment = [&](unsigned n) { resolve_prefetch_segment<GE>(S, vb, n); };
  unsigned seg_lo = 0;
  unsigned n_eff = stage_segment(0);  // walk positions of the segment
  unsigned n_segments = 1;
  if (tid >= COOK_WAVE) {  // the other waves: asleep at the barrier until wave 0 asks for the next segment or ends the round
    for (;;) {
      prefetch_segment(n_eff);
      EMU_SITE("resolve: helper waiting");
      __syncthreads();
      if (L.cmd == 0) break;
      seg_lo = wave_uniform_u32(L.seg_lo);
      n_eff = stage_segment(seg_lo);
    }
    return;
  }
  // wave 0 walks the window
  unsigned long long tk1 = cook_ticks();
  unsigned long long t_stage = tk1 - tk0;
  // ---- sequential phase ---------------------------------------------------------------------------------------------------
  // Lanes own the offers touched in this round (state in registers).  Cross-lane traffic is ballots, v_readlane and DPP
  // reductions (no ds_bpermute); fitness values are first compared through a reciprocal-multiply approximation (relative error
  // < 2^-50) and the two fp64 divides are only executed when candidates are closer than 2^-38 relative — exactness is unaffected.
  int t_v = -1;  // the lane's offer (-1: the lane owns none yet)
  double t_oc = 0, t_om = 0, t_rc = 0, t_rm = 0, t_invc = 0, t_invm = 0;
  double t_ac = 0, t_am = 0, t_basec = 0, t_basem = 0;
  int t_acount = 0, t_run = 0, t_slack = 0;
  unsigned t_k8s = 0, t_host = 0;
  unsigned long long t_col = 0ull;  // the offer's static-constraints-pass bits of job group cur_g of the window (colbits)
  unsigned long long t_coln = 0ull;  // ... and of group col_next, fetched when the walk entered cur_g (nothing waits for it)
  unsigned col_next = 0xFFFFFFFFu;
  // group members placed in THIS round, one per lane in placement order (group, host, match index): what a later member of the same
  // group has to avoid / link to, without asking HBM.  n_log > 64: the log overflowed, no fast path for group members any more
  unsigned lg_group = 0xFFFFFFFFu, lg_host = 0u, n_log = 0u;
  int lg_k = -1;
  unsigned cur_g = 0xFFFFFFFFu;
  unsigned nT = 0;
  unsigned n_retired = 0;  // dead offers whose lanes were given away in this round
  unsigned stop = 0;  // 1 list exhausted, 2 touched set full, 3 group barrier, 5 an unmatched job's summary needs a fresh snapshot
  unsigned matched = 0, head_matched = ctl.head_matched;
  unsigned resolved = nwin;
  unsigned n_trunc = 0;          // walked jobs with a truncated merged list (statistics)
  // guard bands of the approximate fitness (relative 2^-38; the approximation is good to ~2^-50): x - x * 2^-38 and x + x * 2^-38 through
  // v_ldexp_f64 with an inline exponent — as multiplications by 1 -+ 2^-38 the two fp64 constants lived in VGPRs, were spilled, and the
  // walk's fast path reloaded them from scratch memory for every job (two dependent scratch loads on the critical path)
  // fp32 threshold below which a touched offer's approximate fitness cannot be "above good-enough" nor "maybe above" (rounding to fp32 is
  // monotone; the margin of 2^-30 covers the 2^-38 guard band): the fast path's first look in launches with the good-enough rule
  const float ge_near_f = (float)(good_enough - ldexp(good_enough < 0.0 ? -good_enough : good_enough, -30));
  auto eps_lo = [](double x) { return x - ldexp(x, -38); };
  auto eps_hi = [](double x) { return x + ldexp(x, -38); };
  struct JobRegs {   // exactly what the LDS loads deliver: nothing is decoded before the job's own iteration (a decode right after
                     // the load would wait for it)
    double c, m;
    unsigned info, group;
    unsigned f4b;      // JobL::f4 | JobL::b << 16
    double e_fit;      // list entry `lane` (lanes >= LM: none)
    int e_off;
    unsigned owner;    // lane owning the entry's offer, 0xFF untouched, 0xFE no entry
    int g_off;         // (GEF) good-enough list entry `lane` (lanes >= LG: none): offer, owner as above
    unsigned g_owner;
  };
  // record + list entry of walk position i of the segment: addresses depend on i only, so the loads of job i+1 are issued a whole turn
  // ahead and nothing waits for them (OPAQUE_V: see gpu_prims.hpp)
  auto load_rec = [&](unsigned i) {
    JobRegs r;
    unsigned ii = i < n_eff ? i : 0u;
    OPAQUE_V(ii);
    const JobL* jp = &s_job[ii];
    r.c = jp->c;
    r.m = jp->m;
    r.info = jp->info;
    r.group = jp->group;
    r.f4b = *reinterpret_cast<const unsigned*>(&jp->f4);
    r.owner = 0xFEu;
    r.g_off = -1;
    r.g_owner = 0xFEu;
    // (no branch on the lane number in the walk loop, here or below — see take_job for what one costs the whole loop — and no select
    //  BEHIND a load either, which would wait for it on the spot: a lane without an entry loads the "none" record instead)
    {
      const bool has = lane < (unsigned)LM;
      const double* fp = has ? &s_efit[(size_t)ii * LM + lane] : &L.fit_none;
      const int* op = has ? &s_eoff[(size_t)ii * LM + lane] : &L.off_none;
      r.e_fit = *fp;
      r.e_off = *op;
    }
    if constexpr (GEF) {
      const int* gp = (use_ge && lane < (unsigned)LG) ? &s_goff[(size_t)ii * LG + lane] : &L.off_none;
      r.g_off = *gp;
    }
    return r;
  };
  // the owner look-up needs the entry's offer: issued at the end of the turn before the job's own (a commit in between patches it, see below)
  auto load_owner = [&](JobRegs& r) {
    {
      const unsigned char* op = (lane < (unsigned)LM && r.e_off >= 0) ? &s_owner[(unsigned)r.e_off] : &L.owner_none[0];
      r.owner = *op;
    }
    if constexpr (GEF) {
      const unsigned char* op = (use_ge && lane < (unsigned)LG && r.g_off >= 0) ? &s_owner[(unsigned)r.g_off] : &L.owner_none[0];
      r.g_owner = *op;
    }
  };
  // The fast path's result store, by ALL lanes: lane 0 into the result row, the others into a sink.  As `if (lane == 0) store` it is a
  // divergent branch whose join is the block where the fast path's exits meet, and the compiler's uniformity analysis then takes every
  // value that meets there for divergent — the walk position, the count of touched offers, the fast path's verdict itself: the loop
  // became a divergent loop (execution masks, its counters in vector registers, the walker's state copied at every join).
  auto store_result = [&](unsigned pos, int w) {
    int* const p = lane == 0 ? &s_j2o[pos] : &L.sink[lane];
    *p = w;
  };
  // The colbits word of job group g of the window for the lane's offer (0 for a lane without one): one gather from global memory when
  // the walk enters a new group of 64 window positions (at most nwin / 64 times per round).
  auto fetch_col = [&](unsigned g) -> unsigned long long {
    const unsigned v = t_v >= 0 ? (unsigned)t_v : 0u;
    const unsigned long long w = vb.colbits[(size_t)v * MV_JGL + g];
    return t_v >= 0 ? w : 0ull;
  };
  // the walk enters group g of the window: its word from the prefetch if that is the group fetched ahead, and the word of the group
  // after it ordered now (a long window's visited jobs may skip groups: then the word is fetched on the spot)
  auto enter_group = [&](unsigned g) {
    if (__builtin_expect(g == col_next, 1)) {
      t_col = t_coln;
    } else if (nT != 0u) {
      t_col = fetch_col(g);
      WAIT_ALL_MEM();
    }
    cur_g = g;
    col_next = g + 1u < (unsigned)MV_JGL ? g + 1u : g;
    if (nT != 0u) t_coln = fetch_col(col_next);
  };
  // Lane nT becomes the owner of the untouched offer `off` that takes a job of (c, m).  Its record, snapshot state and colbits word come
  // from GLOBAL memory (wave-uniform addresses: every lane reads them, one transaction each, a single round trip for all of them).
  // Branch-free: every lane keeps its own state through selects unless it is the new owner.  As `if (lane == nT) { state = record }`
  // the loads were masked writes into a second set of registers: the compiler kept the walker's state in two homes from then on and
  // moved all of it from one to the other and back in every iteration (~45 v_mov per job on the path of a job that goes to an offer
  // touched before, which never opens a lane).
  auto open_lane = [&](unsigned nl, int off, double jc, double jm) {
    const unsigned v = wave_uniform_u32((unsigned)off);
    const OfferW w = vb.ow[v];  // one cache line (pulled into this XCD's L2 when the segment was staged)
    const unsigned long long colw = vb.colbits[(size_t)v * MV_JGL + cur_g], colwn = vb.colbits[(size_t)v * MV_JGL + col_next];
    const bool me = lane == nl;
    t_v = me ? off : t_v;
    t_oc = me ? w.oc : t_oc;
    t_om = me ? w.om : t_om;
    t_rc = me ? w.rc : t_rc;
    t_rm = me ? w.rm : t_rm;
    t_invc = me ? w.inv_dc : t_invc;
    t_invm = me ? w.inv_dm : t_invm;
    t_k8s = me ? w.k8s : t_k8s;
    t_host = me ? w.host : t_host;
    t_run = me ? w.run_count : t_run;
    t_slack = me ? w.task_slack : t_slack;
    t_ac = me ? w.ac + jc : t_ac;
    t_am = me ? w.am + jm : t_am;
    t_acount = me ? w.acount + 1 : t_acount;
    t_basec = t_rc + t_ac;
    t_basem = t_rm + t_am;
    t_col = me ? colw : t_col;
    t_coln = me ? colwn : t_coln;
    L.ac0[nl] = w.ac;  // (every lane, same value)
    L.am0[nl] = w.am;
    L.acount0[nl] = w.acount;
    unsigned char* const p = me ? &s_owner[v] : &L.sinkb[lane];
    *p = (unsigned char)nl;
  };
  // the lane for a newly touched offer: the next free one, or — all 64 taken — the lane of a DEAD offer, which is retired first: its
  // state goes to global memory now (nothing reads it before the next round), its alive bit is cleared, the owner table says "dead".
  // -> MV_T: none (the round ends).  `nxt`'s owner look-up was issued before: patched here.
  auto alloc_lane = [&](JobRegs& nxt) -> unsigned {
    if (__builtin_expect(nT < (unsigned)MV_T, 1)) return nT;
    if (!can_retire || n_retired >= MV_RETIRE_CAP) return (unsigned)MV_T;
    const bool dead = t_ac + jmin_c > t_oc || t_am + jmin_m > t_om;  // (all 64 lanes own an offer)
    const unsigned long long dm = __ballot(dead);
    if (dm == 0ull) return (unsigned)MV_T;
    const unsigned nl = (unsigned)__ffsll((unsigned long long)dm) - 1u;
    if (lane == nl) {
      st.ac[t_v] = t_ac;
      st.am[t_v] = t_am;
      st.acount[t_v] = t_acount;
      vb.ow[t_v].ac = t_ac;
      vb.ow[t_v].am = t_am;
      vb.ow[t_v].acount = t_acount;
      atomicAnd(&st.alive[(unsigned)t_v >> 6], ~(1ull << ((unsigned)t_v & 63u)));
      s_owner[(unsigned)t_v] = (unsigned char)OWNER_DEAD;
    }
    if (nxt.owner == nl) nxt.owner = OWNER_DEAD;
    if constexpr (GEF) {
      if (nxt.g_owner == nl) nxt.g_owner = OWNER_DEAD;
    }
    ++n_retired;
    wave_sync();
    return nl;
  };
  // The owner lane of a touched offer books a job of (jc, jm) — through selects as well: a branch on the lane number anywhere in the fast
  // path makes its whole region "divergent control flow" for the compiler, which then rebuilds it with flow blocks whose undefined
  // inputs keep the register coalescer from giving the walker's state ONE home (the v_mov trains of open_lane's comment).
  auto take_job = [&](bool me, double jc, double jm) {
    t_ac = me ? t_ac + jc : t_ac;
    t_am = me ? t_am + jm : t_am;
    t_acount = me ? t_acount + 1 : t_acount;
    t_basec = t_rc + t_ac;
    t_basem = t_rm + t_am;
  };
  // publish a placed member of a group whose hosts the staging gathered (fast paths): the chain in HBM (later rounds' evaluation and the
  // general path read it) and the round's log.  ghits = the log entries of the job's group.
  auto publish_group_member = [&](unsigned long long ghits, unsigned gslot, unsigned g, unsigned k, int w_offer, unsigned w_host) {
    const int prev = ghits != 0ull ? wave_read_lane(lg_k, 63 - __clzll((long long)ghits)) : s_glast[gslot];
    if (lane == 0) {
      st_agent(&st.job_to_offer[k], w_offer);
      st_agent(&st.job_prev[k], prev);
      st_agent(&st.group_last[g], (int)k);
    }
    const bool me = lane == n_log;
    lg_group = me ? g : lg_group;
    lg_host = me ? w_host : lg_host;
    lg_k = me ? (int)k : lg_k;
    ++n_log;
  };
  auto store_fail = [&](unsigned pos, unsigned char f) {
    unsigned char* const p = lane == 0 ? &s_fail[pos] : &L.sinkb[lane];
    *p = f;
  };
  // ---- the segments of the round ---------------------------------------------------------------------------------------------
  for (;;) {
  JobRegs cur = load_rec(0);
  load_owner(cur);
  JobRegs nxt = cur;
  WAIT_LDS();  // nothing pending at loop entry either (the loop's own waits sit at the END of its iterations)
  unsigned i = 0;  // walk position in the segment; after the loop: the number of the segment's walk positions done
  // The decoded form of the job in `cur` (wave-uniform values in scalar registers).  Declared by a macro because both loops below
  // need it in their own scope: the walker's state must not flow through a join of the two paths (see the loop comment).
#define WALK_DECODE()                                                                                                            \
  const unsigned cinfo_u = wave_uniform_u32(cur.info), cb_u = wave_uniform_u32(cur.f4b) >> 16;                                    \
  const bool cur_no_zero_fit = (wave_uniform_u32(cur.f4b) & 0xFFFFu) == 0u; /* no offer had zero fitness for this job under S */ \
  const unsigned b = cb_u, k = head + b;                                                                                          \
  /* the job's bit in the colbits words: by window position */                                                                   \
  const unsigned bl = b & 63u;                                                                                                    \
  const double c = cur.c, m = cur.m;                                                                                              \
  const bool grouped = (cinfo_u & JL_GROUPED) != 0;                                                                               \
  const bool job_gpu = (cinfo_u & JL_GPU) != 0;                                                                                   \
  const bool has_group = (cinfo_u & JL_HASGROUP) != 0;                                                                            \
  const unsigned gtype = (cinfo_u >> 18) & 3u;                                                                                    \
  const int nc = (int)(cinfo_u & 0xFFu);                                                                                          \
  const bool t_on = t_v >= 0;                                                                                                     \
  (void)cur_no_zero_fit, (void)k, (void)bl, (void)c, (void)m, (void)grouped, (void)job_gpu, (void)has_group, (void)gtype, (void)nc, (void)t_on
#ifdef COOK_WALK_PROF
#define WALK_PROF_BEGIN() const unsigned long long pk0 = __builtin_readcyclecounter()
#define WALK_END(cat)                                                \
  do {                                                               \
    const unsigned long long pk1_ = __builtin_readcyclecounter();    \
    ctl.prof_cyc[cat] += pk1_ - pk0;                                 \
    ctl.prof_cnt[cat] += 1u;                                         \
  } while (0)
#else
#define WALK_PROF_BEGIN() ((void)0)
#define WALK_END(cat) ((void)0)
#endif
  // TWO loops: the inner one holds nothing but the fast path and runs from job to job while that settles them; a job it cannot settle
  // leaves it for one turn of the outer loop's general path.  As ONE loop body (fast path, else general path, one latch) every variable
  // of the walker's state reached the latch through a join of the two paths, and the compiler resolved those joins with register
  // copies: ~70 v_mov per job on the fast path (state -> temporaries -> state), a quarter of its time.
  // The fast loop is unrolled by two with the job records in two register sets that swap roles (`cur` / `nxt` of one turn are `nxt` /
  // `cur` of the next): the look-ahead costs no register rotation.  fast_turn = one job: 0 = settled, on to the next; 1 = the segment
  // is used up; 2 = not settled (or settled by an untouched offer: open_off), this job leaves the loop.
  int open_off = -1;  // >= 0: the fast path gave the job to an untouched offer (committed below the loop)
  bool open_group = false;
  auto fast_turn = [&](JobRegs& cur, JobRegs& nxt) __attribute__((always_inline)) -> int {
      if (__builtin_expect(i >= n_eff, 0)) return 1;
      EMU_SITE("resolve: walk loop");
      WALK_PROF_BEGIN();
      nxt = load_rec(i + 1);  // in flight while job i is decided (its owner look-up follows at the end of this turn, when the entry's offer is there)
      WALK_DECODE();
      if (__builtin_expect((b >> 6) != cur_g, 0)) enter_group(b >> 6);  // next word of the columns
    // ======== FAST PATH ======================================================================================================
    // self-contained: decision AND commit, then straight on to the next job (its control flow never joins the general path's).
    // Two instantiations: plain jobs, and members of unique / unconstrained groups whose hosts-to-avoid the staging gathered
    // (JL_GSLOT) — kept apart so that the group code costs the plain jobs nothing.
    const unsigned gslot = (cinfo_u >> JL_GSLOT_SHIFT) & JL_GSLOT_NONE;
    auto fast_path = [&](auto group_tag) -> bool {
      constexpr bool GROUP = decltype(group_tag)::value;
      const unsigned g = GROUP ? wave_uniform_u32(cur.group) : 0xFFFFFFFFu;  // (jobs without a group never read the word)
      (void)g;
      const bool res_ok = t_on && !(t_ac + c > t_oc || t_am + m > t_om);
      bool con_ok = ((t_col >> bl) & 1ull) != 0 && t_acount < t_slack;
      if (job_gpu && t_k8s && t_run + t_acount != 0) con_ok = false;
      unsigned long long ghits = 0ull;  // log entries of this job's group
      if constexpr (GROUP) {
        ghits = __ballot(lane < n_log && lg_group == g);
        if (gtype == 1u) {  // unique host placement (constraints.clj:586-598): not where a cotask runs or was placed
          unsigned fhv[MV_FH];
#pragma unroll
          for (int q = 0; q < MV_FH; ++q) fhv[q] = s_gfh[gslot][q];
          bool forb = false;
#pragma unroll
          for (int q = 0; q < MV_FH; ++q) forb = forb | (t_host == fhv[q]);
          for (unsigned long long hm = ghits; hm != 0ull; hm &= hm - 1ull) {
            const unsigned h = (unsigned)wave_read_lane((int)lg_host, __ffsll((unsigned long long)hm) - 1);  // (every lane takes part)
            forb = forb | (t_host == h);
          }
          con_ok = con_ok & !forb;
        }
      }
      auto publish_member = [&](int w_offer, unsigned w_host) { publish_group_member(ghits, gslot, g, k, w_offer, w_host); };
      double a1 = (t_basec + c) * t_invc, a2 = (t_basem + m) * t_invm;
      fitness_terms(fit_mode, a1, a2);  // (a one-resource packer: fa is that resource's term, exactly; the fp32 margins' derivation is at fitness_terms)
      const double fa = (a1 + a2) * 0.5;
      const bool cand = res_ok && con_ok;
      // fp32 image of the approximate fitness: monotone in fa; a candidate whose approximation cannot be trusted for ordering
      // (negative terms, zero, below fp32's normal range) takes +inf, which sends the job to the general path
      const bool sane = a1 >= 0.0 && a2 >= 0.0 && fa > 0x1p-100;
      const float kf = cand ? (sane ? (float)fa : __int_as_float(0x7F800000)) : 0.0f;
      // (best-fit launches reduce here; launches with the good-enough rule only once that rule has left the job undecided — most of
      //  their jobs go to an offer above the threshold, and a reduction they never look at is ~25 instructions of the walking wave)
      float mx = 0.0f;
      if constexpr (!GEF) mx = wave_max_f32(kf);
      // first untouched entry of the list: the best untouched offer under S (a touched entry that is still feasible and sits in
      // front of it only gained fitness: it beats this one in the comparison below, so "first untouched" is all the list has to give)
      const unsigned long long untouched_mask = __ballot(cur.owner == 0xFFu);
      double u_fit = -1.0;
      int u_off = -1;
      if (__builtin_expect(untouched_mask != 0ull, 1)) {
        const int qs = __ffsll((unsigned long long)untouched_mask) - 1;
        u_fit = wave_read_lane_f64(cur.e_fit, qs);
        u_off = wave_read_lane(cur.e_off, qs);
      }
      int f_lane = -1;      // >= 0: that touched offer wins
      bool f_new = false;   // the untouched offer u_off wins
      bool ge_done = false;  // (GEF) the good-enough rule settled the job
      if constexpr (GEF) {
        if (use_ge) {
          // scheduler.clj:2312-2314: the first offer in array order whose fitness exceeds good-enough wins outright.  Untouched offers keep
          // the fitness they had under S, so their part of that order is the job's good-enough list; a touched offer is above the
          // threshold for sure when its approximate fitness clears it with a margin, below for sure the other way round — anything in
          // between (or a list that may not reach far enough) goes to the general path and its exact divisions
          // (first a look through the fp32 image the best-fit reduction uses anyway: while no touched offer comes near the threshold — the
          //  filling phase of a cycle: two thirds of the walked jobs of a C4 pool at 0.8 — the exact tests and the index reduction are skipped)
          int tg = 0x7FFFFFFF;  // lowest offer index among the touched offers above the threshold
          int tl = -1;          // ... and its lane
          if (__ballot(kf >= ge_near_f) != 0ull) {
            const bool above = cand && sane && eps_lo(fa) > good_enough;
            const bool maybe = cand && !above && (!sane || eps_hi(fa) > good_enough);
            if (__builtin_expect(__any(maybe), 0)) return false;
            const unsigned long long above_mask = __ballot(above);
            if (above_mask != 0ull) {
              if ((above_mask & (above_mask - 1ull)) == 0ull) {  // one touched offer above the threshold — the common case — needs no reduction
                tl = __ffsll((unsigned long long)above_mask) - 1;
                tg = wave_read_lane(t_v, tl);
              } else {
                const unsigned tkey = above ? 0x7FFFFFFFu - (unsigned)t_v : 0u;
                const unsigned tmx = wave_max_u32(tkey);
                tg = 0x7FFFFFFF - (int)tmx;
                tl = __ffsll((unsigned long long)__ballot(above && tkey == tmx)) - 1;
              }
            }
          }
          const int ng = (int)((cinfo_u >> 8) & 0xFFu);
          int ge_pick = 0x7FFFFFFF;
          if (ng != 0) {
            const unsigned long long gun = __ballot((int)lane < ng && cur.g_owner == 0xFFu);
            if (__builtin_expect(gun != 0ull, 1)) {
              const int q = __ffsll((unsigned long long)gun) - 1;
              ge_pick = wave_read_lane(cur.g_off, q);
            } else if (cinfo_u & JL_GTRUNC) {
              // every listed offer is touched by now: untouched ones above the threshold may exist beyond the list, below the best touched index or not
              if (tg > wave_read_lane(cur.g_off, ng - 1)) return false;
            }
          } else if (cinfo_u & JL_GTRUNC) {
            return false;
          }
          if (tg < ge_pick) {
            f_lane = tl;
            ge_done = true;
          } else if (ge_pick != 0x7FFFFFFF) {
            f_new = true;
            u_off = ge_pick;
            ge_done = true;
          }  // else: nobody above the threshold — best fit among what is below it
        }
      }
      if constexpr (GEF) {
        if (!ge_done) mx = wave_max_f32(kf);
      }
      if (ge_done) {
        // (decided above)
      } else if (__builtin_expect(mx == 0.0f, 0)) {  // no touched offer can take the job
        f_new = u_off >= 0;  // else: unmatched or list exhausted -> general path
      } else if (__builtin_expect(mx < __int_as_float(0x7F800000), 1)) {
        const unsigned long long near = __ballot(kf >= mx * (1.0f - 0x1p-20f));
        if (__builtin_expect((near & (near - 1ull)) == 0ull, 1)) {  // one touched offer clearly ahead of the other touched ones
          const int wl = __ffsll((unsigned long long)near) - 1;
          const double fw = wave_read_lane_f64(fa, wl);
          if (__builtin_expect(u_off < 0, 0)) {
            // no untouched entry: fine unless the list is truncated and none of its entries is still a candidate (then better
            // untouched offers may exist beyond the list: exhausted, general path)
            bool ok = COOK_L_COMPLETE();
            if (!ok) {
              const unsigned long long cand_mask = __ballot(cand);
              const bool e_live = cur.owner < (unsigned)MV_T && ((cand_mask >> (cur.owner & 63u)) & 1ull);
              ok = __any(e_live);
            }
            if (ok) f_lane = wl;
          } else if (__builtin_expect(eps_lo(fw) > u_fit, 1)) {
            f_lane = wl;
          } else if (eps_hi(fw) < u_fit) {
            f_new = true;
          }
        }
      }
      // the booking by the winner's lane, on EVERY way out of here (f_lane = -1: no lane): as a statement of the branch below the booked
      // fields met their unbooked selves where the fast path's exits join, and were moved between two sets of registers for it
      take_job((int)lane == f_lane, c, m);
      if (__builtin_expect(f_lane >= 0, 1)) {  // an offer touched earlier in this round takes the job
        const int w = wave_read_lane(t_v, f_lane);
        store_result(i, w);  // (s_fail[i] = 0 since the staging)
        if constexpr (GROUP) publish_member(w, (unsigned)wave_read_lane((int)t_host, f_lane));
        WALK_STAT(3, 1);
        WALK_STAT(8, 1);
        WALK_END(GROUP ? 4u : ((GEF && ge_done) ? 6u : 1u));
        return true;
      }
      if (__builtin_expect(f_new && (nT < (unsigned)MV_T || can_retire), 1)) {  // an untouched offer: a lane takes ownership — outside this loop (see below)
        open_off = u_off;
        open_group = GROUP;
      }
      return false;
    };
    bool fast_done = false;
    if (GEF || !(good_enough < 1.0)) {
      if (__builtin_expect(!(cinfo_u & (JL_GROUPED | JL_HASGROUP | JL_XRES)), 1))
        fast_done = fast_path(std::false_type{});
      else if (gslot != JL_GSLOT_NONE && n_log < (unsigned)COOK_WAVE)
        fast_done = fast_path(std::true_type{});
    }
    load_owner(nxt);  // (before a commit of the paths below: they patch it)
    if (__builtin_expect(!fast_done, 0)) {
      WALK_END(7u);  // (measurement build: the turn's share of a job that the paths below the loop finish)
      return 2;
    }
    WAIT_LDS_BUT_2();  // the record of the next job has arrived (see common.hpp); the result store and the owner look-up may still fly
    ++i;
    return 0;
  };
  for (;;) {
    bool walk_over = false;
    open_off = -1;
    open_group = false;
    for (;;) {  // ---- fast loop ----
      int r = fast_turn(cur, nxt);
      if (__builtin_expect(r == 0, 1)) r = fast_turn(nxt, cur) | 4;  // (bit 2: the register sets are swapped)
      if (__builtin_expect((r & 3) == 0, 1)) continue;
      walk_over = (r & 3) == 1;
      if (r & 4) {  // back to `cur` = this job, `nxt` = the next one
        const JobRegs t = cur;
        cur = nxt;
        nxt = t;
      }
      break;
    }  // ---- fast loop ----
    if (__builtin_expect(walk_over, 0)) break;
    // (prefetches and the column word of the job in `cur` are in place: the fast loop's turn for it issued them)
    WALK_PROF_BEGIN();
    unsigned pcat = 0;
    (void)pcat;
    WALK_DECODE();
    if (__builtin_expect(open_off >= 0, 1)) {
      // ---- the fast path's other verdict: an untouched offer takes the job and the next free lane becomes its owner.  Committed HERE,
      // outside the fast loop: the fields open_lane writes (an offer's totals, reciprocals, host ...) are then loop-invariant inside
      // it, and only there does the compiler keep them in ONE set of registers without moving them about
      const unsigned g = open_group ? wave_uniform_u32(cur.group) : 0xFFFFFFFFu;
      const unsigned gslot = (cinfo_u >> JL_GSLOT_SHIFT) & JL_GSLOT_NONE;
      const unsigned long long ghits = open_group ? __ballot(lane < n_log && lg_group == g) : 0ull;
      const unsigned nl = alloc_lane(nxt);
      if (__builtin_expect(nl == (unsigned)MV_T, 0)) {
        stop = 2;  // no lane to track a new touched offer: end the round before this job (the fast path booked nothing for it)
        resolved = b;
        break;
      }
      open_lane(nl, open_off, c, m);
      WAIT_ALL_MEM();
      if (open_group) publish_group_member(ghits, gslot, g, k, open_off, (unsigned)wave_read_lane((int)t_host, (int)nl));
      // the owner look-up of the next job was issued before this commit: patch it
      if (nxt.owner == 0xFFu && nxt.e_off == open_off) nxt.owner = nl;
      if constexpr (GEF) {
        if (nxt.g_owner == 0xFFu && nxt.g_off == open_off) nxt.g_owner = nl;
      }
      nT += nT < (unsigned)MV_T ? 1u : 0u;
      store_result(i, open_off);
      wave_sync();  // the owner table update is visible to the whole wave before the next look-up reads it
      WALK_STAT(4, 1);
      WALK_STAT(8, 1);
      WALK_END(open_group ? 4u : 2u);
      WAIT_LDS_BUT_LAST();
      cur = nxt;
      ++i;
      continue;
    }
    const unsigned g = has_group ? wave_uniform_u32(cur.group) : 0xFFFFFFFFu;
    int win = -1, win_lane = -1;  // win_lane >= 0: a touched offer wins; else win >= 0: that untouched offer
    bool need_exact = false;
    bool exhausted = false;  // the job's list ran out: the round ends here
    unsigned pe_bits = 8u;   // exact verdict of this lane's offer (only when the exact path ran)
    double pe_fit = 0.0;
    unsigned jj = 0;
    // values of the general path that the unmatched branch of the commit reads
    bool res_ok_g = false, con_ok_g = false;
    double nc_g = 0.0, nm_g = 0.0;
    // ======== GENERAL PATH ===================================================================================================
    {
      bool gok = true;
      if (grouped) {
        jj = j_index ? j_index[k] : k;
        // a second member of a balanced / attribute-equals group after one was placed in this round: re-snapshot first
        // (the loaded word through a scalar register: to the compiler a load through a generic pointer is a per-lane value, the branch on
        //  it a divergent exit of the walk loop, and everything the loop carries — walk position, touched count — divergent with it)
        if (gtype >= 2 && (int)wave_uniform_u32((unsigned)ld_agent(&st.group_last[g])) >= (int)head) {
          stop = 3;
          resolved = b;
          break;
        }
        if (t_v >= 0) gok = group_pass_dev(vb.in_dev, st, jj, (unsigned)t_v);
      }
      // every touched offer re-evaluated under the current state: verdict + approximate fitness
      bool res_ok = t_on && !(t_ac + c > t_oc || t_am + m > t_om);
      if (cinfo_u & JL_XRES) {  // ports / named scalars: the counters of the call live in HBM (only such jobs move them)
        jj = j_index ? j_index[k] : k;
        if (res_ok) res_ok = xres_fail_dev(vb.in_dev, st, jj, (unsigned)t_v) == 0u;
      }
      bool con_ok = ((t_col >> bl) & 1ull) != 0 && t_acount < t_slack && gok;
      if (job_gpu && t_k8s && t_run + t_acount != 0) con_ok = false;
      const double nc_ = t_basec + c, nm_ = t_basem + m;  // (rc + ac) + c, (rm + am) + m
      double a1 = nc_ * t_invc, a2 = nm_ * t_invm;
      fitness_terms(fit_mode, a1, a2);
      const double fa = (a1 + a2) * 0.5;
      const bool cand = res_ok && con_ok;
      res_ok_g = res_ok, con_ok_g = con_ok, nc_g = nc_, nm_g = nm_;
      // the approximation is trusted for ordering only when both terms are non-negative and the result is positive
      const bool sane = a1 >= 0.0 && a2 >= 0.0 && fa > 0.0;
      need_exact = (good_enough < 1.0) || __any(cand && !sane);
      const unsigned long long cand_mask = __ballot(cand);
      double u_fit = -1.0;     // best untouched candidate: fitness under S, offer
      int u_off = -1;
      bool decided = false;
      do {
        // No feasible offer under S, no zero-fitness offer, no constrained group: placements only take capacity away and the
        // job's constraints can only get worse on a touched offer, so it stays unmatched whatever happened in this round;
        // only its failure summary may change (handled below from the touched offers' current verdicts).
        WALK_STAT(0, 1);
        WALK_STAT(6, nT);
        if (nc == 0 && !grouped && cur_no_zero_fit) {
          WALK_STAT(1, 1);
          break;
        }
        // --- arg-max path: first list entry that is untouched, or touched and still a candidate -------------------------------
        // (a touched offer that is still feasible only gained fitness, so it dominates every untouched offer behind it; a
        //  zero-fitness verdict cannot appear on an offer that was feasible under S)
        const bool e_untouched = cur.owner == 0xFFu;
        const bool e_live = cur.owner < (unsigned)MV_T && ((cand_mask >> (cur.owner & 63u)) & 1ull);
        const unsigned long long settle_mask = __ballot(e_untouched || e_live), untouched_mask = __ballot(e_untouched);
        if (settle_mask == 0ull && COOK_L_TRUNC()) {
          exhausted = true;
          break;
        }
        if (settle_mask != 0ull) {
          const int qs = __ffsll((unsigned long long)settle_mask) - 1;
          if ((untouched_mask >> qs) & 1ull) {
            u_fit = wave_read_lane_f64(cur.e_fit, qs);
            u_off = wave_read_lane(cur.e_off, qs);
          }
        }
        // --- best touched candidate ----------------------------------------------------------------------------------------------
        if (!need_exact) {
          if (cand_mask == 0ull) {
            win = u_off;
            decided = true;
          } else {
            const unsigned long long key = cand ? (unsigned long long)__double_as_longlong(fa) : 0ull;  // positive doubles
            const double mx = __longlong_as_double((long long)wave_max_u64(key));
            const unsigned long long near = __ballot(cand && fa >= eps_lo(mx));
            if ((near & (near - 1ull)) == 0ull) {  // one touched offer clearly ahead of the other touched ones
              if (u_off < 0 || eps_lo(mx) > u_fit) {
                win_lane = __ffsll((unsigned long long)near) - 1;
                decided = true;
              } else if (eps_hi(mx) < u_fit) {
                win = u_off;
                decided = true;
              }
            }
            if (!decided) need_exact = true;
          }
        }
        if (need_exact) {
          WALK_STAT(2, 1);
          if (t_on) {
            pe_bits = 0u;
            if (!res_ok) {
              pe_bits = 1u;
            } else if (!con_ok) {
              pe_bits = 2u;
            } else {
              pe_fit = fitness_calc(fit_mode, nc_, t_oc + t_rc, nm_, t_om + t_rm);
              if (!(pe_fit > 0.0)) pe_bits = 4u;
            }
          }
          const bool t_feas = t_on && pe_bits == 0u;
          const unsigned long long feas_mask = __ballot(t_feas);
          // with exact verdicts a list entry settles only if its owner is still FEASIBLE (zero fitness excluded)
          const bool e_live2 = cur.owner < (unsigned)MV_T && ((feas_mask >> (cur.owner & 63u)) & 1ull);
          const unsigned long long settle2 = __ballot(e_untouched || e_live2);
          if (settle2 == 0ull && COOK_L_TRUNC()) {
            exhausted = true;
            break;
          }
          u_fit = -1.0;
          u_off = -1;
          if (settle2 != 0ull) {
            const int qs = __ffsll((unsigned long long)settle2) - 1;
            if ((untouched_mask >> qs) & 1ull) {
              u_fit = wave_read_lane_f64(cur.e_fit, qs);
              u_off = wave_read_lane(cur.e_off, qs);
            }
          }
          // good-enough path: lowest offer index with fitness > good-enough (scheduler.clj:2312-2314)
          int ge_pick = 0x7FFFFFFF, ge_lane = -1;
          if (good_enough < 1.0) {
            if constexpr (!GE) {  // (launches for good-enough-fitness < 1 are GE launches: the host sees to it)
              exhausted = true;
              break;
            } else {
              const int ng = (int)((cinfo_u >> 8) & 0xFFu);
              int ge_off = -1;
              unsigned g_owner = 0xFEu;
              if ((int)lane < ng) {
                ge_off = s_goff[(size_t)i * LG + lane];
                g_owner = ge_off >= 0 ? (unsigned)s_owner[(unsigned)ge_off] : 0xFEu;
              }
              const unsigned long long gun = __ballot(g_owner == 0xFFu);
              int last_idx = -1;
              if (ng > 0) last_idx = wave_read_lane(ge_off, ng - 1);
              if (gun != 0ull) {
                const int q = __ffsll((unsigned long long)gun) - 1;
                ge_pick = wave_read_lane(ge_off, q);
              }
              // lowest-index touched offer that is feasible with fitness > good-enough
              const unsigned long long tkey = (t_feas && pe_fit > good_enough)
                                                  ? (((unsigned long long)(unsigned)(0x7FFFFFFF - t_v) << 32) | (unsigned long long)lane)
                                                  : 0ull;
              const unsigned long long tmx = feas_mask != 0ull ? wave_max_u64(tkey) : 0ull;
              const int tg = tmx != 0ull ? 0x7FFFFFFF - (int)(unsigned)(tmx >> 32) : 0x7FFFFFFF;
              if (gun == 0ull && (cinfo_u & JL_GTRUNC) && tg > last_idx) {
                // untouched good-enough offers beyond the list may exist with an index below the best touched one
                exhausted = true;
                break;
              }
              if (tg < ge_pick) {
                ge_pick = tg;
                ge_lane = (int)(unsigned)(tmx & 63ull);
              }
            }
          }
          if (ge_pick != 0x7FFFFFFF) {
            if (ge_lane >= 0) {
              win_lane = ge_lane;
            } else {
              win = ge_pick;
            }
          } else {
            // best touched (max fitness, lowest offer index on ties) vs best untouched
            Cand best{-1.0, -1};
            int best_lane = -1;
            if (feas_mask != 0ull) {
              const unsigned long long key = t_feas ? (unsigned long long)__double_as_longlong(pe_fit) : 0ull;
              const unsigned long long mx = wave_max_u64(key);
              unsigned long long tie = __ballot(t_feas && key == mx);
              int wl = __ffsll((unsigned long long)tie) - 1;
              int wv = wave_read_lane(t_v, wl);
              tie &= tie - 1ull;
              while (tie != 0ull) {  // equal fitness on several touched offers: the lowest offer index wins
                const int l2 = __ffsll((unsigned long long)tie) - 1;
                const int v2 = wave_read_lane(t_v, l2);
                if (v2 < wv) {
                  wv = v2;
                  wl = l2;
                }
                tie &= tie - 1ull;
              }
              best = Cand{__longlong_as_double((long long)mx), wv};
              best_lane = wl;
            }
            if (u_off >= 0 && cand_better(Cand{u_fit, u_off}, best)) {
              win = u_off;
            } else if (best_lane >= 0) {
              win_lane = best_lane;
            }
          }
        }
      } while (0);
    }
    if (exhausted) {  // end the round here: the next round evaluates the rest of the window afresh
      stop = 1;
      resolved = b;
      break;
    }
    // --- commit --------------------------------------------------------------------------------------------------------------
    if (win_lane >= 0) WALK_STAT(3, 1);
    else if (win >= 0) WALK_STAT(4, 1);
    else WALK_STAT(5, 1);
    WALK_STAT_PREV_LANE(i, win_lane, win, nT);
#ifdef COOK_WALK_PROF
    pcat = grouped ? 4u : (win >= 0 || win_lane >= 0 ? 5u : 3u);
#endif
    unsigned new_lane = (unsigned)MV_T;  // the lane an untouched winner was given
    if (win_lane >= 0) {  // an offer touched earlier in this round takes the job
      take_job((int)lane == win_lane, c, m);
      win = wave_read_lane(t_v, win_lane);
    } else if (win >= 0) {  // an untouched offer: a lane takes ownership
      new_lane = alloc_lane(nxt);
      if (new_lane == (unsigned)MV_T) {
        stop = 2;  // no lane to track a new touched offer: end the round before this job
        resolved = b;
        break;
      }
      open_lane(new_lane, win, c, m);
      WAIT_ALL_MEM();
      // the owner look-up of the next job was issued before this commit: patch it
      if (nxt.owner == 0xFFu && nxt.e_off == win) nxt.owner = new_lane;
      if constexpr (GEF) {
        if (nxt.g_owner == 0xFFu && nxt.g_off == win) nxt.g_owner = new_lane;
      }
      nT += nT < (unsigned)MV_T ? 1u : 0u;
      wave_sync();  // the owner table update is visible to the whole wave before the next look-up reads it
    }
    if (win >= 0) {
      if (cinfo_u & JL_XRES) {  // the offer's owner lane books the job's ports / named scalars
        const int ol = win_lane >= 0 ? win_lane : (int)new_lane;
        if ((int)lane == ol) {
          const MatchIn& in = *vb.in_dev;
          if (!L.x0set[lane]) {
            L.x0set[lane] = 1;
            L.x0p[lane] = ld_agent(&st.xports[win]);
            _Pragma("unroll") for (unsigned sc = 0; sc < 3u; ++sc)
              if (sc < in.n_scal) L.x0s[lane][sc] = ld_agent(&st.xscal[(size_t)sc * in.M + (unsigned)win]);
          }
          xres_commit(in, st, jj, (unsigned)win);
        }
      }
      store_result(i, win);
      store_fail(i, 0);
      if (g != 0xFFFFFFFFu) {
        if (lane == 0) {  // cotasks look each other up through HBM (group_pass): publish at once
          st_agent(&st.job_to_offer[k], win);
          st_agent(&st.job_prev[k], ld_agent(&st.group_last[g]));
          st_agent(&st.group_last[g], (int)k);
        }
        wave_sync();  // later cotasks of this wave read what lane 0 just published
        // ... and the round's log, for the members that take the fast path (the owner lane of the winning offer knows its host)
        const int ol = win_lane >= 0 ? win_lane : (int)new_lane;
        const unsigned w_host = (unsigned)wave_read_lane((int)t_host, ol);
        if (n_log < (unsigned)COOK_WAVE) {
          if (lane == n_log) {
            lg_group = g;
            lg_host = w_host;
            lg_k = (int)k;
          }
          ++n_log;
        } else {
          n_log = COOK_WAVE + 1u;  // overflow: the log is incomplete from here on
        }
      }
    } else {
      // unmatched: failure summary = OR over offers of the first failing check under the CURRENT state.  Start from the
      // snapshot counts and swap each touched offer's snapshot verdict for its current one (exact verdicts needed).
      // (only the general path gets here: the fast path never leaves a job unmatched)
      const JobL jl = s_job[i];
      int d1 = 0, d2 = 0, d4 = 0;
      if (nT != 0) {  // wave-uniform
        if (pe_bits == 8u && t_on) {  // the exact path did not run for this job
          pe_bits = 0u;
          if (!res_ok_g) {
            pe_bits = 1u;
          } else if (!con_ok_g) {
            pe_bits = 2u;
          } else {
            pe_fit = fitness_calc(fit_mode, nc_g, t_oc + t_rc, nm_g, t_om + t_rm);
            if (!(pe_fit > 0.0)) pe_bits = 4u;
          }
        }
        unsigned p0 = 0u;  // snapshot verdict: state at round start, group placements of this round ignored via the cutoff
        if (t_on) {
          const double ac0 = L.ac0[lane], am0 = L.am0[lane];  // the offer's state as the round began
          const int acount0 = L.acount0[lane];
          bool x0_fail = false;
          if (cinfo_u & JL_XRES) {  // ports / named scalars as the round began: saved if a job of this round moved them, else current
            const MatchIn& in = *vb.in_dev;
            const bool sv = L.x0set[lane] != 0;
            const int jp = in.j_ports ? in.j_ports[jj] : 0;
            const long long up = sv ? L.x0p[lane] : ld_agent(&st.xports[t_v]);
            if (jp > 0 && up + jp > (long long)(in.o_ports ? in.o_ports[t_v] : 0)) x0_fail = true;
            _Pragma("unroll") for (unsigned sc = 0; sc < 3u; ++sc) {
              if (sc >= in.n_scal) break;
              const double rq = in.j_scal[sc][jj];
              const double us = sv ? L.x0s[lane][sc] : ld_agent(&st.xscal[(size_t)sc * in.M + (unsigned)t_v]);
              if (rq == rq && us + rq > (in.o_scal[sc] ? in.o_scal[sc][t_v] : 0.0)) x0_fail = true;
            }
          }
          if (ac0 + c > t_oc || am0 + m > t_om || x0_fail) {
            p0 = 1u;
          } else {
            bool ok = ((t_col >> bl) & 1ull) != 0 && acount0 < t_slack;
            if (job_gpu && t_k8s && t_run + acount0 != 0) ok = false;
            if (ok && grouped) {
              MatchState st0 = st;
              st0.cutoff = (int)head;
              ok = group_pass_dev(vb.in_dev, st0, jj, (unsigned)t_v);
            }
            if (!ok) {
              p0 = 2u;
            } else {
              const double f0 = fitness_calc(fit_mode, t_rc + ac0 + c, t_oc + t_rc, t_rm + am0 + m, t_om + t_rm);
              if (!(f0 > 0.0)) p0 = 4u;
            }
          }
        }
        d1 = __popcll(__ballot(t_on && (pe_bits & 1u))) - __popcll(__ballot(t_on && (p0 & 1u)));
        d2 = __popcll(__ballot(t_on && (pe_bits & 2u))) - __popcll(__ballot(t_on && (p0 & 2u)));
        d4 = __popcll(__ballot(t_on && (pe_bits & 4u))) - __popcll(__ballot(t_on && (p0 & 4u)));
      }
      // ... and the RETIRED offers of the round: each fails on resources now (dead), so class 1 is not empty; what class each was in
      // under S for THIS job nobody kept, so classes 2 / 4 are only certain when the snapshot count is zero (no retired offer can have
      // been in the class) or larger than every offer that may have left it.  Anything in between needs a fresh snapshot: the round
      // ends before this job (rare: unmatched jobs that are walked at all are, and only after a round's 65th offer).
      if (n_retired != 0u) {
        const int hi2 = (int)jl.f2 + d2, hi4 = (int)jl.f4 + d4;  // (upper bounds: the retired offers can only take away)
        const bool amb2 = jl.f2 != 0 && hi2 > 0 && hi2 - (int)n_retired <= 0, amb4 = jl.f4 != 0 && hi4 > 0 && hi4 - (int)n_retired <= 0;
        if (amb2 || amb4) {
          stop = 5;
          resolved = b;
          break;
        }
        d1 += (int)n_retired;
      }
      const unsigned bits = (((int)jl.f1 + d1) > 0 ? 1u : 0u) | (((int)jl.f2 + d2) > 0 ? 2u : 0u) | (((int)jl.f4 + d4) > 0 ? 4u : 0u);
      store_result(i, -1);  // (branch-free like the fast path's: this is the last statement before the paths of the iteration meet)
      store_fail(i, (unsigned char)(bits ? bits : 8u));
    }
    WALK_END(pcat);
    WAIT_ALL_MEM();
    cur = nxt;
    ++i;
  }
#undef WALK_DECODE
#undef WALK_PROF_BEGIN
#undef WALK_END
  // ---- the segment is over (used up, or the round stopped inside it): flush its results ----------------------------------------
  wave_sync();
  // the segment's counts, read off the results (counters carried through the walk loop cost it instructions in every job): matched
  // jobs, "the head of the queue was matched", walked jobs with a truncated list (incl. the job the round stopped at, if any)
  {
    const unsigned n_seen = i < n_eff ? i + 1u : i;
    for (unsigned x0 = 0; x0 < n_seen; x0 += COOK_WAVE) {
      const unsigned x = x0 + lane;
      const bool got = x < i && s_j2o[x] >= 0;
      matched += (unsigned)__popcll(__ballot(got));
      if (__ballot(got && head + (unsigned)s_job[x < n_seen ? x : 0u].b == 0u) != 0ull) head_matched = 1;
      n_trunc += (unsigned)__popcll(__ballot(x < n_seen && (s_job[x < n_seen ? x : 0u].info & JL_TRUNC) != 0u));
    }
  }
  for (unsigned x = lane; x < i; x += COOK_WAVE) {  // the walked jobs (the others were settled, and written, in the parallel phase)
    const unsigned bx = s_job[x].b;
    st.job_to_offer[head + bx] = s_j2o[x];
    if (st.fail_code) st.fail_code[head + bx] = s_fail[x];
  }
  // The next segment of the same window, if the round did not stop and there is one: the lists of its jobs were computed against the
  // same snapshot, the walker keeps its lanes (the offers it touched are exactly the ones whose list entries it re-evaluates), so the
  // walk simply goes on — the workgroup stages the segment, no launch and no evaluation in between.
  if (stop != 0 || seg_lo + n_eff >= n_list) break;
  seg_lo += n_eff;
  if (lane == 0) {
    L.seg_lo = seg_lo;
    L.cmd = 1;
    s_ngslots = 0;
  }
  {
    const unsigned long long ts0 = cook_ticks();
    EMU_SITE("resolve: walker asks for the next segment");
    __syncthreads();  // (releases the other waves into stage_segment)
    n_eff = stage_segment(seg_lo);
    if (lane == 0) L.cmd = 0;  // (read by the others only behind the next barrier)
    ++n_segments;
    t_stage += cook_ticks() - ts0;
  }
  }  // ---- segments ----
  // ---- the round is over: release the other waves, write the touched offers' state back and publish the new head ------------------
  if (lane == 0) L.cmd = 0;
  EMU_SITE("resolve: walker done");
  __syncthreads();
  if (t_v >= 0) {
    st.ac[t_v] = t_ac;
    st.am[t_v] = t_am;
    st.acount[t_v] = t_acount;
    vb.ow[t_v].ac = t_ac;
    vb.ow[t_v].am = t_am;
    vb.ow[t_v].acount = t_acount;
    if (t_ac + st.jmin[0] > t_oc || t_am + st.jmin[1] > t_om)  // full for every job of this call, for good
      atomicAnd(&st.alive[(unsigned)t_v >> 6], ~(1ull << ((unsigned)t_v & 63u)));
  }
  if (lane == 0)
    resolve_finish(ctl, vb, head, nwin, resolved, stop, matched, head_matched, nT + n_retired, n_list, n_segments, n_trunc, t_stage,
                   cook_ticks() - tk0, L.dbg_h);
}

template <bool GE>
__global__ void __launch_bounds__(MV_RTHREADS) match_resolve2(MatchState st, V2Buf vb) {
  __shared__ __attribute__((aligned(16))) char lds[MV_RLDS_BYTES];
  resolve_round<GE>(lds, st, vb);
}
