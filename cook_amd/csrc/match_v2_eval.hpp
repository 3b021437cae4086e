// match_v2_eval.hpp — the evaluation of a window: the cheap parts of the constraint check (static_fast ...), the wave's offer loop, match_eval2.
// Part of match_v2.hpp: needs match_v2_shapes.hpp (records, ChunkRecT, V2Buf); reads what match_v2_pack.hpp's kernels wrote.
#pragma once

// ---- the cheap parts of the constraint check, from the packed records only ---------------------------------------------
// gpu-host model/count (constraints.clj:122-157) + rebalancer reservation (constraints.clj:242-252)
static __device__ __forceinline__ bool static_fast(const JobRec& j, const OfferB& o, const MatchIn& in, unsigned v) {
  bool ok;
  if (o.flags & 1u) {
    if (j.g > 0) {
      double avail = (o.gpu_model != 0 && o.gpu_model == j.gpu_model) ? o.gpu_count : 0.0;
      if (o.flags & 4u) avail = map_get_dev(in.o_gpu_model, in.o_gpu_count, in.gpu_slots, v, j.gpu_model);
      ok = avail == j.g;
    } else {
      ok = o.gpu_model == 0;
    }
  } else {
    ok = j.g == 0;
  }
  if ((o.flags & 2u) && j.reserved_host != (int)o.host) ok = false;
  return ok;
}
// gpu-host "no task on the VM" + max-tasks-per-host (constraints.clj:433-456) under `acount` placements of this call
static __device__ __forceinline__ bool dyn_fast(const JobRec& j, const OfferB& o, int acount) {
  if (j.g > 0 && (o.flags & 1u) && o.run_count + acount != 0) return false;
  return acount < o.task_slack;
}
// the pool's fitness calculator (fm = cook_params.fitness; 0 = cpuMemBinPacker, config.clj:108), operation for operation as the oracle computes it.
// Only the bin packers (0..2) reach the window rounds: the walk rests on "a placement never lowers the fitness of the offer it lands on", which
// the spreaders turn round (the host places those by the serial sweep, match_host.hpp).
static __device__ __forceinline__ double fitness_of(unsigned fm, const OfferA& a, double ac, double am, double c, double m) {
  return fitness_calc(fm, a.rc + ac + c, a.oc + a.rc, a.rm + am + m, a.om + a.rm);
}
// The approximate terms a1 ~ cf, a2 ~ mf (numerator times the rounded reciprocal of the denominator) under a one-resource packer: the term that
// does not count is replaced by the one that does, and every expression built for cpuMemBinPacker then stands for the one-resource fitness
// EXACTLY: (x + x) * 0.5 == x in binary floating point (the sum is a change of exponent, the halving another; no overflow: x is a fill ratio).
// So the bounds are derived for ONE term x = fl(n * fl(1 / d)) against the exact fitness fl(n / d), n >= 0, d > 0, u = 2^-53:
//   x = (n / d) (1 + e1) (1 + e2) with |e1|, |e2| <= u (reciprocal, product), fl(n / d) = (n / d) (1 + e3) with |e3| <= u
//   => |x - fl(n / d)| <= fl(n / d) * ((1 + u)^2 / (1 - u) - 1) < fl(n / d) * 2^-51 (3u + O(u^2)).
// (The two-resource form adds the rounding of its sum on either side, 2^-50 in all; its constants below were chosen with that in hand.)
//   pruning bound (eval): a pair is skipped when x < thr = tf * (1 - 2^-40), tf the lane's worst kept fitness.  Then fl(n / d) <= x (1 + 2^-51)
//     < tf (1 - 2^-40) (1 + 2^-51) < tf: the exact fitness could not have entered the list.  Towards good-enough: fl(n / d) > ge implies
//     x >= fl(n / d) (1 - 2^-51) > ge (1 - 2^-40) = ge_lo for ge >= 0, so a pair that clears the threshold is never skipped.
//   guard band (resolve, general path): two fitness values whose approximations differ by more than a factor 1 -+ 2^-38 are ordered as their
//     approximations are, since each lies within 2^-51 relative of its own exact value and 2 * 2^-51 < 2^-38.
//   fp32 image (resolve, fast path): kf = fl32(x) for 2^-100 < x <= 1, round to nearest: monotone, kf = x (1 + d), |d| <= 2^-24.
//     "one touched offer clearly ahead": mx = max kf is lane w's, and every other candidate q has kf_q < fl32(mx (1 - 2^-20))
//     <= mx (1 - 2^-20) (1 + 2^-24).  Then x_q <= kf_q / (1 - 2^-24) < x_w (1 - 2^-20) (1 + 2^-24)^2 / (1 - 2^-24) < x_w (1 - 2^-21), and with
//     each x within 2^-51 relative of its exact value: fl(n_q / d_q) <= x_q (1 + 2^-51) < x_w (1 - 2^-21) (1 + 2^-51) < x_w (1 - 2^-51)
//     <= fl(n_w / d_w), strictly.  All it asks of the approximation is 2 * 2^-51 < 2^-21.  w against the best untouched entry (exact under
//     S) goes through the 2^-38 band above, in fp64.
//     good-enough, first look: ge_near_f = fl32(ge (1 - 2^-30)).  Rounding is monotone, so kf < ge_near_f implies x < ge (1 - 2^-30), hence
//     x (1 + 2^-38) < ge: the lane is neither "above" nor "maybe above" in the fp64 tests that a nearer lane gets (x (1 - 2^-38) > ge
//     implies fl(n / d) >= x (1 - 2^-51) > ge; x (1 + 2^-38) <= ge implies fl(n / d) <= x (1 + 2^-51) <= ge by the same margin).
// The one-resource error (2^-51) is below the two-resource one (2^-50), so the same 2^-40 / 2^-38 / 2^-20 / 2^-30 bands hold, each by the
// inequality written out above for one term.  One-resource fitness values tie far more often than two-resource ones (every offer of a
// pool of equal machines filled alike); a tie is inside every band and goes to the exact divisions, as any near-tie does.
static __device__ __forceinline__ void fitness_terms(unsigned fm, double& a1, double& a2) {
  if (fm != 0u) {  // (uniform over the pool)
    if (fm == 1u) a2 = a1;
    else a1 = a2;
  }
}

template <int N>
static __device__ __forceinline__ void topl_insert(double (&tf)[N], int (&ti)[N], double fit, int idx) {
  // precondition: (fit, idx) is better than the last entry; bubble it up (strictly better only: earlier index stays first)
  tf[N - 1] = fit;
  ti[N - 1] = idx;
#pragma unroll
  for (int q = N - 1; q > 0; --q) {
    const bool sw = tf[q] > tf[q - 1] || (tf[q] == tf[q - 1] && ti[q] >= 0 && (ti[q - 1] < 0 || ti[q] < ti[q - 1]));
    if (sw) {
      const double a = tf[q];
      tf[q] = tf[q - 1];
      tf[q - 1] = a;
      const int x = ti[q];
      ti[q] = ti[q - 1];
      ti[q - 1] = x;
    }
  }
}

// The same for a lane that meets its offers in ASCENDING index order (a wave's walk over its offer batch): a new entry only passes
// entries it beats strictly, so position = number of entries it beats — N independent compares and a shift by selects, no
// dependent compare-swap chain (the insertion was a third of the eval wave's time).
template <int N>
static __device__ __forceinline__ void topl_insert_ascending(double (&tf)[N], int (&ti)[N], double fit, int idx) {
  bool g[N];
#pragma unroll
  for (int q = 0; q < N; ++q) g[q] = fit > tf[q];  // monotone in q: the list descends (empty entries hold -1)
#pragma unroll
  for (int q = N - 1; q > 0; --q) {
    tf[q] = g[q - 1] ? tf[q - 1] : (g[q] ? fit : tf[q]);
    ti[q] = g[q - 1] ? ti[q - 1] : (g[q] ? idx : ti[q]);
  }
  tf[0] = g[0] ? fit : tf[0];
  ti[0] = g[0] ? idx : ti[0];
}

// The rare paths of the offer loops as real calls on the device copy of MatchIn: inlined, their CSR walks kept some forty kernel
// arguments alive across the loop and the compiler spilled scalar registers into VGPR lanes (281 v_readlane restores per offer
// iteration of the eval kernel).
static __device__ __attribute__((noinline)) bool group_pass_dev(const MatchIn* in, MatchState st, unsigned jj, unsigned v) {
  return group_pass(*in, st, jj, v);
}
static __device__ __attribute__((noinline)) bool static_pass_dev(const MatchIn* in, unsigned jj, unsigned v) { return static_pass(*in, jj, v); }
static __device__ __attribute__((noinline)) unsigned xres_fail_dev(const MatchIn* in, MatchState st, unsigned jj, unsigned v) {
  return xres_fail_bits(*in, st, jj, v);
}

// ---- eval ------------------------------------------------------------------------------------------------------------------
struct EvalWaveLds {  // what ONE wave stages for the offers it walks (MV_OCW at a time): the offer loop then reads LDS broadcasts only
  OfferA oa[MV_OCW];
  OfferB ob[MV_OCW];
  double oac[MV_OCW], oam[MV_OCW];
  int oacount[MV_OCW];
  uint32_t attr[MV_OCW][MV_NA];  // the first MV_NA attribute values of the offers (0 = absent)
};
// One workgroup's LDS: the offers its waves stage while they scan, and — in the SAME bytes, behind a workgroup barrier — the waves'
// lists for the tile's epilogue (as two regions a block took 46.6 KB: three blocks per CU whatever the register count).
template <bool GE>
struct EvalLds {
  union {
    EvalWaveLds wave[MV_EW];
    struct {
      double fit[MV_EW][COOK_WAVE][MV_L];
      int idx[MV_EW][COOK_WAVE][MV_L];
      unsigned long long ge[MV_EW][COOK_WAVE];  // (GE) the waves' good-enough bits
      unsigned cnt[MV_EW][COOK_WAVE][3];
    };
  };
};

// the job of one lane and its running results over the offers seen so far
struct EvalLane {
  bool valid, slow, grouped, fastc, use_ge;
  JobRec j;
  unsigned jj;
  unsigned k;  // the job's index in match order (vb.jr / vb.jcons)
  unsigned fh[MV_FH];
  int n_fh;
  int glast;  // the group's last placed job under the snapshot (-1 none; members of a group only)
  double ge, ge_lo;
  double tf[MV_L];
  int ti[MV_L];
  unsigned long long gm[MV_EW];  // (GE launches only) good-enough bits of the batches this lane's wave walked (one batch in a shared tile)
  double thr;  // pruning threshold: (1 - 2^-40) * current L-th best, valid once the list is full
  unsigned c1, c2, c4;
};

// lane = job `b` of the window (64 consecutive jobs per wave): load it and gather what its constraints need
// The job's fast constraints (JobCons) in the form the offer loop checks without a per-lane LDS look-up: per attribute key staged in LDS
// the required value and an all-ones mask when the key is constrained (the offer's values are wave-uniform), the required HOSTNAME
// value, the hosts to avoid (0xFFFFFFFF = unused), and "cannot be satisfied by any offer".  Lives only inside the constraint pass of
// eval_scan_offers (22 registers that the fitness pass does not carry).
struct EvalCons {
  unsigned req[MV_NA], wild[MV_NA];
  unsigned req_host, wild_host;
  unsigned novel[MV_NC];
  bool impossible;
};
static __device__ __forceinline__ void eval_cons_setup(EvalCons& E, bool fastc, const V2Buf& vb, unsigned k) {
#pragma unroll
  for (int q = 0; q < MV_NA; ++q) E.req[q] = E.wild[q] = 0u;
  E.req_host = E.wild_host = 0u;
#pragma unroll
  for (int q = 0; q < MV_NC; ++q) E.novel[q] = 0xFFFFFFFFu;
  E.impossible = false;
  if (fastc) {
    const JobCons jc = vb.jcons[k];
#pragma unroll
    for (int q = 0; q < MV_NC; ++q) {
      if ((unsigned)q < jc.n_novel) E.novel[q] = jc.novel[q];
      if ((unsigned)q < jc.n_eq) {
        const unsigned key = jc.eq_key[q], val = jc.eq_val[q];
        if (key == 0xFFFFFFFFu) {  // "HOSTNAME" (value = host id + 1)
          if (E.wild_host && E.req_host != val) E.impossible = true;
          E.req_host = val;
          E.wild_host = 0xFFFFFFFFu;
        } else if (key >= (unsigned)MV_NA) {  // beyond the offers' attribute table: every offer reads as absent (0)
          if (val != 0u) E.impossible = true;
        } else {
#pragma unroll
          for (int a = 0; a < MV_NA; ++a)
            if ((unsigned)a == key) {
              if (E.wild[a] && E.req[a] != val) E.impossible = true;
              E.req[a] = val;
              E.wild[a] = 0xFFFFFFFFu;
            }
        }
      }
    }
  }
}

// GE = false: the launch was made for good-enough-fitness 1.0 (plain best fit, the parity setting): the good-enough list, its
// threshold and counters are compiled out of the offer loop (10 vector registers)
template <bool GE = true>
static __device__ __forceinline__ void eval_lane_setup(EvalLane& E, const MatchIn& in, const MatchState& st, const V2Buf& vb, unsigned head,
                                                       unsigned wcur, unsigned jg) {
  const unsigned lane = lane_id();
  const unsigned b = jg * COOK_WAVE + lane, k = head + b;
  E.valid = b < wcur && k < in.K;
  E.j.c = E.j.m = E.j.g = 0.0;
  E.j.gpu_model = 0;
  E.j.reserved_host = -1;
  E.j.group = 0xFFFFFFFFu;
  E.j.flags = 0;
  E.jj = 0;
  E.k = k;
  if (E.valid) {
    E.j = vb.jr[k];
    E.jj = in.j_index ? in.j_index[k] : k;
  }
  E.slow = (E.j.flags & JF_SLOW) != 0;
  E.grouped = (E.j.flags & JF_GROUPED) != 0;
  E.fastc = !E.slow && (E.j.flags & JF_FASTC) != 0;
  // unique host-placement groups (constraints.clj:586-598): the hosts to avoid = running cotasks ++ cotasks placed by
  // earlier rounds of this call, gathered ONCE per tile into registers (n_fh = -1: not such a job, -2: too many -> slow path)
  E.n_fh = -1;
  E.glast = -1;
#pragma unroll
  for (int q = 0; q < MV_FH; ++q) E.fh[q] = 0xFFFFFFFFu;
  if (E.valid && E.j.group != 0xFFFFFFFFu) E.glast = ld_agent(&st.group_last[E.j.group]);
  if (E.grouped && ((E.j.flags >> 8) & 3u) == 1u) {
    E.n_fh = 0;
    const unsigned g = E.j.group;
    const unsigned r0 = in.g_run_off ? in.g_run_off[g] : 0u, r1 = in.g_run_off ? in.g_run_off[g + 1] : 0u;
    auto push = [&](unsigned h) {
      if (E.n_fh >= 0 && E.n_fh < MV_FH) {
#pragma unroll
        for (int q = 0; q < MV_FH; ++q)
          if (q == E.n_fh) E.fh[q] = h;
        ++E.n_fh;
      } else {
        E.n_fh = -2;
      }
    };
    for (unsigned x = r0; x < r1 && E.n_fh >= 0; ++x) push(in.g_run_host[x]);
    for (int c = E.glast; c >= 0 && E.n_fh >= 0; c = ld_agent(&st.job_prev[c]))
      if (c < st.cutoff) push(in.o_host[ld_agent(&st.job_to_offer[c])]);
  }
  E.use_ge = GE && in.good_enough < 1.0;
  E.ge = in.good_enough;
  E.ge_lo = in.good_enough * (1.0 - 0x1p-40);
#pragma unroll
  for (int q = 0; q < MV_L; ++q) {
    E.tf[q] = -1.0;
    E.ti[q] = -1;
  }
#pragma unroll
  for (int q = 0; q < MV_EW; ++q) E.gm[q] = 0ull;
  E.thr = -1.0;
  E.c1 = E.c2 = E.c4 = 0;
}

// When a window has fewer job groups than the eval grid has rows (the filling phase resolves ~100 jobs per round: 2 of 8 rows), the
// idle rows take a share of the OFFERS instead: with A active job groups, row gy serves job group gy % A and part gy / A of the
// R = eval_split(wcur) parts every wave's offer batch is cut into, and a chunk contributes R partial lists per job ("virtual
// chunks" ch * R + part; the merge kernel derives the same R from the same window).  R = 1 is the plain layout.
constexpr int MV_SPLIT_MAX = 4;  // a wave keeps at least MV_OCW / 4 offers; V2Buf::split_max (host) caps it: sharing a GPU with other pools'
                                 // launches, the extra blocks and the R-fold chunk lists cost more than the shorter tiles save
static __device__ __forceinline__ unsigned eval_split(unsigned wcur, unsigned split_max) {
  const unsigned active = (wcur + COOK_WAVE - 1) / COOK_WAVE;
  unsigned r = 1;
  while (r * 2u <= split_max && r * 2u * active <= (unsigned)MV_JG && (unsigned)MV_OCW / (r * 2u) >= 8u) r *= 2u;
  return r;
}

// the offers [v0, v0 + nsub) against the wave's 64 jobs (nsub = MV_OCW, or a power-of-two share of it): stage them in the wave's LDS,
// then walk them in a wave-uniform loop
template <bool THROUGH, bool GE = true>
static __device__ __forceinline__ void eval_scan_offers(EvalLane& E, EvalWaveLds& W, const MatchIn& in, const MatchState& st, const V2Buf& vb,
                                                        unsigned v0, unsigned jg, unsigned nsub = MV_OCW, unsigned slot = 0,  // slot: E.gm word of this batch
                                                        unsigned long long* trp = nullptr) {  // (COOK_EVAL_TRACE builds: where the wave's time stamps go)
  (void)trp;
  const unsigned lane = lane_id();
  const unsigned v1 = (v0 + nsub < in.M) ? v0 + nsub : in.M;
  if (v0 + lane < v1) {
    W.oa[lane] = vb.oa[v0 + lane];
    W.ob[lane] = vb.ob[v0 + lane];
    W.oac[lane] = st.ac[v0 + lane];
    W.oam[lane] = st.am[v0 + lane];
    W.oacount[lane] = st.acount[v0 + lane];
#pragma unroll
    for (int q = 0; q < MV_NA; ++q)
      W.attr[lane][q] = (in.o_attr && (unsigned)q < in.n_attr) ? in.o_attr[(size_t)(v0 + lane) * in.n_attr + q] : 0u;
  }
  wave_sync();
#ifdef COOK_EVAL_TRACE
  if (trp && lane == 0) trp[2] = cook_ticks();
#endif
  const bool valid = E.valid;
  const JobRec& j = E.j;
  // offers that cannot take even the smallest job of the call any more fail every job on resources: count, never evaluate
  unsigned long long live = 0ull;
  if (v0 < v1) {
    live = (st.alive[v0 >> 6] >> (v0 & 63u)) & (nsub == 64u ? ~0ull : ((1ull << (nsub & 63u)) - 1ull));  // an aligned slice of one word
    if (v1 - v0 < nsub) live &= (1ull << (v1 - v0)) - 1ull;
  }
  // Two passes over the live offers, so that neither carries the other's registers (one loop held 197 VGPRs = two waves per SIMD
  // while 57 % of its wave cycles were waits): the CONSTRAINT pass — resources under the snapshot, the static checks, the colbits
  // ballot — leaves a bit per offer in two lane masks; the FITNESS pass reads the masks and never sees the constraint form.
  unsigned long long resm = 0ull, statm = 0ull;  // bit vi: the lane's job fits offer v0 + vi on resources / also passes the static checks
  {
    EvalCons Cn;
    eval_cons_setup(Cn, E.fastc, vb, E.k);
    for (unsigned long long m = live; m != 0ull;) {  // wave-uniform
      const unsigned vi = (unsigned)__ffsll((unsigned long long)m) - 1u;
      m &= m - 1ull;
      const unsigned v = v0 + vi;
      // every LDS read of this offer is issued here, in one batch
      const double oc = W.oa[vi].oc, om = W.oa[vi].om;
      const double ac = W.oac[vi], am = W.oam[vi];
      const OfferB o = W.ob[vi];
      unsigned arow[MV_NA];
#pragma unroll
      for (int x = 0; x < MV_NA; ++x) arow[x] = W.attr[vi][x];
      bool res = valid && !(ac + j.c > oc || am + j.m > om);
      if (in.has_x) {  // ports / named scalars (rare): the jobs that ask for any read the offer's counters
        if (res && (j.flags & JF_XRES)) res = xres_fail_dev(vb.in_dev, st, E.jj, v) == 0u;
      }
      if (!__any(res)) {
        if (lane == 0) {
          if (THROUGH) st_agent(&vb.colbits[(size_t)v * MV_JGL + jg], (uint64_t)0ull);
          else vb.colbits[(size_t)v * MV_JGL + jg] = 0ull;
        }
        continue;
      }
      bool stat = res && static_fast(j, o, in, v);
      {  // novel-host (constraints.clj:68-94) and user-defined EQUALS (:356-377): the offer's host and attribute values are wave-uniform
        unsigned diff = (Cn.req_host ^ (o.host + 1u)) & Cn.wild_host;
#pragma unroll
        for (int x = 0; x < MV_NA; ++x) diff |= (Cn.req[x] ^ arow[x]) & Cn.wild[x];
        bool hit = Cn.impossible;
#pragma unroll
        for (int q = 0; q < MV_NC; ++q) hit = hit | (Cn.novel[q] == o.host);
        stat = stat && diff == 0u && !hit;
      }
      if (stat && E.slow) stat = static_pass_dev(vb.in_dev, E.jj, v);
      const unsigned long long bits = __ballot(stat);
      if (lane == 0) {
        if (THROUGH) st_agent(&vb.colbits[(size_t)v * MV_JGL + jg], (uint64_t)bits);
        else vb.colbits[(size_t)v * MV_JGL + jg] = bits;
      }
      resm |= res ? 1ull << vi : 0ull;
      statm |= stat ? 1ull << vi : 0ull;
    }
  }
#ifdef COOK_EVAL_TRACE
  if (trp && lane == 0) trp[3] = cook_ticks();
#endif
  unsigned long long feasm = 0ull, gem = 0ull;  // gem: bit vi = the fitness on offer v0 + vi exceeds good-enough
  const unsigned fm = wave_uniform_u32(in.fitness);
  for (unsigned long long m = live; m != 0ull;) {  // wave-uniform
    const unsigned vi = (unsigned)__ffsll((unsigned long long)m) - 1u;
    m &= m - 1ull;
    const bool stat = ((statm >> vi) & 1ull) != 0ull;
    if (!__any(stat)) continue;
    const unsigned v = v0 + vi;
    const OfferA a = W.oa[vi];
    const double ac = W.oac[vi], am = W.oam[vi];
    const OfferB o = W.ob[vi];
    const int acount = W.oacount[vi];
    bool feas = stat && dyn_fast(j, o, acount);
    {  // unique host-placement groups: the hosts to avoid sit in registers (0xFFFFFFFF for everybody else)
      bool taken = false;
#pragma unroll
      for (int q = 0; q < MV_FH; ++q) taken = taken | (E.fh[q] == o.host);
      feas = feas && !taken;
    }
    if (__any(E.grouped && E.n_fh < 0)) {  // (wave-uniform) balanced / attribute-equals groups, or too many hosts: the general walk
      if (feas && E.grouped && E.n_fh < 0) feas = group_pass_dev(vb.in_dev, st, E.jj, v);
    }
    feasm |= feas ? 1ull << vi : 0ull;
    if (feas) {
      double t1 = (a.rc + ac + j.c) * a.inv_dc, t2 = (a.rm + am + j.m) * a.inv_dm;
      fitness_terms(fm, t1, t2);  // (a one-resource packer: ub is that resource's term; the bound's derivation is at fitness_terms)
      const double ub = (t1 + t2) * 0.5;
      bool prune = E.ti[MV_L - 1] >= 0 && t1 >= 0.0 && t2 >= 0.0 && ub < E.thr;
      if (GE && E.use_ge && !(ub < E.ge_lo)) prune = false;  // (it may clear the threshold: the exact value decides)
      if (!prune) {
        const double fit = fitness_of(fm, a, ac, am, j.c, j.m);
        if (!(fit > 0.0)) {
          E.c4 += 1u;
        } else {
          if (fit > E.tf[MV_L - 1]) {
            topl_insert_ascending<MV_L>(E.tf, E.ti, fit, (int)v);
            if (E.ti[MV_L - 1] >= 0) E.thr = E.tf[MV_L - 1] * (1.0 - 0x1p-40);
          }
          if (GE && E.use_ge && fit > E.ge) gem |= 1ull << vi;
        }
      }
    }
  }
  // failure classes: offers failing on resources (the dead ones too), offers fitting on resources but infeasible (a constraint)
  const unsigned n_res = (unsigned)__popcll(resm);
  E.c1 += valid ? (v1 > v0 ? v1 - v0 : 0u) - n_res : 0u;
  E.c2 += n_res - (unsigned)__popcll(feasm);
  if (GE) {
#pragma unroll
    for (int q = 0; q < MV_EW; ++q)
      if ((unsigned)q == slot) E.gm[q] = gem;
  }
  wave_sync();  // every lane is done with the staged offers before the wave stages the next ones
}

// the group data of the lane's job for the walk (the tile of chunk 0 writes it, once per round)
template <bool THROUGH>
static __device__ __forceinline__ void eval_store_group(const EvalLane& E, const V2Buf& vb, unsigned b) {
  if (E.j.group == 0xFFFFFFFFu) return;
  unsigned* row = vb.jfh + (size_t)b * (MV_FH + 2);
#pragma unroll
  for (int q = 0; q < MV_FH; ++q) {
    if (THROUGH) st_agent(&row[q], E.fh[q]);
    else row[q] = E.fh[q];
  }
  if (THROUGH) {
    st_agent(&row[MV_FH], (unsigned)E.n_fh);
    st_agent(&row[MV_FH + 1], (unsigned)E.glast);
  } else {
    row[MV_FH] = (unsigned)E.n_fh;
    row[MV_FH + 1] = (unsigned)E.glast;
  }
}

// One tile = 64 jobs (job group jg of the window) x MV_OCB offers (chunk ch); the whole workgroup (MV_EW waves) takes part.
// Ends with every thread past its last LDS access only after the caller's next __syncthreads().
// The MV_EW waves may be a whole workgroup (w = wave_id(), sync = __syncthreads) or a TEAM of waves inside a larger workgroup of
// a larger workgroup (w = wave in team, sync = the team's barrier; THROUGH = write-through stores: no shipped launch uses either).
template <bool THROUGH, bool GE = true, class Sync>
static __device__ __forceinline__ void eval_tile_t(char* lds, const MatchIn& in, const MatchState& st, const V2Buf& vb, unsigned head,
                                                   unsigned wcur, unsigned ch, unsigned jg, unsigned w, Sync sync, unsigned part = 0,
                                                   unsigned split = 1) {
  EvalLds<GE>& L = *reinterpret_cast<EvalLds<GE>*>(lds);
  auto& s_fit = L.fit;
  auto& s_idx = L.idx;
  auto& s_ge = L.ge;
  auto& s_cnt = L.cnt;
  if (jg * COOK_WAVE >= wcur || head + jg * COOK_WAVE >= in.K) return;  // uniform over the waves of the tile
  const unsigned lane = lane_id();
  const unsigned b = jg * COOK_WAVE + lane;
  EvalLane E;
#ifdef COOK_EVAL_TRACE
  unsigned long long* trp = vb.eval_trace ? vb.eval_trace + (size_t)vb.C * MV_JG * 3 + ((size_t)jg * vb.C + ch) * 32 + w * 8 : nullptr;
  if (trp && lane == 0) trp[0] = cook_ticks();
#endif
  eval_lane_setup<GE>(E, in, st, vb, head, wcur, jg);
#ifdef COOK_EVAL_TRACE
  if (trp && lane == 0) trp[1] = cook_ticks();
#endif
#ifdef COOK_EVAL_TRACE
  eval_scan_offers<THROUGH, GE>(E, L.wave[w], in, st, vb, ch * MV_OCB + w * MV_OCW + part * ((unsigned)MV_OCW / split), jg, (unsigned)MV_OCW / split, 0, trp);
  if (trp && lane == 0) trp[4] = cook_ticks();
#else
  eval_scan_offers<THROUGH, GE>(E, L.wave[w], in, st, vb, ch * MV_OCB + w * MV_OCW + part * ((unsigned)MV_OCW / split), jg, (unsigned)MV_OCW / split);
#endif
  const bool valid = E.valid, use_ge = GE && E.use_ge;
  // ---- merge the block's MV_EW wave lists per job through LDS -------------------------------------------------------
  sync();  // (the lists go where the waves' staged offers were: every wave of the tile is done scanning)
#pragma unroll
  for (int q = 0; q < MV_L; ++q) {
    s_fit[w][lane][q] = E.tf[q];
    s_idx[w][lane][q] = E.ti[q];
  }
  if constexpr (GE) s_ge[w][lane] = E.gm[0];
  s_cnt[w][lane][0] = E.c1;
  s_cnt[w][lane][1] = E.c2;
  s_cnt[w][lane][2] = E.c4;
  sync();
  if (w != 0 || !valid) return;  // (the caller synchronises the waves before the LDS is reused)
  if (ch == 0 && part == 0) eval_store_group<THROUGH>(E, vb, b);
  int p[MV_EW];
#pragma unroll
  for (int x = 0; x < MV_EW; ++x) p[x] = 0;
  ChunkRecT<GE> R;
  int n_out = 0;
#pragma unroll
  for (int q = 0; q < MV_L; ++q) {
    R.fit[q] = -1.0;
    R.idx[q] = -1;
  }
#pragma unroll
  for (int q = 0; q < (GE ? MV_EW : 2); ++q) R.gm[q] = 0ull;
  {
    bool more = true;
#pragma unroll
    for (int q = 0; q < MV_L; ++q) {
      Cand best{-1.0, -1};
      int bx = -1;
      if (more) {
#pragma unroll
        for (int x = 0; x < MV_EW; ++x) {
          if (p[x] < MV_L) {
            const Cand o{s_fit[x][lane][p[x]], s_idx[x][lane][p[x]]};
            if (o.idx >= 0 && cand_better(o, best)) {
              best = o;
              bx = x;
            }
          }
        }
      }
      if (bx < 0) {
        more = false;
      } else {
        R.fit[q] = best.fit;
        R.idx[q] = best.idx;
        ++n_out;
#pragma unroll
        for (int x = 0; x < MV_EW; ++x)
          if (x == bx) ++p[x];
      }
    }
  }
  int n_g = 0;
  if constexpr (GE) {
    if (use_ge) {
#pragma unroll
      for (int x = 0; x < MV_EW; ++x) {
        R.gm[x] = s_ge[x][lane];
        n_g += __popcll(R.gm[x]);
      }
      n_g = n_g < 255 ? n_g : 255;
    }
  }
  unsigned t1 = 0, t2 = 0, t4 = 0;
#pragma unroll
  for (int x = 0; x < MV_EW; ++x) {
    t1 += s_cnt[x][lane][0];
    t2 += s_cnt[x][lane][1];
    t4 += s_cnt[x][lane][2];
  }
  R.cnt[0] = (unsigned)n_out | ((unsigned)n_g << 8);
  R.cnt[1] = t1;
  R.cnt[2] = t2;
  R.cnt[3] = t4;
  chunk_store(&reinterpret_cast<ChunkRecT<GE>*>(vb.prec)[(size_t)b * (vb.C * split) + ch * split + part], R, THROUGH, (n_out | n_g) == 0 ? chunk_count_piece<GE>() : 0u);
#ifdef COOK_EVAL_TRACE
  if (trp && lane == 0) trp[5] = cook_ticks();
#endif
}
template <bool GE = true>
static __device__ __forceinline__ void eval_tile(char* lds, const MatchIn& in, const MatchState& st, const V2Buf& vb, unsigned head,
                                                 unsigned wcur, unsigned ch, unsigned jg, unsigned part = 0, unsigned split = 1) {
  eval_tile_t<false, GE>(lds, in, st, vb, head, wcur, ch, jg, wave_id(), [] { __syncthreads(); }, part, split);
}

// The same tile by ONE wave on its own (the persistent placement kernel's evaluator waves, match_world.hpp): 64 jobs x the
// MV_OCB offers of chunk ch in MV_EW batches of MV_OCW; no workgroup barrier anywhere, the chunk list goes straight to HBM.
template <bool THROUGH, bool GE = true>
static __device__ __forceinline__ void eval_tile_wave(EvalWaveLds& W, const MatchIn& in, const MatchState& st, const V2Buf& vb, unsigned head,
                                                      unsigned wcur, unsigned ch, unsigned jg) {
  if (jg * COOK_WAVE >= wcur || head + jg * COOK_WAVE >= in.K) return;  // wave-uniform
  const unsigned lane = lane_id();
  const unsigned b = jg * COOK_WAVE + lane;
  EvalLane E;
  eval_lane_setup<GE>(E, in, st, vb, head, wcur, jg);
  for (int s = 0; s < MV_EW; ++s) {
    const unsigned v0 = ch * MV_OCB + (unsigned)s * MV_OCW;
    if (v0 >= in.M) break;
    eval_scan_offers<THROUGH, GE>(E, W, in, st, vb, v0, jg, MV_OCW, (unsigned)s);
  }
  if (!E.valid) return;
  if (ch == 0) eval_store_group<THROUGH>(E, vb, b);
  ChunkRecT<GE> R;
  int n_out = 0, n_g = 0;
#pragma unroll
  for (int q = 0; q < MV_L; ++q) {
    R.fit[q] = E.tf[q];
    R.idx[q] = E.ti[q];
    n_out += E.ti[q] >= 0 ? 1 : 0;
  }
#pragma unroll
  for (int q = 0; q < (GE ? MV_EW : 2); ++q) {
    R.gm[q] = GE ? E.gm[q < MV_EW ? q : 0] : 0ull;
    n_g += GE ? __popcll(R.gm[q]) : 0;
  }
  n_g = n_g < 255 ? n_g : 255;
  R.cnt[0] = (unsigned)n_out | ((unsigned)n_g << 8);
  R.cnt[1] = E.c1;
  R.cnt[2] = E.c2;
  R.cnt[3] = E.c4;
  chunk_store(&reinterpret_cast<ChunkRecT<GE>*>(vb.prec)[(size_t)b * vb.C + ch], R, THROUGH, (n_out | n_g) == 0 ? chunk_count_piece<GE>() : 0u);
}

// What one block of the eval grid (offer chunks x MV_JG) does.  A window of the usual size: the block's MV_EW waves share ONE tile
// (job group gy of chunk ch, a batch of offers each).  A LONG window (more job groups than the grid has rows; nearly all its offers
// are dead by then, so a tile is little more than its prologue): every wave takes a job group of its own and walks the whole chunk,
// eval_tile_wave — MV_EW job groups per pass instead of one.
template <bool GE = true>
static __device__ __forceinline__ void eval_block(char* lds, const MatchIn& in, const MatchState& st, const V2Buf& vb, unsigned head,
                                                  unsigned wcur, unsigned ch, unsigned gy, unsigned ny) {
  if (wcur <= ny * COOK_WAVE) {
    const unsigned split = ny == (unsigned)MV_JG ? eval_split(wcur, vb.split_max) : 1u;  // (the grid's rows are MV_JG in every launch path)
    if (split == 1u) {
      eval_tile<GE>(lds, in, st, vb, head, wcur, ch, gy);
    } else {
      const unsigned active = (wcur + COOK_WAVE - 1) / COOK_WAVE;
      if (gy < active * split) eval_tile<GE>(lds, in, st, vb, head, wcur, ch, gy % active, gy / active, split);
    }
    return;
  }
  EvalLds<GE>& L = *reinterpret_cast<EvalLds<GE>*>(lds);
  const unsigned w = wave_id();
  for (unsigned jg = gy * MV_EW + w; jg * COOK_WAVE < wcur; jg += ny * MV_EW) eval_tile_wave<false, GE>(L.wave[w], in, st, vb, head, wcur, ch, jg);
}
template <bool GE>
__global__ void __launch_bounds__(COOK_WAVE* MV_EW) COOK_EVAL_OCCUPANCY match_eval2(MatchIn in, MatchState st, V2Buf vb) {
  __shared__ __attribute__((aligned(16))) char lds[sizeof(EvalLds<GE>)];
#ifdef COOK_EVAL_TRACE
  const unsigned long long t0 = cook_ticks();
#endif
  eval_block<GE>(lds, in, st, vb, vb.ctl->head, vb.ctl->wcur, blockIdx.x, blockIdx.y, gridDim.y);
#ifdef COOK_EVAL_TRACE
  __syncthreads();
  if (vb.eval_trace && threadIdx.x == 0) {
    const unsigned blk = blockIdx.y * gridDim.x + blockIdx.x;
    vb.eval_trace[blk * 3 + 0] = t0;
    vb.eval_trace[blk * 3 + 1] = cook_ticks();
    vb.eval_trace[blk * 3 + 2] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));  // HW_REG_HW_ID
  }
#endif
}
