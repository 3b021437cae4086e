// match_v2_merge.hpp — the merge of a window's chunk lists into every job's candidate lists: match_merge2.  Part of match_v2.hpp: needs
// match_v2_shapes.hpp (ChunkRecT, V2Buf, the list shapes); reads what match_v2_eval.hpp's kernel wrote.
#pragma once

// ---- merge: one wave per job ---------------------------------------------------------------------------------------------
// lane = offer chunk (its per-chunk list as it is; further chunks of the same lane by the ascending insertion).  The merged best-fit
// list is cut — and marked truncated — the moment a lane whose chunk list(s) may continue beyond what it holds pops its last entry.
// The good-enough list is the first LG set bits of the chunks' masks in offer order (a prefix sum of the chunks' bit counts gives
// every lane the list positions of its offers): exact to its last entry, truncated only when more than LG offers clear the threshold.
template <bool GE>
static __device__ __forceinline__ void merge_job(const MatchIn& in, const V2Buf& vb, unsigned head, unsigned wcur, unsigned b,
                                                 unsigned split = 1) {  // split: eval_split(wcur) behind the launch path's eval grid
  if (b >= wcur || head + b >= in.K) return;
  constexpr int LM = VShape<GE>::LM, LG = VShape<GE>::LG;
  const unsigned lane = lane_id();
  const bool use_ge = GE && in.good_enough < 1.0;
  double tf[MV_L];
  int ti[MV_L];
#pragma unroll
  for (int q = 0; q < MV_L; ++q) {
    tf[q] = -1.0;
    ti[q] = -1;
  }
  unsigned n_g_total = 0;  // (GE) offers above the threshold seen so far, over all chunks (wave-uniform)
  unsigned c1 = 0, c2 = 0, c4 = 0;
  int n_seen = 0;     // entries of all the lane's chunks
  bool hide = false;  // the lane's best-fit list may end before its chunks' feasible offers do
  const unsigned cv = vb.C * split;  // chunk lists per job (virtual chunks, eval_split)
  const ChunkRecT<GE>* const prec = reinterpret_cast<const ChunkRecT<GE>*>(vb.prec);
  for (unsigned ch0 = 0; ch0 < cv; ch0 += COOK_WAVE) {  // (wave-uniform: the good-enough part scans over the lanes)
    const unsigned ch = ch0 + lane;
    const bool have = ch < cv;
    ChunkRecT<GE> R;
    if (have) R = prec[(size_t)b * cv + ch];  // 16-byte loads, all in flight together
    const unsigned info = have ? R.cnt[0] : 0u;
    if (have) {
      c1 += R.cnt[1];
      c2 += R.cnt[2];
      c4 += R.cnt[3];
    }
    const int n = (int)(info & 0xFFu);
    n_seen += n;
    hide = hide || n == MV_L || n_seen > MV_L;
    if (ch0 == 0u) {  // the lane's first chunk (its only one up to 64 chunks = 8 192 offers): the sorted list as it is
#pragma unroll
      for (int q = 0; q < MV_L; ++q)
        if (q < n) tf[q] = R.fit[q], ti[q] = R.idx[q];
    } else {  // a later (virtual) chunk holds higher offer indices than everything the lane has seen: an entry only passes entries it
              // beats strictly, and equal-fitness entries of its own list arrive in index order
#pragma unroll
      for (int q = 0; q < MV_L; ++q) {
        if (q >= n) break;
        if (!(R.fit[q] > tf[MV_L - 1])) break;  // chunk list is sorted: nothing further can enter
        topl_insert_ascending<MV_L>(tf, ti, R.fit[q], R.idx[q]);
      }
    }
    if constexpr (GE) {
      if (use_ge && n_g_total < (unsigned)LG) {  // (wave-uniform) chunks ascend with the lane, offers with the word and the bit
        const bool any_bits = have && ((info >> 8) & 0xFFu) != 0u;
        unsigned cnt = 0;
#pragma unroll
        for (int x = 0; x < MV_EW; ++x) cnt += any_bits ? (unsigned)__popcll(R.gm[x]) : 0u;
        unsigned incl = cnt;  // inclusive prefix sum over the lanes
        for (unsigned d = 1; d < (unsigned)COOK_WAVE; d <<= 1) {
          const unsigned o = (unsigned)__shfl_up((int)incl, d, COOK_WAVE);
          if (lane >= d) incl += o;
        }
        unsigned pos = n_g_total + incl - cnt;  // list position of this lane's first offer
        if (cnt != 0u && pos < (unsigned)LG) {
#pragma unroll
          for (int x = 0; x < MV_EW; ++x) {
            for (unsigned long long m = R.gm[x]; m != 0ull && pos < (unsigned)LG; m &= m - 1ull, ++pos)
              vb.ge_idx[(size_t)b * LG + pos] = (int)(ch * (unsigned)MV_OCB + (unsigned)x * (unsigned)MV_OCW + (unsigned)__ffsll((unsigned long long)m) - 1u);
          }
        }
        n_g_total += (unsigned)__shfl((int)incl, COOK_WAVE - 1, COOK_WAVE);
      }
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    c1 += __shfl_xor(c1, d, COOK_WAVE);
    c2 += __shfl_xor(c2, d, COOK_WAVE);
    c4 += __shfl_xor(c4, d, COOK_WAVE);
  }
  int n_out = 0;
  bool trunc = false;  // the merged list may not hold every feasible offer
  for (int round = 0; round < LM; ++round) {
    // the best head over the lanes: greatest fitness (positive doubles order like their bit patterns), lowest offer index among
    // equal ones — two DPP reductions instead of six rounds of three ds_bpermute shuffles
    const unsigned long long key = ti[0] >= 0 ? (unsigned long long)__double_as_longlong(tf[0]) : 0ull;
    const unsigned long long mk = wave_max_u64(key);
    if (mk == 0ull) break;  // wave-uniform
    const unsigned long long tie = __ballot(key == mk);
    Cand best{__longlong_as_double((long long)mk), 0};
    if ((tie & (tie - 1ull)) == 0ull)
      best.idx = wave_read_lane(ti[0], __ffsll((unsigned long long)tie) - 1);
    else
      best.idx = (int)(0x7FFFFFFFu - wave_max_u32(key == mk ? 0x7FFFFFFFu - (unsigned)ti[0] : 0u));
    if (lane == 0) {
      vb.cand_fit[(size_t)b * LM + round] = best.fit;
      vb.cand_idx[(size_t)b * LM + round] = best.idx;
    }
    ++n_out;
    bool emptied = false;
    if (ti[0] == best.idx) {  // the owner pops its head
#pragma unroll
      for (int q = 0; q < MV_L - 1; ++q) {
        tf[q] = tf[q + 1];
        ti[q] = ti[q + 1];
      }
      tf[MV_L - 1] = -1.0;
      ti[MV_L - 1] = -1;
      emptied = ti[0] < 0 && hide;
    }
    if (__any(emptied)) {  // a list that may continue beyond what the lane holds just ran out: stop here
      trunc = true;
      break;
    }
  }
  if (!trunc) trunc = __any(ti[0] >= 0);  // LM entries emitted and some lane still holds more
  const unsigned n_g = GE ? (n_g_total < (unsigned)LG ? n_g_total : (unsigned)LG) : 0u;
  // (the chunks' bit counts saturate at 255 only in the record's count byte, never in the masks; once LG offers are listed the scan
  //  above stops, so "more than LG" is all n_g_total can say beyond that point)
  const bool gtrunc = GE && n_g_total >= (unsigned)LG && LG > 0;
  if (lane == 0) {
    vb.cinfo[(size_t)b * 4 + 0] = (unsigned)n_out | (n_g << 8) | (trunc ? 1u << 16 : 0u) | (gtrunc ? 1u << 17 : 0u);
    vb.cinfo[(size_t)b * 4 + 1] = c1;
    vb.cinfo[(size_t)b * 4 + 2] = c2;
    vb.cinfo[(size_t)b * 4 + 3] = c4;
  }
}

// one wave per job; a block of MV_MW waves takes MV_MW jobs per pass
constexpr int MV_MW = 4;
constexpr int MV_MERGE_BLOCKS = COOK_SHAPE(240, 16);  // blocks of the merge grid (x MV_MW waves: one pass for the windows of the tile path)
template <bool GE>
static __device__ __forceinline__ void merge_block(const MatchIn& in, const V2Buf& vb) {
  const unsigned head = vb.ctl->head, wcur = vb.ctl->wcur;
  const unsigned split = wcur <= (unsigned)MV_WEVAL ? eval_split(wcur, vb.split_max) : 1u;  // as match_eval2's grid cut the offers
  for (unsigned b = blockIdx.x * MV_MW + wave_id(); b < wcur; b += gridDim.x * MV_MW) merge_job<GE>(in, vb, head, wcur, b, split);
}
template <bool GE>
__global__ void __launch_bounds__(COOK_WAVE* MV_MW) match_merge2(MatchIn in, V2Buf vb) {
  merge_block<GE>(in, vb);
}
