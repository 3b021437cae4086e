// match_v2_pack.hpp — the kernels that run once per match call, in front of its rounds: match_pack_offers, match_pack_jobs, match_job_minima,
// match_init_alive.  Part of match_v2.hpp: needs the records of match_v2_shapes.hpp.
#pragma once

// ---- once per match call: pack offers and jobs -----------------------------------------------------------------------
COOK_KERNEL void match_pack_offers(const MatchIn* __restrict__ inp /* device copy of the call's MatchIn */, OfferA* __restrict__ oa,
                                   OfferB* __restrict__ ob, OfferW* __restrict__ ow) {
  const MatchIn& in = *inp;
  const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= in.M) return;
  OfferA a;
  a.oc = in.o_cpus[v];
  a.om = in.o_mem[v];
  a.rc = in.o_run_cpus ? in.o_run_cpus[v] : 0.0;
  a.rm = in.o_run_mem ? in.o_run_mem[v] : 0.0;
  a.inv_dc = 1.0 / (a.oc + a.rc);
  a.inv_dm = 1.0 / (a.om + a.rm);
  oa[v] = a;
  OfferB b;
  b.host = in.o_host[v];
  b.gpu_model = 0u;  // the one entry of the host's "gpus" map (or, bit2, one of several)
  b.gpu_count = 0.0;
  unsigned n_keys = 0;
  for (unsigned q = 0; in.o_gpu_model && q < in.gpu_slots; ++q) {
    const unsigned md = in.o_gpu_model[(size_t)v * in.gpu_slots + q];
    if (md != 0u) {
      if (n_keys == 0) {
        b.gpu_model = md;
        b.gpu_count = in.o_gpu_count ? in.o_gpu_count[(size_t)v * in.gpu_slots + q] : 0.0;
      }
      ++n_keys;
    }
  }
  b.run_count = in.o_run_count ? in.o_run_count[v] : 0;
  b.task_slack = (in.o_max_tasks && in.o_max_tasks[v] >= 0) ? in.o_max_tasks[v] - (in.o_num_tasks ? in.o_num_tasks[v] : 0) : 0x7FFFFFFF;
  const bool k8s = in.o_k8s && in.o_k8s[v];
  const bool rsv = in.reserved_bits && (b.host >> 5) < in.reserved_words && ((in.reserved_bits[b.host >> 5] >> (b.host & 31)) & 1u);
  b.flags = (k8s ? 1u : 0u) | (rsv ? 2u : 0u) | (n_keys > 1u ? 4u : 0u);
  b.pad = 0;
  ob[v] = b;
  OfferW w;
  w.oc = a.oc, w.om = a.om, w.rc = a.rc, w.rm = a.rm, w.inv_dc = a.inv_dc, w.inv_dm = a.inv_dm;
  w.host = b.host, w.k8s = b.flags & 1u, w.run_count = b.run_count, w.task_slack = b.task_slack;
  w.ac = 0.0, w.am = 0.0, w.acount = 0;  // (nothing assigned yet: a match call starts from the offers as staged)
#pragma unroll
  for (int q = 0; q < 11; ++q) w.pad[q] = 0u;
  ow[v] = w;
}

COOK_KERNEL void match_pack_jobs(const MatchIn* __restrict__ inp, JobRec* __restrict__ jr, JobCons* __restrict__ jcons) {
  const MatchIn& in = *inp;
  const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= in.K) return;
  const unsigned jj = in.j_index ? in.j_index[k] : k;
  JobRec j;
  j.c = in.j_cpus[jj];
  j.m = in.j_mem[jj];
  j.g = in.j_gpus ? in.j_gpus[jj] : 0.0;
  j.gpu_model = in.j_gpu_model ? in.j_gpu_model[jj] : 0u;
  j.reserved_host = in.j_reserved_host ? in.j_reserved_host[jj] : -1;
  j.group = in.j_group ? in.j_group[jj] : 0xFFFFFFFFu;
  unsigned f = 0;
  JobCons jc;
  jc.n_eq = jc.n_novel = 0;
#pragma unroll
  for (int q = 0; q < MV_NC; ++q) jc.eq_key[q] = jc.eq_val[q] = jc.novel[q] = 0u;
  const unsigned n0 = in.j_novel_off ? in.j_novel_off[jj] : 0u, n1 = in.j_novel_off ? in.j_novel_off[jj + 1] : 0u;
  const unsigned e0 = in.j_eq_off ? in.j_eq_off[jj] : 0u, e1 = in.j_eq_off ? in.j_eq_off[jj + 1] : 0u;
  bool fits = (n1 - n0) <= (unsigned)MV_NC && (e1 - e0) <= (unsigned)MV_NC;
  for (unsigned x = e0; x < e1 && fits; ++x) {
    const unsigned key = in.j_eq_key[x];
    if (key != 0xFFFFFFFFu && key >= (unsigned)MV_NA && key < in.n_attr) fits = false;  // beyond the keys staged in LDS
  }
  if (fits) {
    for (unsigned x = n0; x < n1; ++x) {
#pragma unroll
      for (int q = 0; q < MV_NC; ++q)
        if ((unsigned)q == x - n0) jc.novel[q] = in.j_novel_host[x];
    }
    for (unsigned x = e0; x < e1; ++x) {
#pragma unroll
      for (int q = 0; q < MV_NC; ++q)
        if ((unsigned)q == x - e0) {
          jc.eq_key[q] = in.j_eq_key[x];
          jc.eq_val[q] = in.j_eq_val[x];
        }
    }
    jc.n_novel = n1 - n0;
    jc.n_eq = e1 - e0;
    if (jc.n_novel || jc.n_eq) f |= JF_FASTC;
  } else {
    f |= JF_SLOW;
  }
  if (in.j_disk_req && in.j_disk_req[jj] >= 0) f |= JF_SLOW;
  if (in.j_est_end && in.j_est_end[jj] != 0) f |= JF_SLOW;
  if (in.j_ckpt && in.j_ckpt[jj] != 0) f |= JF_SLOW;
  if (in.has_x && job_has_xres(in, jj)) f |= JF_XRES;
  if (j.group != 0xFFFFFFFFu) {
    const unsigned t = in.g_type[j.group];
    if (t != 0) f |= JF_GROUPED | (t << 8);
  }
  j.flags = f;
  jr[k] = j;
  jcons[k] = jc;
}

// minimum cpus / mem over the jobs of the call (positive doubles order like their bit patterns; jmin starts at +inf)
COOK_KERNEL void match_job_minima(const JobRec* __restrict__ jr, unsigned K, unsigned long long* __restrict__ jmin_bits, unsigned nblk /* blocks of this launch */) {
  double c = __longlong_as_double(0x7FF0000000000000ll), m = c;
  bool odd = false;  // a negative or non-finite request (jmin_bits[2]: match_v3 leaves such calls to the window rounds)
  for (unsigned k = blockIdx.x * blockDim.x + threadIdx.x; k < K; k += nblk * blockDim.x) {
    const JobRec j = jr[k];
    c = j.c < c ? j.c : c;
    m = j.m < m ? j.m : m;
    odd = odd || !(j.c >= 0.0 && j.m >= 0.0 && j.c < 1e300 && j.m < 1e300);
  }
  if (__any(odd) && lane_id() == 0) atomicOr(&jmin_bits[2], 1ull);
  // negative or NaN resources would break the ordering trick: such inputs switch the dead-offer shortcut off (minimum 0)
  if (!(c >= 0.0)) c = 0.0;
  if (!(m >= 0.0)) m = 0.0;
  for (int d = 32; d >= 1; d >>= 1) {
    const double oc = __shfl_xor(c, d, COOK_WAVE), om = __shfl_xor(m, d, COOK_WAVE);
    c = oc < c ? oc : c;
    m = om < m ? om : m;
  }
  if (lane_id() == 0) {
    atomicMin(&jmin_bits[0], (unsigned long long)__double_as_longlong(c));
    atomicMin(&jmin_bits[1], (unsigned long long)__double_as_longlong(m));
  }
}
// alive bits at the start of a call (nothing assigned yet)
COOK_KERNEL void match_init_alive(const OfferA* __restrict__ oa, unsigned M, const double* __restrict__ jmin,
                                                        unsigned long long* __restrict__ alive) {
  const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
  bool a = false;
  if (v < M) {
    const OfferA o = oa[v];
    a = !(0.0 + jmin[0] > o.oc || 0.0 + jmin[1] > o.om);
  }
  const unsigned long long bits = __ballot(a);
  if (lane_id() == 0 && (v >> 6) < (M + 63u) / 64u) alive[v >> 6] = bits;
}
