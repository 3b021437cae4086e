// rebal_resident_kernels.hpp — device side of cook_cycle_rebalance_stage (cookmatch.h): the rebalancer's stage built from
// the pool's resident cycle state.  Included by rebal_resident_host.hpp inside engine.hip's anonymous namespace, behind cycle_update.hpp
// (upd_copy_elem, upd_store_elem).
//
// Index spaces: i = row of the resident task table; o = ordinal among its running rows (= slot [0, R) of the rebalancer);
//               q = position in the standing queue (e->ranked, task rows); ord = pending ordinal (the j_* columns);
//               p = position in the selected list (slot R + p); h = host id; v = row of the staged offers.
// Everything that decides an ORDER is a scan and a cut (no atomics): the running rows keep their row order, the selected jobs their
// queue order.  Atomics only fold order-free integers: a maximum (greatest host id, fullest host, longest cotask list) or a count
// per host.  No floating-point sum is formed here except the gpus of one offer row over its slots, in slot order, by one thread.
#pragma once
#include "common.hpp"
#include "scan.hpp"

constexpr unsigned RR_MAX_COLS = 12;
struct RrCol {
  const void* src;  // resident column; null: zeros
  void* dst;
  unsigned esize;  // 1, 4 or 8
  unsigned pad;
};
struct RrColSet {
  RrCol c[RR_MAX_COLS];
  unsigned n_cols;
};
struct RrCtl {  // what the host reads back (zero beforehand)
  unsigned R, P;              // running rows; selected jobs
  unsigned maxh1;             // greatest host id + 1 over running rows, offers, cotasks (the host adds its own lists)
  unsigned eq_vals, nv_vals;  // values the selected jobs' two CSR columns hold
  unsigned bad;               // bit 0: a group id out of range; bit 1: a user id out of range
  unsigned max_run;           // cotasks of the group that has most
  unsigned max_seg;           // running rows on the fullest host
  unsigned spare_unsafe;      // a spare figure from the offers that can make a sum round
  unsigned pad[7];
};
constexpr unsigned RR_BAD_GROUP = 1u, RR_BAD_USER = 2u;

struct LoadRunningFlag {  // 1 for a running row
  const uint8_t* pending;
  __device__ __forceinline__ SumI operator()(unsigned i) const { return SumI{pending[i] ? 0 : 1}; }
};
// does queue position q count as a pending job of the rebalancer?  (eligible byte by pending ordinal; matched byte by queue position)
static __device__ __forceinline__ bool rr_keeps(const uint32_t* __restrict__ ranked, const uint32_t* __restrict__ pend_ord,
                                                const uint8_t* __restrict__ elig, const uint8_t* __restrict__ matched, unsigned q) {
  if (matched && matched[q]) return false;
  return !elig || elig[pend_ord[ranked[q]]] != 0;
}
struct LoadQueueKeep {
  const uint32_t *ranked, *pend_ord;
  const uint8_t *elig, *matched;
  __device__ __forceinline__ SumI operator()(unsigned q) const { return SumI{rr_keeps(ranked, pend_ord, elig, matched, q) ? 1 : 0}; }
};
struct LoadSelCsrLen {  // length of selected job p's list in a CSR column (0 behind the selected list)
  const uint32_t *off, *sel_ord;
  const RrCtl* ctl;
  __device__ __forceinline__ SumI operator()(unsigned p) const {
    if (p >= ctl->P) return SumI{0};
    const unsigned ord = sel_ord[p];
    return SumI{(int)(off[ord + 1] - off[ord])};
  }
};

// every running row to its slot, all columns at once (in the manner of upd_compact_cols): thread i moves row i when it runs.
// run_row[o] = i is the way back (cook_cycle_rebalance_fetch).  The greatest host id is folded per wave.
__global__ void __launch_bounds__(256) rr_gather_running(RrColSet cs, const uint8_t* __restrict__ pending, const SumI* __restrict__ incl,
                                                         const uint32_t* __restrict__ t_host, unsigned n, uint32_t* __restrict__ host_out,
                                                         uint32_t* __restrict__ run_row, uint8_t* __restrict__ pending_out,
                                                         RrCtl* __restrict__ ctl) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned h1 = 0u;
  if (i < n && !pending[i]) {
    const unsigned o = (unsigned)incl[i].v - 1u;
    for (unsigned k = 0; k < cs.n_cols; ++k) {
      if (cs.c[k].src) upd_copy_elem(cs.c[k].dst, o, cs.c[k].src, i, cs.c[k].esize);
      else upd_store_elem(cs.c[k].dst, o, 0ull, cs.c[k].esize);
    }
    const uint32_t h = t_host[i];
    host_out[o] = h;
    run_row[o] = i;
    pending_out[o] = 0;
    h1 = h + 1u;
  }
  h1 = wave_max_u32(h1);
  if (lane_id() == 0 && h1) atomicMax(&ctl->maxh1, h1);
  if (i == 0) ctl->R = n ? (unsigned)incl[n - 1].v : 0u;
}

// greatest value + 1 of a list of host ids (the offers' hosts, the groups' cotask hosts)
COOK_KERNEL void rr_max_host(const uint32_t* __restrict__ a, unsigned n, RrCtl* __restrict__ ctl) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned h1 = wave_max_u32(i < n ? a[i] + 1u : 0u);
  if (lane_id() == 0 && h1) atomicMax(&ctl->maxh1, h1);
}
// cotasks of the group that has most (sizes the run's cotask scratch)
COOK_KERNEL void rr_max_run(const uint32_t* __restrict__ run_off, unsigned G, RrCtl* __restrict__ ctl) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned m = wave_max_u32(g < G ? run_off[g + 1] - run_off[g] : 0u);
  if (lane_id() == 0 && m) atomicMax(&ctl->max_run, m);
}

// matched[q] = 1 for the queue positions of the jobs the last placement considered, matched and kept (matched zeroed before): the
// predicate of q_mark_removed.  Every thread writes a byte of its own.
COOK_KERNEL void rr_mark_matched(const uint32_t* __restrict__ cons_pos, const int32_t* __restrict__ j2o, unsigned k, unsigned n,
                                 const uint8_t* __restrict__ offer_skipped, uint8_t* __restrict__ matched) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int o = j2o[i];
  const unsigned q = cons_pos ? cons_pos[i] : i;
  if (o >= 0 && !(offer_skipped && offer_skipped[o]) && q < n) matched[q] = 1;
}

// the cut: the first `cap` queue positions that count -> the selected list, in queue order (incl: inclusive scan of LoadQueueKeep)
COOK_KERNEL void rr_select(const uint32_t* __restrict__ ranked, const uint32_t* __restrict__ pend_ord, const uint8_t* __restrict__ elig,
                           const uint8_t* __restrict__ matched, const SumI* __restrict__ incl, unsigned n, unsigned cap,
                           uint32_t* __restrict__ sel_task, uint32_t* __restrict__ sel_ord, RrCtl* __restrict__ ctl) {
  const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  if (q == 0) {
    const unsigned kept = (unsigned)incl[n - 1].v;
    ctl->P = kept < cap ? kept : cap;
  }
  if (!rr_keeps(ranked, pend_ord, elig, matched, q)) return;
  const unsigned p = (unsigned)incl[q].v - 1u;
  if (p >= cap) return;
  const unsigned task = ranked[q];
  sel_task[p] = task;
  sel_ord[p] = pend_ord[task];
}

// the selected jobs: slot R + p of the slot columns, row p of the job columns, its lists in the two CSR columns — one launch
struct RrJobsArgs {
  RrColSet js;  // the job columns, gathered by pending ordinal into row p
  const uint32_t *sel_task, *sel_ord;
  RrCtl* ctl;  // P and R are read, the CSR value counts and the range checks written
  // the task row's part of a slot
  const uint32_t* t_user;
  const int32_t* t_prio;
  const int64_t* t_job;
  // resident job columns the slots read
  const double *j_cpus, *j_mem, *j_gpus;  // j_gpus may be null
  const uint32_t *j_user, *j_group;       // either may be null
  unsigned U, G;
  // slot columns (A space)
  double *s_cpus, *s_mem, *s_gpus;
  uint32_t* s_user;
  int32_t* s_prio;
  int64_t *s_start, *s_task, *s_job;
  uint8_t* s_pending;
  uint32_t* o_user;  // the job table's user column
  // CSR columns: resident offsets / values, scans of the selected lengths, outputs
  const uint32_t *eq_off, *eq_key, *eq_val, *nv_off, *nv_host;
  const SumI *eq_incl, *nv_incl;
  uint32_t *o_eq_off, *o_eq_key, *o_eq_val, *o_nv_off, *o_nv_host;
};
__global__ void __launch_bounds__(256) rr_gather_jobs(RrJobsArgs a, unsigned cap) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned P = a.ctl->P, R = a.ctl->R;
  if (p >= cap || p >= P) return;
  const unsigned task = a.sel_task[p], ord = a.sel_ord[p];
  const size_t s = (size_t)R + p;
  const uint32_t user = a.j_user ? a.j_user[ord] : a.t_user[task];
  a.s_cpus[s] = a.j_cpus[ord];
  a.s_mem[s] = a.j_mem[ord];
  a.s_gpus[s] = a.j_gpus ? a.j_gpus[ord] : 0.0;
  a.s_user[s] = user;
  a.s_prio[s] = a.t_prio[task];
  a.s_start[s] = 0;
  a.s_task[s] = 0;
  a.s_job[s] = a.t_job[task];
  a.s_pending[s] = 1;
  a.o_user[p] = user;
  for (unsigned k = 0; k < a.js.n_cols; ++k) upd_copy_elem(a.js.c[k].dst, p, a.js.c[k].src, ord, a.js.c[k].esize);
  unsigned bad = user >= a.U ? RR_BAD_USER : 0u;
  if (a.j_group && a.G) {
    const uint32_t g = a.j_group[ord];
    if (g != COOK_NONE_U32 && g >= a.G) bad |= RR_BAD_GROUP;
  }
  if (bad) atomicOr(&a.ctl->bad, bad);
  if (a.eq_off) {
    const unsigned src = a.eq_off[ord], len = a.eq_off[ord + 1] - src, end = (unsigned)a.eq_incl[p].v, dst = end - len;
    a.o_eq_off[p] = dst;
    for (unsigned x = 0; x < len; ++x) a.o_eq_key[dst + x] = a.eq_key[src + x], a.o_eq_val[dst + x] = a.eq_val[src + x];
    if (p + 1u == P) a.o_eq_off[P] = end, a.ctl->eq_vals = end;
  }
  if (a.nv_off) {
    const unsigned src = a.nv_off[ord], len = a.nv_off[ord + 1] - src, end = (unsigned)a.nv_incl[p].v, dst = end - len;
    a.o_nv_off[p] = dst;
    for (unsigned x = 0; x < len; ++x) a.o_nv_host[dst + x] = a.nv_host[src + x];
    if (p + 1u == P) a.o_nv_off[P] = end, a.ctl->nv_vals = end;
  }
}

// ---- behind the read-back of H --------------------------------------------------------------------------------------------------------
// running rows per host (cnt zeroed before; integers: exact in any order)
COOK_KERNEL void rr_host_count(const uint32_t* __restrict__ host, unsigned R, unsigned H, unsigned* __restrict__ cnt) {
  const unsigned o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o < R && host[o] < H) atomicAdd(&cnt[host[o]], 1u);
}
COOK_KERNEL void rr_host_fullest(const unsigned* __restrict__ cnt, unsigned H, RrCtl* __restrict__ ctl) {
  const unsigned h = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned m = wave_max_u32(h < H ? cnt[h] : 0u);
  if (lane_id() == 0 && m) atomicMax(&ctl->max_seg, m);
}
// a spare figure that cannot make a sum round (the test of rebal_stage_host_tables)
static __device__ __forceinline__ bool rr_spare_ok(double v) {
  if (!(v >= 0.0 && v < 4194304.0)) return false;
  const double s = v * 1024.0;
  return s == (double)(long long)s;
}
// the dense per-host tables from the staged offer rows (one row per host: the host refuses host_dup): the attribute row of a host,
// its spare resources.  gpus = the row's gpu_count slots added in slot order.
COOK_KERNEL void rr_scatter_offers(const uint32_t* __restrict__ o_host, const double* __restrict__ o_cpus, const double* __restrict__ o_mem,
                                   const double* __restrict__ o_gpu_count, unsigned gpu_slots, unsigned M, unsigned H, unsigned do_row,
                                   unsigned do_spare, int32_t* __restrict__ row_of_host, double* __restrict__ spare_c,
                                   double* __restrict__ spare_m, double* __restrict__ spare_g, uint8_t* __restrict__ has_spare,
                                   RrCtl* __restrict__ ctl) {
  const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= M) return;
  const unsigned h = o_host[v];
  if (h >= H) return;
  if (do_row) row_of_host[h] = (int32_t)v;
  if (!do_spare) return;
  const double c = o_cpus[v], m = o_mem[v];
  double g = 0.0;
  if (o_gpu_count)
    for (unsigned s = 0; s < gpu_slots; ++s) g += o_gpu_count[(size_t)v * gpu_slots + s];
  spare_c[h] = c, spare_m[h] = m, spare_g[h] = g;
  has_spare[h] = 1;
  if (!(rr_spare_ok(c) && rr_spare_ok(m) && rr_spare_ok(g))) ctl->spare_unsafe = 1u;
}

// the preempted slots of a run in the host's space: a running slot -> its row of the resident task table
COOK_KERNEL void rr_translate(const uint32_t* __restrict__ preempted, unsigned n, const uint32_t* __restrict__ run_row, unsigned R,
                              uint32_t* __restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = preempted[i];
  out[i] = s < R ? run_row[s] : COOK_NONE_U32;
}
