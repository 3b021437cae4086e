// engine.hip — libcookmatch.so: the one translation unit.  It holds the includes in their one valid order, struct cook_engine, guarded()
// and the C ABI (include/cookmatch.h); the host orchestration of the HIP kernels is in the *_host.hpp files, by subject ("Source map").
// One engine = one pool = one HIP stream.  Built by hipcc for gfx950 only (cook_amd/build.py).
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <ucontext.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <limits>
#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/cookmatch.h"
#include "common.hpp"
#include "multi.hpp"
#include "considerable_kernels.hpp"
#include "match_kernels.hpp"
#include "match_v2.hpp"
#include "classfit.hpp"
#include "offers_kernels.hpp"
#include "explain_kernels.hpp"
#include "rank_kernels.hpp"
#include "tile_sort.hpp"
#include "rebalance_kernels.hpp"
#include "scan.hpp"
#include "sort.hpp"

#ifndef HIP_KERNEL_NAME
#define HIP_KERNEL_NAME(...) __VA_ARGS__
#endif

namespace {

#include "device_buf.hpp"   // ahead of the engine: its members are DArr
#include "offer_table.hpp"  // ... and an OfferStore

struct KernelStat {
  double ms = 0;
  unsigned launches = 0;
};

struct RebalBufs;  // rebalance_host.hpp
struct ConsBufs;   // considerable_host.hpp
struct OfferBufs;  // offers_host.hpp
struct PodTableBufs;  // podtable_host.hpp
struct ExplainBufs;  // explain_host.hpp
struct UpdateBufs;   // cycle_update.hpp
struct UserStatsBufs;  // user_stats_host.hpp
struct AutoscaleBufs;  // autoscale_host.hpp
struct SweepBufs;      // sweep_host.hpp
struct KubeBufs;       // kube_host.hpp
struct UnschedBufs;    // unscheduled_host.hpp
struct UsageBufs;      // usage_host.hpp
struct QueueBufs;      // queue_host.hpp
struct CarryBufs;      // carry_host.hpp
struct ReleaseBufs;    // release_host.hpp
struct ChurnBufs;      // churn_host.hpp
struct ReserveBufs;    // reserve_host.hpp
struct ResidentRebalBufs;  // rebal_resident_host.hpp
struct LimiterBufs;    // limiter_host.hpp
struct LaunchBufs;     // launch_res_host.hpp

}  // namespace

struct cook_engine {
  cook_params params;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // profiling
  bool profiling = false;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  struct Pending {
    const char* name;
    hipEvent_t a, b;
  };
  std::vector<Pending> ev_pending;
  std::map<std::string, KernelStat> kstats;
  std::vector<std::string> kstat_names;  // stable storage for cook_kernel_timings
  hipEvent_t ev_stage[4] = {nullptr, nullptr, nullptr, nullptr};
  double rank_ms = 0, match_ms = 0;
  // pinned readback scratch
  unsigned long long* h_scratch = nullptr;  // 64 words
  DArr<unsigned long long> d_scratch64;
  DArr<unsigned> d_counters;

  // ---- rank state ----
  bool rank_staged = false, rank_done = false;
  unsigned upd_phase_us[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // ... by phase (cycle_update.hpp)
  uint32_t upd_us = 0, upd_sync_us = 0, upd_allocs = 0;  // the last cook_cycle_update: microseconds in the call, of them in stream synchronisations, device buffers (re)allocated
  bool pool_usage_known = false;  // pool_usage_val is the running usage of the resident task table (it only changes when the table does)
  cook_usage pool_usage_val{0, 0, 0, 0};
  unsigned N = 0, U = 0, n_pending = 0;
  bool has_gpus = false;
  cook_pool_quota quota{};
  DArr<double> t_cpus, t_mem, t_gpus, u_divc, u_divm, u_divg, u_qcount, u_qcpus, u_qmem, u_qgpus;
  DArr<uint32_t> t_user, permA, permB2, s_user, seg_start, seg_end, inexact_user, rank_of_item, gstart, tpos, titem, tsorted,
      tsorted2, qitemA, qitemB, ranked, pend_ord, hist;
  DArr<int32_t> t_prio;
  DArr<int64_t> t_start, t_task, t_job;
  DArr<uint8_t> t_pending, s_pending, head, keep, thead, dhead;
  // the running rows' host ids (cook_tasks.host), kept when a stage passes them: has_t_host = the column exists, t_host_complete = every
  // running row has a value (a cook_cycle_update that adds running rows without host clears it until the next stage with host)
  DArr<uint32_t> t_host;
  bool has_t_host = false, t_host_complete = false;
  DArr<TieCtl> tie_ctl;
  DArr<uint64_t> w0, w1, w2, dkey, nkkey, ckey;
  DArr<SumU4> s_use, pre, quseA, quseB, qpre, pool_usage;
  DArr<SumI> scanI;
  DArr<int> iflag, ones_buf, tied_buf, run_isf, run_nonf, run_posf;
  DArr<SumI> run_scan, run_scan2;
  DArr<uint32_t> run_user, run_orig, run_seg, run_b2c, run_perm;
  DArr<uint64_t> run_dkey;
  DArr<double> uu_out;
  DArr<SumU4> uu_pre;
  DArr<uint32_t> uu_bad;             // users of rank_user_usage whose running-usage prefixes were not all exact
  DArr<SumBound4> pool_usage_bound;  // pool_usage_partial's exactness bounds
  DArr<double> dru, dru_out;
  ScanTmp<SumU4> tmpU4;
  ScanTmp<SumI> tmpI;
  uint32_t* permB = nullptr;  // final per-user order (points into permA or permB2)
  uint32_t* permC = nullptr;  // final global order
  // the last cook_cycle_run_rank_multi led by this engine: pools, launches, of them for several pools, operations issued alone, synchronisations
  unsigned batch_stats[5] = {0, 0, 0, 0, 0};
  unsigned any_batch_stats[5] = {0, 0, 0, 0, 0};  // the same five of the last pool batch of ANY call led by this engine (cook_batch_stats)
  DArr<uint32_t> permC1, permC2;
  unsigned n_ranked = 0;

  // ---- match state ----
  bool match_staged = false;
  unsigned K = 0, M = 0, G = 0, Kjobs = 0;
  OfferStore offers;  // the offer columns a stage uploads (match_stage_offers)
  DArr<double> j_scal[3], m_xscal;
  DArr<int32_t> j_ports, m_xports;
  DArr<double> j_cpus, j_mem, j_gpus, j_disk_req, m_ac, m_am;
  DArr<uint32_t> j_gpu_model, j_group, j_eq_off, j_eq_key, j_eq_val, j_novel_off, j_novel_host, j_ckpt, j_disk_type, j_index,
      g_attr_key, g_run_off, g_run_host, g_run_attr, reserved_bits, m_fail;
  DArr<int32_t> j_reserved_host, g_min, m_acount, m_group_last, m_job_prev, m_j2o;
  DArr<int64_t> j_est_end;
  DArr<uint8_t> g_type;
  DArr<unsigned> m_summary;
  DArr<OfferA> v_oa;
  DArr<OfferB> v_ob;
  DArr<OfferW> v_ow;
  DArr<JobRec> v_jr;
  DArr<JobCons> v_jcons;
  DArr<unsigned long long> m_alive, m_jmin;
  DArr<double> v_cand_fit;
  DArr<char> v_prec;
  DArr<int> v_cand_idx, v_ge_idx;
  DArr<uint32_t> v_cinfo, v_jfh;
  DArr<uint64_t> v_colbits;
  DArr<WinCtl> w_ctl;
  DArr<RoundLog> w_rlog;
  DArr<PoolCtx> w_pctx;      // contexts of a multi-pool match led by this engine
  // Where this pool's match is.  A set-up (cook_cycle_run_rank) waits for cook_cycle_match_multi with what its form needs; placement_drop and
  // placement_complete are the ways out of a set-up and the only writers of NONE and DONE.
  struct Placement {
    enum State { NONE, ROUNDS, WALK, DONE } state = NONE;  // nothing; window rounds set up; class-ordered walk set up; a match has run
    PoolCtx rounds{};  // ROUNDS: the pool's context, ...
    WinCtl c0{};       // ... the control block its rounds start from (after a served match that gave up: where lockstep rounds go on),
    unsigned k = 0;    // ... its jobs, and whether it needs the GE launches (good-enough-fitness < 1)
    bool ge = false;
    CfPoolCtx walk{};  // WALK
  } placement;
  bool match_ran() const { return placement.state == Placement::DONE; }
  void placement_drop() { placement.state = Placement::NONE; }  // before the tables a set-up points into change: the set-up is forgotten, no match has run
  void placement_complete(unsigned form, const WinCtl& c) { last_ctl = c, last_form = form, placement.state = Placement::DONE; }
  WinCtl* h_multi = nullptr;  // pinned: the pools' WinCtl read-backs
  // served walkers (match_rounds_served): the two streams of a served match led by this engine, its control blocks, what it did
  static constexpr unsigned kMaxServers = 4;
  hipStream_t s_walk = nullptr, s_serve[kMaxServers] = {};
  DArr<ServeSlot> w_slots;
  DArr<ServeCtl> w_sctl;
  ServeHost* h_serve = nullptr;  // pinned, one per server
  struct ServedStats {
    unsigned mode = 0;  // 0 not served, 1 walkers beside serve launches, 2 stepping form
    unsigned pools = 0, servers = 0, iterations = 0, empty_iterations = 0, pools_served = 0, fell_back = 0;
    double latch_wait_ms = 0;
  } served;
  int n_cus = 256;
  DArr<MatchIn> v_in;
  void* h_inbuf = nullptr;  // pinned staging copy of MatchIn
  WinCtl last_ctl{};
  bool groups_simple = true;  // no balanced / attribute-equals group staged (cook_match_stage)
  MatchIn min{};
  bool cycle_staged = false;
  unsigned cycle_considered = 0;
  // the last cycle ran the considerable filters under a staged user state, and nothing has replaced that state, the rank or the match
  // since (cook_cycle_autoscale reads all three)
  bool cycle_cons_ran = false;
  bool kube_last = false;  // the last cycle ended in a distribution (cook_cycle_run_kube): job_to_offer holds 0 / -1 = launched / not, no placement ran
  // ---- the standing queue of the queue cycles (queue_host.hpp): `ranked` is the queue a match cycle may consume — the last cycle took its
  // jobs from it and nothing has shifted or dropped the rows it points at since (with rank_done and a match that has run: that cycle is complete)
  bool q_valid = false;
  bool q_stepped = false;  // a queue cycle has advanced since the last rank: the task table no longer lists what runs (rebal_resident_host.hpp)
  const uint32_t* q_last_pos = nullptr;  // device: rank positions of the last cycle's considered jobs; null: 0 .. cycle_considered - 1
  bool q_groups_own = false;             // min.g_run_* point at a queue cycle's table; the staged one is q_sg_*
  const uint32_t *q_sg_off = nullptr, *q_sg_host = nullptr, *q_sg_attr = nullptr;
  uint32_t q_sg_total = 0;
  uint32_t q_advance_us = 0;             // host microseconds in the last queue cycle's advance, its synchronisation included (stats [31])
  std::vector<uint8_t> h_g_type;         // the staged groups' type / attr_key / minimum (a queue step's table must agree)
  std::vector<uint32_t> h_g_key;
  std::vector<int32_t> h_g_min;
  std::unique_ptr<QueueBufs> qb;               // (allocated on first use)
  std::unique_ptr<CarryBufs> cyb;              // the carry of a queue cycle (allocated on first use)
  std::unique_ptr<ReleaseBufs> rlb;            // the release of a queue cycle (allocated on first use)
  std::unique_ptr<ChurnBufs> chb;              // the host churn of a queue cycle (allocated on first use)
  std::unique_ptr<ReserveBufs> rvb;            // the rebalancer's host reservations kept across cycles (allocated on first use)
  std::unique_ptr<LimiterBufs> lmb;            // the launch-rate limiters kept across cycles (allocated on first use)
  // the host's mirror of the staged offers' host ids, ascending (match_stage_offers, cook_cycle_update's offers; a host churn edits it per
  // list entry): what a churn is checked against and sized by before its first launch.  Not known: offers built on the device
  std::vector<uint32_t> o_hosts;
  bool o_hosts_known = false;
  bool o_run_cols_made = false;  // a carry or a release into this offer table has been asked for: its run_* / num_tasks / ports count as present (churn_host.hpp)

  // ---- rebalancer state (allocated on first use) ----
  std::unique_ptr<RebalBufs> rb;
  std::unique_ptr<ResidentRebalBufs> rrb;  // cook_cycle_rebalance_stage (allocated on first use)
  // ---- considerable-jobs filters (allocated on first use) ----
  std::unique_ptr<ConsBufs> cb;
  // ---- offer construction (allocated on first use) ----
  std::unique_ptr<OfferBufs> ofb;
  std::unique_ptr<PodTableBufs> ptb;  // the resident pod table's identity and delta (allocated on first use)
  bool offers_built = false;          // the staged offers are rows of this engine's cook_offers_run, in place (offers_note_hosts)
  // ---- why-unscheduled summaries / match-cycle metrics (allocated on first use) ----
  std::unique_ptr<ExplainBufs> xb;
  std::unique_ptr<UpdateBufs> ub;  // cook_cycle_update (allocated on first use)
  std::unique_ptr<UserStatsBufs> usb;  // cook_user_stats* (allocated on first use)
  std::unique_ptr<AutoscaleBufs> asb;  // cook_cycle_autoscale (allocated on first use)
  std::unique_ptr<SweepBufs> swb;      // cook_sweep_running (allocated on first use)
  std::unique_ptr<KubeBufs> kub;       // cook_kube_distribute (allocated on first use)
  std::unique_ptr<UnschedBufs> unb;    // cook_unscheduled (allocated on first use)
  std::unique_ptr<UsageBufs> ugb;      // cook_usage_breakdown* (allocated on first use)
  std::unique_ptr<LaunchBufs> lrb;     // cook_match_launch_resources (allocated on first use)
  MatchIn last_in{};  // the MatchIn of the last match run (K, j_index as used)
  bool last_in_valid = false;
  bool v_in_is_last = false;  // v_in holds last_in on the device (the window rounds' set-up of the last match uploaded it)
  unsigned rlog_id = 0;  // suffix of this engine's COOK_ROUND_LOG file
  DArr<uint32_t> j_user;
  bool has_j_user = false;
  // (hash uuid) of the pending jobs by pending ordinal (cook_cycle_set_job_hashes): the leading hash_set rows are set
  DArr<int32_t> j_hash;
  unsigned hash_set = 0;
  // ---- class-ordered best fit (classfit.hpp)
  DArr<CfCtl> cf_ctl;
  DArr<uint64_t> cf_attr8;
  DArr<uint32_t> cf_h2o, cf_pos[3], cf_scr[3], cf_gcount, cf_gmem;
  DArr<CfJob> cf_jobs;
  uint32_t cf_max_host = 0xFFFFFFFFu;   // greatest host id of the staged offers (match_stage_offers, cook_cycle_update's offers); 0xFFFFFFFF: not known (offers built on the device)
  uint32_t cf_group_run_total = 0;      // running cotasks over all staged groups
  unsigned last_form = 0;               // how the last match was placed: 0 window rounds, 1 serial sweep, 3 class-ordered best fit
  unsigned spread_serial_calls = 0;     // matches that match_algo 0 / 2 / 3 would have placed in window rounds and the sweep placed: a spreader (cook_match_stats_ex [39])
  unsigned cf_inelig = 0;               // why the last match that asked for class-ordered best fit did not get it (CF_X_* bits; 0x10000: switched off / the host's checks)
  uint32_t cf_stats[48] = {};
  char* h_cf = nullptr;                 // pinned: summaries and statistics of the pools of a cf_run led by this engine

  void fail(int code, const std::string& m) { throw cook_error(code, m); }
  ~cook_engine();  // (defined behind the *_host.hpp includes, where the side features' blocks are complete types)
};

namespace {

template <class F>
int guarded(cook_engine* e, F&& f) {
  if (!e) return COOK_E_INVALID;
  try {
    COOK_HIP(hipSetDevice(e->device));
    f();
    e->err.clear();
    return COOK_OK;
  } catch (const cook_error& ce) {
    e->err = ce.msg;
    (void)hipStreamSynchronize(e->stream);
    e->ev_pending.clear();
    e->ev_used = 0;
    return ce.code;
  } catch (const std::exception& ex) {
    e->err = ex.what();
    return COOK_E_NOMEM;
  } catch (...) {  // nothing may cross the C boundary
    e->err = "unknown exception";
    return COOK_E_STATE;
  }
}

// An array of engines as the *_multi entry points take it: every engine there and none twice (two flows, or two runs of rounds, would
// work on one engine's buffers); same_device: all on the first one's device.
bool engines_valid(cook_engine* const* engines, uint32_t n, bool same_device) {
  for (uint32_t i = 0; i < n; ++i) {
    if (!engines[i] || (same_device && engines[i]->device != engines[0]->device)) return false;
    for (uint32_t k = 0; k < i; ++k)
      if (engines[i] == engines[k]) return false;
  }
  return true;
}

// a side feature's block of buffers (cook_engine: rb, cb, ofb, ...), made on first use
template <class B>
B& bufs(std::unique_ptr<B>& p) {
  if (!p) p.reset(new B());
  return *p;
}

// engines alive per device: sizes the persistent placement kernel so that the kernels of all pools sharing a GPU are resident
static std::atomic<int> g_engines_on_device[64];

// The one valid order: every file may use what the files above it define (each says so in its first comment).
#include "launch.hpp"          // launches, copies, synchronisation, timing: what every host flow is written in
#include "pool_batch.hpp"      // the flows of several pools on one stream (defines what launch.hpp and device_buf.hpp only declare)
#include "rank_host.hpp"       // scan and radix drivers, the rank
#include "classfit_host.hpp"   // class-ordered best fit: set-up and launch (match_host.hpp attempts it)
static void reserve_drop(cook_engine* e);  // reserve_host.hpp: a stage or an update drops the engine's own reservation map
#include "match_host.hpp"      // match staging, one pool's placement, several pools in lockstep rounds
#include "served_host.hpp"     // several pools by served walkers
// limiter_host.hpp: what the considerable filters, a cycle's front part and the carry ask of the launch-rate limiters the engine may hold
static bool limiter_own(const cook_engine* e);
static void limiter_check_user_state(cook_engine* e, const cook_user_state* us);
static void limiter_new_cycle(cook_engine* e);
static LimView limiter_view(cook_engine* e, unsigned U, bool cycle);
static void limiter_commit_earn(cook_engine* e, const LimView& v, unsigned U, const uint32_t* passed, const uint32_t* rate_limited, unsigned* fcnt);
static void limiter_filter_finish(cook_engine* e, const unsigned* h);
#include "considerable_host.hpp"
#include "rebalance_host.hpp"
#include "offers_host.hpp"
#include "explain_host.hpp"
#include "cycle_update.hpp"
#include "user_stats_host.hpp"
#include "autoscale_host.hpp"
#include "carry_host.hpp"      // a queue cycle's carry: needs the staged user state (considerable_host.hpp)
#include "launch_res_host.hpp"  // the launch resources of the last match: the carry's keys and segments
#include "release_host.hpp"    // a queue cycle's release: the carry's segments and column sets
#include "churn_host.hpp"      // a queue cycle's host churn: the release's host-indexed table, the carry's segments
#include "reserve_host.hpp"    // the host reservations kept across cycles: the advance's counters (churn_kernels.hpp)
#include "limiter_host.hpp"    // the launch-rate limiters kept across cycles: QueueArgs (carry_host.hpp), the advance's counters
#include "podtable_host.hpp"   // the resident pod table: OfferBufs (offers_host.hpp), QueueArgs; queue_host.hpp calls its queue part
#include "queue_host.hpp"
#include "sweep_host.hpp"
#include "unscheduled_host.hpp"
#include "usage_host.hpp"
#include "rebal_resident_host.hpp"  // the rebalancer's stage from the resident cycle state: RebalBufs, ConsBufs' eligible mask, cycle_update.hpp's element copies
#include "cycle_host.hpp"      // a cycle's front parts (rank or queue step, considerable filters) and its single-pool entry: needs the two above them
#include "kube_host.hpp"       // a Kubernetes-scheduler pool: the distributor, and the cycle that ends in it (needs the front parts above)

}  // namespace

// An engine's end, in this order: (1) its stream is synchronised — the served match's streams are drained by the call that used them —, so
// nothing is running and nothing can be enqueued any more; (2) the guard's self-test writes; (3) events, page-locked blocks and streams go,
// here; (4) the device buffers go LAST: the members and the side features' blocks destroy themselves behind this body.  (4) behind (3) is
// safe because freeing a buffer needs no stream of the engine: DBuf::free_now looks at its guard bands with blocking copies on the null
// stream and calls hipFree, and no block's destructor uses a stream or a page-locked block freed here (UpdateBufs frees page-locked memory
// of its own).  The device set here is still current then.
cook_engine::~cook_engine() {
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  if (g_guard && std::getenv("COOK_GUARD_SELFTEST") && m_j2o.b.p)  // the guard's own test: one byte past the end of the placement column
    (void)hipMemset((char*)m_j2o.b.p + m_j2o.b.cap, 0, 1);
  for (auto ev : ev_pool) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : ev_stage)
    if (ev) (void)hipEventDestroy(ev);
  for (void* h : {(void*)h_scratch, h_inbuf, (void*)h_multi, (void*)h_cf, (void*)h_serve})
    if (h) (void)hipHostFree(h);
  if (s_walk) (void)hipStreamDestroy(s_walk);
  for (hipStream_t sv : s_serve)
    if (sv) (void)hipStreamDestroy(sv);
  if (stream) (void)hipStreamDestroy(stream);
}

// =================================================================================================================
// C ABI
// =================================================================================================================
extern "C" {

const char* cook_version(void) {
  return "cookmatch 0.3.0 (" COOK_BUILD_NAME ")";
}
int cook_abi_version(void) { return COOK_ABI_VERSION; }

// the values of cook_params that are refused where they are set (create, set_params) -> the message, or nullptr
static const char* params_refusal(const cook_params* p) {
  if (p->fitness < 0 || p->fitness >= COOK_FITNESS_N)
    return "cook_params.fitness: 0 = cpuMemBinPacker, 1 = cpuBinPacker, 2 = memoryBinPacker, 3 = cpuMemSpreader, 4 = cpuSpreader, 5 = memorySpreader";
  return nullptr;
}
static thread_local const char* tl_create_err = nullptr;  // cook_last_error(NULL): why the thread's last create refused its params (null: it did not)

int cook_engine_create(const cook_params* params, int device_id, cook_engine** out) {
  if (!params || !out) return COOK_E_INVALID;
  *out = nullptr;
  tl_create_err = params_refusal(params);
  if (tl_create_err) return COOK_E_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return COOK_E_DEVICE;  // no GPU: fail loudly, no CPU fallback
  if (device_id < 0 || device_id >= ndev) return COOK_E_INVALID;
  cook_engine* e = nullptr;
  try {
    e = new cook_engine();
    e->params = *params;
    e->device = device_id;
    COOK_HIP(hipSetDevice(device_id));
    COOK_HIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    {
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) e->n_cus = prop.multiProcessorCount;
    }
    for (int i = 0; i < 4; ++i) COOK_HIP(hipEventCreate(&e->ev_stage[i]));
    COOK_HIP(hipHostMalloc((void**)&e->h_scratch, 64 * 8, hipHostMallocDefault));
    COOK_HIP(hipHostMalloc((void**)&e->h_inbuf, sizeof(MatchIn), hipHostMallocDefault));
    e->d_scratch64.ensure(64);
    e->d_counters.ensure(64);
  } catch (const cook_error&) {
    delete e;
    return COOK_E_DEVICE;
  } catch (...) {
    delete e;
    return COOK_E_NOMEM;
  }
  g_engines_on_device[device_id & 63].fetch_add(1);
  *out = e;
  return COOK_OK;
}

void cook_engine_destroy(cook_engine* e) {
  if (!e) return;
  g_engines_on_device[e->device & 63].fetch_sub(1);
  delete e;
}

int cook_engine_set_params(cook_engine* e, const cook_params* p) {
  if (!e || !p) return COOK_E_INVALID;
  if (const char* why = params_refusal(p)) {  // the engine keeps the params it had
    e->err = why;
    return COOK_E_INVALID;
  }
  e->params = *p;
  return COOK_OK;
}

const char* cook_last_error(const cook_engine* e) { return e ? e->err.c_str() : (tl_create_err ? tl_create_err : "null engine"); }

int cook_rank_stage(cook_engine* e, const cook_tasks* tasks, const cook_users* users) {
  return guarded(e, [&] { rank_stage(e, tasks, users); });
}
int cook_rank_set_quota(cook_engine* e, const cook_pool_quota* q) {
  if (!e) return COOK_E_INVALID;
  if (q)
    e->quota = *q;
  else
    std::memset(&e->quota, 0, sizeof(e->quota));
  return COOK_OK;
}
int cook_rank_pool_usage(cook_engine* e, cook_usage* out) {
  if (!out) return COOK_E_INVALID;
  return guarded(e, [&] { rank_pool_usage(e, out); });
}
int cook_rank_user_usage(cook_engine* e, double* usage, int usage_is_device) {
  return guarded(e, [&] { rank_user_usage(e, usage, usage_is_device != 0); });
}
int cook_rank_run(cook_engine* e) {
  return guarded(e, [&] {
    StageTimer t(e, 0, &e->rank_ms);
    rank_run(e);
    t.stop();
    prof_collect(e);
  });
}
int cook_rank_fetch(cook_engine* e, uint32_t* ranked, uint32_t* n_out, double* dru) {
  return guarded(e, [&] { rank_fetch(e, ranked, n_out, dru); });
}
int cook_rank(cook_engine* e, const cook_tasks* tasks, const cook_users* users, const cook_pool_quota* quota, uint32_t* ranked,
              uint32_t* n_out, double* dru) {
  if (n_out) *n_out = 0;
  int rc = cook_rank_stage(e, tasks, users);
  if (rc) return rc;
  cook_rank_set_quota(e, quota);
  rc = cook_rank_run(e);
  if (rc) return rc;
  return cook_rank_fetch(e, ranked, n_out, dru);
}

int cook_match_stage(cook_engine* e, const cook_jobs* j, const cook_offers* o, const cook_groups* g, const uint32_t* reserved_hosts,
                     uint32_t n_reserved) {
  return guarded(e, [&] {
    match_stage_inputs(e, j, o, g, reserved_hosts, n_reserved);
    e->cycle_staged = false;
  });
}
int cook_match_stage_built_offers(cook_engine* e, const cook_jobs* j, const cook_groups* g, const uint32_t* reserved_hosts,
                                  uint32_t n_reserved, int with_task_limits) {
  return guarded(e, [&] {
    const cook_offers o = built_offers_view(e, with_task_limits);
    match_stage_inputs(e, j, &o, g, reserved_hosts, n_reserved, true);
    e->cycle_staged = false;
  });
}
int cook_cycle_stage_built_offers(cook_engine* e, const cook_tasks* tasks, const cook_users* users, const cook_jobs* pending_jobs,
                                  const cook_groups* groups, const uint32_t* reserved_hosts, uint32_t n_reserved, int with_task_limits) {
  return guarded(e, [&] {
    const cook_offers o = built_offers_view(e, with_task_limits);
    rank_stage(e, tasks, users);
    if (!pending_jobs || pending_jobs->n != e->n_pending)
      e->fail(COOK_E_INVALID, "cook_cycle_stage_built_offers: pending_jobs->n must equal the number of pending tasks");
    match_stage_inputs(e, pending_jobs, &o, groups, reserved_hosts, n_reserved, true);
    e->cycle_staged = true;
    limiter_drop(e);  // (the users are restaged)
    if (e->ub) e->ub->csr_known = false;  // (cycle_update.hpp: the staged CSR columns' sizes are looked up again)
  });
}
int cook_match_run(cook_engine* e) {
  return guarded(e, [&] {
    if (!e->match_staged) e->fail(COOK_E_STATE, "cook_match_run before cook_match_stage");
    // the match of the STAGED jobs replaces the last cycle's job_to_offer and considered count: neither a queue cycle's advance nor
    // cook_cycle_autoscale may read them as that cycle's
    e->q_valid = false;
    e->cycle_cons_ran = false;
    StageTimer t(e, 2, &e->match_ms);
    match_run_device(e, e->K, nullptr);
    t.stop();
    prof_collect(e);
  });
}
int cook_match_fetch(cook_engine* e, int32_t* job_to_offer, uint32_t* fail_code, uint8_t* head_matched) {
  return guarded(e, [&] { match_fetch(e, e->cycle_considered, job_to_offer, fail_code, head_matched); });
}
int cook_match_count(cook_engine* e, uint32_t* n_jobs) {
  return guarded(e, [&] {
    if (!n_jobs) e->fail(COOK_E_INVALID, "cook_match_count: null n_jobs");
    if (!e->match_ran()) e->fail(COOK_E_STATE, "cook_match_count before a match has run");
    *n_jobs = e->cycle_considered;
  });
}
int cook_match(cook_engine* e, const cook_jobs* j, const cook_offers* o, const cook_groups* g, const uint32_t* reserved_hosts,
               uint32_t n_reserved, int32_t* job_to_offer, uint32_t* fail_code, uint8_t* head_matched) {
  if (j && job_to_offer)
    for (uint32_t k = 0; k < j->n; ++k) job_to_offer[k] = -1;  // "no matches" on any error path
  if (head_matched) *head_matched = 1;
  int rc = cook_match_stage(e, j, o, g, reserved_hosts, n_reserved);
  if (rc) return rc;
  rc = cook_match_run(e);
  if (rc) return rc;
  return cook_match_fetch(e, job_to_offer, fail_code, head_matched);
}

int cook_cycle_stage(cook_engine* e, const cook_tasks* tasks, const cook_users* users, const cook_jobs* pending_jobs,
                     const cook_offers* offers, const cook_groups* groups, const uint32_t* reserved_hosts, uint32_t n_reserved) {
  return guarded(e, [&] {
    rank_stage(e, tasks, users);
    if (!pending_jobs || pending_jobs->n != e->n_pending)
      e->fail(COOK_E_INVALID, "cook_cycle_stage: pending_jobs->n must equal the number of pending tasks");
    match_stage_inputs(e, pending_jobs, offers, groups, reserved_hosts, n_reserved);
    e->cycle_staged = true;
    limiter_drop(e);  // (the users are restaged)
    if (e->ub) e->ub->csr_known = false;  // (cycle_update.hpp: the staged CSR columns' sizes are looked up again)
  });
}
int cook_cycle_update(cook_engine* e, const cook_cycle_delta* delta) {
  // where the call's time went, for cook_match_stats_ex [26..28] (an occasional 9 ms call among 1 ms ones: bench.py boundary.update_ms_samples)
  const auto t0 = std::chrono::steady_clock::now();
  const double sync0 = tl_sync_ms;
  const unsigned alloc0 = tl_dbuf_allocs;
  const int rc = guarded(e, [&] {
    ReserveSuspend hold(e);  // the staged reserved hosts are what the update checks, edits and re-points ...
    cycle_update(e, bufs(e->ub), delta);
    hold.drop();  // ... and, the rows having shifted, what the match reads again (a refused update keeps the engine's map)
    prof_collect(e);
  });
  if (e) {
    e->upd_us = (uint32_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    e->upd_sync_us = (uint32_t)((tl_sync_ms - sync0) * 1000.0);
    e->upd_allocs = tl_dbuf_allocs - alloc0;
  }
  return rc;
}
void* cook_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}
void cook_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}
int cook_cycle_run(cook_engine* e, uint32_t num_considerable) {
  return cycle_run_one(e, [&] { return cycle_rank_part(e, num_considerable); }, /*defer=*/false);
}
int cook_cycle_run_rank(cook_engine* e, uint32_t num_considerable) {
  return cycle_run_one(e, [&] { return cycle_rank_part(e, num_considerable); }, /*defer=*/true);
}
int cook_cycle_run_rank_multi(cook_engine** engines, uint32_t n, const uint32_t* num_considerable, double* const* user_usage, int usage_is_device) {
  if (!engines || n == 0 || !num_considerable) return COOK_E_INVALID;
  for (uint32_t i = 0; i < n; ++i)
    if (user_usage && !user_usage[i]) return COOK_E_INVALID;
  return run_pools_batched(
      engines, n,
      [&](uint32_t i) {
        int rc = cook_cycle_run_rank(engines[i], num_considerable[i]);
        if (rc == COOK_OK && user_usage) rc = cook_rank_user_usage(engines[i], user_usage[i], usage_is_device);
        return rc;
      },
      [&](uint32_t i) {
        cook_engine* e = engines[i];
        const unsigned K = cycle_rank_part(e, num_considerable[i]);
        if (user_usage) rank_user_usage(e, user_usage[i], usage_is_device != 0);
        cycle_match(e, K, /*defer=*/true);
      },
      /*rank_part=*/true);
}
// ---- queue cycles: match cycles on the standing ranked queue, without a re-rank (cookmatch.h) -----------------------------------
// The parts of the advance, each behind the one before: the carry (carry_host.hpp), the release (release_host.hpp), the host churn
// (churn_host.hpp), the host reservations (reserve_host.hpp).  One pool; defer: the placement is set up and runs in cook_cycle_match_multi
static int queue_run_one(cook_engine* e, const QueueArgs& q, uint32_t num_considerable, bool defer) {
  return cycle_run_one(e, [&] { return cycle_queue_part(e, q, num_considerable); }, defer);
}
int cook_cycle_run_queue(cook_engine* e, const cook_queue_step* step, uint32_t num_considerable) {
  return queue_run_one(e, QueueArgs{step, nullptr, nullptr, nullptr, nullptr}, num_considerable, /*defer=*/false);
}
int cook_cycle_run_queue_rank(cook_engine* e, const cook_queue_step* step, uint32_t num_considerable) {
  return queue_run_one(e, QueueArgs{step, nullptr, nullptr, nullptr, nullptr}, num_considerable, /*defer=*/true);
}
int cook_cycle_run_queue_carry(cook_engine* e, const cook_queue_step* step, const cook_queue_carry* carry, uint32_t num_considerable) {
  return queue_run_one(e, QueueArgs{step, carry, nullptr, nullptr, nullptr}, num_considerable, /*defer=*/false);
}
int cook_cycle_run_queue_release(cook_engine* e, const cook_queue_step* step, const cook_queue_carry* carry, const cook_finished* finished,
                                 uint32_t num_considerable) {
  return queue_run_one(e, QueueArgs{step, carry, finished, nullptr, nullptr}, num_considerable, /*defer=*/false);
}
int cook_cycle_run_queue_hosts(cook_engine* e, const cook_queue_step* step, const cook_queue_carry* carry, const cook_finished* finished,
                               const cook_host_churn* hosts, uint32_t num_considerable) {
  return queue_run_one(e, QueueArgs{step, carry, finished, hosts, nullptr}, num_considerable, /*defer=*/false);
}
int cook_cycle_run_queue_reserve(cook_engine* e, const cook_queue_step* step, const cook_queue_carry* carry, const cook_finished* finished,
                                 const cook_host_churn* hosts, const cook_reservations* reservations, uint32_t num_considerable) {
  return queue_run_one(e, QueueArgs{step, carry, finished, hosts, reservations}, num_considerable, /*defer=*/false);
}
// ... for every pool of a GPU: one flow per pool in a pool batch, as cook_cycle_run_rank_multi (steps, carries, finished: null = none)
static int queue_run_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps, const cook_queue_carry* const* carries,
                           const cook_finished* const* finished, const cook_host_churn* const* hosts, const cook_reservations* const* reservations,
                           const uint32_t* num_considerable) {
  if (!engines || n == 0 || !num_considerable) return COOK_E_INVALID;
  auto at = [](auto* const* part, uint32_t i) { return part ? part[i] : nullptr; };
  auto args = [&](uint32_t i) { return QueueArgs{at(steps, i), at(carries, i), at(finished, i), at(hosts, i), at(reservations, i)}; };
  return run_pools_batched(
      engines, n,
      [&](uint32_t i) { return queue_run_one(engines[i], args(i), num_considerable[i], /*defer=*/true); },
      [&](uint32_t i) { cycle_match(engines[i], cycle_queue_part(engines[i], args(i), num_considerable[i]), /*defer=*/true); },
      /*rank_part=*/true);
}
int cook_cycle_run_queue_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps, const uint32_t* num_considerable) {
  return queue_run_multi(engines, n, steps, nullptr, nullptr, nullptr, nullptr, num_considerable);
}
int cook_cycle_run_queue_carry_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps, const cook_queue_carry* const* carries,
                                     const uint32_t* num_considerable) {
  return queue_run_multi(engines, n, steps, carries, nullptr, nullptr, nullptr, num_considerable);
}
int cook_cycle_run_queue_release_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps, const cook_queue_carry* const* carries,
                                       const cook_finished* const* finished, const uint32_t* num_considerable) {
  return queue_run_multi(engines, n, steps, carries, finished, nullptr, nullptr, num_considerable);
}
int cook_cycle_run_queue_hosts_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps, const cook_queue_carry* const* carries,
                                     const cook_finished* const* finished, const cook_host_churn* const* hosts, const uint32_t* num_considerable) {
  return queue_run_multi(engines, n, steps, carries, finished, hosts, nullptr, num_considerable);
}
int cook_cycle_run_queue_reserve_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps, const cook_queue_carry* const* carries,
                                       const cook_finished* const* finished, const cook_host_churn* const* hosts,
                                       const cook_reservations* const* reservations, const uint32_t* num_considerable) {
  return queue_run_multi(engines, n, steps, carries, finished, hosts, reservations, num_considerable);
}
// ... of a pool whose offers are built from its pods (podtable_host.hpp): no host churn, the pod delta and the rebuild in its place
static QueueArgs queue_pods_args(const cook_queue_step* step, const cook_queue_carry* carry, const cook_finished* finished, const cook_pod_delta* pods,
                                 const cook_reservations* reservations, int with_task_limits) {
  QueueArgs q{step, carry, finished, nullptr, reservations};
  q.pods = pods, q.pods_on = true, q.with_task_limits = with_task_limits;
  return q;
}
int cook_cycle_run_queue_pods(cook_engine* e, const cook_queue_step* step, const cook_queue_carry* carry, const cook_finished* finished,
                              const cook_pod_delta* pods, const cook_reservations* reservations, int with_task_limits, uint32_t num_considerable) {
  return queue_run_one(e, queue_pods_args(step, carry, finished, pods, reservations, with_task_limits), num_considerable, /*defer=*/false);
}
// the pools one after another (offers_* are launches of their own, not batched behind cook_multi): each exactly its single call, deferred
int cook_cycle_run_queue_pods_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps, const cook_queue_carry* const* carries,
                                    const cook_finished* const* finished, const cook_pod_delta* const* pods,
                                    const cook_reservations* const* reservations, const int32_t* with_task_limits, const uint32_t* num_considerable) {
  if (!engines || n == 0 || !num_considerable || !engines_valid(engines, n, false)) return COOK_E_INVALID;
  auto at = [](auto* const* part, uint32_t i) { return part ? part[i] : nullptr; };
  int first = COOK_OK;
  for (uint32_t i = 0; i < n; ++i) {
    const QueueArgs q = queue_pods_args(at(steps, i), at(carries, i), at(finished, i), at(pods, i), at(reservations, i), with_task_limits ? with_task_limits[i] : 0);
    const int rc = queue_run_one(engines[i], q, num_considerable[i], /*defer=*/true);
    if (rc != COOK_OK && first == COOK_OK) first = rc;
  }
  return first;
}
int cook_cycle_set_reservations(cook_engine* e, const cook_reservations* r) {
  return guarded(e, [&] {
    reserve_set(e, r);
    prof_collect(e);
  });
}
int cook_cycle_reserve_info(cook_engine* e, cook_reserve_info* out) {
  return guarded(e, [&] {
    if (!out) e->fail(COOK_E_INVALID, "cook_cycle_reserve_info: null out");
    *out = e->rvb ? e->rvb->info : cook_reserve_info{};
  });
}
int cook_cycle_fetch_reservations(cook_engine* e, uint32_t* pending, uint32_t* host, uint32_t cap, uint32_t* n_out) {
  return guarded(e, [&] { reserve_fetch(e, pending, host, cap, n_out); });
}
int cook_cycle_set_limiters(cook_engine* e, const cook_limiters* l) {
  return guarded(e, [&] {
    limiter_set(e, l);
    prof_collect(e);
  });
}
int cook_cycle_set_clock(cook_engine* e, const cook_clock* c) {
  return guarded(e, [&] { limiter_set_clock(e, c); });
}
int cook_cycle_limiters_spend(cook_engine* e, const uint8_t* offer_skipped, uint32_t n_offer_skipped, int64_t spend_ms) {
  return guarded(e, [&] {
    limiter_spend(e, offer_skipped, n_offer_skipped, spend_ms);
    prof_collect(e);
  });
}
int cook_cycle_fetch_limiters(cook_engine* e, int64_t* tokens, int64_t* last_update_ms, int64_t* time_until_ms) {
  return guarded(e, [&] { limiter_fetch(e, tokens, last_update_ms, time_until_ms); });
}
int cook_cycle_fetch_rate_limit(cook_engine* e, uint32_t* rate_limited, uint32_t* passed) {
  return guarded(e, [&] { limiter_fetch_counts(e, rate_limited, passed); });
}
int cook_cycle_limiter_info(cook_engine* e, cook_limiter_info* out) {
  return guarded(e, [&] {
    if (!out) e->fail(COOK_E_INVALID, "cook_cycle_limiter_info: null out");
    *out = e->lmb ? e->lmb->info : cook_limiter_info{};
  });
}
int cook_cycle_churn_info(cook_engine* e, cook_churn_info* out) {
  return guarded(e, [&] {
    if (!out) e->fail(COOK_E_INVALID, "cook_cycle_churn_info: null out");
    *out = e->chb ? e->chb->info : cook_churn_info{0u, 0u, 0u, e->M};
  });
}
int cook_cycle_fetch_offers(cook_engine* e, cook_offer_rows* out) {
  return guarded(e, [&] { churn_fetch_offers(e, out); });
}
int cook_cycle_release_info(cook_engine* e, cook_release_info* out) {
  return guarded(e, [&] {
    if (!out) e->fail(COOK_E_INVALID, "cook_cycle_release_info: null out");
    *out = e->rlb ? e->rlb->info : cook_release_info{};
  });
}
int cook_rank_pool_usage_multi(cook_engine** engines, uint32_t n, cook_usage* out) {
  if (!engines || n == 0 || !out) return COOK_E_INVALID;
  return run_pools_batched(
      engines, n, [&](uint32_t i) { return cook_rank_pool_usage(engines[i], &out[i]); },
      [&](uint32_t i) { rank_pool_usage(engines[i], &out[i]); }, /*rank_part=*/false);
}
int cook_user_stats(cook_engine* e, const cook_user_limits* limits, double* per_user, int per_user_is_device, uint8_t* user_state,
                    cook_user_stats_totals* totals) {
  if (!e) return COOK_E_INVALID;
  return guarded(e, [&] { user_stats_run(&e, 1, nullptr, e->U, limits, per_user, per_user_is_device != 0, user_state, totals); });
}
int cook_user_stats_multi(cook_engine** engines, uint32_t n, const uint32_t* const* user_map, uint32_t n_users, const cook_user_limits* group_limits,
                          double* per_user, int per_user_is_device, uint8_t* user_state, cook_user_stats_totals* totals) {
  if (!engines || n == 0 || !group_limits) return COOK_E_INVALID;
  if (!engines_valid(engines, n, true)) return COOK_E_INVALID;
  return guarded(engines[0], [&] {
    user_stats_run(engines, n, user_map, n_users, group_limits, per_user, per_user_is_device != 0, user_state, totals);
  });
}
int cook_unscheduled(cook_engine* e, const cook_unsched_limits* limits, const uint8_t* in_window, const uint32_t* rows, uint32_t n_rows,
                     uint32_t* reasons, uint32_t* queue_pos, double* total, int total_is_device, uint32_t* ahead, uint32_t* list_len) {
  if (!e) return COOK_E_INVALID;
  return guarded(e, [&] {
    unscheduled_run(e, limits, in_window, rows, n_rows, reasons, queue_pos, total, total_is_device != 0, ahead, list_len);
    prof_collect(e);
  });
}
int cook_usage_breakdown(cook_engine* e, const uint32_t* group_of_row, uint32_t n_groups, const uint32_t* users, uint32_t n_list,
                         cook_usage_out* out) {
  if (!e) return COOK_E_INVALID;
  return guarded(e, [&] {
    usage_run(&e, 1, nullptr, e->U, &group_of_row, n_groups, users, n_list, out, false);
    prof_collect(e);
  });
}
int cook_usage_breakdown_multi(cook_engine** engines, uint32_t n, const uint32_t* const* user_map, uint32_t n_users,
                               const uint32_t* const* group_of_row, uint32_t n_groups, const uint32_t* users, uint32_t n_list,
                               cook_usage_out* out) {
  if (!engines || n == 0) return COOK_E_INVALID;
  if (!engines_valid(engines, n, true)) return COOK_E_INVALID;
  return guarded(engines[0], [&] {
    usage_run(engines, n, user_map, n_users, group_of_row, n_groups, users, n_list, out, true);
    prof_collect(engines[0]);
  });
}
int cook_cycle_match_multi(cook_engine** engines, uint32_t n) {
  if (!engines || n == 0 || !engines_valid(engines, n, false)) return COOK_E_INVALID;
  cook_engine* lead = engines[0];
  return guarded(lead, [&] {
    pools_check(engines, n);
    StageTimer tm(lead, 2, &lead->match_ms);
    try {
      // the pools that are placed by class-ordered best fit (classfit.hpp): ONE launch, a workgroup per pool
      const std::vector<cook_engine*> cf = pools_set_up(engines, n, cook_engine::Placement::WALK);
      if (!cf.empty()) cf_run(lead, cf.data(), (unsigned)cf.size(), lead->stream);
      // served walkers (one persistent walker workgroup per pool beside serve launches); lockstep launches when switched off, for more
      // pools than a served call takes, or to finish a served match that gave up
      if (!(served_enabled() && match_rounds_served(engines, n))) match_rounds_multi(engines, n);
    } catch (...) {
      // launches have run, no set-up describes its tables any more: every engine of the call is back to "no match ran" (cook_cycle_fetch: COOK_E_STATE)
      for (uint32_t i = 0; i < n; ++i) engines[i]->placement_drop();
      throw;
    }
    tm.stop();
    for (uint32_t i = 1; i < n; ++i) engines[i]->match_ms = lead->match_ms;  // one joint sequence of launches
    prof_collect(lead);
  });
}
int cook_cycle_fetch(cook_engine* e, uint32_t* ranked, uint32_t* n_ranked, int32_t* job_to_offer, uint32_t* n_considered,
                     uint8_t* head_matched) {
  return guarded(e, [&] {
    rank_fetch(e, ranked, n_ranked, nullptr);
    if (n_considered) *n_considered = e->cycle_considered;
    match_fetch(e, e->cycle_considered, job_to_offer, nullptr, head_matched);
    if (e->kube_last && job_to_offer) std::fill(job_to_offer, job_to_offer + e->cycle_considered, -1);  // (no placement: the launched jobs' marks are the advance's)
  });
}

int cook_considerable(cook_engine* e, const cook_queue* q, const cook_user_state* us, uint32_t num_considerable, uint32_t* out_idx,
                      uint32_t* n_out, uint32_t* rate_limited, uint32_t* passed) {
  if (n_out) *n_out = 0;
  return guarded(e, [&] {
    if (!q || !n_out || (!out_idx && num_considerable && q->n)) e->fail(COOK_E_INVALID, "cook_considerable: null queue / outputs");
    const unsigned n = q->n;
    if (n && (!q->cpus || !q->mem || !q->user)) e->fail(COOK_E_INVALID, "cook_considerable: the queue needs cpus, mem, user");
    ConsBufs& c = bufs(e->cb);
    e->cycle_cons_ran = false;  // (the cycle's user state and considerable result are replaced)
    e->q_valid = false;
    cons_stage_users(e, c, us);
    for (unsigned i = 0; i < n; ++i)
      if (q->user[i] >= c.U) e->fail(COOK_E_INVALID, "cook_considerable: user id out of range");
    h2d(e, c.q_cpus, q->cpus, n);
    h2d(e, c.q_mem, q->mem, n);
    if (q->gpus) h2d(e, c.q_gpus, q->gpus, n);
    h2d(e, c.q_user, q->user, n);
    if (q->eligible) h2d(e, c.q_elig, q->eligible, n);
    cons_run_device(e, c, c, n, c.q_cpus.ptr(), c.q_mem.ptr(), q->gpus ? (const double*)c.q_gpus.ptr() : (const double*)nullptr,
                    c.q_user.ptr(), q->eligible ? (const uint8_t*)c.q_elig.ptr() : (const uint8_t*)nullptr, num_considerable);
    if (c.n_result) copy_async(e, out_idx, c.result, (size_t)c.n_result * 4, hipMemcpyDeviceToHost);
    if (rate_limited && c.U) copy_async(e, rate_limited, c.rate_limited.ptr(), (size_t)c.U * 4, hipMemcpyDeviceToHost);
    if (passed && c.U) copy_async(e, passed, c.passed.ptr(), (size_t)c.U * 4, hipMemcpyDeviceToHost);
    sync(e);
    *n_out = c.n_result;
    prof_collect(e);
  });
}
int cook_cycle_set_considerable(cook_engine* e, const cook_user_state* us, const uint8_t* eligible_by_pending) {
  return guarded(e, [&] {
    ConsBufs& c = bufs(e->cb);
    e->cycle_cons_ran = false;
    if (!us) {
      c.cycle_on = false;
      return;
    }
    if (!e->rank_staged) e->fail(COOK_E_STATE, "cook_cycle_set_considerable before cook_cycle_stage");
    cons_stage_users(e, c, us);
    if (c.U < e->U) e->fail(COOK_E_INVALID, "cook_cycle_set_considerable: fewer users than the staged rank input");
    c.has_elig_by_pending = eligible_by_pending != nullptr;
    if (eligible_by_pending) {
      h2d(e, c.elig_by_pending, eligible_by_pending, e->n_pending);
      sync(e);
    }
    c.cycle_on = true;
  });
}
int cook_cycle_fetch_considerable(cook_engine* e, uint32_t* rank_pos, uint32_t* n_out) {
  if (n_out) *n_out = 0;
  return guarded(e, [&] {
    if (!e->match_ran()) e->fail(COOK_E_STATE, "cook_cycle_fetch_considerable before cook_cycle_run");
    const unsigned K = e->cycle_considered;
    if (e->cb && e->cb->cycle_on) {
      if (K && rank_pos) copy_async(e, rank_pos, e->cb->result, (size_t)K * 4, hipMemcpyDeviceToHost);
      sync(e);
    } else if (rank_pos) {
      for (unsigned k = 0; k < K; ++k) rank_pos[k] = k;
    }
    if (n_out) *n_out = K;
  });
}
int cook_cycle_autoscale(cook_engine* e, const cook_autoscale_params* p, uint32_t* task_idx, uint32_t cap, cook_autoscale_info* info) {
  if (info) *info = cook_autoscale_info{};
  return guarded(e, [&] {
    cycle_autoscale(e, p, task_idx, cap, info);
    prof_collect(e);
  });
}
// ... for every pool of a GPU: one flow per pool in a pool batch; the argument checks run inside the flows (per-engine errors)
int cook_cycle_autoscale_multi(cook_engine** engines, uint32_t n, const cook_autoscale_params* const* params, uint32_t* const* task_idx,
                               const uint32_t* cap, cook_autoscale_info* info, int* rc) {
  if (!engines || n == 0 || !params || !cap) return COOK_E_INVALID;
  for (uint32_t i = 0; i < n; ++i)
    if (!engines[i] || !params[i]) return COOK_E_INVALID;
  if (!engines_valid(engines, n, false)) return COOK_E_INVALID;
  auto out = [&](uint32_t i) { return task_idx ? task_idx[i] : nullptr; };  // (a missing array with cap[i] > 0: engine i's own "null task_idx")
  if (info)
    for (uint32_t i = 0; i < n; ++i) info[i] = cook_autoscale_info{};
  return run_pools_batched(
      engines, n, [&](uint32_t i) { return cook_cycle_autoscale(engines[i], params[i], out(i), cap[i], info ? &info[i] : nullptr); },
      [&](uint32_t i) { cycle_autoscale(engines[i], params[i], out(i), cap[i], info ? &info[i] : nullptr); }, /*rank_part=*/false, rc);
}
int cook_cycle_set_job_hashes(cook_engine* e, const int32_t* hash, uint32_t first, uint32_t n) {
  return guarded(e, [&] { cycle_set_job_hashes(e, hash, first, n); });
}
int cook_cycle_autoscale_clusters(cook_engine* e, const cook_autoscale_params* p, const cook_autoscale_clusters* clusters, uint32_t* task_idx,
                                  uint32_t cap, uint32_t* cluster_off, cook_autoscale_info* info, cook_autoscale_cluster_info* cluster_info,
                                  cook_autoscale_no_cluster* no_cluster) {
  if (info) *info = cook_autoscale_info{};
  if (no_cluster) *no_cluster = cook_autoscale_no_cluster{};
  return guarded(e, [&] {
    const AsClusterReq req{clusters, cluster_off, cluster_info, no_cluster};
    cycle_autoscale(e, p, task_idx, cap, info, &req);
    prof_collect(e);
  });
}
int cook_cycle_autoscale_clusters_multi(cook_engine** engines, uint32_t n, const cook_autoscale_params* const* params,
                                        const cook_autoscale_clusters* const* clusters, uint32_t* const* task_idx, const uint32_t* cap,
                                        uint32_t* const* cluster_off, cook_autoscale_info* info, cook_autoscale_cluster_info* const* cluster_info,
                                        cook_autoscale_no_cluster* no_cluster, int* rc) {
  if (!engines || n == 0 || !params || !clusters || !cap || !cluster_off || !cluster_info) return COOK_E_INVALID;
  for (uint32_t i = 0; i < n; ++i)
    if (!engines[i] || !params[i] || !clusters[i]) return COOK_E_INVALID;
  if (!engines_valid(engines, n, false)) return COOK_E_INVALID;
  auto out = [&](uint32_t i) { return task_idx ? task_idx[i] : nullptr; };
  for (uint32_t i = 0; i < n; ++i) {
    if (info) info[i] = cook_autoscale_info{};
    if (no_cluster) no_cluster[i] = cook_autoscale_no_cluster{};
  }
  auto req = [&](uint32_t i) { return AsClusterReq{clusters[i], cluster_off[i], cluster_info[i], no_cluster ? &no_cluster[i] : nullptr}; };
  return run_pools_batched(
      engines, n,
      [&](uint32_t i) {
        return cook_cycle_autoscale_clusters(engines[i], params[i], clusters[i], out(i), cap[i], cluster_off[i], info ? &info[i] : nullptr,
                                             cluster_info[i], no_cluster ? &no_cluster[i] : nullptr);
      },
      [&](uint32_t i) {
        const AsClusterReq r = req(i);
        cycle_autoscale(engines[i], params[i], out(i), cap[i], info ? &info[i] : nullptr, &r);
      },
      /*rank_part=*/false, rc);
}

int cook_sweep_running(cook_engine* e, const cook_running_set* tasks, const cook_straggler_groups* groups, const cook_sweep_params* p,
                       uint8_t* reason, uint32_t* idx, uint32_t cap, double* group_threshold_s, cook_sweep_info* info) {
  if (info) *info = cook_sweep_info{0u, 0u, 0u, 0u, COOK_NONE_U32};
  return guarded(e, [&] {
    sweep_running(e, tasks, groups, p, reason, idx, cap, group_threshold_s, info);
    prof_collect(e);
  });
}

int cook_kube_distribute(cook_engine* e, uint32_t n_jobs, const uint32_t* location, const double* draw, uint64_t seed,
                         const cook_kube_clusters* clusters, uint8_t* choice, uint32_t* pos_idx, uint32_t cap, uint32_t* cluster_off,
                         cook_kube_cluster_info* cluster_info, cook_kube_info* info) {
  if (info) *info = cook_kube_info{};
  return guarded(e, [&] {
    kube_distribute_run(e, n_jobs, location, draw, seed, clusters, choice, pos_idx, cap, cluster_off, cluster_info, info);
    prof_collect(e);
  });
}

int cook_cycle_run_kube(cook_engine* e, const cook_kube_cycle* c, uint32_t* task_idx, uint32_t cap, uint32_t* cluster_off,
                        cook_kube_cluster_info* cluster_info, cook_kube_info* info) {
  if (info) *info = cook_kube_info{};
  return guarded(e, [&] {
    cycle_run_kube(e, c, task_idx, cap, cluster_off, cluster_info, info);
    prof_collect(e);
  });
}
int cook_cycle_run_kube_multi(cook_engine** engines, uint32_t n, const cook_kube_cycle* const* cycles, uint32_t* const* task_idx,
                              const uint32_t* cap, uint32_t* const* cluster_off, cook_kube_cluster_info* const* cluster_info,
                              cook_kube_info* info, int* rc) {
  if (!engines || n == 0 || !cycles || !cap || !cluster_off || !cluster_info) return COOK_E_INVALID;
  for (uint32_t i = 0; i < n; ++i)
    if (!engines[i] || !cycles[i]) return COOK_E_INVALID;
  if (!engines_valid(engines, n, false)) return COOK_E_INVALID;
  auto out = [&](uint32_t i) { return task_idx ? task_idx[i] : nullptr; };
  if (info)
    for (uint32_t i = 0; i < n; ++i) info[i] = cook_kube_info{};
  return run_pools_batched(
      engines, n,
      [&](uint32_t i) { return cook_cycle_run_kube(engines[i], cycles[i], out(i), cap[i], cluster_off[i], cluster_info[i], info ? &info[i] : nullptr); },
      [&](uint32_t i) { cycle_run_kube(engines[i], cycles[i], out(i), cap[i], cluster_off[i], cluster_info[i], info ? &info[i] : nullptr); },
      /*rank_part=*/false, rc);
}
int cook_cycle_fetch_kube(cook_engine* e, uint8_t* choice, uint32_t* n_out) {
  if (n_out) *n_out = 0;
  return guarded(e, [&] { cycle_fetch_kube(e, choice, n_out); });
}

int cook_rebalance_stage(cook_engine* e, const cook_tasks* running, const uint8_t* running_attrs_cached, const cook_jobs* pending,
                         const int64_t* pending_job_id, const int32_t* pending_priority, const cook_users* users,
                         const cook_host_spare* spare, const cook_offers* host_attrs, const cook_groups* groups,
                         const cook_rebalance_params* params) {
  return guarded(e, [&] {
    rebalance_stage(e, bufs(e->rb), running, running_attrs_cached, pending, pending_job_id, pending_priority, users, spare, host_attrs,
                    groups, params);
  });
}
int cook_rebalance_run(cook_engine* e) {
  return guarded(e, [&] {
    RebalBufs& b = bufs(e->rb);
    StageTimer t(e, 0, &b.ms);
    rebalance_run(e, b);
    t.stop();
    prof_collect(e);
  });
}
int cook_rebalance_fetch(cook_engine* e, cook_preemption* decisions, uint32_t* n_decisions, uint32_t* preempted, uint32_t* n_preempted,
                         double* pending_dru) {
  if (n_decisions) *n_decisions = 0;
  if (n_preempted) *n_preempted = 0;
  return guarded(e, [&] { rebalance_fetch(e, bufs(e->rb), decisions, n_decisions, preempted, n_preempted, pending_dru); });
}
int cook_rebalance(cook_engine* e, const cook_tasks* running, const uint8_t* running_attrs_cached, const cook_jobs* pending,
                   const int64_t* pending_job_id, const int32_t* pending_priority, const cook_users* users, const cook_host_spare* spare,
                   const cook_offers* host_attrs, const cook_groups* groups, const cook_rebalance_params* params,
                   cook_preemption* decisions, uint32_t* n_decisions, uint32_t* preempted, uint32_t* n_preempted, double* pending_dru) {
  if (n_decisions) *n_decisions = 0;  // "no decisions" on any error path
  if (n_preempted) *n_preempted = 0;
  int rc = cook_rebalance_stage(e, running, running_attrs_cached, pending, pending_job_id, pending_priority, users, spare, host_attrs,
                                groups, params);
  if (rc) return rc;
  rc = cook_rebalance_run(e);
  if (rc) return rc;
  return cook_rebalance_fetch(e, decisions, n_decisions, preempted, n_preempted, pending_dru);
}
int cook_rebalance_timing(cook_engine* e, double* ms) {
  if (!e || !ms) return COOK_E_INVALID;
  *ms = e->rb ? e->rb->ms : 0.0;
  return COOK_OK;
}
int cook_cycle_rebalance_stage(cook_engine* e, const cook_cycle_rebalance* req) {
  return guarded(e, [&] {
    rebal_resident_stage(e, req);
    prof_collect(e);
  });
}
int cook_cycle_rebalance_fetch(cook_engine* e, cook_preemption* decisions, uint32_t* n_decisions, uint32_t* preempted_task_idx,
                               uint32_t* n_preempted, double* pending_dru, uint32_t* selected_task_idx, uint32_t* selected_pending_ord,
                               uint32_t* n_selected) {
  if (n_decisions) *n_decisions = 0;
  if (n_preempted) *n_preempted = 0;
  if (n_selected) *n_selected = 0;
  return guarded(e, [&] {
    rebal_resident_fetch(e, decisions, n_decisions, preempted_task_idx, n_preempted, pending_dru, selected_task_idx, selected_pending_ord,
                         n_selected);
    prof_collect(e);
  });
}

int cook_match_explain(cook_engine* e, const uint32_t* job_pos, uint32_t n, uint32_t* counts) {
  return guarded(e, [&] {
    match_explain(e, bufs(e->xb), job_pos, n, counts);
    prof_collect(e);
  });
}
int cook_match_launch_resources(cook_engine* e, const cook_launch_offers* offers, cook_launch_out* out, cook_launch_info* info) {
  return guarded(e, [&] {
    launch_resources(e, offers, out, info);
    prof_collect(e);
  });
}
int cook_match_metrics(cook_engine* e, cook_cycle_metrics* out, uint32_t* user_considerable, uint32_t* user_matched, uint32_t n_users,
                       int64_t* job_gpus_by_model, int64_t* offer_gpus_by_model, uint32_t n_gpu_models) {
  return guarded(e, [&] {
    match_metrics(e, bufs(e->xb), out, user_considerable, user_matched, n_users, job_gpus_by_model, offer_gpus_by_model, n_gpu_models);
    prof_collect(e);
  });
}
int cook_match_metrics_multi(cook_engine** engines, uint32_t n, const cook_metrics_req* req, int* rc) {
  if (!engines || n == 0 || !req) return COOK_E_INVALID;
  if (!engines_valid(engines, n, false)) return COOK_E_INVALID;
  return run_pools_batched(
      engines, n,
      [&](uint32_t i) {
        const cook_metrics_req& r = req[i];
        return cook_match_metrics(engines[i], r.out, r.user_considerable, r.user_matched, r.n_users, r.job_gpus_by_model, r.offer_gpus_by_model,
                                  r.n_gpu_models);
      },
      [&](uint32_t i) {
        const cook_metrics_req& r = req[i];
        match_metrics(engines[i], bufs(engines[i]->xb), r.out, r.user_considerable, r.user_matched, r.n_users, r.job_gpus_by_model,
                      r.offer_gpus_by_model, r.n_gpu_models);
      },
      /*rank_part=*/false, rc);
}
int cook_batch_stats(const cook_engine* lead, uint32_t out[5]) {
  if (!lead || !out) return COOK_E_INVALID;
  for (unsigned k = 0; k < 5u; ++k) out[k] = lead->any_batch_stats[k];
  return COOK_OK;
}

int cook_offers_stage(cook_engine* e, const cook_nodes* nodes, const cook_pods* pods, const cook_offer_params* params) {
  return guarded(e, [&] {
    if (e->ptb) e->ptb->drop_ids();  // (the pods' ids go with the table they named)
    offers_stage(e, bufs(e->ofb), nodes, pods, params);
  });
}
int cook_offers_stage_pod_ids(cook_engine* e, const uint32_t* pod_id, uint32_t n, uint32_t id_cap) {
  return guarded(e, [&] { podtable_stage_ids(e, pod_id, n, id_cap); });
}
int cook_offers_update(cook_engine* e, const cook_pod_delta* d) {
  return guarded(e, [&] {
    podtable_update(e, d);
    prof_collect(e);
  });
}
int cook_offers_update_info(cook_engine* e, cook_pod_delta_info* out) {
  return guarded(e, [&] { podtable_info(e, out); });
}
int cook_offers_fetch_pods(cook_engine* e, cook_pod_rows* out) {
  return guarded(e, [&] { podtable_fetch(e, out); });
}
int cook_cycle_set_built_offers(cook_engine* e, int with_task_limits) {
  return guarded(e, [&] {
    podq_set_built_offers(e, with_task_limits);
    prof_collect(e);
  });
}
int cook_offers_run(cook_engine* e) {
  return guarded(e, [&] {
    OfferBufs& b = bufs(e->ofb);
    StageTimer t(e, 0, &b.ms);
    offers_run(e, b);
    t.stop();
    prof_collect(e);
  });
}
int cook_offers_fetch(cook_engine* e, cook_node_offers* offers, uint32_t* n_offers, uint8_t* node_status, cook_offer_totals* totals,
                      int64_t* gpu_capacity_by_model, int64_t* gpu_consumed_by_model, double* disk_capacity_by_type,
                      double* disk_consumed_by_type) {
  if (n_offers) *n_offers = 0;
  return guarded(e, [&] {
    offers_fetch(e, bufs(e->ofb), offers, n_offers, node_status, totals, gpu_capacity_by_model, gpu_consumed_by_model,
                 disk_capacity_by_type, disk_consumed_by_type);
  });
}
int cook_offers_build(cook_engine* e, const cook_nodes* nodes, const cook_pods* pods, const cook_offer_params* params,
                      cook_node_offers* offers, uint32_t* n_offers, uint8_t* node_status, cook_offer_totals* totals,
                      int64_t* gpu_capacity_by_model, int64_t* gpu_consumed_by_model, double* disk_capacity_by_type,
                      double* disk_consumed_by_type) {
  if (n_offers) *n_offers = 0;  // "no offers" on any error path
  int rc = cook_offers_stage(e, nodes, pods, params);
  if (rc) return rc;
  rc = cook_offers_run(e);
  if (rc) return rc;
  return cook_offers_fetch(e, offers, n_offers, node_status, totals, gpu_capacity_by_model, gpu_consumed_by_model, disk_capacity_by_type,
                           disk_consumed_by_type);
}
int cook_offers_timing(cook_engine* e, double* ms) {
  if (!e || !ms) return COOK_E_INVALID;
  *ms = e->ofb ? e->ofb->ms : 0.0;
  return COOK_OK;
}

int cook_last_timing(cook_engine* e, double* rank_ms, double* match_ms) {
  if (!e) return COOK_E_INVALID;
  if (rank_ms) *rank_ms = e->rank_ms;
  if (match_ms) *match_ms = e->match_ms;
  return COOK_OK;
}
int cook_match_stats(cook_engine* e, uint32_t out[16]) {
  if (!e || !out) return COOK_E_INVALID;
  const WinCtl& c = e->last_ctl;
  out[0] = c.rounds;
  out[1] = c.matched;
  out[2] = c.stop_list;
  out[3] = c.stop_full;
  out[4] = c.stop_group;
  out[5] = c.stop_window;
  out[6] = c.segments;
  out[7] = c.head;
  out[8] = (uint32_t)(c.t_setup / 100ull);  // microseconds
  out[9] = (uint32_t)(c.t_seq / 100ull);
  out[10] = c.touched_sum;
  out[11] = c.visited_sum;
  out[12] = out[13] = out[14] = out[15] = 0u;
  return COOK_OK;
}
int cook_match_stats_ex(cook_engine* e, uint32_t* out, uint32_t cap) {
  if (!e || !out) return COOK_E_INVALID;
  uint32_t v[COOK_MATCH_STATS_EX_N];
  for (auto& x : v) x = 0u;
  const int rc = cook_match_stats(e, v);
  if (rc) return rc;
  const WinCtl& c = e->last_ctl;
  v[16] = c.trunc_lists;
  v[17] = e->served.mode, v[18] = e->served.pools, v[19] = e->served.iterations, v[20] = e->served.empty_iterations;
  v[21] = e->served.pools_served, v[22] = (uint32_t)(e->served.latch_wait_ms * 1000.0), v[23] = e->served.fell_back, v[24] = e->served.servers;
  v[26] = e->upd_us, v[27] = e->upd_sync_us, v[28] = e->upd_allocs;
  for (unsigned k = 0; k < 8u; ++k)
    if (e->upd_phase_us[k] > v[30]) v[29] = k, v[30] = e->upd_phase_us[k];
  for (unsigned k = 0; k < 5u; ++k) v[32 + k] = e->batch_stats[k];
  v[31] = e->q_advance_us;
  v[37] = e->last_form, v[38] = e->cf_inelig, v[39] = e->spread_serial_calls;
  if (e->last_form == 3u)
    for (unsigned k = 0; k < 24u; ++k) v[40 + k] = e->cf_stats[k];
  if (g_guard) {  // COOK_GUARD=1: look at the bands of every live buffer now, this engine's among them; the count is process-wide and includes buffers already freed
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    guard_check_live();
    v[25] = g_guard_hits.load();
  }
  uint32_t n = 0;
  for (; n < cap && n < (uint32_t)COOK_MATCH_STATS_EX_N; ++n) out[n] = v[n];
  return (int)n;
}
COOK_EMU_EXTRA_EXPORTS
int cook_set_profiling(cook_engine* e, int enabled) {
  if (!e) return COOK_E_INVALID;
  e->profiling = enabled != 0;
  e->kstats.clear();
  return COOK_OK;
}
int cook_kernel_timings(cook_engine* e, const char** names, double* ms, uint32_t* launches, uint32_t cap) {
  if (!e) return COOK_E_INVALID;
  e->kstat_names.clear();
  for (auto& kv : e->kstats) e->kstat_names.push_back(kv.first);
  uint32_t n = 0;
  for (auto& nm : e->kstat_names) {
    if (n >= cap) break;
    names[n] = nm.c_str();
    ms[n] = e->kstats[nm].ms;
    launches[n] = e->kstats[nm].launches;
    ++n;
  }
  return (int)n;
}

}  // extern "C"
