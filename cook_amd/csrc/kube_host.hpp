// kube_host.hpp — host orchestration of cook_kube_distribute and cook_cycle_run_kube (included by engine.hip inside its anonymous
// namespace, behind cycle_host.hpp).  cook_kube_distribute is stateless: the call uploads its own columns into KubeBufs and touches no rank, considerable, match, offers or rebalance state.
// One launch (the walk and the lists), one synchronisation: the counts ride in h_scratch, the choices and the lists come back with them.
#pragma once
#include "kube_kernels.hpp"

struct KubeBufs {
  DArr<uint32_t> location, rank, lists, task;
  DArr<double> draw;
  DArr<uint8_t> choice;        // cook_kube_distribute's own (scratch)
  DArr<uint8_t> cycle_choice;  // the last Kubernetes cycle's record: only cook_cycle_run_kube writes it, cook_cycle_fetch_kube reads it
  DArr<KubeOut> out;
};
static_assert(sizeof(KubeOut) <= 64 * 8, "the distribution's counts ride in h_scratch");
static_assert(KUBE_MAX_CLUSTERS == COOK_MAX_CLUSTERS && KUBE_TILE == COOK_KUBE_TILE && KUBE_NONE == COOK_KUBE_NO_CLUSTER &&
                  KUBE_MAX_CLUSTERS < KUBE_TILE,
              "cookmatch.h states the distributor's shapes");

// (reduce + capacities) of :1767 in int64, saturating
static int64_t kube_available(const cook_kube_clusters* cl) {
  int64_t s = 0;
  for (unsigned c = 0; c < cl->n; ++c)
    if (__builtin_add_overflow(s, cl->capacity[c], &s)) s = cl->capacity[c] < 0 ? INT64_MIN : INT64_MAX;
  return s;
}

// ---- what the stateless call and the cycle share: the checks of the cluster table and the outputs, the table in the kernel arguments,
//      and the way from the kernel's result block to the caller's outputs -------------------------------------------------------------
static void kube_check_clusters(cook_engine* e, const std::string& who, const cook_kube_clusters* cl, const uint32_t* cluster_off,
                                const cook_kube_cluster_info* cinfo) {
  if (!cl) e->fail(COOK_E_INVALID, who + ": null clusters");
  if (cl->n > COOK_MAX_CLUSTERS) e->fail(COOK_E_INVALID, who + ": clusters->n > COOK_MAX_CLUSTERS");
  if (cl->n && (!cl->location || !cl->capacity)) e->fail(COOK_E_INVALID, who + ": a column of clusters is NULL");
  if (!cluster_off || (cl->n && !cinfo)) e->fail(COOK_E_INVALID, who + ": null cluster_off / cluster_info");
}
static void kube_check_draws(cook_engine* e, const std::string& who, const double* draw, uint32_t K) {
  for (uint32_t k = 0; draw && k < K; ++k)
    if (!(draw[k] >= 0.0 && draw[k] < 1.0)) e->fail(COOK_E_INVALID, who + ": draw " + std::to_string(k) + " is NaN or outside [0, 1)");
}
static KubeClusterTab kube_tab(const cook_kube_clusters* cl) {
  KubeClusterTab tab{};
  tab.n = cl->n;
  for (unsigned c = 0; c < cl->n; ++c) {
    tab.location[c] = cl->location[c];
    tab.capacity[c] = cl->capacity[c] <= 0 ? 0u : (uint32_t)std::min<int64_t>(cl->capacity[c], 0xFFFFFFFFll);
  }
  return tab;
}
// the result block as read back into h_scratch; the pass bound's error word comes first
static KubeOut kube_read_out(cook_engine* e, const std::string& who) {
  KubeOut h;
  std::memcpy(&h, e->h_scratch, sizeof(KubeOut));
  if (h.err) e->fail(COOK_E_DEVICE, who + ": the walk reached its pass bound (" + std::to_string(h.passes) + " passes): an internal error");
  return h;
}
// counts -> cluster_off, cluster_info, info (whose gate fields the caller has set); then the two checks that can still fail the call
static void kube_fill_outputs(cook_engine* e, const std::string& who, const KubeOut& h, const cook_kube_clusters* cl, uint32_t K, uint32_t cap,
                              uint32_t* cluster_off, cook_kube_cluster_info* cinfo, cook_kube_info* info) {
  cluster_off[0] = 0;
  for (unsigned c = 0; c < cl->n; ++c) {
    cinfo[c] = cook_kube_cluster_info{h.assigned[c], 0u, cl->capacity[c]};
    cluster_off[c + 1] = cluster_off[c] + h.assigned[c];
  }
  if (info) {
    info->n_considered = K;
    info->launched = h.launched, info->no_cluster = h.no_cluster, info->exhaustions = h.exhaustions;
    info->n_first = std::min(h.no_cluster, KUBE_FIRST_TEN);
    for (unsigned x = 0; x < info->n_first; ++x) info->first_task[x] = h.first_task[x];
  }
  if (h.launched != cluster_off[cl->n] || (uint64_t)h.launched + h.no_cluster != K) e->fail(COOK_E_STATE, who + ": the lists' lengths do not add up");
  if (h.launched > cap) e->fail(COOK_E_INVALID, who + ": the lists hold more than cap entries");
}

void kube_distribute_run(cook_engine* e, uint32_t K, const uint32_t* location, const double* draw, uint64_t seed, const cook_kube_clusters* cl,
                         uint8_t* choice, uint32_t* pos_idx, uint32_t cap, uint32_t* cluster_off, cook_kube_cluster_info* cinfo,
                         cook_kube_info* info) {
  const std::string who = "cook_kube_distribute";
  // ---- everything the host can know, in front of the first launch -------------------------------------------------------------------
  if (K > (uint32_t)INT32_MAX) e->fail(COOK_E_INVALID, who + ": n_jobs > INT32_MAX");
  kube_check_clusters(e, who, cl, cluster_off, cinfo);
  if (K && !choice) e->fail(COOK_E_INVALID, who + ": null choice");
  if (cap && !pos_idx) e->fail(COOK_E_INVALID, who + ": null pos_idx");
  kube_check_draws(e, who, draw, K);
  // ---- one launch: the walk and the lists (every buffer it writes is this call's own: the last cycle's record stays) ----------------------
  KubeBufs& b = bufs(e->kub);
  KubeOut* out = b.out.ensure(1);
  const uint32_t* d_loc = K ? h2d_opt(e, b.location, location, K) : nullptr;
  const double* d_draw = K ? h2d_opt(e, b.draw, draw, K) : nullptr;
  uint8_t* d_choice = b.choice.ensure(K);
  KM<kube_distribute, KUBE_TILE>(e, "kube_distribute", 1u, kube_tab(cl), d_loc, d_draw, (unsigned long long)seed, (const uint32_t*)nullptr, (unsigned)K,
                                 d_choice, b.rank.ensure(K), b.lists.ensure(K), out, (int32_t*)nullptr, (unsigned*)nullptr);
  pinned_copy(e, e->h_scratch, out, sizeof(KubeOut), hipMemcpyDeviceToHost);
  if (K) copy_async(e, choice, d_choice, K, hipMemcpyDeviceToHost);
  const unsigned n_copy = std::min<unsigned>(K, cap);  // (the lists are no longer than the jobs)
  if (n_copy) copy_async(e, pos_idx, b.lists.ptr(), (size_t)n_copy * 4, hipMemcpyDeviceToHost);
  sync(e);
  const KubeOut h = kube_read_out(e, who);
  if (info) *info = cook_kube_info{}, info->available = kube_available(cl), info->max_considerable = K;
  kube_fill_outputs(e, who, h, cl, K, cap, cluster_off, cinfo, info);
}

// ---- cook_cycle_run_kube: gate -> (rank | queue step, remove_mode 1) -> considerable filters -> the distributor over the considered jobs ----
// Included behind cycle_host.hpp.  Synchronisations: those of the front part, then ONE for the result block (h_scratch) and the lists.
// The distributor writes job_to_offer = 0 / -1 for launched / not launched jobs: carry_kept, lim_count_kept, resv_release and
// q_mark_removed of the NEXT advance then read the launched jobs as kept placements with no change of their own (there is no offer
// table, so no offer_skipped); e->kube_last keeps that advance from folding cotasks and the readers of a placement away.
struct KubeGate {
  int64_t available;
  uint32_t max_considerable;
  bool paused;
};
static KubeGate kube_gate(const cook_kube_cycle* c) {
  const int64_t av = kube_available(c->clusters);
  const uint64_t room = av > 0 ? (uint64_t)av : 0u;
  return KubeGate{av, (uint32_t)std::min<uint64_t>(c->max_jobs_considered, std::min<uint64_t>(room, 0xFFFFFFFFull)), !(av > c->min_capacity_threshold)};
}

void cycle_run_kube(cook_engine* e, const cook_kube_cycle* c, uint32_t* task_idx, uint32_t cap, uint32_t* cluster_off,
                    cook_kube_cluster_info* cinfo, cook_kube_info* info) {
  // ---- everything the host can know, in front of the first launch -------------------------------------------------------------------
  const std::string who = "cook_cycle_run_kube";
  if (!c) e->fail(COOK_E_INVALID, who + ": null cycle");
  const cook_kube_clusters* cl = c->clusters;
  kube_check_clusters(e, who, cl, cluster_off, cinfo);
  const unsigned n = cl->n;
  if (cap && !task_idx) e->fail(COOK_E_INVALID, "cook_cycle_run_kube: null task_idx");
  if (c->rank_first > 1u) e->fail(COOK_E_INVALID, "cook_cycle_run_kube: rank_first is 0 or 1");
  if ((c->step && c->step->offers) || (c->carry && c->carry->offers) || (c->finished && c->finished->offers))
    e->fail(COOK_E_INVALID, "cook_cycle_run_kube: step->offers, carry->offers = 1 and finished->offers = 1 are refused: a Kubernetes-scheduler pool has no offer table to edit");
  const KubeGate g = kube_gate(c);
  if (c->draw) {
    if (c->n_draw < g.max_considerable) e->fail(COOK_E_INVALID, "cook_cycle_run_kube: n_draw < max_considerable");
    kube_check_draws(e, who, c->draw, g.max_considerable);
  }
  if (e->placement.state == cook_engine::Placement::ROUNDS || e->placement.state == cook_engine::Placement::WALK)
    e->fail(COOK_E_STATE, "cook_cycle_run_kube between a deferred set-up (cook_cycle_run_rank*) and cook_cycle_match_multi");
  cluster_off[0] = 0;
  for (unsigned x = 0; x < n; ++x) cinfo[x] = cook_kube_cluster_info{0u, 0u, cl->capacity[x]}, cluster_off[x + 1] = 0;
  if (info) *info = cook_kube_info{}, info->available = g.available, info->max_considerable = g.max_considerable, info->paused = g.paused ? 1u : 0u;
  if (g.paused) return;  // (:1801-1808: nothing ran, nothing changed)
  // ---- the front part: a fresh rank, or the advance with every considered job leaving the queue; the filters; take ----------------------
  unsigned K;
  if (c->rank_first) {
    K = cycle_rank_part(e, g.max_considerable);
  } else {
    cook_queue_step s = c->step ? *c->step : cook_queue_step{};
    s.remove_mode = 1u;
    K = cycle_queue_part(e, QueueArgs{&s, c->carry, c->finished, nullptr, nullptr}, g.max_considerable);
  }
  // ---- no placement: the cycle's record is (positions, job_to_offer = launched ? 0 : -1) ------------------------------------------------
  e->placement_drop();
  e->last_in_valid = false;
  e->v_in_is_last = false;
  WinCtl no_rounds{};
  no_rounds.head = K;
  KubeBufs& b = bufs(e->kub);
  KubeOut* out = b.out.ensure(1);
  uint32_t* d_task = b.task.ensure(K);
  uint32_t* d_loc = b.location.ensure(K);
  if (K)
    KM<kube_gather, 256>(e, "kube_gather", div_up(K, 256), e->q_last_pos, (const uint32_t*)e->ranked.ptr(), (const uint32_t*)e->j_index.ptr(),
                         e->min.j_ckpt ? (const uint32_t*)e->j_ckpt.ptr() : (const uint32_t*)nullptr, K, d_task, d_loc);
  const double* d_draw = (K && c->draw) ? h2d_opt(e, b.draw, c->draw, K) : nullptr;
  KM<kube_distribute, KUBE_TILE>(e, "kube_distribute", 1u, kube_tab(cl), (const uint32_t*)d_loc, d_draw, (unsigned long long)c->seed, (const uint32_t*)d_task, K,
                                 b.cycle_choice.ensure(K), b.rank.ensure(K), b.lists.ensure(K), out, e->m_j2o.ensure(K), e->m_summary.ensure(4));
  pinned_copy(e, e->h_scratch, out, sizeof(KubeOut), hipMemcpyDeviceToHost);
  const unsigned n_copy = std::min<unsigned>(K, cap);
  if (n_copy) copy_async(e, task_idx, b.lists.ptr(), (size_t)n_copy * 4, hipMemcpyDeviceToHost);
  sync(e);
  const KubeOut h = kube_read_out(e, who);
  e->placement_complete(0, no_rounds);
  e->cycle_considered = K;
  e->kube_last = true;
  kube_fill_outputs(e, who, h, cl, K, cap, cluster_off, cinfo, info);
}

void cycle_fetch_kube(cook_engine* e, uint8_t* choice, uint32_t* n_out) {
  if (!e->kube_last || !e->match_ran() || !e->kub) e->fail(COOK_E_STATE, "cook_cycle_fetch_kube: the last cycle was no Kubernetes cycle");
  const unsigned K = e->cycle_considered;
  if (K && choice) copy_async(e, choice, e->kub->cycle_choice.ptr(), K, hipMemcpyDeviceToHost);
  sync(e);
  if (n_out) *n_out = K;
}
