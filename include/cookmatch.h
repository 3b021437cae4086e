/*
 * cookmatch.h — C ABI of libcookmatch.so, the MI355X (gfx950) fair-share match engine.
 *
 * This is the drop-in boundary for ONE path of twosigma/Cook: per-cycle DRU ranking, the jobs x offers
 * feasibility/constraint evaluation, rank-ordered bin-pack placement (what Cook delegates to Netflix Fenzo's
 * TaskScheduler.scheduleOnce) and the rebalancer's preemption decisions.  The reference has no FFI on this
 * path; each entry point below names the Clojure function(s) it replaces (paths relative to the reference's
 * scheduler/ directory).  INTEGRATION.md shows the JNI binding a Cook maintainer would add.
 *
 * Conventions
 *  - Plain C.  No exceptions, no callbacks, no torch types.  All buffers are caller-allocated SoA arrays.
 *  - Identity: users, hosts, attribute keys/values, gpu models, disk types, groups, locations are dense
 *    uint32 ids interned by the host (Clojure keeps id->entity tables).  The engine never sees strings.
 *    USER IDS AND HOST IDS MUST BE ASSIGNED IN ASCENDING NAME ORDER (java String.compareTo): the reference
 *    breaks ties by user name (dru.clj:123, rebalancer.clj:252-256) and orders hosts by name
 *    (rebalancer.clj:383).
 *  - Every function returns COOK_OK (0) or a negative COOK_E_* code; cook_last_error() has the message.
 *    On error the outputs are "no ranking / no matches / no decisions", so the Clojure caller's
 *    catch-Throwable path (scheduler.clj:1521-1535) can restore its offers exactly as today.
 *  - A handle is NOT re-entrant: hold the mutual exclusion the reference holds on the Fenzo object
 *    ((locking fenzo ...), scheduler.clj:665).  Distinct handles (pools) may be used from distinct threads.
 *  - The engine is stateless across calls except for buffers it caches on the device; everything that
 *    Fenzo's TaskTracker would remember (tasks already running on a host) is passed in by the caller.
 *  - All arithmetic on the path is IEEE fp64, round-to-nearest, no flush-to-zero (share.clj:95 makes
 *    DRUs of magnitude 1e-305 legal).
 */
#ifndef COOKMATCH_H
#define COOKMATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the functions declared here are the library's ONLY exports: libcookmatch.so is built with -fvisibility=hidden */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define COOK_OK 0
#define COOK_E_INVALID (-1) /* bad argument / inconsistent sizes            */
#define COOK_E_DEVICE (-2)  /* HIP runtime error (message has the hipError) */
#define COOK_E_NOMEM (-3)
#define COOK_E_STATE (-4)   /* call order violated (run before stage ...)   */

#define COOK_NONE_U32 0xFFFFFFFFu

typedef struct cook_engine cook_engine; /* opaque; one per pool */

/* ---- knobs (every hot-path configuration value of the reference) ------------------------- */
typedef struct cook_params {
  int32_t dru_mode;            /* 0 = :pool.dru-mode/default (cpus,mem), 1 = :pool.dru-mode/gpu (scheduler.clj:2178-2183) */
  int32_t max_over_quota_jobs; /* config.clj:413-416, default 100 (scheduler.clj:2057-2071)                     */
  double offensive_max_mem_mb; /* task-constraints :memory-gb * 1024.0 (scheduler.clj:2219); +inf disables      */
  double offensive_max_cpus;   /* task-constraints :cpus (scheduler.clj:2198-2203); +inf disables               */
  double good_enough_fitness;  /* config.clj:111 default 0.8; (> fitness x) at scheduler.clj:2312-2314; >=1 = off */
  int64_t host_lifetime_mins;  /* estimated-completion-config :host-lifetime-mins (constraints.clj:392-397)     */
  int32_t match_algo;          /* 0 = engine default (= 2; = 3 when six or more engines share the device, COOK_CLASSFIT=0 / 1 forbids /
                                  forces that), 1 serial sweep (one workgroup, one job at a time: the reference form of the
                                  chain), 2 window rounds (eval / merge / resolve launches), 3 class-ordered best fit (one workgroup per pool,
                                  no evaluation launches) where the call's numbers and constraints allow it, else as 2.
                                  Other values: COOK_E_INVALID.  Identical results */
  int32_t fitness;             /* :fenzo-fitness-calculator of the pool (config.clj:108 default cpuMemBinPacker; docs/configuration.adoc:263-264).
                                  With cf = (run_cpus + assigned_cpus + job.cpus) / (offer.cpus + run_cpus) and mf the same over mem:
                                  Fenzo 0.10.0's own BinPackingFitnessCalculators: 0 = cpuMemBinPacker (cf + mf) / 2.0, 1 = cpuBinPacker cf,
                                  2 = memoryBinPacker mf; their spreading counterparts: 3 = cpuMemSpreader ((1.0 - cf) + (1.0 - mf)) / 2.0,
                                  4 = cpuSpreader 1.0 - cf, 5 = memorySpreader 1.0 - mf.  The spreaders' arithmetic (the operations and their
                                  order, as written here) is oracle-defined, as the tie order between offers already is: Fenzo's source is
                                  not part of the reference tree.  A fitness that is not > 0.0 is a failure under every calculator (a spreader
                                  refuses the offer a job would fill to the brim); winner, ties and good-enough as under cook_match below.
                                  match_algo 3 / the engine's own choice of it serve fitness 0 only (else window rounds); the spreaders are
                                  placed by the serial sweep whatever match_algo says (cook_match_stats_ex [39] counts those calls).
                                  networkBinPacker / cpuMemNetworkBinPacker: not offered.
                                  Other values: COOK_E_INVALID from cook_engine_create and cook_engine_set_params.  (This field was `reserved`,
                                  always 0, before: the layout and COOK_ABI_VERSION are unchanged.) */
} cook_params;
#define COOK_FITNESS_CPU_MEM_BIN_PACKER 0
#define COOK_FITNESS_CPU_BIN_PACKER 1
#define COOK_FITNESS_MEMORY_BIN_PACKER 2
#define COOK_FITNESS_CPU_MEM_SPREADER 3
#define COOK_FITNESS_CPU_SPREADER 4
#define COOK_FITNESS_MEMORY_SPREADER 5
#define COOK_FITNESS_N 6

/* ---- resource 4-vector used for quotas and usage: {count, cpus, mem, gpus} (tools.clj:883-889) ---------- */
typedef struct cook_usage {
  double count, cpus, mem, gpus;
} cook_usage;

/* ---- tasks: running instances ++ synthetic tasks for pending jobs (tools.clj:582-588) ------------------- */
typedef struct cook_tasks {
  uint32_t n;
  const double* cpus;      /* job resources (tools.clj:247-273)                                        */
  const double* mem;
  const double* gpus;      /* may be NULL (all 0.0)                                                    */
  const uint32_t* user;    /* user id = rank of the user name                                          */
  const int32_t* priority; /* :job/priority, default 50 (tools.clj:612)                                */
  const int64_t* start_ms; /* :instance/start-time in ms; ignored for pending (treated as Long.MAX)    */
  const int64_t* task_id;  /* :db/id of the instance; ignored for pending (nil sorts first)            */
  const int64_t* job_id;   /* :db/id of the job                                                        */
  const uint8_t* pending;  /* 1 = synthetic task of a waiting job, 0 = running instance                */
  const uint32_t* host;    /* running: host id (cook_rebalance; kept resident by cook_cycle_stage / cook_cycle_update for
                              cook_cycle_rebalance_stage); may be NULL for cook_rank; never read for pending rows */
} cook_tasks;

/* ---- users: DRU divisors (share.clj:75-119,189-210) and quotas (quota.clj:272-295) ---------------------- */
typedef struct cook_users {
  uint32_t n;
  const double* div_cpus; /* share, Double.MAX_VALUE when unset                                         */
  const double* div_mem;
  const double* div_gpus;
  const double* quota_count; /* quota per resource, Double.MAX_VALUE (count: 2^31-1) when unset          */
  const double* quota_cpus;
  const double* quota_mem;
  const double* quota_gpus;
} cook_users;

/* ---- pool-level quota inputs of filter-based-on-quota (scheduler.clj:2134-2157) ------------------------- */
typedef struct cook_pool_quota {
  int32_t has_pool_quota; /* 0: (tools/global-pool-quota pool) is nil -> no filtering (tools.clj:925)    */
  int32_t has_group_quota;
  cook_usage pool_quota;
  cook_usage group_quota;
  cook_usage group_usage; /* aggregate-quota-groups over the member pools (scheduler.clj:2125-2132);
                             the cross-pool sum is the only collective on the path (RCCL all-reduce)   */
  int32_t pool_usage_given; /* 0: engine computes the pool's running usage itself (scheduler.clj:2173)  */
  int32_t reserved;
  cook_usage pool_usage;
} cook_pool_quota;

/* ---- the ranked queue and the per-user state of pending-jobs->considerable-jobs (scheduler.clj:729-762) --- */
typedef struct cook_queue { /* the pool's pending jobs in rank order (the output of cook_rank) */
  uint32_t n;
  const double* cpus;
  const double* mem;
  const double* gpus;      /* may be NULL */
  const uint32_t* user;
  const uint8_t* eligible; /* job-allowed-to-start? (scheduler.clj:747) AND the launch-plugin filter (:748), both
                              evaluated by the host; NULL = all eligible */
} cook_queue;

typedef struct cook_user_state {
  uint32_t n;                 /* users */
  const double* quota_count;  /* user->quota (quota.clj:272-295) */
  const double* quota_cpus;
  const double* quota_mem;
  const double* quota_gpus;
  const double* usage_count;  /* user->usage of the pool's running jobs (scheduler.clj:715-727); 0 for users without any */
  const double* usage_cpus;
  const double* usage_mem;
  const double* usage_gpus;
  const int64_t* tokens_left; /* ratelimit/get-token-count! of the per-user-per-pool launch rate limiter
                                 (tools.clj:943-945); NULL = no limiter (every job counts as passed) */
  int32_t enforce_rate_limit; /* ratelimit/enforce? (tools.clj:936) */
  int32_t has_pool_quota;     /* 0: (tools/global-pool-quota pool) is nil -> no pool filtering (tools.clj:925) */
  cook_usage pool_quota;
  int32_t pool_usage_given;   /* 0: the engine sums the users' usage itself in user-id order (tools.clj:966; the
                                 reference sums in hash-map order, which only matters for non-integer usages) */
  int32_t reserved;
  cook_usage pool_usage;
} cook_user_state;

/* ---- considerable jobs, in rank order (scheduler.clj:729-762, 456-509) ---------------------------------- */
typedef struct cook_jobs {
  uint32_t n;
  const double* cpus;
  const double* mem;
  const double* gpus;            /* may be NULL                                                         */
  const uint32_t* gpu_model;     /* requested model id (constraints.clj:96-103); 0 = none; may be NULL  */
  const uint32_t* user;          /* may be NULL for cook_match                                          */
  const uint32_t* group;         /* group id or COOK_NONE_U32; may be NULL                              */
  const uint32_t* eq_off;        /* CSR [n+1] of user-defined EQUALS constraints (constraints.clj:356)  */
  const uint32_t* eq_key;        /*   attribute key id                                                  */
  const uint32_t* eq_val;        /*   required value id                                                 */
  const uint32_t* novel_off;     /* CSR [n+1] of hosts the job already ran on (constraints.clj:68-94)   */
  const uint32_t* novel_host;
  const int32_t* reserved_host;  /* host reserved FOR this job by the rebalancer, -1 none (scheduler.clj:645-653) */
  const uint32_t* ckpt_location; /* location id of last checkpoint, 0 = none (constraints.clj:201-240)  */
  const int64_t* est_end_ms;     /* estimated end time, 0 = no constraint (constraints.clj:385-431)     */
  const double* disk_request;    /* MiB, <0 = constraint not in effect (constraints.clj:164-199)        */
  const uint32_t* disk_type;
  /* Fenzo's remaining additive resource dimensions (TaskRequestAdapter getPorts / getScalarRequests, scheduler.clj:456-471) */
  const int32_t* ports;          /* (:ports resources) = :job/ports, the NUMBER of ports asked for (tools.clj:271); may be
                                    NULL (all 0)                                                        */
  uint32_t n_scalars;            /* named scalar requests (job->scalar-request, scheduler.clj:177-189): column s is the
                                    request under name s of the caller's name table (<= COOK_MAX_SCALARS names)        */
  uint32_t reserved_;
  const double* scalars;         /* n_scalars columns of n doubles (column s at scalars + s * n); NaN = the job has no
                                    request under that name; may be NULL                                               */
} cook_jobs;
/* Which named scalars a binding has to pass: job->scalar-request yields every :job/resource that carries :resource/amount
 * except gpus, i.e. "cpus" and "mem" (the disk resource stores :resource.disk/request, not an amount: api.clj:818-830), and
 * whatever legacy or custom resource types a deployment's database holds ("disk" among them).  Fenzo tests each as
 * used + request > total against the lease's getScalarValues (offer.clj:57-65) and sums the placed requests by name.  For "cpus"
 * and "mem" that is the SAME comparison on the SAME operands as the cpus / mem test when the TaskRequest's cpus / mem are the
 * job's own (no job-resource-adjustments for the pool, scheduler.clj:473-479): such columns are redundant and need not be
 * passed.  With an adjuster, pass the un-adjusted amounts as scalars 0 / 1 and the adjusted ones as cpus / mem. */
#define COOK_MAX_SCALARS 3

/* ---- offers, one per host (offer.clj:31-76), plus Fenzo's view of tasks already on that host ------------ */
typedef struct cook_offers {
  uint32_t n;
  const double* cpus;        /* cpuCores of the lease (offer.clj:55)                                    */
  const double* mem;         /* memoryMB                                                                */
  const uint32_t* host;      /* host id (hostname rank)                                                 */
  const uint8_t* k8s;        /* attr "compute-cluster-type" == "kubernetes"; NULL = all 0               */
  const uint32_t* gpu_model; /* k8s "gpus" text->scalar map, one model per host; 0 = no gpus; may be NULL */
  const double* gpu_count;
  const uint32_t* disk_type; /* k8s "disk" map, one type per host; may be NULL                          */
  const double* disk_space;
  uint32_t n_attr_keys;      /* attribute table is [n][n_attr_keys], value id 0 = attribute absent      */
  const uint32_t* attr;
  const int32_t* max_tasks;  /* COOK_MAX_TASKS_PER_HOST, -1 absent; may be NULL                         */
  const int32_t* num_tasks;  /* COOK_NUM_TASKS_ON_HOST                                                  */
  const uint32_t* location;  /* COOK_COMPUTE_CLUSTER_LOCATION id; may be NULL                           */
  const int64_t* host_start_s; /* "host-start-time", -1 absent; may be NULL                             */
  const double* run_cpus;    /* sum over tasks Fenzo tracks as running on the host (getTaskAssigner,    */
  const double* run_mem;     /*   scheduler.clj:877-881); NULL = 0                                      */
  const int32_t* run_count;
  /* more than one entry in the k8s "gpus" / "disk" maps of a host (constraints.clj:122-157 reads (get model->count model 0)
     and (count model->count); :164-199 likewise for disk): gpu_model / gpu_count are then [n][gpu_slots] row-major, model 0 =
     empty slot, models distinct within a row; 0 means 1 (the plain per-host columns).  At most COOK_MAX_RES_SLOTS. */
  uint32_t gpu_slots;
  uint32_t disk_slots;       /* likewise disk_type / disk_space as [n][disk_slots]                      */
  const int32_t* ports;      /* number of ports in the lease's "ports" ranges (portRanges, offer.clj:71-73: sum of
                                end - begin + 1); may be NULL (no ports: a job asking for any never fits) */
  uint32_t n_scalars;        /* lease getScalarValues (offer.clj:57-65) under the names of cook_jobs.scalars */
  uint32_t reserved_;
  const double* scalars;     /* n_scalars columns of n doubles: the totals, 0.0 = the lease has no scalar of that name;
                                may be NULL (all 0)                                                      */
} cook_offers;
#define COOK_MAX_RES_SLOTS 4

/* ---- job groups with host-placement constraints (constraints.clj:519-678) ------------------------------- */
typedef struct cook_groups {
  uint32_t n;
  const uint8_t* type;      /* 0 all (none), 1 unique, 2 balanced, 3 attribute-equals                    */
  const uint32_t* attr_key; /* balanced / attribute-equals attribute key id                              */
  const int32_t* minimum;   /* :host-placement.balanced/minimum                                          */
  const uint32_t* run_off;  /* CSR [n+1]: cotasks of the group already running per the DB + Fenzo tracker */
  const uint32_t* run_host; /*   host id of each running cotask                                          */
  const uint32_t* run_attr; /*   value id of attr_key on that host (0 = absent)                          */
} cook_groups;

/* ---- rebalancer ---------------------------------------------------------------------------------------- */
typedef struct cook_rebalance_params { /* rebalancer.clj:535-557 (Datomic :rebalancer/config) */
  double safe_dru_threshold;
  double min_dru_diff;
  int32_t max_preemption;
  int32_t reserved;
} cook_rebalance_params;

typedef struct cook_host_spare { /* host->spare-resources from view-incubating-offers (rebalancer.clj:577-582) */
  uint32_t n;
  const uint32_t* host;
  const double* cpus;
  const double* mem;
  const double* gpus;
} cook_host_spare;

typedef struct cook_preemption { /* one preemption decision (rebalancer.clj:384-404) */
  uint32_t pending_index; /* index into the pending jobs passed in                                       */
  uint32_t host;          /* :hostname                                                                   */
  double dru;             /* :dru of the decision (Double.MAX_VALUE = spare resources only)              */
  double cpus, mem, gpus; /* resources freed on the host                                                 */
  uint32_t task_off;      /* preempted tasks = preempted[task_off .. task_off+task_n)                    */
  uint32_t task_n;
} cook_preemption;

/* ---- lifecycle ------------------------------------------------------------------------------------------ */
int cook_engine_create(const cook_params* params, int device_id, cook_engine** out);
void cook_engine_destroy(cook_engine* e);
int cook_engine_set_params(cook_engine* e, const cook_params* params);
/* e == NULL: why the calling thread's last cook_engine_create refused its params; "null engine" when it did not (a create that
 * failed for a device reason included: its code is all it reports) */
const char* cook_last_error(const cook_engine* e);
const char* cook_version(void);
/* Layout version of the structs and buffer sizes of this header (cook_jobs / cook_offers / cook_offer_params / COOK_WHY_SLOTS changed
 * in 2: ports, named scalars, gpu / disk slot tables, 20 why-slots; 3 adds cook_match_stats_ex and the mask rule of
 * cook_cycle_update; 4: cook_params.match_algo takes 0 / 1 / 2 only, the words [6], [12..17] of the placement statistics changed).
 * A binding compares its compiled-in COOK_ABI_VERSION with the library's before the first call (cook_amd/engine.py load_library,
 * bindings/jni/cookmatch_jni.c Native.create). */
#define COOK_ABI_VERSION 4
int cook_abi_version(void);

/* ---- RANK: replaces sort-jobs-by-dru-helper + filter-based-on-quota + filter-offensive-jobs --------------
 * (scheduler.clj:2073-2091, 2134-2157, 2198-2229; dru.clj:50-126; tools.clj:614-641, 917-933).
 * ranked_pending_idx receives indices into `tasks` of the surviving pending jobs in rank order (capacity =
 * number of pending tasks); dru_of_task (optional, len tasks->n) receives each task's DRU score, NaN for
 * tasks cut by the over-quota limiter.
 * The staged form keeps inputs resident in HBM between cycles: stage (H2D) -> run (kernels only) -> fetch (D2H). */
int cook_rank(cook_engine* e, const cook_tasks* tasks, const cook_users* users, const cook_pool_quota* quota,
              uint32_t* ranked_pending_idx, uint32_t* n_out, double* dru_of_task);
int cook_rank_stage(cook_engine* e, const cook_tasks* tasks, const cook_users* users);
int cook_rank_set_quota(cook_engine* e, const cook_pool_quota* quota);
/* running usage of the pool {count,cpus,mem,gpus} (scheduler.clj:2118-2123, 2173): input to the cross-pool all-reduce */
int cook_rank_pool_usage(cook_engine* e, cook_usage* out);
/* ... of n engines of one device in ONE call from one thread: the pools' sums side by side as pool batches (one launch per kernel for all of them, one
 * stream synchronisation; cook_cycle_run_rank_multi has the mechanism), out[i] for engines[i].  Same numbers as the calls one by one (the reduction order
 * of a pool does not depend on its neighbours).  An engine twice: COOK_E_INVALID. */
int cook_rank_pool_usage_multi(cook_engine** engines, uint32_t n, cook_usage* out /* [n] */);
int cook_rank_run(cook_engine* e);
/* per-user running usage of the pool after cook_rank_run / cook_cycle_run*: usage[u*3 + {0,1,2}] = {cpus, mem, gpus} summed over user
 * u's RUNNING tasks in the user's task order (tools.clj:614-641).  This is the [U x 3] vector BASELINE.json's north_star
 * all-reduces across pools ("cross-pool per-user DRU totals": divide by the user's share, share.clj:189-210); Cook itself
 * keeps usage per pool (scheduler.clj:2167-2194), so no reference function consumes the cross-pool sum.  usage_is_device != 0:
 * `usage` is a DEVICE pointer (e.g. the buffer of the collective): nothing is copied to the host. */
int cook_rank_user_usage(cook_engine* e, double* usage, int usage_is_device);
int cook_rank_fetch(cook_engine* e, uint32_t* ranked_pending_idx, uint32_t* n_out, double* dru_of_task);

/* ---- CONSIDERABLE: replaces pending-jobs->considerable-jobs + tools/filter-pending-jobs-for-quota ----------
 * (scheduler.clj:729-762; tools.clj:654-668, 903-973).  In queue order: per-user quota filter seeded with the user's
 * running usage (state advances on rejected jobs too), launch-rate-limit filter (the n-th surviving job of a user is
 * limited iff n > tokens_left; dropped only when enforcing), pool quota filter seeded with the pool usage, eligible
 * mask, take num_considerable.  considerable_idx receives queue positions (capacity min(num_considerable, queue->n)).
 * rate_limited / passed (optional, len users): per-user counts of the rate-limit stage over the WHOLE queue.  These are UPPER
 * BOUNDS of what the reference stores in pool->user->num-rate-limited-jobs: its lazy pipeline only counts the jobs it consumed
 * (in chunks of 32) before `take num-considerable` was satisfied, so for a queue longer than that the reference's counts stop
 * early.  The considerable jobs themselves do not depend on it.  A caller that shows the counts (the /unscheduled_jobs reason)
 * should present them as "at least one job rate-limited" rather than as exact numbers (oracle-defined). */
int cook_considerable(cook_engine* e, const cook_queue* queue, const cook_user_state* users, uint32_t num_considerable,
                      uint32_t* considerable_idx, uint32_t* n_out, uint32_t* rate_limited, uint32_t* passed);
/* Same filters inside cook_cycle_run, between rank and match, with no host round trip: `users` as above (copied to the
 * device now); eligible_by_pending (optional) is indexed by pending ordinal like cook_cycle_stage's pending_jobs, whose
 * `user` array must be present.  NULL users = plain (take num-considerable) again. */
int cook_cycle_set_considerable(cook_engine* e, const cook_user_state* users, const uint8_t* eligible_by_pending);
/* rank positions of the jobs the last cook_cycle_run considered: cook_cycle_fetch's job_to_offer[k] belongs to the job at
 * ranked_pending_idx[rank_pos[k]] (identity when the considerable filters are off). */
int cook_cycle_fetch_considerable(cook_engine* e, uint32_t* rank_pos, uint32_t* n_out);

/* ---- AUTOSCALE: the pending-job candidates of handle-resource-offers-autoscaling-helper (scheduler.clj:1283-1335) from the last cycle --
 * Reads the pool's last cook_cycle_run (or cook_cycle_run_rank + cook_cycle_match_multi): the ranked queue R, the k considered rank
 * positions C with their job_to_offer, and the user state S staged by cook_cycle_set_considerable.
 *  1. kept matches: the job at C[i] is matched iff job_to_offer[i] >= 0 and offer_skipped[job_to_offer[i]] == 0 (offer_skipped: 1 where
 *     filter-matches-for-ratelimit, :887-924, dropped every match of the offer's compute cluster); m matched, u = k - m unmatched.
 *  2. N (:1288-1306) = max(u, trunc(min(fraction * scale_factor, 1) * max_jobs)), fraction = k > 0 ? (double)(float)u / k : 0.
 *  3. Q' = R without the matched jobs, in order (remove-matched-jobs-from-pending-jobs, :790-795).
 *  4. A = the first N jobs of Q' that pass filter-pending-jobs-for-quota (tools.clj:961-973) under S with fresh rate-limit counters:
 *     user quota seeded with the running usage, launch rate (the n-th survivor of a user is limited iff n > tokens_left, dropped only
 *     when enforcing), pool quota.  The eligible mask is NOT applied (job-allowed-to-start? is the considerable path's only, :747-748).
 *  5. Out = A without the excluded tasks (caches/recent-synthetic-pod-job-uuids, removed after the take, :1319: no refill), in order.
 * task_idx receives Out as task indices (cook_cycle_fetch's ranked_pending_idx space); cap >= max(max_jobs, k) always suffices, |Out| > cap:
 * COOK_E_INVALID (info says |Out|).  An in-range excluded task that is no candidate is ignored; one out of range, a non-finite
 * scale_factor or max_jobs > INT32_MAX: COOK_E_INVALID.  Before any cycle, after a stage / cook_cycle_update / cook_considerable /
 * cook_cycle_set_considerable / cook_match_run that no cycle has followed, and after a cycle without a staged user state: COOK_E_STATE.  Changes no rank,
 * considerable or match state. */
typedef struct cook_autoscale_params {
  uint32_t max_jobs;              /* :max-jobs-for-autoscaling (<= INT32_MAX)                                            */
  uint32_t n_exclude;
  double scale_factor;            /* :autoscaling-scale-factor (finite)                                                  */
  const uint8_t* offer_skipped;   /* [staged offers] or NULL                                                             */
  const uint32_t* exclude_task;   /* [n_exclude] task indices (cook_cycle_fetch's index space) or NULL                   */
} cook_autoscale_params;
typedef struct cook_autoscale_info {
  uint32_t considered, matched, unmatched, scaled /* N */, autoscalable /* |A| */, n_out /* |Out| */;
  double fraction_unmatched;
} cook_autoscale_info;
int cook_cycle_autoscale(cook_engine* e, const cook_autoscale_params* p, uint32_t* task_idx, uint32_t cap, cook_autoscale_info* info);
/* cook_cycle_autoscale for every pool of a GPU in ONE call from one thread: the pools' flows in one pool batch (the mechanism of
 * cook_cycle_run_rank_multi), so the pools share every stream synchronisation and launch the same kernel once.  Engine i's result
 * is exactly what cook_cycle_autoscale(engines[i], params[i], task_idx[i], cap[i], &info[i]) gives: outputs, info, error code and message,
 * state rule.  Returns the first engine's code that is not COOK_OK; rc[i], when given, is engine i's code; every engine keeps its own
 * cook_last_error; an engine that fails (COOK_E_STATE, a bad exclude index, |Out| > cap with info still filled ...) does not spoil the
 * others.  COOK_E_INVALID with nothing run: engines, params or cap NULL, n == 0, a NULL entry of engines or params, an engine twice.
 * One after another, with the same results: one engine, engines of several devices, COOK_RANK_BATCH=0, a call from inside a flow. */
int cook_cycle_autoscale_multi(cook_engine** engines, uint32_t n,
                               const cook_autoscale_params* const* params, /* [n], every entry required            */
                               uint32_t* const* task_idx,                  /* [n]; entry i may be NULL iff cap[i]==0 */
                               const uint32_t* cap,                        /* [n]                                    */
                               cook_autoscale_info* info,                  /* [n] or NULL                            */
                               int* rc);                                   /* [n] or NULL: every engine's own code   */

/* ---- AUTOSCALE, the next step: Out distributed to the pool's autoscaling compute clusters and cut per cluster ------------------------
 * What trigger-autoscaling! (scheduler.clj:1178-1202) does with Out: distribute-jobs-to-compute-clusters (:1078-1103) with
 * job->acceptable-compute-clusters (:1059-1076), then autoscale!'s cut per cluster (kubernetes/compute_cluster.clj:606-731), up to the
 * list of jobs each cluster launches synthetic pods for.  Building the pods stays with the host.
 *
 * The pick needs Clojure's (hash uuid) of every pending job: for a java.util.UUID that is UUID.hashCode, with hilo = msb ^ lsb
 * (the two 64-bit halves) it is (int32)(hilo >> 32) ^ (int32)hilo.  cook_cycle_set_job_hashes writes rows [first, first + n) of an
 * engine-owned int32 column indexed by PENDING ORDINAL (like cook_cycle_set_considerable's eligible mask).  The engine tracks how many
 * LEADING rows are set: a range past the pending count, or one that starts behind the set prefix (a gap): COOK_E_INVALID; before
 * cook_cycle_stage*: COOK_E_STATE; a refused call changes nothing.  cook_cycle_stage* drops the column.  cook_cycle_update moves it with
 * the job rows when EVERY row was set (the rows a delta appends are unset: the host sets them with first = the kept pending count,
 * i.e. the new pending count minus the delta's new pending jobs); a column that was only partly set is dropped by an update.  The
 * call touches no rank, considerable or match state: it may come before or after the cycle. */
int cook_cycle_set_job_hashes(cook_engine* e, const int32_t* hash, uint32_t first, uint32_t n);

#define COOK_MAX_CLUSTERS 32
/* The pool's AUTOSCALING compute clusters only, in the order of the reference's collection (nth indexes it: the order is a contract). */
typedef struct cook_autoscale_clusters {
  uint32_t n;                          /* 1 .. COOK_MAX_CLUSTERS                                                                 */
  uint32_t reserved;                   /* 0                                                                                      */
  const uint32_t* location;            /* [n] compute-cluster->location in the id space of cook_jobs.ckpt_location; 0 = none     */
  const int64_t* max_pods_outstanding; /* [n] synthetic-pods-config                                                              */
  const int64_t* num_synthetic_pods;   /* [n] the host's full count of outstanding synthetic pods                                */
  const int64_t* max_total_nodes;      /* [n]                                                                                    */
  const int64_t* total_nodes;          /* [n]                                                                                    */
  const int64_t* max_total_pods;       /* [n]                                                                                    */
  const int64_t* total_pods;           /* [n]                                                                                    */
  const uint32_t* out_off;             /* [n + 1] CSR offsets into out_task, from 0, not decreasing; NULL: no outstanding pods   */
  const uint32_t* out_task;            /* task indices of the still-resident jobs with an outstanding synthetic pod per cluster  */
} cook_autoscale_clusters;
typedef struct cook_autoscale_cluster_info {
  uint32_t assigned;             /* jobs of Out the distribution gave the cluster                                                */
  uint32_t outstanding_removed;  /* of them, those with an outstanding synthetic pod there                                       */
  int64_t max_launchable;        /* min(max_pods_outstanding - num_synthetic_pods, max_total_nodes - total_nodes, max_total_pods - total_pods) */
  uint32_t launched;             /* length of the cluster's launch list                                                          */
  uint32_t reserved;
} cook_autoscale_cluster_info;
typedef struct cook_autoscale_no_cluster {
  uint32_t no_cluster;           /* jobs of Out no cluster is acceptable to (:no-acceptable-compute-cluster)                     */
  uint32_t n_first;              /* min(no_cluster, 10)                                                                          */
  uint32_t first_task[10];       /* the first of them in Out's order (:first-ten-jobs)                                           */
} cook_autoscale_no_cluster;
/* Steps 1-5 are cook_cycle_autoscale's (the same code, state rule and refusals), then for every job j of Out, in Out's order:
 *  6. acceptable clusters: L = ckpt_location[j] (0 when the staged jobs carry no such column).  L == 0: every cluster; otherwise the
 *     clusters with location == L, in cluster order (a cluster without a location never equals a job's).  None: the job counts
 *     towards no_cluster.
 *  7. the choice is the (hash mod count)-th acceptable cluster, Clojure's mod: a floor modulus, in [0, count) for every int32.
 *  8. each cluster's jobs stay in Out's order (group-by keeps it).
 *  9. per cluster the jobs named in its outstanding list go; of the rest the first max_launchable stay (<= 0: none).  An outstanding
 *     index that is in range and no candidate is ignored, as exclude_task is.
 * task_idx receives the clusters' launch lists one after another, cluster_off[n + 1] delimits them (cluster c: task_idx[cluster_off[c]
 * .. cluster_off[c + 1])); cluster_info[n]; no_cluster (optional).  info as cook_cycle_autoscale's (n_out = |Out|, whatever was cut).
 * COOK_E_INVALID: clusters NULL or n out of range, a NULL column, an outstanding index out of range, out_off not from 0 or decreasing
 * or without out_task, NULL cluster_off / cluster_info, the launch lists longer than cap (info, cluster_info and no_cluster are still
 * filled) — cap >= max(max_jobs, k) always suffices.  COOK_E_STATE: the hash column does not cover every pending row.  Everything the
 * host can know is checked in front of the first launch; a refused call changes nothing.  The call makes the stream synchronisations
 * cook_cycle_autoscale makes on the same inputs with cap > 0: the distribution is enqueued behind Out and its counts and lists come
 * back in the read-back that returns |Out|.  Integers only.
 * scheduling-capacity-constrained-job-distributor (:1110-1151), the distributor of a Kubernetes-scheduler pool, is cook_kube_distribute
 * below. */
int cook_cycle_autoscale_clusters(cook_engine* e, const cook_autoscale_params* p, const cook_autoscale_clusters* clusters, uint32_t* task_idx,
                                  uint32_t cap, uint32_t* cluster_off /* [n + 1] */, cook_autoscale_info* info,
                                  cook_autoscale_cluster_info* cluster_info /* [n] */, cook_autoscale_no_cluster* no_cluster /* or NULL */);
/* ... for every pool of a GPU in one pool batch, exactly as cook_cycle_autoscale_multi: engine i's results, code and message are those
 * of cook_cycle_autoscale_clusters(engines[i], params[i], clusters[i], task_idx[i], cap[i], cluster_off[i], &info[i], cluster_info[i],
 * &no_cluster[i]).  COOK_E_INVALID with nothing run: engines, params, clusters, cap, cluster_off or cluster_info NULL, n == 0, a NULL
 * entry of engines, params or clusters, an engine twice. */
int cook_cycle_autoscale_clusters_multi(cook_engine** engines, uint32_t n, const cook_autoscale_params* const* params,
                                        const cook_autoscale_clusters* const* clusters, uint32_t* const* task_idx, const uint32_t* cap,
                                        uint32_t* const* cluster_off, cook_autoscale_info* info /* [n] or NULL */,
                                        cook_autoscale_cluster_info* const* cluster_info, cook_autoscale_no_cluster* no_cluster /* [n] or NULL */,
                                        int* rc /* [n] or NULL */);

/* ---- KUBE: the distributor of a Kubernetes-scheduler pool ----------------------------------------------------------------------------
 * scheduling-capacity-constrained-job-distributor (scheduler.clj:1110-1151), which handle-kubernetes-scheduler-pool (:1747-1810) hands
 * its considerable jobs to.  Stateless, like cook_sweep_running: the engine handle only picks the device and stream; no rank,
 * considerable, match, offers or rebalance state is read or written.
 * The clusters are the pool's n compute clusters in the caller's order, 0 <= n <= COOK_MAX_CLUSTERS; capacity is cc/max-launchable
 * (kubernetes/compute_cluster.clj:571-604), computed by the host; it may be zero or negative (such a cluster is never available).
 * The jobs 0 .. n_jobs-1 go in order, sequentially, with cap[c] starting at capacity[c].  For job k:
 *  1. acceptable clusters: step 6 of cook_cycle_autoscale_clusters with L = location[k] (location NULL: 0).  L == 0: every cluster;
 *     otherwise the clusters with location == L, in cluster order.
 *  2. available clusters: the acceptable ones with cap[c] > 0 (:1128-1139), still in cluster order; m = their number.
 *  3. m == 0: the job counts towards no_cluster (:no-acceptable-compute-cluster, :1140-1141), choice[k] = COOK_KUBE_NO_CLUSTER; the first
 *     ten such jobs are reported (:first-ten-jobs, :1147-1150).
 *  4. otherwise rand-nth (:1142), which is (nth coll (int (* (count coll) (Math/random)))), with the draw u_k as the random number:
 *     r = min((uint32)(int32)trunc((double)m * u_k), m - 1) — ONE fp64 multiply, round to nearest —, the job goes to the r-th available
 *     cluster c, choice[k] = c, and cap[c] -= 1 (:1143-1144).  No u < 1 reaches the clamp: for m <= 32 the product m * u rounds to a
 *     double below m (m * 2^-53 is at least half a unit in the last place below m, and exactly half only for a power of two, where the
 *     product is exact).
 *  5. each cluster's jobs stay in job order (group-by keeps it): pos_idx holds the clusters' lists of job positions one after another,
 *     cluster_off[n + 1] delimits them.
 * The draws.  draw non-NULL: u_k = draw[k]; a value that is NaN or outside [0, 1): COOK_E_INVALID, checked on the host before the first
 * launch.  draw NULL: u_k = (double)(cook_splitmix64(seed + k) >> 11) * 2^-53 (exact: a 53-bit integer scaled), where, in uint64
 * arithmetic modulo 2^64,
 *     cook_splitmix64(x): z = x + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                         z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31).
 * One draw per POSITION is the contract: the reference draws only for the jobs with a non-empty available set, which has the same
 * distribution (the draws are independent and a job without an available cluster ignores its own) but not the same stream.
 * cluster_info[c] = {jobs given to c, capacity[c]}.  info: paused = 0, available = the saturated int64 sum of the raw capacities
 * (negatives included, the reduce + of :1767), max_considerable = n_considered = n_jobs, launched = the lists' total length, no_cluster,
 * n_first = min(no_cluster, 10) with first_task = their positions, exhaustions = clusters whose capacity the walk brought to zero.
 * COOK_E_INVALID: n_jobs > INT32_MAX, clusters NULL or n > COOK_MAX_CLUSTERS, a NULL column with n > 0, a bad draw, NULL choice with
 * n_jobs > 0, NULL pos_idx with cap > 0, NULL cluster_off or cluster_info (the latter with n > 0), the lists longer than cap (choice,
 * cluster_off, cluster_info and info are still filled) — cap >= n_jobs always suffices.  COOK_E_DEVICE: the walk did not end within
 * its pass bound (an internal error).  The first call on a handle allocates device memory. */
#define COOK_KUBE_NO_CLUSTER 0xFFu
#define COOK_KUBE_TILE 256 /* jobs the walk evaluates at once: a tile holds at most one exhaustion per pass */
typedef struct cook_kube_clusters {
  uint32_t n;               /* 0 .. COOK_MAX_CLUSTERS                                                                  */
  uint32_t reserved;        /* 0                                                                                       */
  const uint32_t* location; /* [n] compute-cluster->location in the id space of cook_jobs.ckpt_location; 0 = none      */
  const int64_t* capacity;  /* [n] cc/max-launchable                                                                   */
} cook_kube_clusters;
typedef struct cook_kube_cluster_info {
  uint32_t assigned;        /* jobs the distribution gave the cluster = the length of its list                         */
  uint32_t reserved;
  int64_t capacity;         /* as given                                                                                */
} cook_kube_cluster_info;
typedef struct cook_kube_info {
  uint32_t paused;          /* 0 (the gate of :1778 belongs to the pool's cycle)                                        */
  uint32_t max_considerable;
  int64_t available;        /* the sum of the raw capacities, saturated                                                 */
  uint32_t n_considered, launched, no_cluster, n_first;
  uint32_t first_task[10];
  uint32_t exhaustions, reserved;
} cook_kube_info;
int cook_kube_distribute(cook_engine* e, uint32_t n_jobs, const uint32_t* location /* [n_jobs] or NULL */,
                         const double* draw /* [n_jobs] or NULL */, uint64_t seed, const cook_kube_clusters* clusters,
                         uint8_t* choice /* [n_jobs] */, uint32_t* pos_idx, uint32_t cap, uint32_t* cluster_off /* [n + 1] */,
                         cook_kube_cluster_info* cluster_info /* [n] */, cook_kube_info* info /* or NULL */);

/* ---- SWEEP: the three task killers over the cluster's running set (scheduler.clj:1888-2016, group.clj:17-44) --------------------
 * Stateless, like cook_offers_build: the engine handle only picks the device and stream; no rank, considerable, match, offers or
 * rebalance state is read or written.  The running set is every :instance.status/running or /unknown instance (tools.clj:494-506).
 *  bit 0 lingering (get-lingering-tasks): start_ms present and now_ms > start_ms + min(rt, max_timeout_ms), rt = max_runtime_ms if >= 0
 *        else default_timeout_ms (strict: time/after?; evaluated without overflow).  Running and unknown rows.
 *  bit 1 straggler (find-stragglers :quantile-deviation, type-1 groups only): idx = (int)trunc((double)((int64)job_count - 1) * quantile);
 *        the group is READY iff its successful instances number more than idx; s = (end - start) / 1000 truncated (t/in-seconds; end < 0:
 *        now_ms); threshold = (double)(idx-th smallest s) * multiplier (NaN: not ready or not type 1).  A running (not unknown) row of a
 *        ready group is a straggler iff (double)((now_ms - start_ms) / 1000) > threshold.
 *  bit 2 cancelled (killable-cancelled-tasks): cancelled[i] != 0, running or unknown.
 * reason[i] = the bits of the killers that picked row i.  idx = lingering ++ stragglers ++ cancelled, each list in ascending row order (the
 * reference's Datomic set order is unpinned: this order is oracle-defined); a row may sit in several lists.  A killer whose bit is off in
 * `what` yields nothing and reads nothing.  More than cap entries: COOK_E_INVALID with info filled in.
 * COOK_E_INVALID with info->bad_row where the reference throws, for the rows it evaluates (successful instances and running rows of ready
 * type-1 groups): start absent, a negative interval or one above INT32_MAX seconds; bad_row = the lowest such running row, else n + the
 * lowest such successful instance; a group index out of range counts as an offending row.  Also COOK_E_INVALID (bad_row = COOK_NONE_U32
 * unless a row is at fault too) for a type-1 group with quantile outside (0, 1), multiplier <= 1 or either not finite, job_count >
 * INT32_MAX, a type > 1, a decreasing succ_off or one that does not start at 0, a negative timeout, n > INT32_MAX.  The reference's straggler handler stops at the first group that throws;
 * this call fails as a whole.  The first call on a handle allocates device memory. */
typedef struct cook_running_set {
  uint32_t n;
  const int64_t* start_ms;        /* :instance/start-time; INT64_MIN = absent                                             */
  const uint8_t* unknown;         /* 1 = :instance.status/unknown, 0 = running; NULL = all running                         */
  const int64_t* max_runtime_ms;  /* :job/max-runtime of the row's job, < 0 = absent; NULL = all absent                     */
  const uint8_t* cancelled;       /* :instance/cancelled; NULL = none                                                       */
  const uint32_t* group;          /* the job's group (index into cook_straggler_groups) or COOK_NONE_U32; NULL = none       */
} cook_running_set;
typedef struct cook_straggler_groups {
  uint32_t n;
  const uint8_t* type;            /* 0 :straggler-handling.type/none, 1 :quantile-deviation                                */
  const double* quantile;         /* type 1: 0 < q < 1 (api.clj:495-497)                                                   */
  const double* multiplier;       /* type 1: > 1.0                                                                          */
  const uint32_t* job_count;      /* (count (:group/job g)), jobs without instances included                                */
  const uint32_t* succ_off;       /* [n + 1], succ_off[0] = 0: the :instance.status/success instances of the group's jobs  */
  const int64_t* succ_start_ms;   /* [succ_off[n]]; INT64_MIN = absent                                                     */
  const int64_t* succ_end_ms;     /* [succ_off[n]]; < 0 = no :instance/end-time -> now_ms (tools.clj:670-676)              */
} cook_straggler_groups;
typedef struct cook_sweep_params {
  int64_t now_ms;
  int64_t default_timeout_ms;     /* (or default-timeout-hours timeout-hours) in ms, >= 0                                  */
  int64_t max_timeout_ms;         /* (or max-timeout-hours timeout-hours) in ms, >= 0                                      */
  uint32_t what;                  /* bit 0 lingering, bit 1 stragglers, bit 2 cancelled                                     */
  uint32_t reserved;              /* 0                                                                                      */
} cook_sweep_params;
typedef struct cook_sweep_info {
  uint32_t lingering, stragglers, cancelled, groups_ready, bad_row;
} cook_sweep_info;
int cook_sweep_running(cook_engine* e, const cook_running_set* tasks, const cook_straggler_groups* groups, const cook_sweep_params* p,
                       uint8_t* reason, uint32_t* idx, uint32_t cap, double* group_threshold_s, cook_sweep_info* info);

/* ---- MATCH: replaces the body of match-offer-to-schedule, i.e. TaskScheduler.scheduleOnce -----------------
 * (scheduler.clj:617-687; Fenzo 0.10.0 pinned at project.clj:46-50; constraints.clj).
 * job_to_offer[k] = offer index or -1.  head_matched mirrors scheduler.clj:1495 (first considerable job matched,
 * or nothing matched at all).  fail_code (optional, len K): 0 matched, else first reason no offer accepted it
 * (bit 0 resources, bit 1 constraints).  reserved_hosts: hosts reserved by the rebalancer for ANY job.
 * Ties between offers of equal fitness go to the lowest offer INDEX (array position).  The reference's recorded simulator run
 * (simulator_files/example-out-trace.csv) is reproduced row for row when the offers of a cycle are passed in DESCENDING hostname
 * order (ascending order yields the mirror image on identical hosts): that is the order a binding should use.
 * A pool of more offers than the placement walk's offer table holds (about 150 000; the serial sweep and the spreaders have no such
 * table) is refused with COOK_E_INVALID by the STAGE call (cook_match_stage, cook_cycle_stage and their built-offers forms, cook_match),
 * under the params in force then: behind a refused cook_match_stage the engine's last match is untouched and cook_match_fetch still
 * returns it.  cook_match_run asks again under the params in force at the run. */
int cook_match(cook_engine* e, const cook_jobs* considerable, const cook_offers* offers, const cook_groups* groups,
               const uint32_t* reserved_hosts, uint32_t n_reserved, int32_t* job_to_offer, uint32_t* fail_code,
               uint8_t* head_matched);
int cook_match_stage(cook_engine* e, const cook_jobs* considerable, const cook_offers* offers,
                     const cook_groups* groups, const uint32_t* reserved_hosts, uint32_t n_reserved);
int cook_match_run(cook_engine* e);
int cook_match_fetch(cook_engine* e, int32_t* job_to_offer, uint32_t* fail_code, uint8_t* head_matched);

/* ---- CYCLE: rank followed by match of the first K ranked jobs, without a host round trip ------------------
 * (pending-jobs->considerable-jobs "take num-considerable", scheduler.clj:751).  `jobs` must describe the same
 * pending tasks as the staged rank input, indexed by position among the pending tasks (pending ordinal).
 * job_to_offer is indexed by rank position (len = min(K, n_ranked)). */
int cook_cycle_stage(cook_engine* e, const cook_tasks* tasks, const cook_users* users, const cook_jobs* pending_jobs,
                     const cook_offers* offers, const cook_groups* groups, const uint32_t* reserved_hosts,
                     uint32_t n_reserved);

/* What changed between two match cycles of a pool whose inputs are RESIDENT (cook_cycle_stage once, then one delta per cycle):
 * handle-resource-offers! (scheduler.clj:1339-1385) meets almost the same pool every cycle — instances finished or were killed
 * (their task rows leave), jobs were submitted (new pending rows) or launched (the pending row leaves, a running row arrives), and
 * the offers are fresh.  The columns are edited on the device: a STABLE compaction, then the new rows at the end.  Task indices
 * reported afterwards (cook_cycle_fetch's ranked_pending_idx) refer to the updated arrays: row i of the old arrays that was kept is
 * now at i minus the number of removed rows in front of it; add_tasks[r] is at n_kept + r.  add_pending describes the pending tasks
 * of add_tasks, in order, and may only carry optional columns that the staged jobs carry too (else restage); cpus and mem are
 * required, and so is `user` when the staged jobs carry one.  Users, groups and reserved hosts stay as staged (a map installed by cook_cycle_set_reservations or a
 * cook_cycle_run_queue_reserve step is dropped by this call: THE HOST RESERVATIONS below).  The eligible mask
 * of cook_cycle_set_considerable moves with the job rows (the jobs a delta adds start out eligible; send a fresh mask to say
 * otherwise).  The call is all-or-nothing: a delta it refuses (COOK_E_INVALID — a row it cannot append, a remove_task entry out of
 * range or named twice, which the device finds) leaves the resident state as it was; the host arrays are read during the call only.
 * ABI note: the struct layouts of this header are versioned by COOK_ABI_VERSION (cook_abi_version()). */
typedef struct cook_cycle_delta {
  uint32_t n_remove;
  const uint32_t* remove_task;  /* indices into the current task arrays, each at most once */
  const cook_tasks* add_tasks;  /* may be NULL */
  const cook_jobs* add_pending; /* may be NULL when no added task is pending */
  const cook_offers* offers;    /* NULL: the staged offers stay; else they are replaced wholesale */
} cook_cycle_delta;
int cook_cycle_update(cook_engine* e, const cook_cycle_delta* delta);

/* Page-locked host memory for input columns and result buffers: copies from / to it run at link speed (pageable memory goes
 * through a bounce buffer at a fraction of it).  NULL on failure. */
void* cook_host_alloc(size_t bytes);
void cook_host_free(void* p);
int cook_cycle_run(cook_engine* e, uint32_t num_considerable);
/* Several pools of one rank (same device) in ONE placement call: cook_cycle_run_rank does the rank / considerable / take-K part of
 * cook_cycle_run for ONE engine (call it for each engine, from any threads), then cook_cycle_match_multi places all of them; results
 * are fetched per engine with cook_cycle_fetch as usual.  Same results as cook_cycle_run on each engine.  How: served walkers — one
 * persistent walker workgroup per pool (one launch per call) beside up to three streams of evaluation launches for whichever pools
 * have a window waiting — or, with COOK_MATCH_SERVED=0 in the environment and as the library's own fall-back, one
 * sequence of launches with blockIdx.z = pool on engines[0]'s stream (pools in lockstep).  Many independent streams of small kernels
 * interfere on one GPU; either form keeps to four.  The call occupies the calling thread until every pool is placed.  Hold every
 * engine's lock across both calls. */
int cook_cycle_run_rank(cook_engine* e, uint32_t num_considerable);
/* cook_cycle_run_rank for n engines of one device in ONE call from ONE thread (replaces scheduler.clj:2425-2435's thread per pool for
 * the rank part; same results per engine as n separate calls; num_considerable[i] is engine i's K — the head-of-queue scaleback,
 * scheduler.clj:1613-1651, moves it per pool).  A pool's rank is a chain of about a hundred small launches and the
 * stage is bound by their number: here the pools' flows run side by side on engines[0]'s stream and a kernel that stands at the same
 * point of several flows is launched ONCE for all of them (blockIdx.y = pool), with one stream synchronisation where each flow would
 * have had its own.  user_usage != NULL: user_usage[i] also receives engine i's per-user running usage [U x 3] exactly as
 * cook_rank_user_usage(engines[i], user_usage[i], usage_is_device) would deliver it after the rank (the collective's payload), inside the
 * same joint sequence.  COOK_RANK_BATCH=0 in the environment: the engines one after another, as cook_cycle_run_rank (+ cook_rank_user_usage).
 * Every engine ONCE: a handle twice in the array is COOK_E_INVALID (here and in cook_cycle_match_multi).
 * Returns the first engine's error that is not COOK_OK; every engine keeps its own message (cook_last_error). */
int cook_cycle_run_rank_multi(cook_engine** engines, uint32_t n, const uint32_t* num_considerable /* [n]: every pool its own K */,
                              double* const* user_usage, int usage_is_device);
int cook_cycle_match_multi(cook_engine** engines, uint32_t n);
int cook_cycle_fetch(cook_engine* e, uint32_t* ranked_pending_idx, uint32_t* n_ranked, int32_t* job_to_offer,
                     uint32_t* n_considered, uint8_t* head_matched);

/* ---- QUEUE CYCLES: match cycles on the standing ranked queue, without a re-rank ------------------------------------------------
 * The reference runs on two clocks: rank-jobs (scheduler.clj:2262-2296) writes pool-name->pending-jobs-atom every few seconds;
 * handle-resource-offers! (:1339-1520) runs far more often, does NOT rank, reads the atom (:1360), matches its considerable jobs and
 * takes the matched jobs out of it (remove-matched-jobs-from-pending-jobs, :790-795, at :1506-1508; the Kubernetes pool handler removes
 * every considered job, :1792-1794).  After a rank (cook_cycle_run, cook_cycle_run_rank*, + cook_cycle_match_multi) the engine holds
 * the STANDING QUEUE Q = the rank's output order.  A queue cycle does, in this order, with no rank and no host round trip of per-job data:
 *  1. Advance.  From the pool's last cycle (rank cycle or queue cycle): the considered rank positions, their job_to_offer and
 *     offer_skipped (1 = filter-matches-for-ratelimit, :887-924, dropped every match of that offer's compute cluster; indexed by the
 *     offers of THAT cycle, as in cook_autoscale_params).  remove_mode 0 removes from Q the jobs with a KEPT match, remove_mode 1 every
 *     considered job.  The survivors keep their order.
 *  2. Groups.  groups non-NULL: the groups' running-cotask table is replaced by it (layout of cook_groups; n, type, attr_key, minimum
 *     must equal the staged ones).  NULL: every job of step 1 WITH A KEPT MATCH and a group g becomes a running cotask of g on the host
 *     of its offer (run_host = the offer's host, run_attr = that offer's value of attr_key[g], 0 = absent), appended on the device:
 *     what the reference sees once the launched instances are in the DB (constraints.clj:553-566).  The order inside a group's list
 *     is not defined (unique, balanced and attribute-equals read it as a set / as counts).
 *  3. Offers.  offers non-NULL replaces the staged offers wholesale (as cook_cycle_delta.offers).  NULL leaves them as they are, which
 *     only describes the cluster when step 1 removed nothing: these entry points do not subtract placements from the offers
 *     (cook_cycle_run_queue_carry below does, on the device).
 *  4. Considerable -> take num_considerable -> match over Q, exactly as a rank cycle does over the rank's output: the user state is
 *     whatever cook_cycle_set_considerable staged last (refresh usage and tokens between cycles with that call: it does not invalidate
 *     Q; or let cook_cycle_run_queue_carry add the kept placements to the staged usage on the device), the eligible mask follows the job rows, reserved hosts stay as staged
 *     (unless the engine holds a reservation map of its own, which cook_cycle_run_queue_reserve keeps in step with the matches and the
 *     rebalancer: THE HOST RESERVATIONS below), all placement forms apply unchanged.
 * Afterwards cook_cycle_fetch / cook_cycle_fetch_considerable / cook_match_explain / cook_match_metrics / cook_cycle_autoscale describe
 * THIS cycle: ranked_pending_idx is the current Q (task indices, the index space of the rank), n_ranked its length, rank_pos positions
 * in it.  cook_user_stats / cook_unscheduled / cook_usage_breakdown keep describing the last RANK (they read the per-user order, which a
 * queue cycle does not touch): a job matched since the rank still shows as waiting there until the next rank.
 * State: a queue cycle needs a completed cycle since the last cook_cycle_stage / cook_cycle_update / cook_rank* / cook_considerable /
 * cook_match_stage / cook_match_run (those shift or drop the rows Q points at, or replace the last cycle's job_to_offer), else
 * COOK_E_STATE and nothing changes.  A refused step (COOK_E_INVALID: remove_mode > 1, offer_skipped given with n_offer_skipped other than
 * the last cycle's offer count, a groups table of another shape, offers the stage would refuse) leaves Q, the groups and the offers
 * as they were.  A call that fails later than that (a device error) leaves no standing queue: rank again.
 * Timing: cook_last_timing's rank_ms of a queue cycle is the time of its advance + considerable filters + take (no rank ran);
 * cook_match_stats_ex [31] has the host's microseconds in the advance alone.  Any rank call resets Q to the fresh order and the groups' cotasks to the staged table.  step NULL: all defaults. */
typedef struct cook_queue_step {
  const uint8_t* offer_skipped;  /* [offers of the LAST cycle] or NULL */
  uint32_t remove_mode;          /* 0 kept matches, 1 every considered job */
  uint32_t n_offer_skipped;      /* entries of offer_skipped: must equal the offer count of the LAST cycle (ignored when offer_skipped is NULL) */
  const cook_offers* offers;     /* NULL: stay */
  const cook_groups* groups;     /* NULL: fold the kept matches' cotasks on the device */
} cook_queue_step;
/* like cook_cycle_run */
int cook_cycle_run_queue(cook_engine* e, const cook_queue_step* step, uint32_t num_considerable);
/* like cook_cycle_run_rank: the placement is set up and runs in cook_cycle_match_multi */
int cook_cycle_run_queue_rank(cook_engine* e, const cook_queue_step* step, uint32_t num_considerable);
/* n pools of a device in ONE call from one thread, then cook_cycle_match_multi: the pools' advances and filters side by side, the same
 * kernel of several pools launched once (blockIdx.y = pool), one synchronisation where each pool's flow would have its own (the
 * mechanism of cook_cycle_run_rank_multi).  steps NULL or steps[i] NULL: defaults.  An engine twice: COOK_E_INVALID.  Returns the first
 * engine's error that is not COOK_OK; a pool whose step was refused stays as it was, the others go on.  cook_cycle_match_multi accepts any
 * mix of engines prepared by a rank call and by a queue call. */
int cook_cycle_run_queue_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps, const uint32_t* num_considerable);

/* ---- THE CARRY: a queue cycle that moves the last cycle's kept placements into the staged offers and the staged user state ----------
 * In the reference neither is the caller's arithmetic: Fenzo keeps its leases and per-host running totals across scheduleOnce calls
 * (getTaskAssigner, scheduler.clj:877-881), a host's remainder returns as a smaller offer, and generate-user-usage-map (:711-727) sees
 * the launched jobs as running.  The carry runs inside step 1 of a queue cycle, over the OLD offers and the OLD considered jobs, before
 * they leave the queue, with no synchronisation of its own.  A KEPT placement is job_to_offer >= 0 with the offer not skipped: the
 * predicate of step 1 and of the groups' fold.  remove_mode does not change what is carried; unmatched considered jobs carry nothing.
 * Order rule (oracle-defined, like the winner rule): every sum runs over the kept placements in CONSIDERED order (= rank order), the
 * order in which the placement itself accumulated "assigned this call"; strictly left to right, x = x + r one job after another, fp64,
 * no re-association.  The result does not depend on the placement form: it is computed from job_to_offer alone.
 *  offers = 1.  For offer v, with A_c, A_m, A_n, A_ports, A_s[s] the left-to-right sums (each from 0) of its kept jobs' cpus, mem,
 *     count, positive port counts and non-NaN named scalars: cpus -= A_c, mem -= A_m, run_cpus += A_c, run_mem += A_m, run_count += A_n,
 *     num_tasks += A_n, ports -= A_ports, scalars[s] -= A_s[s].  For a k8s offer, job after job in considered order: a kept job with
 *     gpus > 0 subtracts its gpus from the gpu_count slot whose model equals the job's; a kept job with disk_request >= 0 subtracts it
 *     from the disk_space slot of its disk_type; no such slot: nothing changes.  run_cpus / run_mem / run_count / num_tasks / ports that
 *     were staged as NULL (all 0) come into existence first.  A named scalar the offers have no column for stays absent (total 0).
 *     max_tasks, attributes, host, location, host_start_s, k8s and the model / type ids are untouched.  The carried offers ARE the staged
 *     offers from then on, exactly as a wholesale replacement would be, through later cycles and ranks until replaced.  The engine
 *     writes a copy of its own: neither the caller's arrays nor the rows of cook_offers_run (cook_cycle_stage_built_offers) are written.
 *  usage = 1.  For user u the sums of its kept jobs in considered order are added to the staged arrays: usage_count[u] += count,
 *     usage_cpus[u] / usage_mem[u] / usage_gpus[u] += the left-to-right sums (each from 0) of cpus / mem / gpus.  With pool_usage_given
 *     the pool usage grows by the same four quantities summed over ALL kept jobs in considered order; otherwise the engine keeps
 *     summing the users itself.  Tokens: tokens_left non-NULL replaces the staged counts and nothing is spent (the host has done both);
 *     tokens_left NULL with tokens staged: tokens[u] -= kept jobs of u (the spend; the refill with time is the host's, or the engine's: THE LAUNCH-RATE LIMITERS below).
 *     tokens_left is honoured whatever the two flags say.  Quotas, enforce_rate_limit and the eligible mask stay as staged.
 * Refused before anything changes: offers = 1 together with step->offers, a flag above 1, tokens_left while the staged state has no
 * limiter (COOK_E_INVALID); usage = 1 or tokens_left without a staged user state (COOK_E_STATE).
 * Not carried: finished tasks (cook_cycle_run_queue_release below takes their list), hosts that join or leave
 * (cook_cycle_run_queue_hosts below takes their lists); the time-based token refill (tokens_left from the host, or the engine's own limiters, which need only the time: cook_cycle_set_limiters below).  carry NULL, or both flags 0 and no tokens: exactly cook_cycle_run_queue / _multi. */
typedef struct cook_queue_carry {
  uint32_t offers;            /* 1: carry the kept placements into the staged offers (then step->offers must be NULL) */
  uint32_t usage;             /* 1: carry them into the staged user state (needs cook_cycle_set_considerable staged)   */
  const int64_t* tokens_left; /* optional [users]: replaces the staged token counts (the host's refill); NULL: see above */
} cook_queue_carry;
int cook_cycle_run_queue_carry(cook_engine* e, const cook_queue_step* step, const cook_queue_carry* carry, uint32_t num_considerable);
/* as cook_cycle_run_queue_multi (then cook_cycle_match_multi); steps / carries NULL or an entry NULL: defaults */
int cook_cycle_run_queue_carry_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps,
                                     const cook_queue_carry* const* carries, const uint32_t* num_considerable);

/* ---- THE RELEASE: a queue cycle that gives the resources of FINISHED tasks back, the inverse of the carry -----------------------------
 * In the reference this is nobody's arithmetic either: Fenzo unassigns finished tasks before scheduleOnce (scheduler.clj:665-669), so
 * the host's lease and running totals get the resources back; generate-user-usage-map (:711-727) no longer counts the task; the group
 * constraints no longer see the instance as a running cotask (constraints.clj:553-566).  A queue cycle takes the short list of the tasks
 * that ended since the last cycle and, on the device, returns their resources to the staged offers, takes them out of the staged user
 * state and of the pool usage, and removes them from the groups' running-cotask lists, with no synchronisation of its own.
 * Position in the advance: behind the carry and behind the groups' fold (a task placed last cycle may have finished already), in
 * front of the step's considerable filters; it also runs when the last cycle considered nothing or the queue is empty.
 * Order rule (oracle-defined, like the carry's): every fp64 sum runs over the entries of its segment in LIST order, left to right,
 * from 0.0, x = x + r one entry after another, no re-association.
 *  offers = 1.  The row of an entry is the staged offer whose host equals the entry's host; an entry whose host has no row changes no
 *     offer and is counted in without_row.  For a row, with R_c, R_m, R_n, R_ports, R_s[s] the sums over its entries (count, positive
 *     port counts, non-NaN named scalars): cpus += R_c, mem += R_m, run_cpus -= R_c, run_mem -= R_m, run_count = max(0, run_count - R_n),
 *     num_tasks = max(0, num_tasks - R_n), ports += R_ports, scalars[s] += R_s[s]; a row where either count was clamped adds one to
 *     counts_clamped.  For a k8s row, entry after entry in list order: gpus > 0 with a model adds the gpus to the gpu_count slot of that
 *     model, disk_request >= 0 with a type adds it to the disk_space slot of that type; no such slot: nothing changes.  run_cpus /
 *     run_mem / run_count / num_tasks / ports that were staged as NULL (all 0) come into existence first, as in the carry; a named
 *     scalar or a slot table the offers have no column for stays absent.  Neither the caller's arrays nor the rows of cook_offers_run
 *     are written, and the columns the last match read stay as they were (cook_match_explain): behind a carry of the same advance the
 *     release updates the carry's fresh copy in place, without one it writes a fresh copy of its own.
 *  usage = 1.  Per user, over its entries in list order: usage_count[u] -= count, usage_cpus[u] / usage_mem[u] / usage_gpus[u] -= the
 *     left-to-right sums.  With pool_usage_given the pool usage shrinks by the same four quantities summed over ALL entries in list
 *     order.  Tokens, quotas and the eligible mask are untouched.
 *  groups = 1.  On the table as it stands after this advance's fold: for every entry with a group g, in list order, the first row of
 *     g's list (in the list's order) whose run_host equals the entry's host and that no earlier entry took leaves the list; an entry
 *     that finds none is counted in cotasks_missing.  The survivors keep their order.
 * Refused before anything changes.  COOK_E_INVALID: a flag above 1; offers = 1 together with step->offers; groups = 1 together with
 * step->groups; offers = 1 while two staged offers are on one host; host / cpus / mem missing (user missing with usage = 1);
 * n_scalars > COOK_MAX_SCALARS; cpus, mem, gpus or a scalar negative or infinite, cpus / mem / gpus / disk_request NaN; a user >= the
 * staged users; a group >= the staged groups that is not COOK_NONE_U32.  COOK_E_STATE: usage = 1 without a user state staged by
 * cook_cycle_set_considerable.  A refused step leaves the queue, the offers, the usage and the groups as they were.
 * finished NULL, n = 0 or all three flags 0: exactly cook_cycle_run_queue_carry / _carry_multi.  The arrays are read until the call
 * returns.  cook_user_stats / cook_unscheduled / cook_usage_breakdown keep describing the last RANK.  Taking finished rows out of the
 * rank's task table stays with cook_cycle_update and the next rank; hosts that join or leave go through cook_cycle_run_queue_hosts
 * below.  (Additive: no existing layout changes.) */
typedef struct cook_finished {      /* tasks that ended since the last cycle, in the host's order (the order rule above) */
  uint32_t n;
  const uint32_t* host;             /* [n] host id, as cook_offers.host / cook_groups.run_host */
  const uint32_t* user;             /* [n]; required with usage = 1 */
  const double *cpus, *mem;         /* [n] required */
  const double* gpus;               /* [n] or NULL (all 0) */
  const int32_t* ports;             /* [n] or NULL; only positive counts are returned */
  const double* scalars; uint32_t n_scalars;   /* n_scalars columns of n doubles as cook_jobs.scalars, NaN = no request under that name */
  const uint32_t* gpu_model; const double* disk_request; const uint32_t* disk_type;  /* as cook_jobs; NULL = none */
  const uint32_t* group;            /* [n] or NULL; COOK_NONE_U32 = no group */
  uint32_t offers, usage, groups;   /* 0 / 1 each: what to release into */
} cook_finished;
typedef struct cook_release_info {
  uint32_t with_row, without_row;            /* entries whose host has / has no row in the staged offers (offers = 1) */
  uint32_t counts_clamped;                   /* offers whose run_count or num_tasks would have gone below 0 */
  uint32_t cotasks_removed, cotasks_missing; /* groups = 1 */
} cook_release_info;
int cook_cycle_run_queue_release(cook_engine* e, const cook_queue_step* step, const cook_queue_carry* carry, const cook_finished* finished,
                                 uint32_t num_considerable);
/* as cook_cycle_run_queue_carry_multi (then cook_cycle_match_multi); finished NULL or an entry NULL: no release for that pool */
int cook_cycle_run_queue_release_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps,
                                       const cook_queue_carry* const* carries, const cook_finished* const* finished,
                                       const uint32_t* num_considerable);
/* the counts of the last queue cycle's release; all 0 when it had none */
int cook_cycle_release_info(cook_engine* e, cook_release_info* out);

/* ---- THE HOST CHURN: a queue cycle that takes the rows of hosts that LEAVE out of the staged offers and puts rows that JOIN in -------
 * In the reference nobody does this arithmetic: generate-offers (kubernetes/compute_cluster.clj:68-190) lists the nodes that exist and
 * are schedulable now, Mesos rescinds offers and sends new ones, Fenzo expires a lost host's lease and meets a new lease on the next
 * scheduleOnce (scheduler.clj:665-678).  A queue cycle takes a short list of hosts that leave and of rows that join and edits the
 * staged offer table on the device inside the advance: a stable compaction plus an ordered insertion over every offer column, with no
 * synchronisation of its own (its counters ride in the advance's one read-back) and no upload of the table.
 * Position in the advance: behind the carry, the groups' fold and the release, which all still work on the OLD rows (the last cycle's
 * job_to_offer and offer_skipped index them, and a task may finish on a host that leaves in the same call); in front of the step's
 * considerable filters; it also runs when the last cycle considered nothing or the queue is empty.
 * Order rule (oracle-defined and a contract: the lowest offer index wins ties in the placement).  OLD = the table as it stands behind the
 * release.  The rows whose host is in leave_host go; the surviving rows keep their relative order.  Join row i is placed directly in
 * front of the position of the OLD row whose host is join_before[i], whether or not that row leaves; rows with the same anchor keep
 * list order; COOK_NONE_U32 = behind the last OLD row (join_before NULL: all of them).  A host that both leaves and joins with itself
 * as the anchor is therefore replaced in place.  The new row indices are what job_to_offer, cook_match_explain, cook_match_metrics,
 * cook_cycle_autoscale and the next step's offer_skipped / n_offer_skipped refer to from this cycle on; a host can reproduce them from
 * this rule without a fetch.
 * Columns: every column of the staged table moves with its row (the resources, run_*, num_tasks, max_tasks, ports, the named scalars,
 * k8s, the [n][slots] gpu / disk maps, the [n][n_attr_keys] attributes, host, location, host_start_s).  A joining row's values are the
 * list's, unchanged (the host states run_* and num_tasks of a host that returns).  A column the staged table has and join lacks gets,
 * for the joining rows, the value a NULL column means for every row: 0, and -1 (absent) for max_tasks and host_start_s.  The five
 * columns a carry or a release brings into existence (run_cpus, run_mem, run_count, num_tasks, ports) count as present from the first
 * step on these offers that asked for offers = 1 in either, this very step included.  The churned
 * table IS the staged table from then on, through later cycles and ranks until replaced, exactly as the carried one is.  The caller's
 * arrays, the engine's originally staged arrays and the rows of cook_offers_run are never written, and the columns the last match read
 * stay as they were.
 * Refused before anything changes.  COOK_E_INVALID: join carries a column the staged table lacks, or another n_attr_keys / gpu_slots /
 * disk_slots / n_scalars (0 slots means 1); join lacks cpus, mem or host (or has gpu_model without gpu_count, disk_type without
 * disk_space); n_leave without leave_host; a host twice in leave_host or twice in join; a joining host that is already staged and does
 * not leave in this call; join_before names a host that is not an OLD row; the staged offers have two rows on one host; step->offers
 * together with a churn; a new row count that a stage would refuse.  COOK_E_STATE: the staged offers were built on the device
 * (cook_cycle_stage_built_offers): build them again from the nodes.  A refused step leaves the queue, the offers, the usage and the
 * groups as they were.  Not an error: a leave_host that has no row is counted in leave_missing.  hosts NULL, or both lists empty:
 * exactly cook_cycle_run_queue_release / _release_multi.  The arrays are read until the call returns.  The groups' running cotasks
 * are keyed by host id, not by row: a cotask on a host that leaves and returns still counts.  (Additive: no existing layout changes.) */
typedef struct cook_host_churn {
  uint32_t n_leave;
  const uint32_t* leave_host;   /* [n_leave] host ids whose rows leave the staged offers */
  const cook_offers* join;      /* rows that join (join->n of them), layout of cook_offers; NULL = none */
  const uint32_t* join_before;  /* [join->n] host id of the OLD row in front of which the row goes; COOK_NONE_U32 = behind the last row; NULL = all at the end */
} cook_host_churn;
typedef struct cook_churn_info {
  uint32_t left, leave_missing; /* leave_host entries that had / had no row */
  uint32_t joined;              /* rows that joined */
  uint32_t n_offers;            /* rows of the staged offers behind the advance */
} cook_churn_info;
int cook_cycle_run_queue_hosts(cook_engine* e, const cook_queue_step* step, const cook_queue_carry* carry, const cook_finished* finished,
                               const cook_host_churn* hosts, uint32_t num_considerable);
/* as cook_cycle_run_queue_release_multi (then cook_cycle_match_multi); hosts NULL or an entry NULL: no churn for that pool */
int cook_cycle_run_queue_hosts_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps,
                                     const cook_queue_carry* const* carries, const cook_finished* const* finished,
                                     const cook_host_churn* const* hosts, const uint32_t* num_considerable);
/* the counts of the last queue cycle's churn; all 0 (n_offers = the staged row count) when it had none */
int cook_cycle_churn_info(cook_engine* e, cook_churn_info* out);

/* The staged offer table as the next match will read it, behind any carry, release and churn: one caller-allocated array per column of
 * cook_offers, each with room for cap rows of its width; NULL = skip that column.  The call sets n and the widths: gpu_model / gpu_count
 * are [n][gpu_slots], disk_type / disk_space [n][disk_slots], attr [n][n_attr_keys] (row-major, as staged; a width of 0: nothing is
 * written), scalars n_scalars columns of n doubles one behind the other (as cook_offers.scalars).  cap < n: COOK_E_INVALID with n and
 * the widths set and no column written.  A column the staged table does not have is filled with what NULL means for it (0; -1 for
 * max_tasks and host_start_s).  Changes no state, invalidates nothing, costs one synchronisation; COOK_E_STATE before offers were staged. */
typedef struct cook_offer_rows {
  uint32_t cap;                 /* in: rows every non-NULL array has room for */
  uint32_t n;                   /* out: rows of the staged offers */
  uint32_t gpu_slots, disk_slots, n_attr_keys, n_scalars; /* out: the staged widths */
  double* cpus;
  double* mem;
  uint32_t* host;
  uint8_t* k8s;
  uint32_t* gpu_model;
  double* gpu_count;
  uint32_t* disk_type;
  double* disk_space;
  uint32_t* attr;
  int32_t* max_tasks;
  int32_t* num_tasks;
  uint32_t* location;
  int64_t* host_start_s;
  double* run_cpus;
  double* run_mem;
  int32_t* run_count;
  int32_t* ports;
  double* scalars;
} cook_offer_rows;
int cook_cycle_fetch_offers(cook_engine* e, cook_offer_rows* out);

/* ---- THE HOST RESERVATIONS: the rebalancer's reserved hosts, kept on the device across match cycles -----------------------------------
 * In the reference one atom {job-uuid->reserved-host, launched-job-uuids} moves on both clocks.  match-offer-to-schedule
 * (scheduler.clj:645-653) reads reserved-hosts = the values of the map, and every job is kept off all of them except its own
 * (constraints.clj:242-252).  After every match that matched something update-host-reservations! (scheduler.clj:1050-1057, called at
 * :1517) removes the matched jobs' reservations and adds those jobs to launched-job-uuids.  After every rebalancer run reserve-hosts!
 * (rebalancer.clj:419-432, called at :466) REPLACES the map by the decisions that preempt more than one task, minus the jobs in
 * launched-job-uuids, and clears that set.
 * The engine keeps exactly that atom, per engine: map = pending row -> host, launched = a set of pending rows.  On the device: a
 * reservation list (row or COOK_NONE_U32, host id), an engine-owned reserved_host column over the staged pending rows, an engine-owned
 * bitmap rebuilt from the live list, a byte per pending row.  Reservations are keyed by host ID, not by offer row: the host churn does
 * not touch them, and a reserved host that leaves and returns is still reserved.  An entry whose pending is COOK_NONE_U32 reserves a
 * host for a job that is not among this pool's pending rows (the reference's atom is one for all pools, mesos.clj:184): no match
 * releases it, only a replacement removes it.
 * 1. Inside a queue cycle's advance (cook_cycle_run_queue_reserve), in this order, behind the host churn and in front of the
 *    considerable filters, also when the last cycle considered nothing or the queue is empty:
 *    RELEASE (release_matched = 1): every considered job of the pool's LAST cycle — rank cycle or queue cycle — that has a KEPT match
 *    (job_to_offer >= 0 and the offer not skipped by step->offer_skipped: the predicate of step 1 of the queue cycles, the fold and the
 *    carry; remove_mode does not change it) joins `launched`; if it holds a reservation, the reservation goes and is counted in
 *    `released`.
 *    REPLACE (replace = 1), then: every old reservation goes; list entry i becomes a reservation unless its row is in `launched`
 *    (counted in dropped_launched); `launched` is cleared.  This is (apply dissoc reservations launched-job-uuids) followed by
 *    :launched-job-uuids #{}, literally.
 *    The bitmap is rebuilt from the live list; the counts ride in the advance's ONE synchronisation.  When nothing is alive behind
 *    the advance the match reads no bitmap at all, and the class-ordered walk (match_algo 3) is eligible again in that very cycle.
 * 2. cook_cycle_set_reservations is the REPLACE of point 1 on its own (same drop rule, `launched` cleared, release_matched ignored;
 *    replace = 0: the list is ignored and nothing changes — a map the engine holds stays, and without one the staged reservations
 *    keep being read): the way to hand a rebalancer result to the next RANK cycle.
 *    Like cook_cycle_set_considerable it touches none of the standing queue, the rank or the placement, and the match that ran last
 *    stays described as it ran: cook_match_explain and cook_match_metrics called behind it still answer from the map that match
 *    read (the new map goes into a second column and bitmap; the ones that match read are left alone until the next match).  It
 *    needs cook_cycle_stage (else COOK_E_STATE), and it is refused (COOK_E_STATE, nothing changed) while a placement is set up and
 *    has not run (between cook_cycle_run_rank* / cook_cycle_run_queue_*_multi and cook_cycle_match_multi): that placement was set
 *    up with the map as it stands.  r NULL, or n = 0 with replace = 1: no reservations.  From the first such call, or the first _reserve step
 *    with replace = 1, the engine's own map is what every later match reads, rank cycles and queue cycles alike, the older queue entry
 *    points included (they leave the map as it stands).
 * 3. Lifetime: cook_cycle_stage, cook_match_stage* and cook_cycle_update (one that is not refused) drop the engine's map and
 *    `launched` — they shift the rows —, and the staged reserved_hosts / reserved_host are what the match reads again.  A rank without
 *    those calls keeps the map.  A _reserve step with replace = 0 and release_matched = 1 on an engine that holds no map of its own is
 *    refused (COOK_E_STATE): install one first; the staged bitmap does not say which job a host belongs to.
 * 4. Refused before anything changes (COOK_E_INVALID): a flag above 1; n without pending / host; a pending index >= the staged pending
 *    count that is not COOK_NONE_U32; a pending row twice in the list; a host id above 2^31 - 1 (cook_jobs.reserved_host is int32).  A
 *    refused step leaves the queue, the offers, the usage, the groups and the reservations as they were.  reservations NULL, or both
 *    flags 0: exactly cook_cycle_run_queue_hosts / _hosts_multi.  The arrays are read until the call returns.
 *    Dense host ids are assumed, as by the host churn: the bitmap has one bit per host id up to the greatest id of the list and is
 *    filled anew in every step that can change it (a single id near 2^31 costs a 256 MB fill per step).
 * 5. Afterwards cook_match_explain, cook_match_metrics and cook_cycle_autoscale describe this cycle's match, which read the new map.
 * (Additive: no existing layout changes.) */
typedef struct cook_reservations {
  uint32_t release_matched; /* 1: update-host-reservations! over the LAST cycle's kept matches                    */
  uint32_t replace;         /* 1: reserve-hosts! with the list below; 0: the list is ignored, the map stays       */
  uint32_t n;
  const uint32_t* pending;  /* [n] pending ordinal (index space of cook_cycle_stage's pending_jobs), or
                               COOK_NONE_U32 = a job outside this pool; a pending row at most once                 */
  const uint32_t* host;     /* [n] host id, as cook_offers.host                                                   */
} cook_reservations;
typedef struct cook_reserve_info {
  uint32_t released;         /* reservations the kept matches of the last cycle released in this advance          */
  uint32_t installed;        /* list entries that became reservations                                             */
  uint32_t dropped_launched; /* list entries whose row was in `launched`                                          */
  uint32_t alive;            /* reservations held behind the call                                                 */
} cook_reserve_info;
int cook_cycle_set_reservations(cook_engine* e, const cook_reservations* r);
int cook_cycle_run_queue_reserve(cook_engine* e, const cook_queue_step* step, const cook_queue_carry* carry, const cook_finished* finished,
                                 const cook_host_churn* hosts, const cook_reservations* reservations, uint32_t num_considerable);
/* as cook_cycle_run_queue_hosts_multi (then cook_cycle_match_multi); reservations NULL or an entry NULL: none for that pool */
int cook_cycle_run_queue_reserve_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps,
                                       const cook_queue_carry* const* carries, const cook_finished* const* finished,
                                       const cook_host_churn* const* hosts, const cook_reservations* const* reservations,
                                       const uint32_t* num_considerable);
/* the counts of the last call that could change the map (a queue cycle, cook_cycle_set_reservations); all 0 (alive = the live
 * reservations) when it changed nothing; all 0 without a map of the engine's own */
int cook_cycle_reserve_info(cook_engine* e, cook_reserve_info* out);
/* the live reservations in list order: pending[i] (a pending ordinal or COOK_NONE_U32) holds host[i]; either array may be NULL;
 * *n_out = their count; cap smaller than that: COOK_E_INVALID with *n_out set and nothing written.  No map of the engine's own: 0.
 * Changes no state; one synchronisation */
int cook_cycle_fetch_reservations(cook_engine* e, uint32_t* pending, uint32_t* host, uint32_t cap, uint32_t* n_out);

/* ---- THE LAUNCH-RATE LIMITERS: the per-user-per-pool token buckets, refilled by time on the device --------------------------------------
 * The considerable filter's rate-limit stage (tools.clj:935-959) reads ratelimit/get-token-count! of the per-user-per-pool launch limiter;
 * launch-matches! spends one token per launched task (scheduler.clj:871).  With cook_user_state.tokens_left the host computes the
 * refill every cycle and uploads an int64 per user.  Here the engine keeps the reference's token bucket filter
 * (rate_limit/token_bucket_filter.clj, rate_limit/generic.clj) per user and the host passes two integers per cycle: the time.  The
 * compute-cluster launch limiter (filter-matches-for-ratelimit) stays with the host: it arrives as offer_skipped.
 * The bucket, restated (the device and the tests' oracle follow this to the bit).  Per user {rate (fp64, tokens per ms), bucket, last (ms),
 * tokens (may be negative)}:
 *   rate        = per_minute / 60000.0, ONE fp64 division (generic.clj:50).
 *   earn(t)     : t' = max(t, last).  If t' != last: d = (int64) trunc((double)(t' - last) * rate) — one fp64 multiply, truncation toward
 *                 zero, the product clamped at 2^62 before the conversion (the reference would throw there).  d != 0: last = t', tokens =
 *                 min(tokens + d, bucket).  d == 0: NOTHING changes; last stays, so the fraction of a token is not lost.
 *   spend(t, w) : earn(t); then, w != 0: tokens = min(tokens - w, bucket), last as the earn left it.  n spends at one time t are
 *                 earn(t); tokens -= n.
 *   time_until  = max(0, (int64) ceil((double)(-tokens) / rate)), fp64 division (time-until-out-of-debt-millis! without its earn).
 * Who earns (oracle-defined, like the winner rule).  The reference earns a bucket when it is accessed, and an earn in between changes
 * the result (each one drops a fraction: at rate 0.01, earn(199); earn(300) gives 2 tokens, earn(300) alone 3).  In a cycle WITH a clock
 * user u earns at now_ms iff at least one of its jobs reaches the rate-limit stage of that cycle's considerable filter, i.e.
 * passed[u] + rate_limited[u] > 0 over the whole standing queue (the upper bound of the reference's lazy access set that
 * cook_considerable documents).  The filter compares the n-th job of a user with tokens AFTER that earn (tools.clj:951-953).  One
 * clock reading serves the whole cycle (the reference reads the clock per job).  cook_cycle_autoscale reads the tokens as that cycle
 * left them and earns nothing.
 *  1. Ownership.  From the first cook_cycle_set_limiters the engine's state is what every later considerable filter of a cycle reads:
 *     rank cycles and queue cycles, single and _multi (pools with limiters beside pools without), every placement form.  user NULL: n
 *     must equal the staged users (those of cook_cycle_set_considerable's state if one is staged, else cook_cycle_stage's) and entry i
 *     is user i.  With a user list only the listed users' four values are replaced (the host's flush! after set-quota! /
 *     retract-quota!: tokens = bucket, last = now); the first call must cover every user, and its tokens are taken as current: the
 *     placements of the cycle in front of it do not spend again.  enforce_rate_limit stays in cook_user_state.
 *     While limiters are held a cook_user_state.tokens_left, a cook_user_state of another n, or a cook_queue_carry.tokens_left is
 *     refused with COOK_E_INVALID and nothing changes.  cook_cycle_set_limiters(NULL) drops them: the staged tokens_left is read again
 *     as it was staged.  cook_considerable (the stand-alone filter) never reads them.
 *  2. Clock.  cook_cycle_set_clock is host-only state: the time of the NEXT cycle.  It is consumed by the next cycle that runs the
 *     considerable filters on that engine (every existing cook_cycle_run* entry reads it; there are no new ones); a refused step
 *     leaves it staged; NULL takes it back.  Without a clock nobody earns; spends still subtract, as a spend at t <= last.
 *  3. Spend, once per cycle, at the first of: (a) the advance of the next queue cycle, in front of the filters, whether or not a carry
 *     is given: every user with KEPT placements in the pool's last cycle (job_to_offer >= 0 and the offer not in the step's
 *     offer_skipped: the predicate of step 1, the fold and the carry) does earn(spend_ms); tokens -= its kept jobs.  spend_ms is the
 *     staged clock's: when the last cycle's kept matches were launched.  With carry.usage = 1 the spend that the carry would have made
 *     on the staged tokens goes here instead.  (b) cook_cycle_limiters_spend, for the cycle no queue advance follows (the last
 *     queue cycle in front of a rank trigger, where the host restages).  A second call for the same cycle: COOK_E_STATE; an advance
 *     behind an explicit spend spends nothing.  A rank cycle never spends: what the cycle in front of it placed and did not spend
 *     explicitly is the host's to tell (a listed cook_cycle_set_limiters).
 *  4. Lifetime.  Keyed by user id; survives ranks and cook_cycle_update; cook_cycle_stage* drops it (the users are restaged).
 *     COOK_E_INVALID, nothing changed: n other than the staged users (user NULL, or the first call), a user out of range or listed
 *     twice, per_minute not finite or not above 0, bucket outside 0 .. 2^53, |tokens| above 2^53, |last_update_ms| or a clock time above
 *     2^62, pending_jobs->user not staged.  COOK_E_STATE: before cook_cycle_stage; between a deferred set-up (cook_cycle_run_rank*,
 *     cook_cycle_run_queue_rank, the _multi queue steps) and cook_cycle_match_multi, as cook_cycle_set_reservations.
 *  5. Cost.  No synchronisation of its own inside a cycle: at most three small launches of per-user work (two in the advance, one behind
 *     the rate-limit stage), counters in the advance's and the filter's read-backs.  (Additive: no existing layout changes.) */
typedef struct cook_limiters {
  uint32_t n;                    /* entries */
  const uint32_t* user;          /* [n] user ids, each at most once; NULL: n must equal the staged users, entry i is user i */
  const double* per_minute;      /* [n] tokens-replenished-per-minute (launch-rate-per-minute, quota.clj:118-133): finite, > 0 */
  const int64_t* bucket;         /* [n] bucket size, 0 .. 2^53 */
  const int64_t* tokens;         /* [n] current tokens, |tokens| <= 2^53 */
  const int64_t* last_update_ms; /* [n] */
} cook_limiters;
typedef struct cook_clock {
  int64_t now_ms;   /* the filters' clock reading of the next cycle */
  int64_t spend_ms; /* when the LAST cycle's kept matches were launched (read by the next queue cycle's advance) */
} cook_clock;
typedef struct cook_limiter_info {
  uint32_t earned;      /* users whose state the last cycle's earn moved */
  uint32_t spent_users; /* users that spent in the last advance or cook_cycle_limiters_spend */
  uint32_t in_debt;     /* users with tokens < 0 behind the last cycle's filters that ran with limiters */
  uint32_t reserved;
  int64_t spent;        /* tokens spent there */
} cook_limiter_info;
int cook_cycle_set_limiters(cook_engine* e, const cook_limiters* l); /* NULL: drop the engine's limiters */
int cook_cycle_set_clock(cook_engine* e, const cook_clock* c);       /* the time of the NEXT cycle; NULL: none */
/* offer_skipped: [offers of the LAST cycle] or NULL, n_offer_skipped as in cook_queue_step.  Needs limiters and a completed cycle
 * (COOK_E_STATE).  One synchronisation */
int cook_cycle_limiters_spend(cook_engine* e, const uint8_t* offer_skipped, uint32_t n_offer_skipped, int64_t spend_ms);
/* tokens, last_update_ms, time_until_ms: each [users] or NULL.  Changes no state; one synchronisation.  Without limiters: COOK_E_STATE */
int cook_cycle_fetch_limiters(cook_engine* e, int64_t* tokens, int64_t* last_update_ms, int64_t* time_until_ms);
/* the rate-limit stage's counts of the last cycle that ran the considerable filters (cook_considerable's rate_limited / passed, over the
 * whole standing queue): each [users of the staged state] or NULL, with or without limiters.  COOK_E_STATE when the last cycle ran no
 * filters.  One synchronisation */
int cook_cycle_fetch_rate_limit(cook_engine* e, uint32_t* rate_limited, uint32_t* passed);
/* the counts of the last cycle; all 0 without limiters */
int cook_cycle_limiter_info(cook_engine* e, cook_limiter_info* out);

/* ---- KUBE CYCLE (the distributor, cook_kube_distribute, is declared with the autoscaling calls above) ------------------------------
 * A Kubernetes-scheduler pool's cycle as ONE call (handle-kubernetes-scheduler-pool, scheduler.clj:1747-1810): gate, consider, distribute.
 *  Gate (:1767-1778): available = the saturated int64 sum of the raw capacities; max_considerable = min(max_jobs_considered,
 *   max(available, 0)), clamped to uint32.  available > min_capacity_threshold false (strict; n == 0 for any threshold >= 0): the call is
 *   PAUSED — info->paused = 1 with available and max_considerable, cluster_off all 0, cluster_info filled — and changes nothing: no
 *   advance runs, the queue is untouched, the last cycle's record is still pending (:1801-1808 without the sleep, which is the host's).
 *  Consider: rank_first = 1: a fresh rank, as cook_cycle_run; 0: a queue step, as cook_cycle_run_queue_release(step, carry, finished)
 *   with remove_mode taken as 1 whatever step says (every considered job leaves the queue, :1792-1794; step NULL: defaults).  Then the
 *   considerable filters over the standing queue and take max_considerable.  The staged offers are never read.
 *  Distribute: cook_kube_distribute's steps 1-5 over the considered jobs in considered order, L = the job's ckpt_location; the draw of
 *   considered position k is draw[k] (n_draw >= max_considerable values, each of the first max_considerable in [0, 1)) or the seed rule.
 *  task_idx receives the clusters' lists of TASK indices one after another, cluster_off[n + 1] delimits them; info->first_task holds task
 *  indices too.  More than cap entries: COOK_E_INVALID with info, cluster_off and cluster_info filled (the cycle has run); cap >=
 *  max_jobs_considered always suffices.
 * What the engine holds afterwards: the cycle is the last cycle for everything that reads positions — cook_cycle_fetch returns the
 *  queue, n_considered and a job_to_offer of all -1; cook_cycle_fetch_considerable works; cook_cycle_fetch_kube returns the cluster byte
 *  per considered position.  cook_match_explain, cook_match_metrics* and cook_cycle_autoscale* return COOK_E_STATE: no placement ran.
 * The next advance (of a Kubernetes cycle or of any queue cycle) treats a job that got a cluster as the cycle's kept placement for the
 *  user state: with carry->usage = 1 its resources join usage_* and the pool usage in considered order (the order rule of the carry),
 *  its user spends one token (staged tokens, or the engine's limiters), as process-task-post-launch! does for both handlers (:866-872).
 *  It adds nothing to the groups' cotask lists (the host is unknown until kube-scheduler binds; pass step->groups when it is known).
 *  Jobs without a cluster carry nothing and spend nothing.
 *  offer_skipped (of the step, of cook_cycle_limiters_spend) is NOT read behind a Kubernetes cycle: that cycle's job_to_offer names no
 *  offer, so a skipped offer says nothing about its jobs; its length is still checked as the step always checks it.
 * Refused before anything changes: COOK_E_INVALID — c, clusters, cluster_off or (n > 0) cluster_info NULL, n > COOK_MAX_CLUSTERS, a NULL
 *  cluster column, step->offers, carry->offers = 1, finished->offers = 1 (such a pool has no offer table to edit), n_draw <
 *  max_considerable, a draw that is NaN or outside [0, 1), cap > 0 with task_idx NULL, and whatever the queue step refuses;
 *  COOK_E_STATE — before cook_cycle_stage, a queue step without a completed cycle, between a deferred set-up (cook_cycle_run_rank*)
 *  and cook_cycle_match_multi. */
typedef struct cook_kube_cycle {
  uint32_t rank_first;               /* 1: rank, consider, distribute; 0: a queue step                                   */
  uint32_t max_jobs_considered;
  int64_t min_capacity_threshold;
  const cook_queue_step* step;       /* rank_first = 0; NULL: defaults.  offers must be NULL; groups: the cotask table when the hosts are known */
  const cook_queue_carry* carry;     /* rank_first = 0; or NULL */
  const cook_finished* finished;     /* rank_first = 0; or NULL */
  const cook_kube_clusters* clusters;
  const double* draw;                /* [n_draw] or NULL */
  uint32_t n_draw, reserved;
  uint64_t seed;
} cook_kube_cycle;
int cook_cycle_run_kube(cook_engine* e, const cook_kube_cycle* c, uint32_t* task_idx, uint32_t cap, uint32_t* cluster_off /* [n + 1] */,
                        cook_kube_cluster_info* cluster_info /* [n] */, cook_kube_info* info /* or NULL */);
/* ... for the Kubernetes-scheduler pools of a GPU in one pool batch: the pools' advances, filters and distributions side by side, the
 * distributor launched once with blockIdx.y as the pool.  Engine i's results, code and message are those of the single call; a paused
 * pool, a refused pool and a pool that considers nothing can each sit beside good ones.  COOK_E_INVALID with nothing run: engines,
 * cycles, cap, cluster_off or cluster_info NULL, n == 0, a NULL entry of engines or cycles, an engine twice. */
int cook_cycle_run_kube_multi(cook_engine** engines, uint32_t n, const cook_kube_cycle* const* cycles, uint32_t* const* task_idx,
                              const uint32_t* cap, uint32_t* const* cluster_off, cook_kube_cluster_info* const* cluster_info,
                              cook_kube_info* info /* [n] or NULL */, int* rc /* [n] or NULL */);
/* choice[k] = the cluster of considered position k of the last cycle (COOK_KUBE_NO_CLUSTER: none), *n_out = their number.  COOK_E_STATE
 * unless the last cycle was a Kubernetes cycle.  One synchronisation. */
int cook_cycle_fetch_kube(cook_engine* e, uint8_t* choice, uint32_t* n_out);

/* ---- REBALANCE: replaces init-state + the rebalance loop's decisions ---------------------------------------
 * (rebalancer.clj:222-266, 320-407, 270-309, 434-467; dru.clj:128-144).
 * running: the pool's running tasks with host ids.  running_attrs_cached (optional, len running->n): 0 = the instance's
 * slave id has no entry in the agent-attributes-cache (its host then resolves to a nil attribute map when that task is
 * the last scored task of the host, rebalancer.clj:369-375); NULL = all cached.
 * pending: the allowed-to-start pending jobs in rank order (rebalancer.clj:588-590); the loop stops after
 * params->max_preemption decisions.  pending->reserved_host is ignored (the rebalancer evaluates
 * job-constraint-constructors only, constraints.clj:459-466).
 * host_attrs (optional): the agent-attributes-cache as a cook_offers table, one row per cached host (host[i] = host id;
 * cpus/mem and the run_* / *_tasks columns are ignored).  groups (optional): pending->group[p] indexes it; run_host =
 * hosts of the group's running cotasks (run_attr is ignored: attributes come from host_attrs).
 * decisions capacity = pending->n; preempted capacity = running->n + pending->n (task indices into `running`;
 * COOK_NONE_U32 = a job placed earlier in this call, which the caller skips, rebalancer.clj:529).
 * pending_dru (optional, len pending->n): the pending-job DRU of every job examined (rebalancer.clj:157-208), NaN otherwise. */
int cook_rebalance(cook_engine* e, const cook_tasks* running, const uint8_t* running_attrs_cached, const cook_jobs* pending,
                   const int64_t* pending_job_id, const int32_t* pending_priority, const cook_users* users,
                   const cook_host_spare* spare, const cook_offers* host_attrs, const cook_groups* groups,
                   const cook_rebalance_params* params, cook_preemption* decisions, uint32_t* n_decisions,
                   uint32_t* preempted, uint32_t* n_preempted, double* pending_dru);
int cook_rebalance_stage(cook_engine* e, const cook_tasks* running, const uint8_t* running_attrs_cached,
                         const cook_jobs* pending, const int64_t* pending_job_id, const int32_t* pending_priority,
                         const cook_users* users, const cook_host_spare* spare, const cook_offers* host_attrs,
                         const cook_groups* groups, const cook_rebalance_params* params);
int cook_rebalance_run(cook_engine* e);
int cook_rebalance_fetch(cook_engine* e, cook_preemption* decisions, uint32_t* n_decisions, uint32_t* preempted,
                         uint32_t* n_preempted, double* pending_dru);
/* HIP-event time of the last cook_rebalance_run in milliseconds */
int cook_rebalance_timing(cook_engine* e, double* ms);

/* ---- REBALANCE FROM THE RESIDENT CYCLE STATE: cook_rebalance_stage without the host rebuilding and uploading what the engine holds ------
 * For a pool driven through cook_cycle_*: the stage is built on the device from the resident task table (cook_cycle_stage /
 * cook_cycle_update, with cook_tasks.host), the standing ranked queue, the pending-job columns, the staged users, groups and offers.
 * It is followed by cook_rebalance_run, cook_rebalance_timing and cook_cycle_rebalance_fetch; the run and its kernels are those of
 * cook_rebalance.  The host column: cook_cycle_stage keeps cook_tasks.host when it is given (without it there is no column);
 * cook_cycle_update carries it, new rows take add_tasks->host.  A delta that adds RUNNING rows without host to an engine that has the
 * column is not refused: the column counts as incomplete until the next cook_cycle_stage that passes host.
 * THE DERIVED INPUTS.  stage -> run -> fetch equals cook_rebalance called with:
 *  - running: the rows of the resident task table with pending == 0, in ascending row order, every column, host included;
 *    running_attrs_cached = NULL.
 *  - pending: the standing queue in order (the ranked_pending_idx cook_cycle_fetch would return now), without the jobs whose byte in
 *    the eligible mask of cook_cycle_set_considerable is 0 (no mask: all eligible — the host evaluates job-allowed-to-start? there);
 *    with skip_matched also without the jobs the last placement considered, matched and kept (job_to_offer >= 0 and the offer not in
 *    offer_skipped: the predicate of step 1 of the queue cycles; no placement since the rank: none); of those the first
 *    params.max_preemption (<= 0: none).  Job columns: the resident pending-job columns by pending ordinal, the two CSR columns
 *    included (user: the job column, without one the task row's); pending_job_id and pending_priority: the job's task row.
 *  - users: the staged cook_users.  groups: the staged group table as it stands (type, attr_key, minimum, run_off / run_host).
 *  - spare == NULL: one entry per staged offer row: host, cpus and mem are the row's; gpus is the sum of the row's gpu_count slots in
 *    slot order (0.0 without the column).  That sum is defined by the oracle, not by the reference, which reads
 *    host->spare-resources from view-incubating-offers with one gpus figure per host.
 *  - host_attrs == NULL: the staged offer rows are the attribute table.
 *  - a non-NULL spare or host_attrs is uploaded as cook_rebalance_stage does.  Dense host ids are assumed (H = greatest id + 1).
 * COOK_E_INVALID: spare or host_attrs NULL while two staged offers share a host; skip_matched above 1; offer_skipped without
 * skip_matched; reserved not 0; what cook_rebalance_stage refuses.
 * COOK_E_STATE: before a completed rank since the last cook_cycle_stage / cook_cycle_update (as cook_unscheduled); without a
 * complete host column; after any queue cycle since that rank (the task table then no longer lists what runs: a queue cycle adds no
 * running rows); while a placement is set up and has not run.  So the host runs the rebalancer at a rank trigger:
 * cook_cycle_update -> cycle -> cook_cycle_rebalance_stage -> cook_rebalance_run -> cook_cycle_rebalance_fetch ->
 * cook_cycle_set_reservations.  The call changes nothing that a cycle, a queue cycle, explain, metrics, user stats, unscheduled or
 * usage reads.  The arrays are read until the call returns; two stream synchronisations. */
typedef struct cook_cycle_rebalance {
  cook_rebalance_params params;
  const cook_host_spare* spare;  /* NULL: from the staged offers                                                             */
  const cook_offers* host_attrs; /* NULL: the staged offer rows are the attribute table                                      */
  const uint8_t* offer_skipped;  /* with skip_matched: per offer of the last match, as cook_queue_step's; NULL = none skipped */
  uint32_t skip_matched;         /* 1: jobs the last placement matched and kept do not count as pending                      */
  uint32_t reserved;             /* 0 */
} cook_cycle_rebalance;
int cook_cycle_rebalance_stage(cook_engine* e, const cook_cycle_rebalance* req);
/* The result in the host's index spaces (any pointer may be NULL).  decisions[].pending_index indexes the selected list:
 * selected_task_idx[p] is that job's task index (the space of cook_cycle_fetch's ranked_pending_idx), selected_pending_ord[p] its
 * pending ordinal (the key of cook_reservations); *n_selected their count.  preempted_task_idx holds rows of the resident task
 * table, translated on the device (COOK_NONE_U32 = a job placed earlier in this call).  Capacities: decisions, pending_dru and the two
 * maps min(max_preemption, ranked jobs); preempted_task_idx the running rows + that.  COOK_E_STATE unless the last stage was
 * cook_cycle_rebalance_stage and cook_rebalance_run has run.  cook_rebalance_fetch behind a resident stage keeps working and reports
 * the compacted spaces: preempted = ordinal among the running rows, pending_index = index into the selected list. */
int cook_cycle_rebalance_fetch(cook_engine* e, cook_preemption* decisions, uint32_t* n_decisions, uint32_t* preempted_task_idx,
                               uint32_t* n_preempted, double* pending_dru, uint32_t* selected_task_idx,
                               uint32_t* selected_pending_ord, uint32_t* n_selected);

/* ---- EXPLAIN: the placement-failure summary of a job ("why unscheduled") --------------------------------------------
 * Replaces fenzo-utils/summarize-placement-failure over the TaskAssignmentResults Fenzo returns for an unassigned task
 * (scheduler/fenzo_utils.clj:33-55, written to :job/last-fenzo-placement-failure at :71-89 and read back by
 * unscheduled.clj:95-110).  For every job position of job_pos (an index into the jobs of the engine's LAST match: cook_match_run,
 * cook_cycle_run or the lockstep pair) and every offer, against the state that job saw (the placements of the jobs ranked
 * before it): the resources that did not fit ("cpus" / "mem", one count each per host) or else the FIRST failing hard constraint
 * in the order Fenzo walks them ((into (list) constraints), scheduler.clj:493-501: checkpoint-locality, estimated-completion,
 * user-defined, disk-host, gpu-host, novel-host, max_tasks_per_host, rebalancer-reservation, the group constraint) or else a zero
 * fitness.  counts is [n][COOK_WHY_SLOTS] host counts; the reference's map is {:resources {"cpus" c0 "mem" c1} :constraints
 * {<name> count ...}} over the non-zero slots.  For a job that was matched the row describes the hosts that refused it. */
#define COOK_WHY_CPUS 0                /* :resources "cpus"                                        */
#define COOK_WHY_MEM 1                 /* :resources "mem"                                         */
#define COOK_WHY_FITNESS 2             /* fitness calculator returned 0.0                          */
#define COOK_WHY_CHECKPOINT_LOCALITY 3 /* "checkpoint_locality_constraint" (constraints.clj:218)  */
#define COOK_WHY_ESTIMATED_COMPLETION 4 /* "estimated_completion_constraint" (:385)                */
#define COOK_WHY_USER_DEFINED 5        /* "user_defined_constraint" (:356)                         */
#define COOK_WHY_DISK_HOST 6           /* "disk_host_constraint" (:164)                            */
#define COOK_WHY_GPU_HOST 7            /* "gpu_host_constraint" (:122)                             */
#define COOK_WHY_NOVEL_HOST 8          /* "novel_host_constraint" (:68)                            */
#define COOK_WHY_MAX_TASKS 9           /* "max_tasks_per_host" (:438)                              */
#define COOK_WHY_RESERVATION 10        /* "rebalancer_reservation_constraint" (:242)               */
#define COOK_WHY_GROUP_UNIQUE 11       /* "unique_host_placement_group_constraint" (:586)          */
#define COOK_WHY_GROUP_BALANCED 12     /* "balanced_host_placement_group_constraint" (:600)        */
#define COOK_WHY_GROUP_ATTR_EQUALS 13  /* "attribute_equals_host_placement_group_constraint" (:628) */
#define COOK_WHY_SCALAR0 14            /* :resources <name of scalar 0>; 15, 16: scalars 1, 2 (the failure's message is the name,
                                          fenzo_utils.clj:21-45).  COOK_WHY_CPUS / _MEM are the cpus / mem tests, which are
                                          the named "cpus" / "mem" tests unless a pool adjuster makes them differ */
#define COOK_WHY_PORTS 17              /* ports did not fit.  Fenzo's PORTS failure carries no message, so the reference's
                                          summary has no entry for it (count-resource-failure skips it); kept for operators */
#define COOK_WHY_SLOTS 20
int cook_match_explain(cook_engine* e, const uint32_t* job_pos, uint32_t n, uint32_t* counts);

/* ---- METRICS: the numbers of handle-match-cycle-metrics (scheduler.clj:1210-1280) from the last match, on the device -----
 * resource-maps->stats (scheduler.clj:547-582) of "cpus" and "mem": :totals summed in collection order (bit-identical to the
 * reference's reduce), :percentiles by nearest rank over the sorted values (task_stats.clj:59-80), :largest-by = the last
 * element of the stable sort by that resource (index in collection order).  An empty collection gives NaN / COOK_NONE_U32. */
typedef struct cook_resource_stats {
  double total_cpus, total_mem;
  double p50_cpus, p95_cpus, p100_cpus;
  double p50_mem, p95_mem, p100_mem;
  uint32_t largest_by_cpus, largest_by_mem;
} cook_resource_stats;
typedef struct cook_cycle_metrics {
  uint32_t considerable, matched, unmatched; /* number-considerable-jobs / -matched-jobs / -unmatched-jobs (:1383-1385)     */
  uint32_t offers, offers_scheduled;         /* (count offers), (count offers-scheduled) = leases used (:1372-1374)        */
  uint32_t head_matched;                     /* matched-considerable-jobs-head? (:1381): job 0 is among the matched         */
  uint32_t reserved[2];
  cook_resource_stats jobs;                  /* jobs->stats of the considerable jobs (:594-600)                            */
  cook_resource_stats offer_stats;           /* offers->stats (:584-592)                                                   */
} cook_cycle_metrics;
/* user_considerable / user_matched (optional, len n_users): frequencies of the jobs' users (:1216-1227; needs the jobs' user
 * column).  job_gpus_by_model / offer_gpus_by_model (optional, len n_gpu_models + 1, by model id; jobs without a model under
 * 0): the "gpus/<model>" entries of :totals.  match-percent, queue-was-full? and the unmatched-cycles bookkeeping
 * (:1404-1486) are host arithmetic on these numbers. */
int cook_match_metrics(cook_engine* e, cook_cycle_metrics* out, uint32_t* user_considerable, uint32_t* user_matched, uint32_t n_users,
                       int64_t* job_gpus_by_model, int64_t* offer_gpus_by_model, uint32_t n_gpu_models);
/* cook_match_metrics for every pool of a GPU in ONE call from one thread (one pool batch, as cook_cycle_autoscale_multi): the call makes the
 * two stream synchronisations of one pool's call, and the same kernel of several pools is one launch.  Engine i's result, code and message
 * are exactly those of cook_match_metrics with req[i]'s arguments; errors, rc and the one-after-another cases as cook_cycle_autoscale_multi
 * (COOK_E_INVALID with nothing run: engines or req NULL, n == 0, a NULL engine, an engine twice). */
typedef struct cook_metrics_req {   /* the arguments of cook_match_metrics for one engine */
  cook_cycle_metrics* out;          /* required */
  uint32_t* user_considerable; uint32_t* user_matched; uint32_t n_users;
  uint32_t n_gpu_models; int64_t* job_gpus_by_model; int64_t* offer_gpus_by_model;
} cook_metrics_req;
int cook_match_metrics_multi(cook_engine** engines, uint32_t n, const cook_metrics_req* req /* [n] */, int* rc /* [n] or NULL */);

/* ---- LAUNCH RESOURCES: the assigned ports and the per-role takes of every placed task of the last match, on the device ----------
 * What a Mesos pool needs between the match and the launch: TaskAssignmentResult->task-metadata's :ports-assigned = (vec (sort
 * getAssignedPorts)) (mesos/task.clj:162-169; written as :instance/ports, scheduler.clj:817-832; the PORT0..PORTn variables and the
 * docker port mappings, mesos/task.clj:223-236, :322-330) and compile-mesos-messages' split of every placed task's resources over the
 * host's Mesos roles (mesos/task.clj:404-416: resources-by-role, take-resources, take-all-scalar-resources-for-task,
 * add-scalar-resources-to-task-infos, take-ports).  Called after any match of the engine, exactly as cook_match_explain is
 * (cook_match_run, cook_cycle_run*, the queue cycles, cook_cycle_match_multi); it reads that match's resident job_to_offer and job
 * columns (through the match's j_index where the match read them through it) and writes nothing that any other call reads.
 *
 * Inputs (cook_launch_offers): the ROLE VIEW of the offers of that match, indexed by offer row; n must equal the match's offer count.
 *  - n_roles: 1 .. COOK_MAX_ROLES.  Role ids are given in TAKE order: the caller orders them as (sort-by #(= "*" %) (keys avail))
 *    does, the "*" role last.  A role a host does not have is passed as amount 0.0 and no range: the reference's
 *    (or (remaining-resources role-name) 0), which yields no message.
 *  - port ranges as a CSR: range_off[n + 1], range_begin[], range_end[] (INCLUSIVE, as range-contains? is), range_role[] (< n_roles).
 *    The ranges of a row are in the order of the lease's portRanges (offer.clj:70-72); over several Mesos offers of one host, in the
 *    order of resources-by-role's (reduce into).  The ranges of a row must be pairwise disjoint and satisfy 0 <= begin <= end:
 *    otherwise COOK_E_INVALID with the row in info->bad_row, and nothing is written.  Given that, role-containing-port of a port is
 *    the role of the range it came from.
 *  - n_res resource slots, 1 .. 2 + COOK_MAX_SCALARS; res_source[r] says which job column of the match is slot r's request:
 *    COOK_LAUNCH_CPUS, COOK_LAUNCH_MEM or COOK_LAUNCH_SCALAR0 + s (getScalarRequests = job->scalar-request, scheduler.clj:177-189; the
 *    note at COOK_MAX_SCALARS applies: under a pool adjuster, scalars 0 / 1 hold the un-adjusted cpus / mem).  A NaN request means
 *    the job has no request under that name: nothing is taken.
 *  - avail[n_res][n_roles][n] (slot-major, then role, then row): the resources-by-role amount of each (slot, role, row).  Values must
 *    be finite and >= 0; anything else: COOK_E_INVALID with info->bad_row.
 *  - offer_skipped (optional, [n]): filter-matches-for-ratelimit's verdict, as in cook_queue_step.  Tasks on a skipped offer are not
 *    launched and get nothing.
 * bad_row is the LOWEST offending row, whatever its fault (ranges, amounts, ports short).
 *
 * Semantics.  "Kept" is the carry's predicate: placed, and its offer not skipped.  The kept tasks of an offer are taken in considered
 * order: Fenzo's assignment order on the VM, and the order of :tasks in a match.
 *  - PORTS.  Fenzo 0.10.0's source is not in the tree, so this rule is ORACLE-DEFINED, like the tie rules: a fresh set of leases
 *    starts the VM's port cursor at 0; the c-th consumed port is the c-th port of the row's ranges concatenated in their given order;
 *    with c_k = the sum of `ports` over the kept tasks ahead of task k on its offer, task k gets ports number c_k .. c_k + ports_k - 1
 *    of that sequence.  They are returned ASCENDING per task ((vec (sort ...)): a task's slice can span ranges that are not
 *    ascending), each with its role.  A row whose kept tasks ask for more ports than its ranges hold: COOK_E_INVALID with
 *    info->bad_row, nothing written (the match cannot produce this when cook_offers.ports was the ranges' size; under a carry the
 *    caller passes the host's CURRENT ranges).
 *  - SCALARS.  take-resources, literally: per (offer, slot), task after task, role after role in take order:
 *    take = min(still_needed, avail[role]); if take > 0: still_needed -= take, avail[role] -= take, and a message (role, take) is
 *    emitted.  Every subtraction is a plain fp64 operation in exactly that order: the results are bit-identical to the sequential
 *    reduce for ANY inputs (the promise of the carry's folds).
 *
 * Outputs (cook_launch_out), all in the caller's memory and indexed by considered position k in [0, K) (K = cook_match_count):
 * port_off[K + 1], port[cap] (int32) and port_role[cap] (uint8): task k's ports are port[port_off[k] .. port_off[k + 1]);
 * take[K][n_res][n_roles] (fp64; 0.0 = no message); short_mask[K]: bit r set when slot r's :amount-still-needed is not 0.
 * info: kept tasks, ports, offers used (rows with a kept task), tasks with a short slot, bad_row (COOK_NONE_U32: none).  A task that was
 * not kept gets an empty port list and a zero row.  More than cap ports: COOK_E_INVALID with info filled in and nothing else written.
 *
 * Refused before the first launch, whatever the host can know — COOK_E_INVALID: offers, out, info or a needed array NULL, n other
 * than the match's offer count, n_roles / n_res out of range, a res_source that names no column or a scalar the match did not have,
 * range_off not starting at 0 or decreasing.  COOK_E_STATE: no match yet, a deferred set-up that has not run, or a Kubernetes-scheduler
 * cycle (as cook_match_explain answers there).  A refused call changes nothing but *info (zeros, bad_row = COOK_NONE_U32 unless said
 * otherwise above).  Two stream synchronisations: the first brings the error word and the totals (failures are all-or-nothing, as in
 * cook_usage_breakdown), the second ends the copies (and brings one word: COOK_E_STATE "internal inconsistency" after it means that the
 * engine caught itself writing a port out of place — no input can cause it, and the outputs are then not valid).  Left to the host: keeping a host's ranges across a carry or a release, the
 * task-info protobufs, executor choice, slave ids. */
#define COOK_MAX_ROLES 4
#define COOK_LAUNCH_CPUS 0    /* res_source: the match's cook_jobs.cpus */
#define COOK_LAUNCH_MEM 1     /* ... cook_jobs.mem                      */
#define COOK_LAUNCH_SCALAR0 2 /* ... + s: named scalar s                */
typedef struct cook_launch_offers {
  uint32_t n, n_roles, n_res, reserved;
  const uint32_t* range_off;    /* [n + 1]                                  */
  const int32_t* range_begin;   /* [range_off[n]]                           */
  const int32_t* range_end;
  const uint8_t* range_role;
  const uint32_t* res_source;   /* [n_res]                                  */
  const double* avail;          /* [n_res][n_roles][n]                      */
  const uint8_t* offer_skipped; /* [n] or NULL                              */
} cook_launch_offers;
typedef struct cook_launch_out {
  uint32_t cap, reserved;       /* room of port / port_role, in ports       */
  uint32_t* port_off;           /* [K + 1]                                  */
  int32_t* port;                /* [cap]                                    */
  uint8_t* port_role;           /* [cap]                                    */
  double* take;                 /* [K][n_res][n_roles]                      */
  uint32_t* short_mask;         /* [K]                                      */
} cook_launch_out;
typedef struct cook_launch_info {
  uint32_t kept, ports, offers_used, short_tasks, bad_row, reserved[3];
} cook_launch_info;
int cook_match_launch_resources(cook_engine* e, const cook_launch_offers* offers, cook_launch_out* out, cook_launch_info* info);

/* ---- USER STATISTICS: the arithmetic of set-stats-counters! (monitor.clj:40-116, 177-207) from the last rank, on the device --------
 * Per user u and state s (0 running, 1 waiting, 2 starved, 3 waiting-under-quota): per_user[(u*4 + s)*3 + {0,1,2}] = {jobs, cpus, mem};
 * a user absent from a state's map (monitor.clj builds maps) has zeros there and its bit clear in user_state[u] (COOK_USTAT_*).
 *  - running / waiting (get-job-stats, :40-57): sums over the user's running / pending tasks of the engine's task table (cook_rank_stage,
 *    cook_cycle_update) as the LAST rank run saw it.
 *  - starved (:69-90): waiting, and running cpus < share cpus and running mem < share mem (absent running = 0.0); stats
 *    (merge-with min waiting (merge-with - share running)): cpus = min(w.cpus, s.cpus - r.cpus), mem likewise, jobs = min(w.jobs,
 *    r.jobs) — :jobs only exists in running, so with running stats it passes the first merge unchanged —, and without running stats
 *    min(w, share) with jobs = w.jobs.
 *  - waiting-under-quota (:92-116): waiting, and r.jobs < quota count, r.cpus < quota cpus, r.mem < quota mem, 0 < quota gpus and every
 *    other quota key (the launch-rate quotas) > 0; stats min(w, max(quota - r, 0)) on jobs / cpus / mem (min(w, quota) without running
 *    stats).  Only jobs / cpus / mem are returned: the reference's map also carries the user's gpus and launch-rate quotas unchanged,
 *    which the host holds already.
 *  - totals: the "all" row of each state (add-aggregated-stats, :59-67; all zeros when the map is empty) and the counts of :186-194 —
 *    total |running u waiting|, starved, waiting-under-quota, hungry |waiting \ starved|, satisfied |running \ waiting|.
 * Values are doubles; set-counter!'s (long (min v Long/MAX_VALUE)) is the host's.  Oracle-defined summation order (the reference's
 * is Datomic query / hash-map order): per user left to right in the user's task order (tools.clj:614-641), running and pending tasks
 * apart; "all" left to right in user-id order; bit-identical to those sequential sums for any fp64 inputs (exactness tracked, rounded
 * sums folded again).  The rank, considerable and match state stay as they are: a cycle fetched afterwards is the one fetched before.
 * Before any cook_rank_run / cook_cycle_run*, and after a cook_rank_stage or cook_cycle_update that no rank has followed (the rank's
 * per-user order would describe the old table): COOK_E_STATE. */
typedef struct cook_user_limits {
  uint32_t n;                           /* users (the engine's U; n_users of the multi form)                                       */
  const double* share_cpus;             /* [n] get-shares [:cpus :mem] (share.clj:123); unset = DBL_MAX                            */
  const double* share_mem;
  const double* quota_count;            /* [n] get-quota (quota.clj:82-110): :count, :cpus, :mem, :gpus                             */
  const double* quota_cpus;
  const double* quota_mem;
  const double* quota_gpus;
  const uint8_t* extra_quota_positive;  /* [n] every other quota key > 0, or NULL = all positive (the launch-rate defaults are)     */
} cook_user_limits;
typedef struct cook_user_stats_totals {
  double all[4][3];                     /* the "all" row of running, waiting, starved, waiting-under-quota: {jobs, cpus, mem}          */
  uint32_t total, starved, waiting_under_quota, hungry, satisfied, reserved;
} cook_user_stats_totals;
#define COOK_USTAT_RUNNING 1u
#define COOK_USTAT_WAITING 2u
#define COOK_USTAT_STARVED 4u
#define COOK_USTAT_UNDER_QUOTA 8u
/* limits NULL: the engine's staged cook_users (the DRU divisors as shares, the quotas as they are).  per_user (optional) [U][4][3];
 * per_user_is_device != 0: per_user is a DEVICE pointer and nothing of it is copied to the host.  user_state (optional) [U]; totals
 * (optional). */
int cook_user_stats(cook_engine* e, const cook_user_limits* limits, double* per_user, int per_user_is_device, uint8_t* user_state,
                    cook_user_stats_totals* totals);
/* The same for a quota group (monitor.clj:35-38 job-ent-in-pool: the jobs of every member pool) whose pools are engines of ONE device:
 * user_map[i] (NULL, or user_map[i] NULL: the identity) maps engine i's user ids one-to-one into the group's n_users; group_limits
 * (required) are the group's own.  Per-user sums run over the concatenation of the member pools' segments in the order of `engines`.
 * Engines on different devices, an engine twice, a map out of range or not one-to-one: COOK_E_INVALID. */
int cook_user_stats_multi(cook_engine** engines, uint32_t n, const uint32_t* const* user_map, uint32_t n_users,
                          const cook_user_limits* group_limits, double* per_user, int per_user_is_device, uint8_t* user_state,
                          cook_user_stats_totals* totals);

/* ---- UNSCHEDULED: the reasons of /unscheduled_jobs that need the user's whole task list, from the last rank, on the device ----------
 * cook.unscheduled/reasons (unscheduled.clj:178-206) asks, for ONE waiting job, two Datomic queries (the user's running jobs, the
 * user's first 100 waiting jobs of the last 7 days), sorts the tasks with same-user-task-comparator and sums every running job's
 * usage.  cook_unscheduled answers the three reasons that are made of that data for every row of the staged task table at once, or
 * for a list of rows:
 *  - check-exceeds-limit with quota/get-quota and with share/get-share (:37-77, how-job-would-exceed-resource-limits), pending rows
 *    only: total[k] = (sum over the user's running rows of k) + the job's own k, k in {count (1 per row), cpus, mem, gpus (0.0 where
 *    the gpus column is NULL)}; COOK_UNSCHED_QUOTA_{COUNT,CPUS,MEM,GPUS} iff total[k] > quota[k], COOK_UNSCHED_SHARE_{CPUS,MEM,GPUS}
 *    iff total[k] > share[k] (strict, :48).  total holds the :usage numbers of the reason's data map; the :limit numbers are the
 *    caller's inputs.  A running row gets none of these bits and zeros in total.
 *  - check-queue-position (:128-158).  A user's LIST is its running rows plus its pending rows that are in the window, in the user's
 *    task order of the last rank (tools.clj:614-641: sorted-tasks).  A running row stands for "the last running instance of a running
 *    job", as everywhere in the engine (one row per job).  queue_pos = the number of list entries in front of the row when the row is
 *    in the list; otherwise the list's length, and COOK_UNSCHED_AT_LEAST is set ("You have at least N other jobs ...").
 *    COOK_UNSCHED_QUEUE_POSITION iff queue_pos > 0 ((seq tasks-ahead)).  The tasks ahead are the first min(queue_pos, 10) entries of
 *    the user's list: ahead[u][0..9] (task rows, COOK_NONE_U32 beyond the list's length) and list_len[u] are returned once per user.
 * in_window (optional, [tasks.n] bytes by task row): for a pending row, whether the host's "first 100 waiting jobs of the last 7 days"
 * query (:117-126, 196) returns that job; NULL = every pending row.  It is an input mask like cook_queue's eligible: the engine does
 * not know Datomic's order.  Running rows ignore it.
 * Oracle-defined where the reference depends on Datomic order: the reference sums (conj running-jobs job) over a query result; here
 * the running rows are added left to right in the user's task order, starting from the first of them, and the job last.  Every
 * returned sum is bit-identical to that sequential sum for any fp64 inputs (exactness tracked over every prefix, a user whose sums
 * rounded is folded again left to right).
 * What stays with the host: check-exhausted-retries (two Datomic attributes), check-launch-rate-limit (the host holds
 * cook_considerable's rate_limited counts; the caveat at that call applies), check-plugin-filter, check-fenzo-placement
 * (cook_match_explain), the message strings and the job UUIDs behind the row numbers.
 * The call reads the per-user order of the LAST rank run in place and writes nothing that rank, considerable, match, autoscale or any
 * other call reads.  Before any cook_rank_run / cook_cycle_run*, and after a cook_rank_stage or cook_cycle_update that no rank has
 * followed: COOK_E_STATE (the rule of cook_user_stats). */
typedef struct cook_unsched_limits {
  uint32_t n;                 /* users (the engine's U)                                                                       */
  const double* quota_count;  /* [n] get-quota (quota.clj:82-110): :count, :cpus, :mem, :gpus; unset = DBL_MAX (count 2^31 - 1)  */
  const double* quota_cpus;
  const double* quota_mem;
  const double* quota_gpus;
  const double* share_cpus;   /* [n] get-share (share.clj:105-119): :cpus, :mem, :gpus; unset = DBL_MAX                          */
  const double* share_mem;
  const double* share_gpus;
} cook_unsched_limits;
#define COOK_UNSCHED_QUOTA_COUNT 1u
#define COOK_UNSCHED_QUOTA_CPUS 2u
#define COOK_UNSCHED_QUOTA_MEM 4u
#define COOK_UNSCHED_QUOTA_GPUS 8u
#define COOK_UNSCHED_SHARE_CPUS 16u
#define COOK_UNSCHED_SHARE_MEM 32u
#define COOK_UNSCHED_SHARE_GPUS 64u
#define COOK_UNSCHED_QUEUE_POSITION 128u
#define COOK_UNSCHED_AT_LEAST 256u
#define COOK_UNSCHED_AHEAD 10u
/* limits NULL: the engine's staged cook_users (its div_* as shares, its quota_*); a wrong n or a NULL column: COOK_E_INVALID.
 * rows (optional): n_rows task-row indices into the staged cook_tasks, any order, repeats allowed, running or pending; NULL = all
 * tasks.n rows in row order; n_rows is then 0, or the caller's idea of tasks.n, which is checked (a binding that sized its buffers by
 * it: COOK_E_INVALID when it is wrong).  A row >= tasks.n: COOK_E_INVALID, nothing written.
 * Outputs, each optional, caller-allocated, n = n_rows (tasks.n when rows is NULL): reasons[n] (COOK_UNSCHED_* bits), queue_pos[n],
 * total[n][4] = {count, cpus, mem, gpus} (total_is_device != 0: a DEVICE pointer, nothing of it is copied to the host),
 * ahead[U][COOK_UNSCHED_AHEAD], list_len[U]. */
int cook_unscheduled(cook_engine* e, const cook_unsched_limits* limits, const uint8_t* in_window, const uint32_t* rows, uint32_t n_rows,
                     uint32_t* reasons, uint32_t* queue_pos, double* total, int total_is_device, uint32_t* ahead, uint32_t* list_len);

/* ---- USAGE: GET /usage with its job-group breakdown, from the last rank, on the device ---------------------------------------------
 * rest/api.clj:2894-2969 (user-usage, usage, get-user-usage) loads every running job entity, groups by user, by pool and — with
 * group_breakdown=true — by job group, and reduces each bucket with tools/total-resources-of-jobs (tools.clj:294-306: reduce from
 * {:cpus 0.0 :mem 0.0 :gpus 0.0 :jobs n}, merge-with + of the jobs' resources) while collecting the bucket's job list.
 *  - A JOB is a running row (pending == 0) of the engine's staged task table, as everywhere in the engine (one row per running job).
 *    Pending rows take no part.
 *  - group_of_row ([tasks.n] by task row): the host-interned id in [0, n_groups) of job-ent->group-uuid, COOK_NONE_U32 = nil; NULL =
 *    every row ungrouped.  An input column like cook_unscheduled's in_window: the engine does not keep it.  Values of pending rows are
 *    ignored.  A running row's value >= n_groups that is not COOK_NONE_U32: COOK_E_INVALID, nothing written.
 *  - A BUCKET is (user, group or none).  bucket_usage[b] = {cpus, mem, gpus, jobs}: starting from 0.0, the bucket's rows added left to
 *    right in the user's task order of the last rank (tools.clj:614-641); gpus is 0.0 where the gpus column is NULL; jobs = the number
 *    of rows.  rows[row_off[b] .. row_off[b+1]) = the bucket's task rows in that order (:running-jobs; the host holds the UUIDs).
 *  - total[u] (:total-usage, api.clj:2903-2905) = the same reduction over ALL running rows of the user in the user's task order.  It is
 *    not the sum of the user's buckets: for fractional inputs the two differ in the last bits.
 *  - Oracle-defined where the reference's order is a Clojure hash map's or a Datomic query's: users in user-id order (or the order of
 *    `users`); the buckets of user k are bucket_off[k] .. bucket_off[k+1]: the ungrouped bucket FIRST (bucket_group = COOK_NONE_U32),
 *    then the grouped ones in ascending group id.  Only non-empty buckets are stored: a user without an ungrouped job has no
 *    COOK_NONE_U32 bucket, for which the reference answers zero usage and an empty list (:2913-2915); a user without running rows has
 *    no bucket and a zero total (no-usage-map, :2917-2923).
 *  - Every returned double is bit-identical to that sequential sum for any fp64 input (exactness tracked over every prefix of every
 *    bucket and user; one with a rounded prefix, or a -0.0 among its values, is folded again left to right).
 *  - users (optional; n_list user ids, any order, repeats allowed — the ?user= request): the same outputs for the listed users only, in
 *    list order; n_out = n_list.  NULL: all users, n_out = the number of users.  A user id that is no user: COOK_E_INVALID.
 * Outputs (cook_usage_out), each pointer optional and caller-allocated: bucket_off[n_out + 1], bucket_group[cap_rows],
 * bucket_usage[cap_rows][4], row_off[cap_rows + 1], rows[cap_rows] (the multi form: [cap_rows][2] = {engine index, task row}),
 * total[n_out][4]; n_buckets (B) and n_rows (R) are returned.  Every bucket holds a row, so B <= R.  Without `users` R is the number
 * of running rows, which the caller knows; with `users` it is the listed users' rows, a repeated user counting again.  R > cap_rows:
 * COOK_E_INVALID with n_buckets and n_rows filled in and nothing else written.  bucket_usage_is_device / total_is_device != 0: that
 * pointer is a DEVICE pointer and nothing of it is copied to the host.
 * The call reads the per-user order of the LAST rank run in place and writes only buffers of its own: a cycle fetched after it is the
 * cycle fetched before it.  Before any cook_rank_run / cook_cycle_run*, and after a cook_rank_stage or cook_cycle_update that no rank
 * has followed: COOK_E_STATE (the rule of cook_user_stats). */
typedef struct cook_usage_out {
  uint32_t cap_rows;              /* in: room of rows / bucket_group / bucket_usage (entries); row_off has one more                 */
  uint32_t n_buckets;             /* out: B                                                                                          */
  uint32_t n_rows;                /* out: R                                                                                          */
  int32_t bucket_usage_is_device;
  int32_t total_is_device;
  uint32_t reserved;
  uint32_t* bucket_off;
  uint32_t* bucket_group;
  double* bucket_usage;
  uint32_t* row_off;
  uint32_t* rows;
  double* total;
} cook_usage_out;
int cook_usage_breakdown(cook_engine* e, const uint32_t* group_of_row, uint32_t n_groups, const uint32_t* users, uint32_t n_list,
                         cook_usage_out* out);
/* `usage` without a pool (api.clj:2930-2944: the user's jobs of every pool) for engines of ONE device.  group_of_row[i] (NULL, or
 * group_of_row[i] NULL: engine i's rows are ungrouped) is engine i's column; group ids are ONE id space over the engines, so a group
 * with jobs in two pools is one bucket.  user_map and n_users as in cook_user_stats_multi (same checks, same errors).  A bucket's and a
 * user's rows are the concatenation over the engines in the order of `engines`, each engine's part in its own per-user order.  The
 * :pools sub-map of the answer is cook_usage_breakdown of each engine. */
int cook_usage_breakdown_multi(cook_engine** engines, uint32_t n, const uint32_t* const* user_map, uint32_t n_users,
                               const uint32_t* const* group_of_row, uint32_t n_groups, const uint32_t* users, uint32_t n_list,
                               cook_usage_out* out);

/* ---- OFFERS: replaces the numeric core of kubernetes.compute-cluster/generate-offers ----------------------
 * (kubernetes/compute_cluster.clj:68-190: available = capacity - consumption per node, the schedulable filter, the
 * offer resources and the capacity / consumption totals it publishes; kubernetes/api.clj:747-765 convert-resource-map,
 * :782-847 node-schedulable?, :849-884 get-capacity, :886-930 get-consumption).  The step BEFORE the match path: its
 * output rows are the cook_offers columns of the same names.  Quantity parsing, label / taint inspection and name
 * interning stay with the host; everything numeric is here. */
#define COOK_NODE_UNSCHEDULABLE 1u   /* .getSpec .getUnschedulable is true (api.clj:795-801)                        */
#define COOK_NODE_OTHER_TAINTS 2u    /* a taint other than the pool / deletion-candidate / gpu / tenured taints (:803-814) */
#define COOK_NODE_BLOCKLIST_LABEL 4u /* carries a label of node-blocklist-labels (:825-832)                         */
#define COOK_NODE_GPU_TAINT 8u       /* carries the gpu-node-taint (:836)                                            */
typedef struct cook_nodes { /* node-name->node of one pool, rows in ascending node-name order (offers come out in this order) */
  uint32_t n;
  const uint32_t* host;      /* host id of the node (hostname rank); copied into the offer rows                  */
  const double* cpus;        /* allocatable "cpu" (api.clj:752-754), 0.0 when absent                             */
  const double* mem;         /* allocatable "memory" / memory-multiplier in MiB (:749-751), 0.0 when absent      */
  const int32_t* gpus;       /* allocatable "nvidia.com/gpu" to-int (:756-758), 0 when absent; may be NULL       */
  const uint32_t* gpu_model; /* id of the "gpu-type" label, 0 = no label (:879); may be NULL                     */
  const double* disk;        /* allocatable "ephemeral-storage" / disk-multiplier (:760-762), < 0 = absent; may be NULL */
  const uint32_t* disk_type; /* id of the pool's disk-type label value, 0 = no label (:880); may be NULL         */
  const uint8_t* flags;      /* COOK_NODE_* bits, evaluated by the host; may be NULL (all 0)                     */
  uint32_t n_attr_keys;      /* label table [n][n_attr_keys] in the cook_offers.attr encoding (labels ++ the     */
  const uint32_t* attr;      /*   "compute-cluster-type" attribute, compute_cluster.clj:165-185); may be NULL    */
} cook_nodes;

#define COOK_POD_SYNTHETIC 1u   /* pod name has the synthetic-pod prefix (api.clj:77)                                */
#define COOK_POD_NO_REQUESTS 2u /* no container carries resource requests: the pod's resource map is nil (:908-913) */
typedef struct cook_pods { /* every pod of node-name->pods; pods of one node must appear in that node's list order */
  uint32_t n;
  const uint32_t* node;      /* index into cook_nodes; COOK_NONE_U32 (or >= nodes->n) = no node assigned, or a node
                                without capacity in this pool: dropped (api.clj:894, compute_cluster.clj:88-90)    */
  const double* cpus;        /* sum over containers of the "cpu" requests (merge-with +, api.clj:904-911)         */
  const double* mem;         /* likewise "memory" / memory-multiplier                                             */
  const int32_t* gpus;       /* likewise "nvidia.com/gpu"; may be NULL                                            */
  const uint32_t* gpu_model; /* id of nodeSelector "cloud.google.com/gke-accelerator", 0 = none (:914); may be NULL */
  const double* disk;        /* likewise "ephemeral-storage" / disk-multiplier, < 0 = no container asks; may be NULL */
  const uint32_t* disk_type; /* id of the nodeSelector disk-type label value, 0 = none (:915); may be NULL         */
  const uint8_t* flags;      /* COOK_POD_* bits; may be NULL                                                      */
} cook_pods;

typedef struct cook_offer_params {
  int32_t clobber_synthetic_pods;       /* (:clobber-synthetic-pods (config/kubernetes)) (compute_cluster.clj:71)  */
  int32_t filter_out_unsound_gpu_nodes; /* (:filter-out-unsound-gpu-nodes? (config/kubernetes)) (api.clj:839)       */
  int32_t max_pods_per_node;            /* (cc/max-tasks-per-host compute-cluster) (compute_cluster.clj:49)         */
  uint32_t n_gpu_models;                /* model ids are 1..n_gpu_models (sizes the per-model totals)               */
  uint32_t n_disk_types;                /* disk type ids are 1..n_disk_types                                        */
  uint32_t gpu_slots;                   /* entries per row of cook_node_offers.gpu_model / gpu_count (0 = 1, at most
                                           COOK_MAX_RES_SLOTS): see cook_node_offers                                 */
  uint32_t disk_slots;                  /* likewise disk_type / disk_space                                           */
} cook_offer_params;

#define COOK_NODE_ST_OFFER 1u         /* the node is schedulable: an offer row was emitted                           */
#define COOK_NODE_ST_CONSUMED 2u      /* the node has an entry in node-name->consumed                                */
#define COOK_NODE_ST_FOREIGN_GPU 4u   /* pods consume gpus under more models than the row's gpu_slots hold (see below): the
                                         row lists the first ones; ask again with more slots (COOK_MAX_RES_SLOTS covers
                                         three models beyond the node's own)                                         */
#define COOK_NODE_ST_FOREIGN_DISK 8u  /* likewise for disk types                                                     */
/* (:gpus available) / (:disk available) of a node are MAPS (compute_cluster.clj:91, 180-181): the node's own model -> capacity
 * minus what its pods consume under that model, plus one entry per model only the pods name -- deep-merge-with finds such a
 * key in the consumption map alone and keeps its value as it is (util.clj:208-225), i.e. {model consumed-count}.  A row holds
 * them as gpu_slots (model, count) pairs: the node's own model first, then the others in the order the node's pod list names
 * them, model 0 = empty slot.  The rows feed cook_offers.gpu_model / gpu_count / gpu_slots unchanged. */
typedef struct cook_node_offers { /* caller-allocated columns, capacity nodes->n rows; any column may be NULL */
  uint32_t* node;      /* row -> index into cook_nodes (ascending)                                                  */
  uint32_t* host;      /* nodes->host of that node (:hostname / :slave-id, compute_cluster.clj:175-176)             */
  double* cpus;        /* (max 0.0 (:cpus available)) (:179)                                                        */
  double* mem;         /* (max 0.0 (:mem available)) (:178)                                                         */
  uint32_t* gpu_model; /* [rows][gpu_slots] keys of (:gpus available), 0 = empty slot (:181)                        */
  double* gpu_count;   /*   their values (capacity - consumption; may be negative, the reference does not clamp it) */
  uint32_t* disk_type; /* [rows][disk_slots] keys of (:disk available) (:180)                                       */
  double* disk_space;
  int32_t* num_pods;   /* pods on the node (api.clj:816, the pod-limit test; = COOK_NUM_TASKS_ON_HOST's count)      */
  uint32_t* attr;      /* [rows][nodes->n_attr_keys]: the nodes' label rows, gathered                               */
} cook_node_offers;

typedef struct cook_offer_totals { /* the gauges generate-offers publishes (compute_cluster.clj:113-160) */
  double cpus_capacity, mem_capacity;  /* total-resource over node-name->capacity, summed in node order (the reference
                                          sums in hash-map order: unpinned for non-integer values)                  */
  double cpus_consumed, mem_consumed;  /* total-resource over node-name->consumed                                    */
  uint32_t nodes_total, nodes_schedulable;
} cook_offer_totals;

/* node_status (optional, len nodes->n): COOK_NODE_ST_* bits.  gpu_capacity_by_model / gpu_consumed_by_model (optional,
 * len n_gpu_models + 1, indexed by model id): total-map-resource of :gpus (compute_cluster.clj:95-96).
 * disk_capacity_by_type / disk_consumed_by_type (optional, len n_disk_types + 1): likewise for :disk, node order;
 * consumption under a type the node's capacity does not list is not included (such nodes carry COOK_NODE_ST_FOREIGN_DISK). */
int cook_offers_build(cook_engine* e, const cook_nodes* nodes, const cook_pods* pods, const cook_offer_params* params,
                      cook_node_offers* offers, uint32_t* n_offers, uint8_t* node_status, cook_offer_totals* totals,
                      int64_t* gpu_capacity_by_model, int64_t* gpu_consumed_by_model, double* disk_capacity_by_type,
                      double* disk_consumed_by_type);
int cook_offers_stage(cook_engine* e, const cook_nodes* nodes, const cook_pods* pods, const cook_offer_params* params);
int cook_offers_run(cook_engine* e);
int cook_offers_fetch(cook_engine* e, cook_node_offers* offers, uint32_t* n_offers, uint8_t* node_status,
                      cook_offer_totals* totals, int64_t* gpu_capacity_by_model, int64_t* gpu_consumed_by_model,
                      double* disk_capacity_by_type, double* disk_consumed_by_type);
/* HIP-event time of the last cook_offers_run in milliseconds */
int cook_offers_timing(cook_engine* e, double* ms);
/* The rows of the engine's last cook_offers_run as the offers of a match / cycle IN PLACE (device columns, no host round trip and
 * no copy): cpus, mem, host, compute-cluster-type = kubernetes, the gpu / disk columns and the label rows; with_task_limits != 0
 * adds COOK_MAX_TASKS_PER_HOST = max_pods_per_node and COOK_NUM_TASKS_ON_HOST = the node's pod count (offer.clj:38-46); Fenzo's
 * running-task view (run_*) is empty.  Otherwise exactly cook_match_stage / cook_cycle_stage.  The rows must stay untouched until
 * the match has run: a later cook_offers_run on the same engine invalidates the staging. */
int cook_match_stage_built_offers(cook_engine* e, const cook_jobs* considerable, const cook_groups* groups,
                                  const uint32_t* reserved_hosts, uint32_t n_reserved, int with_task_limits);
int cook_cycle_stage_built_offers(cook_engine* e, const cook_tasks* tasks, const cook_users* users, const cook_jobs* pending_jobs,
                                  const cook_groups* groups, const uint32_t* reserved_hosts, uint32_t n_reserved,
                                  int with_task_limits);

/* ---- THE RESIDENT POD TABLE: a Kubernetes pool whose offers are rebuilt from its pods every match cycle -------------------------
 * (kubernetes/compute_cluster.clj:539-545 pending-offers -> generate-offers on every match trigger, over the node map and the pod
 * map plus the starting pods, :314-319 add-starting-pods; every offer carries :reject-after-match-attempt, :188: nothing stands
 * between cycles.)  cook_offers_stage uploads both tables; from there on the pod table LIVES on the device and takes what changed
 * between two cycles as short lists.  All of this is additive: cook_offers_stage / _run / _fetch work as before.
 *
 * Identity.  cook_offers_stage_pod_ids gives the staged pods ids: pod_id[i] is the id of staged pod row i (n = the staged row
 * count, else COOK_E_INVALID), dense caller-chosen slot numbers below id_cap in the identity convention at the top of this file,
 * each at most once (COOK_E_INVALID; the table then has no ids).  The engine keeps the id column with the table, an id -> row
 * table of id_cap words on the device and a live-id bitmap on the host, from which every refusal below is decided before anything
 * changes and without a synchronisation.  COOK_E_STATE before cook_offers_stage.  cook_offers_stage drops the ids.
 *
 * cook_offers_update applies a delta on the device.  THE ORDER RULE (a contract: a node's pods are folded left to right, and a
 * 0.1-cpu request is not dyadic): surviving pods keep their relative order; added rows go behind the last survivor, in list
 * order; a pod the watch MODIFIES is a remove plus an add, and it moves to the end; removes apply before adds, so an id may leave
 * and rejoin in one call.  Every staged pod column moves with its row.  A column the table has and `add` lacks gets, for the
 * joining rows, what NULL means for it (0; disk: absent, -1); a column `add` carries and the table lacks is refused (stage again).
 * node_row / node_values replace the listed node rows IN PLACE, column by column under the same rule, the label rows included
 * (node_values->host NULL: the rows keep their host ids).  The node SET, and with it the offer order, does not change: nodes that
 * join or leave mean a fresh cook_offers_stage (the offer order is the node-name order, a tie-break contract).
 * COOK_E_INVALID, nothing changed: an id >= id_cap; an id twice in either list; an added id that is live and does not leave in
 * this call; node_row out of range or listed twice; a column the table lacks; node_values->n != n_node_rows or another
 * n_attr_keys; a NULL list behind a count; add without node / cpus / mem / add_id; node_values without cpus / mem.
 * COOK_E_STATE: before cook_offers_stage + cook_offers_stage_pod_ids.  A remove_id that is not live is no error: it is counted
 * (remove_missing).  The rows of the last cook_offers_run stay as they are until the next one. */
typedef struct cook_pod_delta {
  uint32_t n_remove;
  const uint32_t* remove_id; /* pods that leave                                                                 */
  const cook_pods* add;      /* rows that join (add->n of them; NULL: none) ...                                  */
  const uint32_t* add_id;    /* ... and their ids                                                                */
  uint32_t n_node_rows;
  const uint32_t* node_row;  /* node rows replaced in place ...                                                  */
  const cook_nodes* node_values; /* ... by these (node_values->n == n_node_rows)                                 */
} cook_pod_delta;
int cook_offers_stage_pod_ids(cook_engine* e, const uint32_t* pod_id, uint32_t n, uint32_t id_cap);
int cook_offers_update(cook_engine* e, const cook_pod_delta* d);
/* the counts of the last delta (cook_offers_update, or a queue cycle's): n_pods the table's rows behind it, n_offers the rows of
 * the last cook_offers_run / rebuild (0: none yet) */
typedef struct cook_pod_delta_info {
  uint32_t removed, remove_missing, added, node_rows, n_pods, n_offers;
} cook_pod_delta_info;
int cook_offers_update_info(cook_engine* e, cook_pod_delta_info* out);
/* the pod table as it stands, list order, in one synchronisation (as cook_cycle_fetch_offers: n is always written; cap < n is
 * COOK_E_INVALID; a NULL column is skipped; a column the table lacks reads as what NULL means; id without ids: COOK_NONE_U32) */
typedef struct cook_pod_rows {
  uint32_t cap, n;
  uint32_t* node;
  double* cpus;
  double* mem;
  int32_t* gpus;
  uint32_t* gpu_model;
  double* disk;
  uint32_t* disk_type;
  uint8_t* flags;
  uint32_t* id;
} cook_pod_rows;
int cook_offers_fetch_pods(cook_engine* e, cook_pod_rows* out);
/* The rows of the engine's last cook_offers_run become the STAGED offers of its cycle in place: what cook_cycle_delta.offers does
 * from host arrays, with the columns and the with_task_limits meaning of cook_cycle_stage_built_offers.  Tasks, users, jobs,
 * groups, limiters and reservations stay.  Legal wherever a cook_cycle_update that carries offers is (COOK_E_STATE before a cycle
 * stage or before cook_offers_run); like it, it ends the standing queue: the next cycle is a rank cycle (cook_cycle_run*).  This
 * is how a rank cycle of such a pool gets current offers. */
int cook_cycle_set_built_offers(cook_engine* e, int with_task_limits);
/* A queue cycle of a pool whose offers are built from its pods: cook_cycle_run_queue_reserve without a host churn, plus the pod
 * delta and the offer rebuild inside the advance.  The mark-removed step, the groups' fold, the usage carry, the release, the
 * reservations and the limiters' spend are enqueued first and read the OLD rows (the last cycle's job_to_offer indexes them);
 * then, where the churn has its place, the delta (pods NULL: none, a rebuild from the table as it stands), the rebuild by the
 * kernels of cook_offers_run, and the rebuilt rows become the staged offers as by cook_cycle_set_built_offers, in front of the
 * considerable filters.  The rebuild writes the row buffers the last match read: ONE stream orders it behind every reader, so
 * there is no second set of rows.  The offer count rides in the advance's one read-back: the call makes exactly as many stream
 * synchronisations as cook_cycle_run_queue_reserve, and no upload that grows with the cluster.
 * The offers come from the pods: step->offers, carry->offers = 1 and finished->offers = 1 are COOK_E_INVALID, nothing changed, and
 * so is everything cook_offers_update refuses.  Cook's own launches are rows of pods->add (add-starting-pods), the finished tasks'
 * pods are in pods->remove_id; carry->usage, finished->usage, finished->groups, the reservations and the limiters work as in
 * cook_cycle_run_queue_reserve.  COOK_E_STATE: staged offers that were not built on this engine (cook_cycle_stage_built_offers,
 * cook_cycle_set_built_offers or this call), a delta without ids.  Afterwards cook_offers_fetch, cook_cycle_fetch_offers,
 * cook_match_explain, cook_match_metrics, cook_cycle_autoscale and cook_cycle_rebalance_stage describe this cycle's rows.
 * _multi: the arrays-of-pointers form (an array NULL: that part for no pool; with_task_limits per pool, NULL: 0); the pools run
 * one after another, each exactly its single call with the placement deferred to cook_cycle_match_multi; returns the first code
 * that is not COOK_OK, the other pools go on. */
int cook_cycle_run_queue_pods(cook_engine* e, const cook_queue_step* step, const cook_queue_carry* carry, const cook_finished* finished,
                              const cook_pod_delta* pods, const cook_reservations* reservations, int with_task_limits,
                              uint32_t num_considerable);
int cook_cycle_run_queue_pods_multi(cook_engine** engines, uint32_t n, const cook_queue_step* const* steps,
                                    const cook_queue_carry* const* carries, const cook_finished* const* finished,
                                    const cook_pod_delta* const* pods, const cook_reservations* const* reservations,
                                    const int32_t* with_task_limits, const uint32_t* num_considerable);

/* Number of jobs of the engine's last match (cook_match_run: the staged jobs; cook_cycle_run / the lockstep calls: the
 * considerable jobs actually taken, <= num_considerable): the length cook_match_fetch / cook_cycle_fetch write. */
int cook_match_count(cook_engine* e, uint32_t* n_jobs);

/* ---- measurement hooks (bench.py): HIP-event time of the last *_run, per stage, in milliseconds ----------- */
int cook_last_timing(cook_engine* e, double* rank_ms, double* match_ms);
/* named kernel timings of the last run: fills up to cap entries, returns count */
int cook_kernel_timings(cook_engine* e, const char** names, double* ms, uint32_t* launches, uint32_t cap);
int cook_set_profiling(cook_engine* e, int enabled);
/* placement statistics of the last match: [0] rounds, [1] matched, [2..5] rounds ended by list-exhausted / touched-set-full /
   group barrier / window end, [6] segments of windows staged for the walk (>= rounds; the excess went on without a launch), [7] jobs resolved, [8] microseconds the resolve phase spent staging
   windows, [9] ... walking them, [10] offers touched (sum over rounds), [11] jobs the walk visited (the rest were settled in
   parallel), [12..15] reserved (0) */
int cook_match_stats(cook_engine* e, uint32_t out[16]);
/* the same, open-ended: fills min(cap, COOK_MATCH_STATS_EX_N) words and returns how many.  [0..15] as cook_match_stats;
   [16] walked jobs whose merged candidate list was cut short because one offer chunk had contributed all its entries (the list
   may not hold every feasible offer); [17..24] the last cook_cycle_match_multi LED by this engine: [17] how it ran (0 lockstep
   launches, 1 served walkers — one persistent walker workgroup per pool beside serve launches —, 2 the same in its stepping form), [18] pools,
   [19] serve iterations, [20] of them empty, [21] pool windows served, [22] microseconds the latch waited for requests, [23] 1 = the
   served match gave up and lockstep launches finished it, [24] streams of serve iterations; [25] with COOK_GUARD=1 in the
   environment (diagnostics: every device buffer sits between two bands of a pattern) the writes found outside a buffer so far, process-wide —
   the call looks at this engine's bands first —, else 0; [26..28] the last cook_cycle_update of this engine: microseconds in the call, microseconds of those the host waited in
   stream synchronisations, device buffers it had to (re)allocate, [29..30] the phase of the call that took the host longest (0 checks, 1 the delta's block,
   2 marks and scans, 3 column compactions, 4 CSR columns, 5 the look at the device, 6 swaps and offers) and its microseconds; [31] the last queue cycle of this engine
   (cook_cycle_run_queue*): microseconds the host spent in its advance (steps 1-3), the one synchronisation included — inside
   cook_cycle_run_queue_multi that wait is shared with the other pools' flows;
   [32..36] the last cook_cycle_run_rank_multi LED by this engine: pools, launches made, of them for more than one pool, operations
   issued on their own (copies, fills, kernels outside the batched path), stream synchronisations; [37] how the last match was placed (0 window
   rounds, 1 serial sweep, 3 class-ordered best fit), [38] why a match that could have been placed by class-ordered best fit was not (0 = it was; bits:
   1 resources that are not multiples of 2^-20 below 2^30, 2 a job constraint outside {EQUALS on the first 8 attribute keys with values < 256, <= 4 novel
   hosts, unique group, gpu}, 4 ports / named scalars, 8 balanced / attribute-equals groups or more than 16 pending members of a group, 16 gpu maps with
   several entries / max-tasks-per-host / reserved hosts / two offers of one host / attribute values >= 256, 32 too many classes, gpu kinds or offers
   for one workgroup's LDS, 64 job cpus values outside the 8 levels, 128 a job asking for nothing, 0x10000 good-enough-fitness < 1, COOK_CLASSFIT=0 or
   offers built on the device, 0x20000 a cook_params.fitness other than 0), [39] matches of this engine that match_algo 0 / 2 / 3 would have placed in window rounds and
   the serial sweep placed because the pool's fitness is a spreader (cook_params.fitness 3..5), since the engine was created; [40..59] class-ordered best fit, the last match: jobs visited, matched, of them on an offer the call
   had placed on before (overlay lane), offers opened, of them full at once, placements on gpu hosts, epochs, chunk scans, exact turns (several offers
   within 2^-37 of the best: the literal fitness decided), summary re-computations, [50] reserved, batches of 64 jobs, overlay lanes dropped full,
   [53..56] 100 MHz ticks: the launch, its prologue, the epochs' merges, the bookkeeper's batch pre-checks; [57..63] reserved (0) */
#define COOK_MATCH_STATS_EX_N 64
int cook_match_stats_ex(cook_engine* e, uint32_t* out, uint32_t cap);
/* the last pool batch this engine led, whatever call made it (the rank part, queue cycles, pool usage, cook_cycle_autoscale_multi,
   cook_match_metrics_multi): pools, launches made, of them for more than one pool, operations issued alone (copies, fills, kernels outside
   the batched path), stream synchronisations.  All zeros before any; a call that ran its engines one after another leaves them as they were.
   (cook_match_stats_ex [32..36] stay the rank part's.) */
int cook_batch_stats(const cook_engine* lead, uint32_t out[5]);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* COOKMATCH_H */
