/*
 * cookmatch_jni.c — JNI shim between twosigma/Cook (Clojure on the JVM) and libcookmatch.so (include/cookmatch.h).
 *
 * The reference has no FFI on the fair-share match path; this is the binding a Cook maintainer would
 * add.  Java side: `package cook.hip; final class Native { static native ... }`, loaded with
 * System.loadLibrary("cookmatch_jni") which links against libcookmatch.so.
 *
 * Marshalling rule (one rule for every call): each cook_* input struct crosses as ONE jobjectArray of direct
 * java.nio.ByteBuffers (native byte order), one element per pointer field of the struct IN THE FIELD ORDER OF
 * include/cookmatch.h; a null element = a NULL (optional) pointer.  Scalars of the struct (n, n_attr_keys, flags) are
 * explicit jint arguments.  Plain-data structs (cook_params, cook_pool_quota, cook_rebalance_params) cross as one
 * direct buffer holding the struct itself (cook_params: the last int32, at byte 44, is `fitness` — the pool's
 * :fenzo-fitness-calculator as COOK_FITNESS_*; a value outside 0..5 makes create / setParams return
 * COOK_E_INVALID, and lastError(0) has the message of a refused create).  Outputs are direct buffers sized by the caller as the header documents.
 * cook_jobs / cook_offers take their three extra scalars (n_scalars; gpu_slots, disk_slots) as explicit jints too.
 * GetDirectBufferAddress never copies or pins: the SoA arrays the Clojure side fills are read in place by the
 * H2D copies of the engine.
 *
 * No JDK exists in the build image: the file is compiled in CI against tests/jni_stub/jni.h (type-checks every call
 * against cookmatch.h) and against a real <jni.h> wherever a JDK is present:
 *   cc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude bindings/jni/cookmatch_jni.c \
 *      -Lcook_amd -lcookmatch -o libcookmatch_jni.so
 */
#include <jni.h>
#include <stdint.h>

#include "cookmatch.h"

#define H(h) ((cook_engine*)(intptr_t)(h))
/* Every buffer the JVM hands over is checked against the bytes the call will read or write (GetDirectBufferCapacity of a
 * java.nio.ByteBuffer is in bytes): a short buffer sets *bad and the call returns COOK_E_INVALID before the engine sees a
 * pointer.  `need` = 0 skips the check (sizes only the engine knows; the header documents them). */
static void* buf_n(JNIEnv* env, jobject b, uint64_t need, int* bad) {
  void* p;
  if (!b) return 0;
  p = (*env)->GetDirectBufferAddress(env, b);
  if (!p || (need && (uint64_t)(*env)->GetDirectBufferCapacity(env, b) < need)) {
    *bad = 1;
    return 0;
  }
  return p;
}
#define BUFN(T, b, count) ((T*)buf_n(env, (b), (uint64_t)(count) * sizeof(T), &bad))
#define BUF(T, b) ((T*)buf_n(env, (b), sizeof(T), &bad))
/* element i of an array of direct buffers (null array or null element -> NULL); the local reference GetObjectArrayElement
 * creates is released at once: a cycleStage call walks ~60 elements, the JVM only promises room for 16 */
static void* elem_n(JNIEnv* env, jobjectArray a, jsize i, uint64_t need, int* bad) {
  jobject b;
  void* p;
  if (!a || i >= (*env)->GetArrayLength(env, a)) return 0;
  b = (*env)->GetObjectArrayElement(env, a, i);
  if (!b) return 0;
  p = buf_n(env, b, need, bad);
  (*env)->DeleteLocalRef(env, b);
  return p;
}
#define EL(T, a, i, count) ((T*)elem_n(env, (a), (i), (uint64_t)(count) * sizeof(T), bad))
#define CHECKED(call) (bad ? COOK_E_INVALID : (call))

static cook_tasks tasks_of(JNIEnv* env, jint n, jobjectArray a, int* bad) {
  cook_tasks t;
  t.n = (uint32_t)n;
  t.cpus = EL(const double, a, 0, n);
  t.mem = EL(const double, a, 1, n);
  t.gpus = EL(const double, a, 2, n);
  t.user = EL(const uint32_t, a, 3, n);
  t.priority = EL(const int32_t, a, 4, n);
  t.start_ms = EL(const int64_t, a, 5, n);
  t.task_id = EL(const int64_t, a, 6, n);
  t.job_id = EL(const int64_t, a, 7, n);
  t.pending = EL(const uint8_t, a, 8, n);
  t.host = EL(const uint32_t, a, 9, n);
  return t;
}
static cook_users users_of(JNIEnv* env, jint n, jobjectArray a, int* bad) {
  cook_users u;
  u.n = (uint32_t)n;
  u.div_cpus = EL(const double, a, 0, n);
  u.div_mem = EL(const double, a, 1, n);
  u.div_gpus = EL(const double, a, 2, n);
  u.quota_count = EL(const double, a, 3, n);
  u.quota_cpus = EL(const double, a, 4, n);
  u.quota_mem = EL(const double, a, 5, n);
  u.quota_gpus = EL(const double, a, 6, n);
  return u;
}
/* a CSR pair: offsets [n + 1], then payload columns of offsets[n] entries */
static const uint32_t* csr_off(JNIEnv* env, jobjectArray a, jsize i, jint n, uint32_t* total, int* bad) {
  const uint32_t* off = EL(const uint32_t, a, i, (uint64_t)n + 1u);
  *total = (off && n >= 0) ? off[n] : 0u;
  return off;
}
static cook_jobs jobs_of(JNIEnv* env, jint n, jint n_scalars, jobjectArray a, int* bad) {
  cook_jobs j;
  uint32_t ne = 0, nn = 0;
  j.n = (uint32_t)n;
  j.cpus = EL(const double, a, 0, n);
  j.mem = EL(const double, a, 1, n);
  j.gpus = EL(const double, a, 2, n);
  j.gpu_model = EL(const uint32_t, a, 3, n);
  j.user = EL(const uint32_t, a, 4, n);
  j.group = EL(const uint32_t, a, 5, n);
  j.eq_off = csr_off(env, a, 6, n, &ne, bad);
  j.eq_key = EL(const uint32_t, a, 7, ne);
  j.eq_val = EL(const uint32_t, a, 8, ne);
  j.novel_off = csr_off(env, a, 9, n, &nn, bad);
  j.novel_host = EL(const uint32_t, a, 10, nn);
  j.reserved_host = EL(const int32_t, a, 11, n);
  j.ckpt_location = EL(const uint32_t, a, 12, n);
  j.est_end_ms = EL(const int64_t, a, 13, n);
  j.disk_request = EL(const double, a, 14, n);
  j.disk_type = EL(const uint32_t, a, 15, n);
  j.ports = EL(const int32_t, a, 16, n);
  j.n_scalars = (uint32_t)n_scalars;
  j.reserved_ = 0;
  j.scalars = EL(const double, a, 17, (uint64_t)n * (uint64_t)(n_scalars > 0 ? n_scalars : 0));
  if (n_scalars < 0 || n_scalars > COOK_MAX_SCALARS) *bad = 1;
  return j;
}
/* dims = {n_attr_keys, gpu_slots, disk_slots, n_scalars} */
static cook_offers offers_of(JNIEnv* env, jint n, const jint dims[4], jobjectArray a, int* bad) {
  cook_offers o;
  const uint64_t gs = dims[1] > 0 ? (uint64_t)dims[1] : 1u, ds = dims[2] > 0 ? (uint64_t)dims[2] : 1u;
  o.n = (uint32_t)n;
  o.cpus = EL(const double, a, 0, n);
  o.mem = EL(const double, a, 1, n);
  o.host = EL(const uint32_t, a, 2, n);
  o.k8s = EL(const uint8_t, a, 3, n);
  o.gpu_model = EL(const uint32_t, a, 4, (uint64_t)n * gs);
  o.gpu_count = EL(const double, a, 5, (uint64_t)n * gs);
  o.disk_type = EL(const uint32_t, a, 6, (uint64_t)n * ds);
  o.disk_space = EL(const double, a, 7, (uint64_t)n * ds);
  o.n_attr_keys = (uint32_t)dims[0];
  o.attr = EL(const uint32_t, a, 8, (uint64_t)n * (uint64_t)(dims[0] > 0 ? dims[0] : 0));
  o.max_tasks = EL(const int32_t, a, 9, n);
  o.num_tasks = EL(const int32_t, a, 10, n);
  o.location = EL(const uint32_t, a, 11, n);
  o.host_start_s = EL(const int64_t, a, 12, n);
  o.run_cpus = EL(const double, a, 13, n);
  o.run_mem = EL(const double, a, 14, n);
  o.run_count = EL(const int32_t, a, 15, n);
  o.gpu_slots = (uint32_t)dims[1];
  o.disk_slots = (uint32_t)dims[2];
  o.ports = EL(const int32_t, a, 16, n);
  o.n_scalars = (uint32_t)dims[3];
  o.reserved_ = 0;
  o.scalars = EL(const double, a, 17, (uint64_t)n * (uint64_t)(dims[3] > 0 ? dims[3] : 0));
  if (dims[0] < 0 || dims[1] < 0 || dims[1] > COOK_MAX_RES_SLOTS || dims[2] < 0 || dims[2] > COOK_MAX_RES_SLOTS || dims[3] < 0 ||
      dims[3] > COOK_MAX_SCALARS)
    *bad = 1;
  return o;
}
/* the jint[4] of offers_of as a direct buffer of four native ints */
static const jint* dims_of(JNIEnv* env, jobject b, int* bad_out) {
  static const jint none[4] = {0, 0, 0, 0};
  int bad = 0;
  const jint* d = BUFN(const jint, b, 4);
  if (bad) *bad_out = 1;
  return d ? d : none;
}
static cook_groups groups_of(JNIEnv* env, jint n, jobjectArray a, int* bad) {
  cook_groups g;
  uint32_t nr = 0;
  g.n = (uint32_t)n;
  g.type = EL(const uint8_t, a, 0, n);
  g.attr_key = EL(const uint32_t, a, 1, n);
  g.minimum = EL(const int32_t, a, 2, n);
  g.run_off = csr_off(env, a, 3, n, &nr, bad);
  g.run_host = EL(const uint32_t, a, 4, nr);
  g.run_attr = EL(const uint32_t, a, 5, nr);
  return g;
}
/* the parts of a queue cycle (cycleRunQueue*), each from the jints and buffers its exports take; o / g: the step's offers and groups
 * as the export built them, or null */
#define BUFP(T, b, count) ((T*)buf_n(env, (b), (uint64_t)(count) * sizeof(T), bad))
static cook_queue_step step_of(JNIEnv* env, jint remove_mode, jint n_last_offers, jobject offer_skipped, const cook_offers* o,
                               const cook_groups* g, int* bad) {
  cook_queue_step s;
  const jint nl = n_last_offers > 0 ? n_last_offers : 0;
  s.offer_skipped = BUFP(const uint8_t, offer_skipped, nl);
  s.remove_mode = (uint32_t)remove_mode;
  s.n_offer_skipped = (uint32_t)nl; /* the library refuses a count other than the last cycle's offers */
  s.offers = o;
  s.groups = g;
  return s;
}
static cook_queue_carry carry_of(JNIEnv* env, jint carry_offers, jint carry_usage, jint n_users, jobject tokens_left, int* bad) {
  cook_queue_carry cy;
  cy.offers = (uint32_t)carry_offers;
  cy.usage = (uint32_t)carry_usage;
  cy.tokens_left = BUFP(const int64_t, tokens_left, n_users > 0 ? n_users : 0);
  return cy;
}
static cook_finished finished_of(JNIEnv* env, jint n_finished, jint n_fin_scalars, jobjectArray a, jint release_offers, jint release_usage,
                                 jint release_groups, int* bad) {
  cook_finished f;
  const jint nf = n_finished > 0 ? n_finished : 0, ns = n_fin_scalars > 0 ? n_fin_scalars : 0;
  f.n = (uint32_t)nf;
  f.host = EL(const uint32_t, a, 0, nf);
  f.user = EL(const uint32_t, a, 1, nf);
  f.cpus = EL(const double, a, 2, nf);
  f.mem = EL(const double, a, 3, nf);
  f.gpus = EL(const double, a, 4, nf);
  f.ports = EL(const int32_t, a, 5, nf);
  f.scalars = EL(const double, a, 6, (uint64_t)nf * (uint64_t)ns);
  f.n_scalars = (uint32_t)ns;
  f.gpu_model = EL(const uint32_t, a, 7, nf);
  f.disk_request = EL(const double, a, 8, nf);
  f.disk_type = EL(const uint32_t, a, 9, nf);
  f.group = EL(const uint32_t, a, 10, nf);
  f.offers = (uint32_t)release_offers;
  f.usage = (uint32_t)release_usage;
  f.groups = (uint32_t)release_groups;
  return f;
}
static cook_reservations reservations_of(JNIEnv* env, jint release_matched, jint replace, jint n_reserve, jobject rsv_pending,
                                         jobject rsv_host, int* bad) {
  cook_reservations rv;
  const jint nr = n_reserve > 0 ? n_reserve : 0;
  rv.release_matched = (uint32_t)release_matched;
  rv.replace = (uint32_t)replace;
  rv.n = (uint32_t)nr;
  rv.pending = BUFP(const uint32_t, rsv_pending, nr);
  rv.host = BUFP(const uint32_t, rsv_host, nr);
  return rv;
}
#undef BUFP
#undef EL
#define EL(T, a, i, count) ((T*)elem_n(env, (a), (i), (uint64_t)(count) * sizeof(T), &bad))

/* ---- lifecycle ------------------------------------------------------------------------------------------------ */
JNIEXPORT jlong JNICALL Java_cook_hip_Native_create(JNIEnv* env, jclass c, jobject params, jint device) {
  cook_engine* e = 0;
  int bad = 0, rc;
  const cook_params* p = BUF(const cook_params, params);
  (void)c;
  if (bad) return (jlong)COOK_E_INVALID;
  if (cook_abi_version() != COOK_ABI_VERSION) return (jlong)COOK_E_INVALID; /* a library of another struct layout */
  rc = cook_engine_create(p, device, &e);
  return rc == COOK_OK ? (jlong)(intptr_t)e : (jlong)rc; /* negative = COOK_E_* */
}
JNIEXPORT void JNICALL Java_cook_hip_Native_destroy(JNIEnv* env, jclass c, jlong h) {
  (void)env, (void)c;
  cook_engine_destroy(H(h));
}
JNIEXPORT jint JNICALL Java_cook_hip_Native_setParams(JNIEnv* env, jclass c, jlong h, jobject params) {
  int bad = 0;
  const cook_params* p = BUF(const cook_params, params);
  (void)c;
  return CHECKED(cook_engine_set_params(H(h), p));
}
JNIEXPORT jstring JNICALL Java_cook_hip_Native_lastError(JNIEnv* env, jclass c, jlong h) {
  (void)c;
  return (*env)->NewStringUTF(env, cook_last_error(H(h)));
}
/* page-locked host memory as a direct ByteBuffer (cook_host_alloc): columns filled into it cross the link at full speed */
JNIEXPORT jobject JNICALL Java_cook_hip_Native_hostAlloc(JNIEnv* env, jclass c, jlong bytes) {
  void* p = bytes > 0 ? cook_host_alloc((size_t)bytes) : 0;
  (void)c;
  return p ? (*env)->NewDirectByteBuffer(env, p, bytes) : 0;
}
JNIEXPORT void JNICALL Java_cook_hip_Native_hostFree(JNIEnv* env, jclass c, jobject buffer) {
  (void)c;
  if (buffer) cook_host_free((*env)->GetDirectBufferAddress(env, buffer));
}

/* ---- rank: scheduler/sort-jobs-by-dru-helper + filter-based-on-quota + filter-offensive-jobs ---------------------- */
JNIEXPORT jint JNICALL Java_cook_hip_Native_rank(JNIEnv* env, jclass c, jlong h, jint n, jobjectArray tasks, jint n_users,
                                                 jobjectArray users, jobject quota, jobject ranked_out, jobject n_out,
                                                 jobject dru_out) {
  int bad = 0;
  cook_tasks t = tasks_of(env, n, tasks, &bad);
  cook_users u = users_of(env, n_users, users, &bad);
  const cook_pool_quota* q = BUF(const cook_pool_quota, quota);
  uint32_t* ranked = BUFN(uint32_t, ranked_out, n); /* at most every task is pending */
  uint32_t* n_ranked = BUF(uint32_t, n_out);
  double* dru = BUFN(double, dru_out, n);
  (void)c;
  return CHECKED(cook_rank(H(h), &t, &u, q, ranked, n_ranked, dru));
}
JNIEXPORT jint JNICALL Java_cook_hip_Native_rankPoolUsage(JNIEnv* env, jclass c, jlong h, jint n, jobjectArray tasks,
                                                          jint n_users, jobjectArray users, jobject usage_out) {
  int bad = 0, rc;
  cook_tasks t = tasks_of(env, n, tasks, &bad);
  cook_users u = users_of(env, n_users, users, &bad);
  cook_usage* out = BUF(cook_usage, usage_out);
  (void)c;
  if (bad) return COOK_E_INVALID;
  rc = cook_rank_stage(H(h), &t, &u);
  return rc ? rc : cook_rank_pool_usage(H(h), out);
}
/* the staged tasks' running usage per user, [n_users][3] doubles (count, cpus, mem; gpu pools: count, gpus, -), for the
 * cross-rank sums of a sharded deployment */
JNIEXPORT jint JNICALL Java_cook_hip_Native_rankUserUsage(JNIEnv* env, jclass c, jlong h, jint n_users, jobject usage_out, jint clear) {
  int bad = 0;
  double* out = BUFN(double, usage_out, (uint64_t)(n_users > 0 ? n_users : 0) * 3u);
  (void)c;
  return CHECKED(cook_rank_user_usage(H(h), out, clear));
}

/* ---- considerable: scheduler/pending-jobs->considerable-jobs ------------------------------------------------------- */
JNIEXPORT jint JNICALL Java_cook_hip_Native_considerable(JNIEnv* env, jclass c, jlong h, jint n, jobjectArray queue,
                                                         jint n_users, jobjectArray user_state, jobject tokens,
                                                         jboolean enforce, jobject pool_quota, jobject pool_usage, jint k,
                                                         jobject idx_out, jobject n_out, jobject limited_out,
                                                         jobject passed_out) {
  int bad = 0;
  cook_queue q;
  cook_user_state s;
  const cook_usage *pq = BUF(const cook_usage, pool_quota), *pu = BUF(const cook_usage, pool_usage);
  uint32_t* idx = BUFN(uint32_t, idx_out, (k < n ? k : n) > 0 ? (k < n ? k : n) : 0);
  uint32_t* n_idx = BUF(uint32_t, n_out);
  uint32_t* limited = BUFN(uint32_t, limited_out, n_users);
  uint32_t* passed = BUFN(uint32_t, passed_out, n_users);
  (void)c;
  q.n = (uint32_t)n;
  q.cpus = EL(const double, queue, 0, n);
  q.mem = EL(const double, queue, 1, n);
  q.gpus = EL(const double, queue, 2, n);
  q.user = EL(const uint32_t, queue, 3, n);
  q.eligible = EL(const uint8_t, queue, 4, n);
  s.n = (uint32_t)n_users;
  s.quota_count = EL(const double, user_state, 0, n_users);
  s.quota_cpus = EL(const double, user_state, 1, n_users);
  s.quota_mem = EL(const double, user_state, 2, n_users);
  s.quota_gpus = EL(const double, user_state, 3, n_users);
  s.usage_count = EL(const double, user_state, 4, n_users);
  s.usage_cpus = EL(const double, user_state, 5, n_users);
  s.usage_mem = EL(const double, user_state, 6, n_users);
  s.usage_gpus = EL(const double, user_state, 7, n_users);
  s.tokens_left = BUFN(const int64_t, tokens, n_users);
  s.enforce_rate_limit = enforce ? 1 : 0;
  s.has_pool_quota = pq ? 1 : 0;
  if (pq) s.pool_quota = *pq;
  s.pool_usage_given = pu ? 1 : 0;
  s.reserved = 0;
  if (pu) s.pool_usage = *pu;
  return CHECKED(cook_considerable(H(h), &q, &s, (uint32_t)k, idx, n_idx, limited, passed));
}

/* ---- match: the body of scheduler/match-offer-to-schedule (TaskScheduler.scheduleOnce) ----------------------------- */
JNIEXPORT jint JNICALL Java_cook_hip_Native_match(JNIEnv* env, jclass c, jlong h, jint k, jint n_scalars, jobjectArray jobs, jint m,
                                                  jobject offer_dims, jobjectArray offers, jint n_groups, jobjectArray groups,
                                                  jobject reserved_hosts, jint n_reserved, jobject job_to_offer_out,
                                                  jobject fail_code_out, jobject head_matched_out) {
  int bad = 0;
  cook_jobs j = jobs_of(env, k, n_scalars, jobs, &bad);
  cook_offers o = offers_of(env, m, dims_of(env, offer_dims, &bad), offers, &bad);
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  const uint32_t* res = BUFN(const uint32_t, reserved_hosts, n_reserved);
  int32_t* j2o = BUFN(int32_t, job_to_offer_out, k);
  uint32_t* fail = BUFN(uint32_t, fail_code_out, k);
  uint8_t* head = BUF(uint8_t, head_matched_out);
  (void)c;
  return CHECKED(cook_match(H(h), &j, &o, n_groups ? &g : 0, res, (uint32_t)n_reserved, j2o, fail, head));
}
/* jobs of the engine's last match: the length matchFetch-style outputs need */
JNIEXPORT jint JNICALL Java_cook_hip_Native_matchCount(JNIEnv* env, jclass c, jlong h, jobject n_out) {
  int bad = 0;
  uint32_t* n = BUF(uint32_t, n_out);
  (void)c;
  return CHECKED(cook_match_count(H(h), n));
}

/* ---- cycle: rank -> considerable -> match with inputs resident on the device ------------------------------------------ */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleStage(JNIEnv* env, jclass c, jlong h, jint n, jobjectArray tasks, jint n_users,
                                                       jobjectArray users, jint n_pending, jint n_scalars, jobjectArray pending_jobs,
                                                       jint m, jobject offer_dims, jobjectArray offers, jint n_groups,
                                                       jobjectArray groups, jobject reserved_hosts, jint n_reserved) {
  int bad = 0;
  cook_tasks t = tasks_of(env, n, tasks, &bad);
  cook_users u = users_of(env, n_users, users, &bad);
  cook_jobs j = jobs_of(env, n_pending, n_scalars, pending_jobs, &bad);
  cook_offers o = offers_of(env, m, dims_of(env, offer_dims, &bad), offers, &bad);
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  const uint32_t* res = BUFN(const uint32_t, reserved_hosts, n_reserved);
  (void)c;
  return CHECKED(cook_cycle_stage(H(h), &t, &u, &j, &o, n_groups ? &g : 0, res, (uint32_t)n_reserved));
}
/* what changed since the last cycle (cook_cycle_update): rows to drop, rows to append, optionally fresh offers (offers == null:
 * the staged ones stay) */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleUpdate(JNIEnv* env, jclass c, jlong h, jint n_remove, jobject remove_task, jint n_add,
                                                        jobjectArray add_tasks, jint n_add_pending, jint n_scalars,
                                                        jobjectArray add_pending, jint m, jobject offer_dims, jobjectArray offers) {
  int bad = 0;
  cook_tasks t = tasks_of(env, n_add, add_tasks, &bad);
  cook_jobs j = jobs_of(env, n_add_pending, n_scalars, add_pending, &bad);
  cook_offers o = offers_of(env, m, dims_of(env, offer_dims, &bad), offers, &bad);
  cook_cycle_delta d;
  (void)c;
  d.n_remove = (uint32_t)n_remove;
  d.remove_task = BUFN(const uint32_t, remove_task, n_remove);
  d.add_tasks = add_tasks ? &t : 0;
  d.add_pending = add_pending ? &j : 0;
  d.offers = offers ? &o : 0;
  return CHECKED(cook_cycle_update(H(h), &d));
}
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRun(JNIEnv* env, jclass c, jlong h, jobject quota, jint num_considerable) {
  int bad = 0, rc;
  const cook_pool_quota* q = BUF(const cook_pool_quota, quota);
  (void)c;
  if (bad) return COOK_E_INVALID;
  rc = cook_rank_set_quota(H(h), q);
  return rc ? rc : cook_cycle_run(H(h), (uint32_t)num_considerable);
}
/* several pools of one rank: cycleRunRank per engine (any threads) or one cycleRunRankMulti(handles), then one cycleMatchMulti(handles) */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRunRank(JNIEnv* env, jclass c, jlong h, jobject quota, jint num_considerable) {
  int bad = 0, rc;
  const cook_pool_quota* q = BUF(const cook_pool_quota, quota);
  (void)c;
  if (bad) return COOK_E_INVALID;
  rc = cook_rank_set_quota(H(h), q);
  return rc ? rc : cook_cycle_run_rank(H(h), (uint32_t)num_considerable);
}
/* the rank parts of n engines in ONE call from one thread (cook_cycle_run_rank_multi: the pools' flows side by side, the same kernel of
 * several pools in one launch): quotas = direct buffer of n cook_pool_quota, or NULL when no pool has one; a pool without quota inputs
 * carries has_pool_quota = has_group_quota = 0 in its entry */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRunRankMulti(JNIEnv* env, jclass c, jobject handles /* direct buffer of n jlong */, jint n,
                                                              jobject quotas, jobject num_considerable /* direct buffer of n jint: every pool its own K */) {
  cook_engine* es[64];
  int bad = 0, rc;
  const int64_t* hs = BUFN(const int64_t, handles, n > 0 ? n : 0);
  const cook_pool_quota* qs = BUFN(const cook_pool_quota, quotas, n > 0 ? n : 0);
  const uint32_t* ks = BUFN(const uint32_t, num_considerable, n > 0 ? n : 0);
  jint i;
  (void)c;
  if (bad || !hs || !ks || n <= 0 || n > 64) return COOK_E_INVALID;
  for (i = 0; i < n; ++i) {
    es[i] = H(hs[i]);
    rc = cook_rank_set_quota(es[i], qs ? &qs[i] : 0);
    if (rc) return rc;
  }
  return cook_cycle_run_rank_multi(es, (uint32_t)n, ks, 0, 0);
}
/* a match cycle on the standing ranked queue, without a re-rank (cook_cycle_run_queue; defer != 0: cook_cycle_run_queue_rank, the placement
 * then runs in cycleMatchMulti).  offer_skipped: n_last_offers bytes (the offers of the LAST cycle; the buffer is checked against that
 * length here, and the library refuses a count other than the last cycle's offer count) or null; offers == null: the staged
 * offers stay; groups == null: the kept matches' cotasks are folded into their groups on the device, else the table replaces the groups'
 * running cotasks.  The multi form of the C ABI (cook_cycle_run_queue_multi) takes one step per pool: a binding that wants it calls this
 * with defer for every pool of the device from one thread and then cycleMatchMulti. */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRunQueue(JNIEnv* env, jclass c, jlong h, jint num_considerable, jint remove_mode,
                                                          jint n_last_offers, jobject offer_skipped, jint m, jobject offer_dims,
                                                          jobjectArray offers, jint n_groups, jobjectArray groups, jint defer) {
  int bad = 0;
  cook_offers o = offers_of(env, m, dims_of(env, offer_dims, &bad), offers, &bad);
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  const cook_queue_step s = step_of(env, remove_mode, n_last_offers, offer_skipped, offers ? &o : 0, groups ? &g : 0, &bad);
  (void)c;
  if (bad) return COOK_E_INVALID;
  return defer ? cook_cycle_run_queue_rank(H(h), &s, (uint32_t)num_considerable) : cook_cycle_run_queue(H(h), &s, (uint32_t)num_considerable);
}
/* cycleRunQueue with the carry (cook_cycle_run_queue_carry; defer != 0: cook_cycle_run_queue_carry_multi for this one pool, the placement
 * then runs in cycleMatchMulti): carry_offers / carry_usage = 1 move the last cycle's kept placements into the staged offers (then offers
 * must be null) / the staged user state on the device; tokens_left: direct buffer of n_users int64 that replaces the staged token counts,
 * or null (tokens staged: one is spent per kept job). */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRunQueueCarry(JNIEnv* env, jclass c, jlong h, jint num_considerable, jint remove_mode,
                                                               jint n_last_offers, jobject offer_skipped, jint m, jobject offer_dims,
                                                               jobjectArray offers, jint n_groups, jobjectArray groups, jint carry_offers,
                                                               jint carry_usage, jint n_users, jobject tokens_left, jint defer) {
  int bad = 0;
  cook_offers o = offers_of(env, m, dims_of(env, offer_dims, &bad), offers, &bad);
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  const cook_queue_step s = step_of(env, remove_mode, n_last_offers, offer_skipped, offers ? &o : 0, groups ? &g : 0, &bad);
  const cook_queue_carry cy = carry_of(env, carry_offers, carry_usage, n_users, tokens_left, &bad);
  cook_engine* e = H(h);
  const cook_queue_step* sp = &s;
  const uint32_t k = (uint32_t)num_considerable;
  const cook_queue_carry* cp = &cy;
  (void)c;
  if (bad) return COOK_E_INVALID;
  return defer ? cook_cycle_run_queue_carry_multi(&e, 1, &sp, &cp, &k) : cook_cycle_run_queue_carry(e, sp, cp, k);
}
/* cycleRunQueueCarry with the release (cook_cycle_run_queue_release; defer != 0: cook_cycle_run_queue_release_multi for this one pool, the
 * placement then runs in cycleMatchMulti).  finished: the n_finished tasks that ended since the last cycle, in the host's order, as an
 * array of direct buffers {host u32, user u32, cpus f64, mem f64, gpus f64, ports i32, scalars f64 (n_fin_scalars columns of n_finished),
 * gpu_model u32, disk_request f64, disk_type u32, group u32} (null elements: the column is absent), or null: no release.
 * release_offers / release_usage / release_groups = 1 give their resources back to the staged offers (then offers must be null), take
 * them out of the staged user state, remove them from the groups' running cotasks (then groups must be null), on the device. */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRunQueueRelease(JNIEnv* env, jclass c, jlong h, jint num_considerable, jint remove_mode,
                                                                 jint n_last_offers, jobject offer_skipped, jint m, jobject offer_dims,
                                                                 jobjectArray offers, jint n_groups, jobjectArray groups, jint carry_offers,
                                                                 jint carry_usage, jint n_users, jobject tokens_left, jint n_finished,
                                                                 jint n_fin_scalars, jobjectArray finished, jint release_offers,
                                                                 jint release_usage, jint release_groups, jint defer) {
  int bad = 0;
  cook_offers o = offers_of(env, m, dims_of(env, offer_dims, &bad), offers, &bad);
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  const cook_queue_step s = step_of(env, remove_mode, n_last_offers, offer_skipped, offers ? &o : 0, groups ? &g : 0, &bad);
  const cook_queue_carry cy = carry_of(env, carry_offers, carry_usage, n_users, tokens_left, &bad);
  const cook_finished f = finished_of(env, n_finished, n_fin_scalars, finished, release_offers, release_usage, release_groups, &bad);
  cook_engine* e = H(h);
  const cook_queue_step* sp = &s;
  const uint32_t k = (uint32_t)num_considerable;
  const cook_queue_carry* cp = &cy;
  const cook_finished* fp = finished ? &f : 0;
  (void)c;
  if (bad) return COOK_E_INVALID;
  return defer ? cook_cycle_run_queue_release_multi(&e, 1, &sp, &cp, &fp, &k) : cook_cycle_run_queue_release(e, sp, cp, fp, k);
}
/* the counts of the last queue cycle's release (cook_cycle_release_info): info_out = direct buffer of one cook_release_info */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleReleaseInfo(JNIEnv* env, jclass c, jlong h, jobject info_out) {
  int bad = 0;
  cook_release_info* out = BUF(cook_release_info, info_out);
  (void)c;
  if (bad || !out) return COOK_E_INVALID;
  return cook_cycle_release_info(H(h), out);
}
/* cycleRunQueueRelease with the host churn (cook_cycle_run_queue_hosts; defer != 0: cook_cycle_run_queue_hosts_multi for this one pool, the
 * placement then runs in cycleMatchMulti); the step carries no offers (a churn edits the STAGED ones).  leave_host: n_leave host ids
 * whose rows leave the staged offers, or null.  join: the m_join rows that join, marshalled as the offers of cycleStage (join_dims as
 * offer_dims), or null; join_before: m_join host ids of the OLD rows in front of which they go (COOK_NONE_U32: behind the last row), or
 * null: all at the end. */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRunQueueHosts(JNIEnv* env, jclass c, jlong h, jint num_considerable, jint remove_mode,
                                                               jint n_last_offers, jobject offer_skipped, jint n_groups, jobjectArray groups,
                                                               jint carry_offers, jint carry_usage, jint n_users, jobject tokens_left,
                                                               jint n_finished, jint n_fin_scalars, jobjectArray finished, jint release_offers,
                                                               jint release_usage, jint release_groups, jint n_leave, jobject leave_host,
                                                               jint m_join, jobject join_dims, jobjectArray join, jobject join_before,
                                                               jint defer) {
  int bad = 0;
  const jint mj = m_join > 0 ? m_join : 0, nl = n_leave > 0 ? n_leave : 0;
  cook_offers o = offers_of(env, mj, dims_of(env, join_dims, &bad), join, &bad);
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  const cook_queue_step s = step_of(env, remove_mode, n_last_offers, offer_skipped, 0, groups ? &g : 0, &bad);
  const cook_queue_carry cy = carry_of(env, carry_offers, carry_usage, n_users, tokens_left, &bad);
  const cook_finished f = finished_of(env, n_finished, n_fin_scalars, finished, release_offers, release_usage, release_groups, &bad);
  cook_host_churn hc;
  cook_engine* e = H(h);
  const cook_queue_step* sp = &s;
  const uint32_t k = (uint32_t)num_considerable;
  const cook_queue_carry* cp = &cy;
  const cook_finished* fp = finished ? &f : 0;
  const cook_host_churn* hp = &hc;
  (void)c;
  hc.n_leave = leave_host ? (uint32_t)nl : 0u;
  hc.leave_host = BUFN(const uint32_t, leave_host, nl);
  hc.join = join ? &o : 0;
  hc.join_before = BUFN(const uint32_t, join_before, mj);
  if (bad) return COOK_E_INVALID;
  return defer ? cook_cycle_run_queue_hosts_multi(&e, 1, &sp, &cp, &fp, &hp, &k) : cook_cycle_run_queue_hosts(e, sp, cp, fp, hp, k);
}
/* the counts of the last queue cycle's host churn (cook_cycle_churn_info): info_out = direct buffer of one cook_churn_info */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleChurnInfo(JNIEnv* env, jclass c, jlong h, jobject info_out) {
  int bad = 0;
  cook_churn_info* out = BUF(cook_churn_info, info_out);
  (void)c;
  if (bad || !out) return COOK_E_INVALID;
  return cook_cycle_churn_info(H(h), out);
}
/* The staged offer table as the next match will read it (cook_cycle_fetch_offers).  dims_out: direct buffer of 5 jint that receives
 * {n, gpu_slots, disk_slots, n_attr_keys, n_scalars}; columns: an array of 18 direct buffers in the field order of cook_offer_rows
 * {cpus, mem, host, k8s, gpu_model, gpu_count, disk_type, disk_space, attr, max_tasks, num_tasks, location, host_start_s, run_cpus,
 * run_mem, run_count, ports, scalars} (null elements: skipped), each with room for cap rows at the widest shape the header allows
 * (COOK_MAX_RES_SLOTS map entries, COOK_MAX_SCALARS scalars, max_attr_keys attribute keys); columns == null with cap = 0 asks for the
 * dims alone (COOK_E_INVALID when there are rows). */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleFetchOffers(JNIEnv* env, jclass c, jlong h, jint cap, jint max_attr_keys, jobject dims_out,
                                                             jobjectArray columns) {
  int bad = 0, rc;
  const uint64_t n = cap > 0 ? (uint64_t)cap : 0u, na = max_attr_keys > 0 ? (uint64_t)max_attr_keys : 0u;
  jint* dims = BUFN(jint, dims_out, 5);
  cook_offer_rows r;
  (void)c;
  r.cap = (uint32_t)n;
  r.n = r.gpu_slots = r.disk_slots = r.n_attr_keys = r.n_scalars = 0u;
  r.cpus = EL(double, columns, 0, n);
  r.mem = EL(double, columns, 1, n);
  r.host = EL(uint32_t, columns, 2, n);
  r.k8s = EL(uint8_t, columns, 3, n);
  r.gpu_model = EL(uint32_t, columns, 4, n * COOK_MAX_RES_SLOTS);
  r.gpu_count = EL(double, columns, 5, n * COOK_MAX_RES_SLOTS);
  r.disk_type = EL(uint32_t, columns, 6, n * COOK_MAX_RES_SLOTS);
  r.disk_space = EL(double, columns, 7, n * COOK_MAX_RES_SLOTS);
  r.attr = EL(uint32_t, columns, 8, n * na);
  r.max_tasks = EL(int32_t, columns, 9, n);
  r.num_tasks = EL(int32_t, columns, 10, n);
  r.location = EL(uint32_t, columns, 11, n);
  r.host_start_s = EL(int64_t, columns, 12, n);
  r.run_cpus = EL(double, columns, 13, n);
  r.run_mem = EL(double, columns, 14, n);
  r.run_count = EL(int32_t, columns, 15, n);
  r.ports = EL(int32_t, columns, 16, n);
  r.scalars = EL(double, columns, 17, n * COOK_MAX_SCALARS);
  if (bad || !dims) return COOK_E_INVALID;
  if (r.attr) { /* the staged attribute keys must fit the caller's buffer: ask for the widths first (cap 0 writes no column) */
    cook_offer_rows probe = {0};
    rc = cook_cycle_fetch_offers(H(h), &probe);
    if (rc != COOK_OK && probe.n == 0u) return rc;
    if ((uint64_t)probe.n_attr_keys > na) return COOK_E_INVALID;
  }
  rc = cook_cycle_fetch_offers(H(h), &r);
  dims[0] = (jint)r.n, dims[1] = (jint)r.gpu_slots, dims[2] = (jint)r.disk_slots, dims[3] = (jint)r.n_attr_keys, dims[4] = (jint)r.n_scalars;
  return rc;
}
/* cycleRunQueueHosts with the host reservations (cook_cycle_run_queue_reserve; defer != 0: cook_cycle_run_queue_reserve_multi for this one
 * pool, the placement then runs in cycleMatchMulti).  release_matched / replace: the flags of cook_reservations; rsv_pending / rsv_host:
 * direct buffers of n_reserve uint32 each (pending ordinal or COOK_NONE_U32, host id), or null with n_reserve = 0. */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRunQueueReserve(JNIEnv* env, jclass c, jlong h, jint num_considerable, jint remove_mode,
                                                                 jint n_last_offers, jobject offer_skipped, jint n_groups, jobjectArray groups,
                                                                 jint carry_offers, jint carry_usage, jint n_users, jobject tokens_left,
                                                                 jint n_finished, jint n_fin_scalars, jobjectArray finished, jint release_offers,
                                                                 jint release_usage, jint release_groups, jint n_leave, jobject leave_host,
                                                                 jint m_join, jobject join_dims, jobjectArray join, jobject join_before,
                                                                 jint release_matched, jint replace, jint n_reserve, jobject rsv_pending,
                                                                 jobject rsv_host, jint defer) {
  int bad = 0;
  const jint mj = m_join > 0 ? m_join : 0, nl = n_leave > 0 ? n_leave : 0;
  cook_offers o = offers_of(env, mj, dims_of(env, join_dims, &bad), join, &bad);
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  const cook_queue_step s = step_of(env, remove_mode, n_last_offers, offer_skipped, 0, groups ? &g : 0, &bad);
  const cook_queue_carry cy = carry_of(env, carry_offers, carry_usage, n_users, tokens_left, &bad);
  const cook_finished f = finished_of(env, n_finished, n_fin_scalars, finished, release_offers, release_usage, release_groups, &bad);
  const cook_reservations rv = reservations_of(env, release_matched, replace, n_reserve, rsv_pending, rsv_host, &bad);
  cook_host_churn hc;
  cook_engine* e = H(h);
  const cook_queue_step* sp = &s;
  const uint32_t k = (uint32_t)num_considerable;
  const cook_queue_carry* cp = &cy;
  const cook_finished* fp = finished ? &f : 0;
  const cook_host_churn* hp = &hc;
  const cook_reservations* rp = &rv;
  (void)c;
  hc.n_leave = leave_host ? (uint32_t)nl : 0u;
  hc.leave_host = BUFN(const uint32_t, leave_host, nl);
  hc.join = join ? &o : 0;
  hc.join_before = BUFN(const uint32_t, join_before, mj);
  if (bad) return COOK_E_INVALID;
  return defer ? cook_cycle_run_queue_reserve_multi(&e, 1, &sp, &cp, &fp, &hp, &rp, &k) : cook_cycle_run_queue_reserve(e, sp, cp, fp, hp, rp, k);
}
/* reserve-hosts! on its own, for the next rank cycle (cook_cycle_set_reservations): rsv_pending / rsv_host as above; n_reserve = 0: no
 * reservations */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleSetReservations(JNIEnv* env, jclass c, jlong h, jint n_reserve, jobject rsv_pending,
                                                                 jobject rsv_host) {
  int bad = 0;
  const cook_reservations rv = reservations_of(env, 0, 1, n_reserve, rsv_pending, rsv_host, &bad);
  (void)c;
  if (bad) return COOK_E_INVALID;
  return cook_cycle_set_reservations(H(h), &rv);
}
/* the counts of the last call that could change the reservations (cook_cycle_reserve_info): info_out = direct buffer of one cook_reserve_info */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleReserveInfo(JNIEnv* env, jclass c, jlong h, jobject info_out) {
  int bad = 0;
  cook_reserve_info* out = BUF(cook_reserve_info, info_out);
  (void)c;
  if (bad || !out) return COOK_E_INVALID;
  return cook_cycle_reserve_info(H(h), out);
}
/* the live reservations (cook_cycle_fetch_reservations): pending_out / host_out = direct buffers of cap uint32 each (null: skipped),
 * n_out = direct buffer of one jint that receives their count (also when cap is too small: COOK_E_INVALID, nothing written) */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleFetchReservations(JNIEnv* env, jclass c, jlong h, jint cap, jobject pending_out,
                                                                   jobject host_out, jobject n_out) {
  int bad = 0, rc;
  const jint cp = cap > 0 ? cap : 0;
  uint32_t* pending = BUFN(uint32_t, pending_out, cp);
  uint32_t* host = BUFN(uint32_t, host_out, cp);
  jint* n = BUFN(jint, n_out, 1);
  uint32_t got = 0u;
  (void)c;
  if (bad || !n) return COOK_E_INVALID;
  rc = cook_cycle_fetch_reservations(H(h), pending, host, (uint32_t)cp, &got);
  *n = (jint)got;
  return rc;
}
/* the launch-rate limiters the engine keeps from here on (cook_cycle_set_limiters): cols = {per_minute double[n], bucket int64[n],
 * tokens int64[n], last_update_ms int64[n]} as direct buffers, user = direct buffer of n uint32 or null (entry i is user i);
 * drop != 0: cook_cycle_set_limiters(NULL), everything else ignored */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleSetLimiters(JNIEnv* env, jclass c, jlong h, jint n, jobject user, jobjectArray cols, jint drop) {
  int bad = 0;
  const jint nn = n > 0 ? n : 0;
  cook_limiters l;
  (void)c;
  if (drop) return cook_cycle_set_limiters(H(h), 0);
  l.n = (uint32_t)nn;
  l.user = BUFN(const uint32_t, user, nn);
  l.per_minute = EL(const double, cols, 0, nn);
  l.bucket = EL(const int64_t, cols, 1, nn);
  l.tokens = EL(const int64_t, cols, 2, nn);
  l.last_update_ms = EL(const int64_t, cols, 3, nn);
  if (bad) return COOK_E_INVALID;
  return cook_cycle_set_limiters(H(h), &l);
}
/* the time of the NEXT cycle (cook_cycle_set_clock); has_clock == 0: none */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleSetClock(JNIEnv* env, jclass c, jlong h, jint has_clock, jlong now_ms, jlong spend_ms) {
  cook_clock ck;
  (void)env;
  (void)c;
  ck.now_ms = (int64_t)now_ms;
  ck.spend_ms = (int64_t)spend_ms;
  return cook_cycle_set_clock(H(h), has_clock ? &ck : 0);
}
/* the last cycle's kept placements spend now (cook_cycle_limiters_spend): offer_skipped = direct buffer of n_last_offers uint8, or null */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleLimitersSpend(JNIEnv* env, jclass c, jlong h, jint n_last_offers, jobject offer_skipped,
                                                               jlong spend_ms) {
  int bad = 0;
  const jint nl = n_last_offers > 0 ? n_last_offers : 0;
  const uint8_t* sk = BUFN(const uint8_t, offer_skipped, nl);
  (void)c;
  if (bad) return COOK_E_INVALID;
  return cook_cycle_limiters_spend(H(h), sk, (uint32_t)nl, (int64_t)spend_ms);
}
/* the limiters' state (cook_cycle_fetch_limiters): tokens_out / last_out / until_out = direct buffers of n_users int64 each (null: skipped);
 * n_users must be the user count the limiters were installed for: the engine writes that many */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleFetchLimiters(JNIEnv* env, jclass c, jlong h, jint n_users, jobject tokens_out, jobject last_out,
                                                               jobject until_out) {
  int bad = 0;
  const jint nu = n_users > 0 ? n_users : 0;
  int64_t* tokens = BUFN(int64_t, tokens_out, nu);
  int64_t* last = BUFN(int64_t, last_out, nu);
  int64_t* until = BUFN(int64_t, until_out, nu);
  (void)c;
  if (bad) return COOK_E_INVALID;
  return cook_cycle_fetch_limiters(H(h), tokens, last, until);
}
/* the rate-limit stage's per-user counts of the last cycle (cook_cycle_fetch_rate_limit): direct buffers of n_users uint32 each (null: skipped);
 * n_users must be the staged user state's count */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleFetchRateLimit(JNIEnv* env, jclass c, jlong h, jint n_users, jobject rate_limited_out,
                                                                jobject passed_out) {
  int bad = 0;
  const jint nu = n_users > 0 ? n_users : 0;
  uint32_t* rl = BUFN(uint32_t, rate_limited_out, nu);
  uint32_t* ps = BUFN(uint32_t, passed_out, nu);
  (void)c;
  if (bad) return COOK_E_INVALID;
  return cook_cycle_fetch_rate_limit(H(h), rl, ps);
}
/* the limiters' counts of the last cycle (cook_cycle_limiter_info): info_out = direct buffer of one cook_limiter_info */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleLimiterInfo(JNIEnv* env, jclass c, jlong h, jobject info_out) {
  int bad = 0;
  cook_limiter_info* out = BUF(cook_limiter_info, info_out);
  (void)c;
  if (bad || !out) return COOK_E_INVALID;
  return cook_cycle_limiter_info(H(h), out);
}
/* the running usage of n staged engines of one device in ONE call (cook_rank_pool_usage_multi): usage_out = direct buffer of n cook_usage */
JNIEXPORT jint JNICALL Java_cook_hip_Native_rankPoolUsageMulti(JNIEnv* env, jclass c, jobject handles /* direct buffer of n jlong */, jint n, jobject usage_out) {
  cook_engine* es[64];
  int bad = 0;
  const int64_t* hs = BUFN(const int64_t, handles, n > 0 ? n : 0);
  cook_usage* out = BUFN(cook_usage, usage_out, n > 0 ? n : 0);
  jint i;
  (void)c;
  if (bad || !hs || !out || n <= 0 || n > 64) return COOK_E_INVALID;
  for (i = 0; i < n; ++i) es[i] = H(hs[i]);
  return cook_rank_pool_usage_multi(es, (uint32_t)n, out);
}
/* set-stats-counters! (monitor.clj:177-207) from the last rank: limits = the 7 pointer fields of cook_user_limits (share_cpus, share_mem,
 * quota_count, quota_cpus, quota_mem, quota_gpus, extra_quota_positive or null), n_users = the engine's staged users (the engine checks);
 * per_user_out = direct buffer of n_users x 12 doubles or null, state_out = n_users bytes or null, totals_out = one cook_user_stats_totals */
static cook_user_limits limits_of(JNIEnv* env, jint n, jobjectArray a, int* bad) {
  cook_user_limits l;
  l.n = (uint32_t)n;
  l.share_cpus = (const double*)elem_n(env, a, 0, (uint64_t)n * sizeof(const double), bad);
  l.share_mem = (const double*)elem_n(env, a, 1, (uint64_t)n * sizeof(const double), bad);
  l.quota_count = (const double*)elem_n(env, a, 2, (uint64_t)n * sizeof(const double), bad);
  l.quota_cpus = (const double*)elem_n(env, a, 3, (uint64_t)n * sizeof(const double), bad);
  l.quota_mem = (const double*)elem_n(env, a, 4, (uint64_t)n * sizeof(const double), bad);
  l.quota_gpus = (const double*)elem_n(env, a, 5, (uint64_t)n * sizeof(const double), bad);
  l.extra_quota_positive = (const uint8_t*)elem_n(env, a, 6, (uint64_t)n * sizeof(const uint8_t), bad);
  return l;
}
JNIEXPORT jint JNICALL Java_cook_hip_Native_userStats(JNIEnv* env, jclass c, jlong h, jint n_users, jobjectArray limits, jobject per_user_out,
                                                      jobject state_out, jobject totals_out) {
  int bad = 0;
  cook_user_limits l = limits_of(env, n_users, limits, &bad);
  double* pu = BUFN(double, per_user_out, (uint64_t)(n_users > 0 ? n_users : 0) * 12u);
  uint8_t* st = BUFN(uint8_t, state_out, n_users > 0 ? n_users : 0);
  cook_user_stats_totals* t = BUF(cook_user_stats_totals, totals_out);
  (void)c;
  if (!limits || n_users < 0) return COOK_E_INVALID;
  return CHECKED(cook_user_stats(H(h), &l, pu, 0, st, t));
}
/* ... of a quota group whose pools are n engines of one device (cook_user_stats_multi): user_maps = n direct buffers of the engines'
 * staged users' group ids (a null array or element: the identity; their length is the engine's user count, which only the engine knows),
 * n_users / limits / outputs as userStats over the group's users */
JNIEXPORT jint JNICALL Java_cook_hip_Native_userStatsMulti(JNIEnv* env, jclass c, jobject handles /* direct buffer of n jlong */, jint n,
                                                           jobjectArray user_maps, jint n_users, jobjectArray limits, jobject per_user_out,
                                                           jobject state_out, jobject totals_out) {
  cook_engine* es[64];
  const uint32_t* maps[64];
  int bad = 0;
  const int64_t* hs = BUFN(const int64_t, handles, n > 0 ? n : 0);
  cook_user_limits l = limits_of(env, n_users, limits, &bad);
  double* pu = BUFN(double, per_user_out, (uint64_t)(n_users > 0 ? n_users : 0) * 12u);
  uint8_t* st = BUFN(uint8_t, state_out, n_users > 0 ? n_users : 0);
  cook_user_stats_totals* t = BUF(cook_user_stats_totals, totals_out);
  jint i;
  (void)c;
  if (bad || !hs || !limits || n <= 0 || n > 64 || n_users < 0) return COOK_E_INVALID;
  for (i = 0; i < n; ++i) {
    es[i] = H(hs[i]);
    maps[i] = (const uint32_t*)elem_n(env, user_maps, i, 0, &bad);
  }
  return CHECKED(cook_user_stats_multi(es, (uint32_t)n, maps, (uint32_t)n_users, &l, pu, 0, st, t));
}
/* why the jobs of a pool wait (cook_unscheduled: the quota, share and queue-position reasons of cook.unscheduled/reasons) from the last
 * rank: limits = the 7 pointer fields of cook_unsched_limits (quota_count, quota_cpus, quota_mem, quota_gpus, share_cpus, share_mem,
 * share_gpus) over n_users = the engine's staged users, or a null array = the staged users' own; n_tasks = the staged task rows (the
 * engine checks it, and every row of `rows`, against its own count); in_window = n_tasks bytes or null; rows = n_rows task rows or null
 * (all n_tasks rows, n_rows ignored).  Outputs, direct buffers or null, n = n_rows (n_tasks when rows is null): reasons_out / queue_pos_out
 * n uint32, total_out n x 4 doubles, ahead_out n_users x 10 uint32, list_len_out n_users uint32 */
JNIEXPORT jint JNICALL Java_cook_hip_Native_unscheduled(JNIEnv* env, jclass c, jlong h, jint n_users, jobjectArray limits, jint n_tasks,
                                                        jobject in_window, jobject rows, jint n_rows, jobject reasons_out, jobject queue_pos_out,
                                                        jobject total_out, jobject ahead_out, jobject list_len_out) {
  int bad = 0;
  const uint64_t nu = (uint64_t)(n_users > 0 ? n_users : 0), nt = (uint64_t)(n_tasks > 0 ? n_tasks : 0);
  const uint64_t n = rows ? (uint64_t)(n_rows > 0 ? n_rows : 0) : nt;
  cook_unsched_limits l;
  const uint8_t* win = BUFN(const uint8_t, in_window, nt);
  const uint32_t* rw = BUFN(const uint32_t, rows, n);
  uint32_t* reasons = BUFN(uint32_t, reasons_out, n);
  uint32_t* qpos = BUFN(uint32_t, queue_pos_out, n);
  double* total = BUFN(double, total_out, n * 4u);
  uint32_t* ahead = BUFN(uint32_t, ahead_out, nu * COOK_UNSCHED_AHEAD);
  uint32_t* llen = BUFN(uint32_t, list_len_out, nu);
  (void)c;
  if (n_users < 0 || n_tasks < 0 || n_rows < 0) return COOK_E_INVALID;
  l.n = (uint32_t)n_users;
  l.quota_count = (const double*)elem_n(env, limits, 0, nu * sizeof(const double), &bad);
  l.quota_cpus = (const double*)elem_n(env, limits, 1, nu * sizeof(const double), &bad);
  l.quota_mem = (const double*)elem_n(env, limits, 2, nu * sizeof(const double), &bad);
  l.quota_gpus = (const double*)elem_n(env, limits, 3, nu * sizeof(const double), &bad);
  l.share_cpus = (const double*)elem_n(env, limits, 4, nu * sizeof(const double), &bad);
  l.share_mem = (const double*)elem_n(env, limits, 5, nu * sizeof(const double), &bad);
  l.share_gpus = (const double*)elem_n(env, limits, 6, nu * sizeof(const double), &bad);
  return CHECKED(cook_unscheduled(H(h), limits ? &l : 0, win, rw, (uint32_t)(rows ? n_rows : n_tasks), reasons, qpos, total, 0, ahead, llen));
}
/* GET /usage with its job-group breakdown from the last rank (cook_usage_breakdown): group_of_row = n_tasks uint32 (the staged task rows;
 * interned group ids below n_groups, COOK_NONE_U32 = none) or null; users = n_list user ids or null (all n_users users, n_list ignored);
 * cap_rows = the room of the outputs in rows.  Outputs, direct buffers or null, n_out = n_list (n_users when users is null):
 * bucket_off_out n_out + 1 uint32, bucket_group_out cap_rows uint32, bucket_usage_out cap_rows x 4 doubles, row_off_out cap_rows + 1
 * uint32, rows_out cap_rows uint32, total_out n_out x 4 doubles; counts_out = 2 uint32 {buckets, rows} (also filled in when cap_rows
 * is too small) */
static cook_usage_out usage_out_of(JNIEnv* env, uint64_t n_out, uint64_t cap, uint64_t stride, jobject bucket_off_out, jobject bucket_group_out,
                                   jobject bucket_usage_out, jobject row_off_out, jobject rows_out, jobject total_out, int* badp) {
  cook_usage_out o;
  int bad = 0;
  o.cap_rows = (uint32_t)cap;
  o.n_buckets = 0, o.n_rows = 0, o.bucket_usage_is_device = 0, o.total_is_device = 0, o.reserved = 0;
  o.bucket_off = BUFN(uint32_t, bucket_off_out, n_out + 1u);
  o.bucket_group = BUFN(uint32_t, bucket_group_out, cap);
  o.bucket_usage = BUFN(double, bucket_usage_out, cap * 4u);
  o.row_off = BUFN(uint32_t, row_off_out, cap + 1u);
  o.rows = BUFN(uint32_t, rows_out, cap * stride);
  o.total = BUFN(double, total_out, n_out * 4u);
  if (bad) *badp = 1;
  return o;
}
JNIEXPORT jint JNICALL Java_cook_hip_Native_usageBreakdown(JNIEnv* env, jclass c, jlong h, jint n_users, jint n_tasks, jobject group_of_row,
                                                           jint n_groups, jobject users, jint n_list, jint cap_rows, jobject bucket_off_out,
                                                           jobject bucket_group_out, jobject bucket_usage_out, jobject row_off_out,
                                                           jobject rows_out, jobject total_out, jobject counts_out) {
  int bad = 0, rc;
  const uint64_t nl = (uint64_t)(n_list > 0 ? n_list : 0), n_out = users ? nl : (uint64_t)(n_users > 0 ? n_users : 0);
  const uint32_t* grp = BUFN(const uint32_t, group_of_row, n_tasks > 0 ? n_tasks : 0);
  const uint32_t* ul = BUFN(const uint32_t, users, nl);
  uint32_t* counts = BUFN(uint32_t, counts_out, 2);
  cook_usage_out o = usage_out_of(env, n_out, (uint64_t)(cap_rows > 0 ? cap_rows : 0), 1u, bucket_off_out, bucket_group_out, bucket_usage_out,
                                  row_off_out, rows_out, total_out, &bad);
  (void)c;
  if (bad || n_users < 0 || n_tasks < 0 || n_groups < 0 || n_list < 0 || cap_rows < 0) return COOK_E_INVALID;
  rc = cook_usage_breakdown(H(h), grp, (uint32_t)n_groups, ul, (uint32_t)nl, &o);
  if (counts) counts[0] = o.n_buckets, counts[1] = o.n_rows;
  return rc;
}
/* ... without a pool, over n engines of one device (cook_usage_breakdown_multi): groups = n direct buffers of the engines' group_of_row
 * (a null array or element: ungrouped; their length is the engine's task count, which only the engine knows), user_maps as in
 * userStatsMulti, n_users the users of the call; rows_out holds cap_rows x 2 uint32 {engine index, task row} */
JNIEXPORT jint JNICALL Java_cook_hip_Native_usageBreakdownMulti(JNIEnv* env, jclass c, jobject handles /* direct buffer of n jlong */, jint n,
                                                                jobjectArray user_maps, jint n_users, jobjectArray groups, jint n_groups,
                                                                jobject users, jint n_list, jint cap_rows, jobject bucket_off_out,
                                                                jobject bucket_group_out, jobject bucket_usage_out, jobject row_off_out,
                                                                jobject rows_out, jobject total_out, jobject counts_out) {
  cook_engine* es[64];
  const uint32_t* maps[64];
  const uint32_t* grps[64];
  int bad = 0, rc;
  const uint64_t nl = (uint64_t)(n_list > 0 ? n_list : 0), n_out = users ? nl : (uint64_t)(n_users > 0 ? n_users : 0);
  const int64_t* hs = BUFN(const int64_t, handles, n > 0 ? n : 0);
  const uint32_t* ul = BUFN(const uint32_t, users, nl);
  uint32_t* counts = BUFN(uint32_t, counts_out, 2);
  cook_usage_out o = usage_out_of(env, n_out, (uint64_t)(cap_rows > 0 ? cap_rows : 0), 2u, bucket_off_out, bucket_group_out, bucket_usage_out,
                                  row_off_out, rows_out, total_out, &bad);
  jint i;
  (void)c;
  if (bad || !hs || n <= 0 || n > 64 || n_users < 0 || n_groups < 0 || n_list < 0 || cap_rows < 0) return COOK_E_INVALID;
  for (i = 0; i < n; ++i) {
    es[i] = H(hs[i]);
    maps[i] = (const uint32_t*)elem_n(env, user_maps, i, 0, &bad);
    grps[i] = (const uint32_t*)elem_n(env, groups, i, 0, &bad);
  }
  if (bad) return COOK_E_INVALID;
  rc = cook_usage_breakdown_multi(es, (uint32_t)n, maps, (uint32_t)n_users, grps, (uint32_t)n_groups, ul, (uint32_t)nl, &o);
  if (counts) counts[0] = o.n_buckets, counts[1] = o.n_rows;
  return rc;
}
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleMatchMulti(JNIEnv* env, jclass c, jobject handles /* direct buffer of n jlong */, jint n) {
  cook_engine* es[64];
  int bad = 0;
  const int64_t* hs = BUFN(const int64_t, handles, n > 0 ? n : 0);
  jint i;
  (void)c;
  if (bad || !hs || n <= 0 || n > 64) return COOK_E_INVALID;
  for (i = 0; i < n; ++i) es[i] = H(hs[i]);
  return cook_cycle_match_multi(es, (uint32_t)n);
}
/* n_pending = the pending tasks staged (sizes every output: a cycle ranks at most that many and considers no more) */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleFetch(JNIEnv* env, jclass c, jlong h, jint n_pending, jobject ranked_out,
                                                       jobject n_ranked_out, jobject job_to_offer_out, jobject n_considered_out,
                                                       jobject head_matched_out, jobject rank_pos_out) {
  int bad = 0, rc;
  uint32_t* ranked = BUFN(uint32_t, ranked_out, n_pending);
  uint32_t* n_ranked = BUF(uint32_t, n_ranked_out);
  int32_t* j2o = BUFN(int32_t, job_to_offer_out, n_pending);
  uint32_t* n_cons = BUF(uint32_t, n_considered_out);
  uint8_t* head = BUF(uint8_t, head_matched_out);
  uint32_t* pos = BUFN(uint32_t, rank_pos_out, n_pending);
  (void)c;
  if (bad) return COOK_E_INVALID;
  rc = cook_cycle_fetch(H(h), ranked, n_ranked, j2o, n_cons, head);
  if (rc || !pos) return rc;
  return cook_cycle_fetch_considerable(H(h), pos, 0);
}
/* handle-resource-offers-autoscaling-helper (scheduler.clj:1283-1335) from the last cycle (cook_cycle_autoscale): params = one
 * cook_autoscale_params whose max_jobs, n_exclude and scale_factor are read (its two pointer fields are ignored: offer_skipped = n_offers
 * bytes, the offers the cycle staged, or null; exclude = n_exclude task indices or null), task_idx_out = cap uint32 slots
 * (max(max_jobs, n_pending) always suffices), info_out = one cook_autoscale_info */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleAutoscale(JNIEnv* env, jclass c, jlong h, jobject params, jint n_offers, jobject offer_skipped,
                                                           jobject exclude, jobject task_idx_out, jint cap, jobject info_out) {
  int bad = 0;
  cook_autoscale_params p;
  const cook_autoscale_params* in = BUF(const cook_autoscale_params, params);
  uint32_t* out = BUFN(uint32_t, task_idx_out, cap > 0 ? cap : 0);
  cook_autoscale_info* info = BUF(cook_autoscale_info, info_out);
  (void)c;
  if (bad || !in || n_offers < 0 || cap < 0 || in->n_exclude > 0x7fffffffu) return COOK_E_INVALID;
  p = *in;
  p.offer_skipped = BUFN(const uint8_t, offer_skipped, n_offers);
  p.exclude_task = BUFN(const uint32_t, exclude, p.n_exclude);
  if ((p.n_exclude && !p.exclude_task) || (cap && !out)) return COOK_E_INVALID;
  return CHECKED(cook_cycle_autoscale(H(h), &p, out, (uint32_t)cap, info));
}
/* cycleAutoscale for n engines of one device in ONE call (cook_cycle_autoscale_multi).  params = direct buffer of n cook_autoscale_params
 * (max_jobs, n_exclude, scale_factor read; the pointer fields ignored); n_offers = direct buffer of n jint; offer_skipped / exclude /
 * task_idx_out = arrays of n direct buffers (a null array or element: none): n_offers[i] bytes, n_exclude task indices, caps[i] uint32 slots;
 * caps = direct buffer of n jint; info_out = direct buffer of n cook_autoscale_info or null; rc_out = direct buffer of n jint or null */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleAutoscaleMulti(JNIEnv* env, jclass c, jobject handles /* direct buffer of n jlong */, jint n,
                                                                jobject params, jobject n_offers, jobjectArray offer_skipped,
                                                                jobjectArray exclude, jobjectArray task_idx_out, jobject caps,
                                                                jobject info_out, jobject rc_out) {
  cook_engine* es[64];
  cook_autoscale_params ps[64];
  const cook_autoscale_params* pp[64];
  uint32_t* outs[64];
  uint32_t cs[64];
  int bad = 0;
  const jint cnt = n > 0 ? n : 0;
  const int64_t* hs = BUFN(const int64_t, handles, cnt);
  const cook_autoscale_params* in = BUFN(const cook_autoscale_params, params, cnt);
  const int32_t* no = BUFN(const int32_t, n_offers, cnt);
  const int32_t* cp = BUFN(const int32_t, caps, cnt);
  cook_autoscale_info* info = BUFN(cook_autoscale_info, info_out, cnt);
  int* rcs = BUFN(int, rc_out, cnt);
  jint i;
  (void)c;
  if (bad || !hs || !in || !no || !cp || n <= 0 || n > 64) return COOK_E_INVALID;
  for (i = 0; i < n; ++i) {
    if (no[i] < 0 || cp[i] < 0 || in[i].n_exclude > 0x7fffffffu) return COOK_E_INVALID;
    es[i] = H(hs[i]);
    ps[i] = in[i];
    ps[i].offer_skipped = EL(const uint8_t, offer_skipped, i, no[i]);
    ps[i].exclude_task = EL(const uint32_t, exclude, i, ps[i].n_exclude);
    outs[i] = EL(uint32_t, task_idx_out, i, cp[i]);
    cs[i] = (uint32_t)cp[i];
    pp[i] = &ps[i];
    if ((ps[i].n_exclude && !ps[i].exclude_task) || (cs[i] && !outs[i])) return COOK_E_INVALID;
  }
  return CHECKED(cook_cycle_autoscale_multi(es, (uint32_t)n, pp, outs, cs, info, rcs));
}

/* (hash uuid) of the pending jobs by pending ordinal (cook_cycle_set_job_hashes): hashes = n int32 values for rows [first, first + n) */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleSetJobHashes(JNIEnv* env, jclass c, jlong h, jobject hashes, jint first, jint n) {
  int bad = 0;
  const int32_t* hs = BUFN(const int32_t, hashes, n > 0 ? n : 0);
  (void)c;
  if (bad || first < 0 || n < 0 || (n && !hs)) return COOK_E_INVALID;
  return cook_cycle_set_job_hashes(H(h), hs, (uint32_t)first, (uint32_t)n);
}
/* one cook_autoscale_clusters from its columns: cols = {location uint32 [n], max_pods_outstanding, num_synthetic_pods, max_total_nodes,
 * total_nodes, max_total_pods, total_pods int64 [n], out_off uint32 [n + 1] or null, out_task uint32 [out_off[n]] or null} */
static cook_autoscale_clusters clusters_of(JNIEnv* env, jint n, jobjectArray cols, int* bad_out) {
  cook_autoscale_clusters cl;
  uint32_t total = 0;
  int bad = 0;
  if (n < 0 || n > COOK_MAX_CLUSTERS) {
    bad = 1;
    n = 0;
  }
  cl.n = (uint32_t)n;
  cl.reserved = 0;
  cl.location = EL(const uint32_t, cols, 0, n);
  cl.max_pods_outstanding = EL(const int64_t, cols, 1, n);
  cl.num_synthetic_pods = EL(const int64_t, cols, 2, n);
  cl.max_total_nodes = EL(const int64_t, cols, 3, n);
  cl.total_nodes = EL(const int64_t, cols, 4, n);
  cl.max_total_pods = EL(const int64_t, cols, 5, n);
  cl.total_pods = EL(const int64_t, cols, 6, n);
  cl.out_off = csr_off(env, cols, 7, n, &total, &bad);
  cl.out_task = EL(const uint32_t, cols, 8, total);
  if (bad || (total && !cl.out_task)) *bad_out = 1;
  return cl;
}
/* cycleAutoscale, then the distribution to the pool's autoscaling compute clusters and the cut per cluster
 * (cook_cycle_autoscale_clusters).  params, n_offers, offer_skipped, exclude, cap as cycleAutoscale; n_clusters and cluster_cols as
 * clusters_of; task_idx_out = cap uint32 slots; cluster_off_out = n_clusters + 1 uint32; info_out = one cook_autoscale_info or null;
 * cluster_info_out = n_clusters cook_autoscale_cluster_info; no_cluster_out = one cook_autoscale_no_cluster or null */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleAutoscaleClusters(JNIEnv* env, jclass c, jlong h, jobject params, jint n_offers,
                                                                   jobject offer_skipped, jobject exclude, jint n_clusters,
                                                                   jobjectArray cluster_cols, jobject task_idx_out, jint cap,
                                                                   jobject cluster_off_out, jobject info_out, jobject cluster_info_out,
                                                                   jobject no_cluster_out) {
  int bad = 0;
  cook_autoscale_params p;
  cook_autoscale_clusters cl;
  const jint nc = n_clusters > 0 ? n_clusters : 0;
  const cook_autoscale_params* in = BUF(const cook_autoscale_params, params);
  uint32_t* out = BUFN(uint32_t, task_idx_out, cap > 0 ? cap : 0);
  uint32_t* off = BUFN(uint32_t, cluster_off_out, (uint64_t)nc + 1u);
  cook_autoscale_info* info = BUF(cook_autoscale_info, info_out);
  cook_autoscale_cluster_info* cinfo = BUFN(cook_autoscale_cluster_info, cluster_info_out, nc);
  cook_autoscale_no_cluster* none = BUF(cook_autoscale_no_cluster, no_cluster_out);
  (void)c;
  if (bad || !in || !off || !cinfo || n_offers < 0 || cap < 0 || n_clusters < 1 || in->n_exclude > 0x7fffffffu) return COOK_E_INVALID;
  cl = clusters_of(env, n_clusters, cluster_cols, &bad);
  p = *in;
  p.offer_skipped = BUFN(const uint8_t, offer_skipped, n_offers);
  p.exclude_task = BUFN(const uint32_t, exclude, p.n_exclude);
  if ((p.n_exclude && !p.exclude_task) || (cap && !out)) return COOK_E_INVALID;
  return CHECKED(cook_cycle_autoscale_clusters(H(h), &p, &cl, out, (uint32_t)cap, off, info, cinfo, none));
}
/* cycleAutoscaleClusters for n engines of one device in ONE call (cook_cycle_autoscale_clusters_multi).  As cycleAutoscaleMulti, and
 * n_clusters = direct buffer of n jint; cluster_cols = array of n arrays as clusters_of takes them; cluster_off_out / cluster_info_out =
 * arrays of n direct buffers (n_clusters[i] + 1 uint32; n_clusters[i] cook_autoscale_cluster_info); no_cluster_out = direct buffer of
 * n cook_autoscale_no_cluster or null */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleAutoscaleClustersMulti(JNIEnv* env, jclass c, jobject handles, jint n, jobject params,
                                                                        jobject n_offers, jobjectArray offer_skipped, jobjectArray exclude,
                                                                        jobject n_clusters, jobjectArray cluster_cols,
                                                                        jobjectArray task_idx_out, jobject caps, jobjectArray cluster_off_out,
                                                                        jobject info_out, jobjectArray cluster_info_out,
                                                                        jobject no_cluster_out, jobject rc_out) {
  cook_engine* es[64];
  cook_autoscale_params ps[64];
  const cook_autoscale_params* pp[64];
  cook_autoscale_clusters cls[64];
  const cook_autoscale_clusters* clp[64];
  uint32_t* outs[64];
  uint32_t* offs[64];
  cook_autoscale_cluster_info* cinfos[64];
  uint32_t cs[64];
  int bad = 0;
  const jint cnt = n > 0 ? n : 0;
  const int64_t* hs = BUFN(const int64_t, handles, cnt);
  const cook_autoscale_params* in = BUFN(const cook_autoscale_params, params, cnt);
  const int32_t* no = BUFN(const int32_t, n_offers, cnt);
  const int32_t* ncl = BUFN(const int32_t, n_clusters, cnt);
  const int32_t* cp = BUFN(const int32_t, caps, cnt);
  cook_autoscale_info* info = BUFN(cook_autoscale_info, info_out, cnt);
  cook_autoscale_no_cluster* none = BUFN(cook_autoscale_no_cluster, no_cluster_out, cnt);
  int* rcs = BUFN(int, rc_out, cnt);
  jint i;
  (void)c;
  if (bad || !hs || !in || !no || !ncl || !cp || n <= 0 || n > 64 || !cluster_cols) return COOK_E_INVALID;
  for (i = 0; i < n; ++i) {
    jobjectArray cols;
    if (no[i] < 0 || cp[i] < 0 || ncl[i] < 1 || ncl[i] > COOK_MAX_CLUSTERS || in[i].n_exclude > 0x7fffffffu) return COOK_E_INVALID;
    if (i >= (*env)->GetArrayLength(env, cluster_cols)) return COOK_E_INVALID;
    es[i] = H(hs[i]);
    ps[i] = in[i];
    ps[i].offer_skipped = EL(const uint8_t, offer_skipped, i, no[i]);
    ps[i].exclude_task = EL(const uint32_t, exclude, i, ps[i].n_exclude);
    cols = (jobjectArray)(*env)->GetObjectArrayElement(env, cluster_cols, i);
    if (!cols) return COOK_E_INVALID;
    cls[i] = clusters_of(env, ncl[i], cols, &bad);
    (*env)->DeleteLocalRef(env, cols);
    outs[i] = EL(uint32_t, task_idx_out, i, cp[i]);
    offs[i] = EL(uint32_t, cluster_off_out, i, (uint64_t)ncl[i] + 1u);
    cinfos[i] = EL(cook_autoscale_cluster_info, cluster_info_out, i, ncl[i]);
    cs[i] = (uint32_t)cp[i];
    pp[i] = &ps[i];
    clp[i] = &cls[i];
    if ((ps[i].n_exclude && !ps[i].exclude_task) || (cs[i] && !outs[i]) || !offs[i] || !cinfos[i]) return COOK_E_INVALID;
  }
  return CHECKED(cook_cycle_autoscale_clusters_multi(es, (uint32_t)n, pp, clp, outs, cs, offs, info, cinfos, none, rcs));
}

/* ---- the task killers over the running set (cook_sweep_running) -------------------------------------------------------------------
 * rows = n-entry columns {start_ms int64, unknown uint8, max_runtime_ms int64, cancelled uint8, group uint32} (null elements allowed as
 * the header allows them); group_cols = {type uint8, quantile double, multiplier double, job_count uint32 [n_groups], succ_off uint32
 * [n_groups + 1], succ_start_ms int64, succ_end_ms int64 [succ_off[n_groups]]} or null; params = one cook_sweep_params; reason_out =
 * n bytes or null; idx_out = cap uint32 slots (3n always suffices); threshold_out = n_groups doubles or null; info_out = one
 * cook_sweep_info or null */
JNIEXPORT jint JNICALL Java_cook_hip_Native_sweepRunning(JNIEnv* env, jclass c, jlong h, jint n, jobjectArray rows, jint n_groups,
                                                         jobjectArray group_cols, jobject params, jobject reason_out, jobject idx_out,
                                                         jint cap, jobject threshold_out, jobject info_out) {
  int bad = 0;
  cook_running_set t;
  cook_straggler_groups g;
  const cook_sweep_params* p = BUF(const cook_sweep_params, params);
  uint8_t* reason = BUFN(uint8_t, reason_out, n > 0 ? n : 0);
  uint32_t* idx = BUFN(uint32_t, idx_out, cap > 0 ? cap : 0);
  double* thr = BUFN(double, threshold_out, n_groups > 0 ? n_groups : 0);
  cook_sweep_info* info = BUF(cook_sweep_info, info_out);
  uint32_t ns = 0;
  (void)c;
  if (n < 0 || n_groups < 0 || cap < 0 || !p) return COOK_E_INVALID;
  t.n = (uint32_t)n;
  t.start_ms = EL(const int64_t, rows, 0, n);
  t.unknown = EL(const uint8_t, rows, 1, n);
  t.max_runtime_ms = EL(const int64_t, rows, 2, n);
  t.cancelled = EL(const uint8_t, rows, 3, n);
  t.group = EL(const uint32_t, rows, 4, n);
  g.n = (uint32_t)n_groups;
  g.type = EL(const uint8_t, group_cols, 0, n_groups);
  g.quantile = EL(const double, group_cols, 1, n_groups);
  g.multiplier = EL(const double, group_cols, 2, n_groups);
  g.job_count = EL(const uint32_t, group_cols, 3, n_groups);
  g.succ_off = EL(const uint32_t, group_cols, 4, (uint64_t)n_groups + 1u);
  if (g.succ_off) ns = g.succ_off[n_groups];
  g.succ_start_ms = EL(const int64_t, group_cols, 5, ns);
  g.succ_end_ms = EL(const int64_t, group_cols, 6, ns);
  if (cap && !idx) return COOK_E_INVALID;
  return CHECKED(cook_sweep_running(H(h), &t, group_cols ? &g : 0, p, reason, idx, (uint32_t)cap, thr, info));
}

/* ---- the distributor of a Kubernetes-scheduler pool (cook_kube_distribute) ------------------------------------------------------------
 * location = n_jobs uint32 or null; draw = n_jobs doubles or null (then the draws come from seed); cluster_cols = {location uint32 [n],
 * capacity int64 [n]}; choice_out = n_jobs bytes; pos_idx_out = cap uint32 slots (n_jobs always suffices); cluster_off_out =
 * n_clusters + 1 uint32; cluster_info_out = n_clusters cook_kube_cluster_info; info_out = one cook_kube_info or null */
JNIEXPORT jint JNICALL Java_cook_hip_Native_kubeDistribute(JNIEnv* env, jclass c, jlong h, jint n_jobs, jobject location, jobject draw,
                                                           jlong seed, jint n_clusters, jobjectArray cluster_cols, jobject choice_out,
                                                           jobject pos_idx_out, jint cap, jobject cluster_off_out,
                                                           jobject cluster_info_out, jobject info_out) {
  int bad = 0;
  cook_kube_clusters cl;
  const jint nj = n_jobs > 0 ? n_jobs : 0, nc = n_clusters > 0 ? n_clusters : 0;
  const uint32_t* loc = BUFN(const uint32_t, location, nj);
  const double* dr = BUFN(const double, draw, nj);
  uint8_t* choice = BUFN(uint8_t, choice_out, nj);
  uint32_t* idx = BUFN(uint32_t, pos_idx_out, cap > 0 ? cap : 0);
  uint32_t* off = BUFN(uint32_t, cluster_off_out, (uint64_t)nc + 1u);
  cook_kube_cluster_info* cinfo = BUFN(cook_kube_cluster_info, cluster_info_out, nc);
  cook_kube_info* info = BUF(cook_kube_info, info_out);
  (void)c;
  if (bad || n_jobs < 0 || cap < 0 || n_clusters < 0 || n_clusters > COOK_MAX_CLUSTERS || !off) return COOK_E_INVALID;
  cl.n = (uint32_t)n_clusters;
  cl.reserved = 0;
  cl.location = EL(const uint32_t, cluster_cols, 0, n_clusters);
  cl.capacity = EL(const int64_t, cluster_cols, 1, n_clusters);
  if ((n_jobs && !choice) || (cap && !idx) || (n_clusters && (!cinfo || !cl.location || !cl.capacity))) return COOK_E_INVALID;
  return CHECKED(cook_kube_distribute(H(h), (uint32_t)n_jobs, loc, dr, (uint64_t)seed, &cl, choice, idx, (uint32_t)cap, off, cinfo, info));
}

/* ---- a Kubernetes-scheduler pool's cycle (cook_cycle_run_kube) ------------------------------------------------------------------------
 * rank_first, max_jobs_considered, min_capacity_threshold, seed as cook_kube_cycle; the queue step's parts as cycleRunQueueRelease takes
 * them, without offers (such a pool has none to edit: carry_offers / release_offers other than 0 are refused by the library);
 * cluster_cols = {location uint32 [n], capacity int64 [n]}; draw = n_draw doubles or null; task_idx_out = cap uint32 slots
 * (max_jobs_considered always suffices); cluster_off_out = n_clusters + 1 uint32; cluster_info_out = n_clusters cook_kube_cluster_info;
 * info_out = one cook_kube_info or null */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRunKube(JNIEnv* env, jclass c, jlong h, jint rank_first, jint max_jobs_considered,
                                                         jlong min_capacity_threshold, jlong seed, jint n_last_offers, jobject offer_skipped,
                                                         jint n_groups, jobjectArray groups, jint carry_offers, jint carry_usage, jint n_users,
                                                         jobject tokens_left, jint n_finished, jint n_fin_scalars, jobjectArray finished,
                                                         jint release_offers, jint release_usage, jint release_groups, jint n_clusters,
                                                         jobjectArray cluster_cols, jobject draw, jint n_draw, jobject task_idx_out, jint cap,
                                                         jobject cluster_off_out, jobject cluster_info_out, jobject info_out) {
  int bad = 0;
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  const cook_queue_step s = step_of(env, 1, n_last_offers, offer_skipped, 0, groups ? &g : 0, &bad);
  const cook_queue_carry cy = carry_of(env, carry_offers, carry_usage, n_users, tokens_left, &bad);
  const cook_finished f = finished_of(env, n_finished, n_fin_scalars, finished, release_offers, release_usage, release_groups, &bad);
  const jint nc = n_clusters > 0 ? n_clusters : 0;
  cook_kube_clusters cl;
  cook_kube_cycle k;
  uint32_t* out = BUFN(uint32_t, task_idx_out, cap > 0 ? cap : 0);
  uint32_t* off = BUFN(uint32_t, cluster_off_out, (uint64_t)nc + 1u);
  cook_kube_cluster_info* cinfo = BUFN(cook_kube_cluster_info, cluster_info_out, nc);
  cook_kube_info* info = BUF(cook_kube_info, info_out);
  (void)c;
  if (bad || max_jobs_considered < 0 || cap < 0 || n_draw < 0 || n_clusters < 0 || n_clusters > COOK_MAX_CLUSTERS || !off) return COOK_E_INVALID;
  cl.n = (uint32_t)n_clusters;
  cl.reserved = 0;
  cl.location = EL(const uint32_t, cluster_cols, 0, n_clusters);
  cl.capacity = EL(const int64_t, cluster_cols, 1, n_clusters);
  k.rank_first = (uint32_t)rank_first;
  k.max_jobs_considered = (uint32_t)max_jobs_considered;
  k.min_capacity_threshold = (int64_t)min_capacity_threshold;
  k.step = &s;
  k.carry = &cy;
  k.finished = finished ? &f : 0;
  k.clusters = &cl;
  k.draw = BUFN(const double, draw, n_draw);
  k.n_draw = (uint32_t)n_draw;
  k.reserved = 0;
  k.seed = (uint64_t)seed;
  if ((cap && !out) || (n_clusters && (!cinfo || !cl.location || !cl.capacity)) || (n_draw && !k.draw)) return COOK_E_INVALID;
  return CHECKED(cook_cycle_run_kube(H(h), &k, out, (uint32_t)cap, off, cinfo, info));
}
/* cycleRunKube for n pools of one device in ONE call (cook_cycle_run_kube_multi), for cycles without a release and without a groups
 * table (a pool that has either goes through cycleRunKube).  params = direct buffer of n records of eight int64 {rank_first,
 * max_jobs_considered, min_capacity_threshold, seed, n_clusters, n_draw, carry_usage, cap}; cluster_cols = array of n arrays {location,
 * capacity}; draws = array of n direct buffers or null elements; the outputs as arrays of n direct buffers; info_out = n cook_kube_info
 * or null; rc_out = n jint or null */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRunKubeMulti(JNIEnv* env, jclass c, jobject handles, jint n, jobject params,
                                                              jobjectArray cluster_cols, jobjectArray draws, jobjectArray task_idx_out,
                                                              jobjectArray cluster_off_out, jobjectArray cluster_info_out, jobject info_out,
                                                              jobject rc_out) {
  cook_engine* es[64];
  cook_kube_clusters cls[64];
  cook_kube_cycle ks[64];
  const cook_kube_cycle* kp[64];
  cook_queue_step steps[64];
  cook_queue_carry carries[64];
  uint32_t* outs[64];
  uint32_t* offs[64];
  cook_kube_cluster_info* cinfos[64];
  uint32_t caps[64];
  int bad = 0;
  const jint cnt = n > 0 ? n : 0;
  const int64_t* hs = BUFN(const int64_t, handles, cnt);
  const int64_t* ps = BUFN(const int64_t, params, (uint64_t)cnt * 8u);
  cook_kube_info* info = BUFN(cook_kube_info, info_out, cnt);
  int* rcs = BUFN(int, rc_out, cnt);
  jint i;
  (void)c;
  if (bad || !hs || !ps || n <= 0 || n > 64 || !cluster_cols) return COOK_E_INVALID;
  for (i = 0; i < n; ++i) {
    const int64_t* p = ps + 8 * i;
    jobjectArray cols;
    if (p[1] < 0 || p[1] > 0xffffffffll || p[4] < 0 || p[4] > COOK_MAX_CLUSTERS || p[5] < 0 || p[5] > 0x7fffffff || p[7] < 0 || p[7] > 0x7fffffff)
      return COOK_E_INVALID;
    if (i >= (*env)->GetArrayLength(env, cluster_cols)) return COOK_E_INVALID;
    cols = (jobjectArray)(*env)->GetObjectArrayElement(env, cluster_cols, i);
    cls[i].n = (uint32_t)p[4];
    cls[i].reserved = 0;
    cls[i].location = EL(const uint32_t, cols, 0, p[4]);
    cls[i].capacity = EL(const int64_t, cols, 1, p[4]);
    if (cols) (*env)->DeleteLocalRef(env, cols);
    steps[i].offer_skipped = 0;
    steps[i].remove_mode = 1;
    steps[i].n_offer_skipped = 0;
    steps[i].offers = 0;
    steps[i].groups = 0;
    carries[i].offers = 0;
    carries[i].usage = p[6] ? 1u : 0u;
    carries[i].tokens_left = 0;
    es[i] = H(hs[i]);
    ks[i].rank_first = p[0] ? 1u : 0u;
    ks[i].max_jobs_considered = (uint32_t)p[1];
    ks[i].min_capacity_threshold = p[2];
    ks[i].step = &steps[i];
    ks[i].carry = &carries[i];
    ks[i].finished = 0;
    ks[i].clusters = &cls[i];
    ks[i].draw = EL(const double, draws, i, p[5]);
    ks[i].n_draw = (uint32_t)p[5];
    ks[i].reserved = 0;
    ks[i].seed = (uint64_t)p[3];
    kp[i] = &ks[i];
    caps[i] = (uint32_t)p[7];
    outs[i] = EL(uint32_t, task_idx_out, i, p[7]);
    offs[i] = EL(uint32_t, cluster_off_out, i, (uint64_t)p[4] + 1u);
    cinfos[i] = EL(cook_kube_cluster_info, cluster_info_out, i, p[4]);
    if ((caps[i] && !outs[i]) || !offs[i] || (p[4] && (!cinfos[i] || !cls[i].location || !cls[i].capacity)) || (p[5] && !ks[i].draw))
      return COOK_E_INVALID;
  }
  return CHECKED(cook_cycle_run_kube_multi(es, (uint32_t)n, kp, outs, caps, offs, cinfos, info, rcs));
}
/* the cluster byte per considered position of the last Kubernetes cycle (cook_cycle_fetch_kube): choice_out = cap bytes, cap >= the
 * cycle's max_considerable; n_out = one uint32 */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleFetchKube(JNIEnv* env, jclass c, jlong h, jobject choice_out, jint cap, jobject n_out) {
  int bad = 0;
  uint8_t* choice = BUFN(uint8_t, choice_out, cap > 0 ? cap : 0);
  uint32_t* n = BUF(uint32_t, n_out);
  uint32_t k = 0;
  int rc;
  (void)c;
  if (bad || cap < 0 || !n) return COOK_E_INVALID;
  rc = cook_cycle_fetch_kube(H(h), 0, &k); /* (the count first: the buffer's capacity is checked against it) */
  if (rc != COOK_OK) return rc;
  if (k > (uint32_t)cap || (k && !choice)) return COOK_E_INVALID;
  return cook_cycle_fetch_kube(H(h), choice, n);
}

/* ---- rebalance: rebalancer/init-state + the rebalance loop's decisions ------------------------------------------------- */
JNIEXPORT jint JNICALL Java_cook_hip_Native_rebalance(JNIEnv* env, jclass c, jlong h, jint r, jobjectArray running,
                                                      jobject running_attrs_cached, jint p, jobjectArray pending,
                                                      jobject pending_job_id, jobject pending_priority, jint n_users,
                                                      jobjectArray users, jint n_spare, jobjectArray spare, jint n_attr_rows,
                                                      jobject attr_dims, jobjectArray host_attrs, jint n_groups,
                                                      jobjectArray groups, jobject rparams, jint max_preemption, jobject decisions_out,
                                                      jobject n_decisions_out, jobject preempted_out, jobject n_preempted_out,
                                                      jobject pending_dru_out) {
  int bad = 0;
  cook_tasks t = tasks_of(env, r, running, &bad);
  cook_jobs j = jobs_of(env, p, 0, pending, &bad);
  cook_users u = users_of(env, n_users, users, &bad);
  cook_offers a = offers_of(env, n_attr_rows, dims_of(env, attr_dims, &bad), host_attrs, &bad);
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  cook_host_spare s;
  const uint8_t* cached = BUFN(const uint8_t, running_attrs_cached, r);
  const int64_t* job_id = BUFN(const int64_t, pending_job_id, p);
  const int32_t* prio = BUFN(const int32_t, pending_priority, p);
  const cook_rebalance_params* rp = BUF(const cook_rebalance_params, rparams);
  /* at most max_preemption decisions (one per pending job examined) and r preempted tasks */
  cook_preemption* dec = BUFN(cook_preemption, decisions_out, (max_preemption < p ? max_preemption : p) > 0 ? (max_preemption < p ? max_preemption : p) : 0);
  uint32_t* n_dec = BUF(uint32_t, n_decisions_out);
  uint32_t* pre = BUFN(uint32_t, preempted_out, r);
  uint32_t* n_pre = BUF(uint32_t, n_preempted_out);
  double* pdru = BUFN(double, pending_dru_out, p);
  (void)c;
  s.n = (uint32_t)n_spare;
  s.host = EL(const uint32_t, spare, 0, n_spare);
  s.cpus = EL(const double, spare, 1, n_spare);
  s.mem = EL(const double, spare, 2, n_spare);
  s.gpus = EL(const double, spare, 3, n_spare);
  return CHECKED(cook_rebalance(H(h), &t, cached, &j, job_id, prio, &u, &s, host_attrs ? &a : 0, n_groups ? &g : 0, rp, dec, n_dec, pre,
                                n_pre, pdru));
}
/* the rebalancer's stage from the pool's resident cycle state (cook_cycle_rebalance_stage), then rebalanceRun / cycleRebalanceFetch.
 * spare (host, cpus, mem, gpus) null: from the staged offers; host_attrs null: the staged offer rows are the attribute table;
 * offer_skipped (n_offer_skipped bytes, one per offer of the last match) only with skip_matched != 0 */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRebalanceStage(JNIEnv* env, jclass c, jlong h, jobject rparams, jint n_spare, jobjectArray spare,
                                                                jint n_attr_rows, jobject attr_dims, jobjectArray host_attrs,
                                                                jint skip_matched, jint n_offer_skipped, jobject offer_skipped) {
  int bad = 0;
  cook_offers a = offers_of(env, n_attr_rows, dims_of(env, attr_dims, &bad), host_attrs, &bad);
  cook_host_spare s;
  cook_cycle_rebalance req;
  const cook_rebalance_params* rp = BUF(const cook_rebalance_params, rparams);
  const jint ns = n_spare > 0 ? n_spare : 0;
  (void)c;
  if (bad || !rp) return COOK_E_INVALID;
  s.n = (uint32_t)ns;
  s.host = EL(const uint32_t, spare, 0, ns);
  s.cpus = EL(const double, spare, 1, ns);
  s.mem = EL(const double, spare, 2, ns);
  s.gpus = EL(const double, spare, 3, ns);
  req.params = *rp;
  req.spare = spare ? &s : 0;
  req.host_attrs = host_attrs ? &a : 0;
  req.offer_skipped = BUFN(const uint8_t, offer_skipped, n_offer_skipped > 0 ? n_offer_skipped : 0);
  req.skip_matched = (uint32_t)skip_matched;
  req.reserved = 0u;
  return CHECKED(cook_cycle_rebalance_stage(H(h), &req));
}
/* the decision sweep over what was staged (cook_rebalance_run), between cycleRebalanceStage and cycleRebalanceFetch */
JNIEXPORT jint JNICALL Java_cook_hip_Native_rebalanceRun(JNIEnv* env, jclass c, jlong h) {
  (void)env;
  (void)c;
  return cook_rebalance_run(H(h));
}
/* the result in the host's index spaces (cook_cycle_rebalance_fetch): decisions_out / pending_dru_out / selected_task_out /
 * selected_ord_out hold cap_selected entries (min(max_preemption, ranked jobs)), preempted_out cap_preempted uint32 (running rows +
 * cap_selected); the three counts go to direct buffers of one uint32 each.  Any output may be null */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRebalanceFetch(JNIEnv* env, jclass c, jlong h, jint cap_selected, jint cap_preempted,
                                                                jobject decisions_out, jobject n_decisions_out, jobject preempted_out,
                                                                jobject n_preempted_out, jobject pending_dru_out, jobject selected_task_out,
                                                                jobject selected_ord_out, jobject n_selected_out) {
  int bad = 0;
  const jint cs = cap_selected > 0 ? cap_selected : 0, cp = cap_preempted > 0 ? cap_preempted : 0;
  cook_preemption* dec = BUFN(cook_preemption, decisions_out, cs);
  uint32_t* n_dec = BUF(uint32_t, n_decisions_out);
  uint32_t* pre = BUFN(uint32_t, preempted_out, cp);
  uint32_t* n_pre = BUF(uint32_t, n_preempted_out);
  double* pdru = BUFN(double, pending_dru_out, cs);
  uint32_t* st = BUFN(uint32_t, selected_task_out, cs);
  uint32_t* so = BUFN(uint32_t, selected_ord_out, cs);
  uint32_t* n_sel = BUF(uint32_t, n_selected_out);
  (void)c;
  return CHECKED(cook_cycle_rebalance_fetch(H(h), dec, n_dec, pre, n_pre, pdru, st, so, n_sel));
}

/* ---- offers: the numeric core of kubernetes.compute-cluster/generate-offers (compute_cluster.clj:68-190) ------------ */
static cook_nodes nodes_of(JNIEnv* env, jint n, jint n_attr_keys, jobjectArray a, int* bad_out) {
  cook_nodes v;
  int bad = 0;
  v.n = (uint32_t)n;
  v.host = EL(const uint32_t, a, 0, n);
  v.cpus = EL(const double, a, 1, n);
  v.mem = EL(const double, a, 2, n);
  v.gpus = EL(const int32_t, a, 3, n);
  v.gpu_model = EL(const uint32_t, a, 4, n);
  v.disk = EL(const double, a, 5, n);
  v.disk_type = EL(const uint32_t, a, 6, n);
  v.flags = EL(const uint8_t, a, 7, n);
  v.n_attr_keys = (uint32_t)n_attr_keys;
  v.attr = EL(const uint32_t, a, 8, (uint64_t)n * (uint64_t)(n_attr_keys > 0 ? n_attr_keys : 0));
  if (bad || n_attr_keys < 0) *bad_out = 1;
  return v;
}
static cook_pods pods_of(JNIEnv* env, jint n, jobjectArray a, int* bad_out) {
  cook_pods p;
  int bad = 0;
  p.n = (uint32_t)n;
  p.node = EL(const uint32_t, a, 0, n);
  p.cpus = EL(const double, a, 1, n);
  p.mem = EL(const double, a, 2, n);
  p.gpus = EL(const int32_t, a, 3, n);
  p.gpu_model = EL(const uint32_t, a, 4, n);
  p.disk = EL(const double, a, 5, n);
  p.disk_type = EL(const uint32_t, a, 6, n);
  p.flags = EL(const uint8_t, a, 7, n);
  if (bad) *bad_out = 1;
  return p;
}
/* the ten output columns of cook_node_offers as direct buffers, header field order, each with room for every node */
static cook_node_offers offer_cols_of(JNIEnv* env, jint n_nodes, jint n_attr_keys, const cook_offer_params* op, jobjectArray cols,
                                      int* bad_out) {
  cook_node_offers o;
  int bad = 0;
  const uint64_t gs = (op && op->gpu_slots) ? op->gpu_slots : 1u, ds = (op && op->disk_slots) ? op->disk_slots : 1u;
  o.node = EL(uint32_t, cols, 0, n_nodes);
  o.host = EL(uint32_t, cols, 1, n_nodes);
  o.cpus = EL(double, cols, 2, n_nodes);
  o.mem = EL(double, cols, 3, n_nodes);
  o.gpu_model = EL(uint32_t, cols, 4, (uint64_t)n_nodes * gs);
  o.gpu_count = EL(double, cols, 5, (uint64_t)n_nodes * gs);
  o.disk_type = EL(uint32_t, cols, 6, (uint64_t)n_nodes * ds);
  o.disk_space = EL(double, cols, 7, (uint64_t)n_nodes * ds);
  o.num_pods = EL(int32_t, cols, 8, n_nodes);
  o.attr = EL(uint32_t, cols, 9, (uint64_t)n_nodes * (uint64_t)(n_attr_keys > 0 ? n_attr_keys : 0));
  if (bad) *bad_out = 1;
  return o;
}
/* totals: one direct buffer holding a cook_offer_totals; by_model_type: {gpu capacity, gpu consumed, disk capacity, disk consumed}
 * buffers (n_gpu_models + 1 / n_disk_types + 1 entries) or nulls */
JNIEXPORT jint JNICALL Java_cook_hip_Native_offersBuild(JNIEnv* env, jclass c, jlong h, jint n_nodes, jint n_attr_keys,
                                                        jobjectArray nodes, jint n_pods, jobjectArray pods, jobject oparams,
                                                        jobjectArray offer_cols, jobject n_offers_out, jobject node_status_out,
                                                        jobject totals_out, jobjectArray by_model_type) {
  int bad = 0;
  cook_nodes nd = nodes_of(env, n_nodes, n_attr_keys, nodes, &bad);
  cook_pods pd = pods_of(env, n_pods, pods, &bad);
  const cook_offer_params* op = BUF(const cook_offer_params, oparams);
  cook_node_offers o = offer_cols_of(env, n_nodes, n_attr_keys, op, offer_cols, &bad);
  uint32_t* n_off = BUF(uint32_t, n_offers_out);
  uint8_t* status = BUFN(uint8_t, node_status_out, n_nodes);
  cook_offer_totals* tot = BUF(cook_offer_totals, totals_out);
  const uint64_t ng = op ? (uint64_t)op->n_gpu_models + 1u : 0u, nt = op ? (uint64_t)op->n_disk_types + 1u : 0u;
  int64_t *gcap = EL(int64_t, by_model_type, 0, ng), *gcons = EL(int64_t, by_model_type, 1, ng);
  double *dcap = EL(double, by_model_type, 2, nt), *dcons = EL(double, by_model_type, 3, nt);
  (void)c;
  return CHECKED(cook_offers_build(H(h), &nd, &pd, op, &o, n_off, status, tot, gcap, gcons, dcap, dcons));
}
/* staged form: node / pod state stays resident between cycles, run = kernels only */
JNIEXPORT jint JNICALL Java_cook_hip_Native_offersStage(JNIEnv* env, jclass c, jlong h, jint n_nodes, jint n_attr_keys, jobjectArray nodes,
                                                        jint n_pods, jobjectArray pods, jobject oparams) {
  int bad = 0;
  cook_nodes nd = nodes_of(env, n_nodes, n_attr_keys, nodes, &bad);
  cook_pods pd = pods_of(env, n_pods, pods, &bad);
  const cook_offer_params* op = BUF(const cook_offer_params, oparams);
  (void)c;
  return CHECKED(cook_offers_stage(H(h), &nd, &pd, op));
}
JNIEXPORT jint JNICALL Java_cook_hip_Native_offersRun(JNIEnv* env, jclass c, jlong h) {
  (void)env, (void)c;
  return cook_offers_run(H(h));
}
/* oparams: the cook_offer_params the rows were staged with (sizes the columns) */
JNIEXPORT jint JNICALL Java_cook_hip_Native_offersFetch(JNIEnv* env, jclass c, jlong h, jint n_nodes, jint n_attr_keys, jobject oparams,
                                                        jobjectArray offer_cols, jobject n_offers_out, jobject node_status_out,
                                                        jobject totals_out, jobjectArray by_model_type) {
  int bad = 0;
  const cook_offer_params* op = BUF(const cook_offer_params, oparams);
  cook_node_offers o = offer_cols_of(env, n_nodes, n_attr_keys, op, offer_cols, &bad);
  uint32_t* n_off = BUF(uint32_t, n_offers_out);
  uint8_t* status = BUFN(uint8_t, node_status_out, n_nodes);
  cook_offer_totals* tot = BUF(cook_offer_totals, totals_out);
  const uint64_t ng = op ? (uint64_t)op->n_gpu_models + 1u : 0u, nt = op ? (uint64_t)op->n_disk_types + 1u : 0u;
  int64_t *gcap = EL(int64_t, by_model_type, 0, ng), *gcons = EL(int64_t, by_model_type, 1, ng);
  double *dcap = EL(double, by_model_type, 2, nt), *dcons = EL(double, by_model_type, 3, nt);
  (void)c;
  return CHECKED(cook_offers_fetch(H(h), offer_cols ? &o : 0, n_off, status, tot, gcap, gcons, dcap, dcons));
}

/* ---- consumers of the placement's by-products ----------------------------------------------------------------------- */
/* fenzo-utils/summarize-placement-failure (fenzo_utils.clj:33-55): counts_out = direct buffer of n x COOK_WHY_SLOTS uint32 */
JNIEXPORT jint JNICALL Java_cook_hip_Native_matchExplain(JNIEnv* env, jclass c, jlong h, jobject job_pos, jint n, jobject counts_out) {
  int bad = 0;
  const uint32_t* pos = BUFN(const uint32_t, job_pos, n);
  uint32_t* counts = BUFN(uint32_t, counts_out, (uint64_t)(n > 0 ? n : 0) * COOK_WHY_SLOTS);
  (void)c;
  return CHECKED(cook_match_explain(H(h), pos, (uint32_t)n, counts));
}
/* handle-match-cycle-metrics (scheduler.clj:1210-1280): metrics_out = direct buffer holding a cook_cycle_metrics */
JNIEXPORT jint JNICALL Java_cook_hip_Native_matchMetrics(JNIEnv* env, jclass c, jlong h, jobject metrics_out, jobject user_considerable_out,
                                                         jobject user_matched_out, jint n_users, jobject job_gpus_out,
                                                         jobject offer_gpus_out, jint n_gpu_models) {
  int bad = 0;
  cook_cycle_metrics* m = BUF(cook_cycle_metrics, metrics_out);
  uint32_t *uc = BUFN(uint32_t, user_considerable_out, n_users), *um = BUFN(uint32_t, user_matched_out, n_users);
  int64_t *jg = BUFN(int64_t, job_gpus_out, (uint64_t)n_gpu_models + 1u), *og = BUFN(int64_t, offer_gpus_out, (uint64_t)n_gpu_models + 1u);
  (void)c;
  return CHECKED(cook_match_metrics(H(h), m, uc, um, (uint32_t)n_users, jg, og, (uint32_t)n_gpu_models));
}
/* matchMetrics for n engines of one device in ONE call (cook_match_metrics_multi).  metrics_out = direct buffer of n cook_cycle_metrics;
 * n_users / n_gpu_models = direct buffers of n jint; user_considerable_out / user_matched_out (n_users[i] uint32 each) and job_gpus_out /
 * offer_gpus_out (n_gpu_models[i] + 1 int64 each) = arrays of n direct buffers, a null array or element: left out; rc_out = n jint or null */
JNIEXPORT jint JNICALL Java_cook_hip_Native_matchMetricsMulti(JNIEnv* env, jclass c, jobject handles /* direct buffer of n jlong */, jint n,
                                                              jobject metrics_out, jobject n_users, jobjectArray user_considerable_out,
                                                              jobjectArray user_matched_out, jobject n_gpu_models, jobjectArray job_gpus_out,
                                                              jobjectArray offer_gpus_out, jobject rc_out) {
  cook_engine* es[64];
  cook_metrics_req rq[64];
  int bad = 0;
  const jint cnt = n > 0 ? n : 0;
  const int64_t* hs = BUFN(const int64_t, handles, cnt);
  cook_cycle_metrics* ms = BUFN(cook_cycle_metrics, metrics_out, cnt);
  const int32_t* nu = BUFN(const int32_t, n_users, cnt);
  const int32_t* nm = BUFN(const int32_t, n_gpu_models, cnt);
  int* rcs = BUFN(int, rc_out, cnt);
  jint i;
  (void)c;
  if (bad || !hs || !ms || !nu || !nm || n <= 0 || n > 64) return COOK_E_INVALID;
  for (i = 0; i < n; ++i) {
    if (nu[i] < 0 || nm[i] < 0) return COOK_E_INVALID;
    es[i] = H(hs[i]);
    rq[i].out = &ms[i];
    rq[i].user_considerable = EL(uint32_t, user_considerable_out, i, nu[i]);
    rq[i].user_matched = EL(uint32_t, user_matched_out, i, nu[i]);
    rq[i].n_users = (uint32_t)nu[i];
    rq[i].n_gpu_models = (uint32_t)nm[i];
    rq[i].job_gpus_by_model = EL(int64_t, job_gpus_out, i, (uint64_t)nm[i] + 1u);
    rq[i].offer_gpus_by_model = EL(int64_t, offer_gpus_out, i, (uint64_t)nm[i] + 1u);
  }
  return CHECKED(cook_match_metrics_multi(es, (uint32_t)n, rq, rcs));
}
/* ---- the launch resources of the last match's placed tasks (cook_match_launch_resources) ----------------------------------------------
 * n = the match's offers, k = its considered jobs (matchCount; another value: COOK_E_INVALID).  role_cols = {range_off uint32 [n + 1], range_begin int32, range_end int32,
 * range_role uint8 [range_off[n]], res_source uint32 [n_res], avail double [n_res * n_roles * n], offer_skipped uint8 [n] or null};
 * out_cols = {port_off uint32 [k + 1], port int32 [cap], port_role uint8 [cap], take double [k * n_res * n_roles], short_mask uint32 [k]};
 * info_out = one cook_launch_info */
JNIEXPORT jint JNICALL Java_cook_hip_Native_matchLaunchResources(JNIEnv* env, jclass c, jlong h, jint n, jint k, jint n_roles, jint n_res,
                                                                 jobjectArray role_cols, jint cap, jobjectArray out_cols, jobject info_out) {
  int bad = 0;
  cook_launch_offers o;
  cook_launch_out out;
  cook_launch_info* info = BUF(cook_launch_info, info_out);
  uint64_t n_ranges = 0, cells;
  uint32_t k_match = 0;
  (void)c;
  /* the engine writes cook_match_count entries, whatever k says: a k that is not that count would pass the size checks below and overrun
   * the buffers (before a match there is no count: the call itself then refuses with COOK_E_STATE and writes nothing) */
  if (cook_match_count(H(h), &k_match) == COOK_OK && (k < 0 || k_match != (uint32_t)k)) return COOK_E_INVALID;
  if (n < 0 || k < 0 || cap < 0 || n_roles < 1 || n_roles > COOK_MAX_ROLES || n_res < 1 || n_res > 2 + COOK_MAX_SCALARS || !info || !role_cols || !out_cols)
    return COOK_E_INVALID;
  cells = (uint64_t)n_res * (uint64_t)n_roles;
  o.n = (uint32_t)n, o.n_roles = (uint32_t)n_roles, o.n_res = (uint32_t)n_res, o.reserved = 0;
  o.range_off = EL(const uint32_t, role_cols, 0, (uint64_t)n + 1u);
  if (bad || !o.range_off) return COOK_E_INVALID;
  n_ranges = o.range_off[n];
  o.range_begin = EL(const int32_t, role_cols, 1, n_ranges);
  o.range_end = EL(const int32_t, role_cols, 2, n_ranges);
  o.range_role = EL(const uint8_t, role_cols, 3, n_ranges);
  o.res_source = EL(const uint32_t, role_cols, 4, n_res);
  o.avail = EL(const double, role_cols, 5, cells * (uint64_t)n);
  o.offer_skipped = EL(const uint8_t, role_cols, 6, n);
  out.cap = (uint32_t)cap, out.reserved = 0;
  out.port_off = EL(uint32_t, out_cols, 0, (uint64_t)k + 1u);
  out.port = EL(int32_t, out_cols, 1, cap);
  out.port_role = EL(uint8_t, out_cols, 2, cap);
  out.take = EL(double, out_cols, 3, cells * (uint64_t)k);
  out.short_mask = EL(uint32_t, out_cols, 4, k);
  return CHECKED(cook_match_launch_resources(H(h), &o, &out, info));
}
/* the rows of the last offersRun as the offers of a match / cycle, in place on the device */
JNIEXPORT jint JNICALL Java_cook_hip_Native_matchStageBuiltOffers(JNIEnv* env, jclass c, jlong h, jint k, jint n_scalars, jobjectArray jobs,
                                                                  jint n_groups, jobjectArray groups, jobject reserved_hosts,
                                                                  jint n_reserved, jint with_task_limits) {
  int bad = 0;
  cook_jobs j = jobs_of(env, k, n_scalars, jobs, &bad);
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  const uint32_t* res = BUFN(const uint32_t, reserved_hosts, n_reserved);
  (void)c;
  return CHECKED(cook_match_stage_built_offers(H(h), &j, groups ? &g : 0, res, (uint32_t)n_reserved, with_task_limits));
}
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleStageBuiltOffers(JNIEnv* env, jclass c, jlong h, jint n, jobjectArray tasks, jint n_users,
                                                                  jobjectArray users, jint n_pending, jint n_scalars,
                                                                  jobjectArray pending_jobs, jint n_groups, jobjectArray groups,
                                                                  jobject reserved_hosts, jint n_reserved, jint with_task_limits) {
  int bad = 0;
  cook_tasks t = tasks_of(env, n, tasks, &bad);
  cook_users u = users_of(env, n_users, users, &bad);
  cook_jobs j = jobs_of(env, n_pending, n_scalars, pending_jobs, &bad);
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  const uint32_t* res = BUFN(const uint32_t, reserved_hosts, n_reserved);
  (void)c;
  return CHECKED(cook_cycle_stage_built_offers(H(h), &t, &u, &j, groups ? &g : 0, res, (uint32_t)n_reserved, with_task_limits));
}

/* ---- the resident pod table: a pool whose offers are rebuilt from its pods every cycle (cook_offers_stage_pod_ids, cook_offers_update,
 * cook_offers_update_info, cook_offers_fetch_pods, cook_cycle_set_built_offers, cook_cycle_run_queue_pods*) ------------------------------
 * A pod delta: remove_id = direct buffer of n_remove uint32; add = the eight pod columns of pods_of (n_add rows), add_id = n_add uint32;
 * node_row = n_node_rows uint32, node_values = the nine node columns of nodes_of (n_node_rows rows, n_attr_keys keys).  Null arrays: none. */
static cook_pod_delta pod_delta_of(JNIEnv* env, jint n_remove, jobject remove_id, jint n_add, jobjectArray add, jobject add_id, jint n_node_rows,
                                   jobject node_row, jint n_attr_keys, jobjectArray node_values, cook_pods* pd, cook_nodes* nd, int* bad_out) {
  cook_pod_delta d;
  int bad = 0;
  const jint nr = n_remove > 0 ? n_remove : 0, na = n_add > 0 ? n_add : 0, nn = n_node_rows > 0 ? n_node_rows : 0;
  *pd = pods_of(env, na, add, &bad);
  *nd = nodes_of(env, nn, n_attr_keys, node_values, &bad);
  d.n_remove = remove_id ? (uint32_t)nr : 0u;
  d.remove_id = BUFN(const uint32_t, remove_id, nr);
  d.add = add ? pd : 0;
  d.add_id = BUFN(const uint32_t, add_id, na);
  d.n_node_rows = node_row ? (uint32_t)nn : 0u;
  d.node_row = BUFN(const uint32_t, node_row, nn);
  d.node_values = node_values ? nd : 0;
  if (bad || n_remove < 0 || n_add < 0 || n_node_rows < 0) *bad_out = 1;
  return d;
}
/* pod_id: direct buffer of n uint32 (the staged pods' ids, row order) */
JNIEXPORT jint JNICALL Java_cook_hip_Native_offersStagePodIds(JNIEnv* env, jclass c, jlong h, jint n, jobject pod_id, jint id_cap) {
  int bad = 0;
  const jint np = n > 0 ? n : 0;
  const uint32_t* ids = BUFN(const uint32_t, pod_id, np);
  (void)c;
  if (bad || n < 0 || id_cap < 0) return COOK_E_INVALID;
  return cook_offers_stage_pod_ids(H(h), ids, (uint32_t)np, (uint32_t)id_cap);
}
JNIEXPORT jint JNICALL Java_cook_hip_Native_offersUpdate(JNIEnv* env, jclass c, jlong h, jint n_remove, jobject remove_id, jint n_add,
                                                         jobjectArray add, jobject add_id, jint n_node_rows, jobject node_row,
                                                         jint n_attr_keys, jobjectArray node_values) {
  int bad = 0;
  cook_pods pd;
  cook_nodes nd;
  const cook_pod_delta d = pod_delta_of(env, n_remove, remove_id, n_add, add, add_id, n_node_rows, node_row, n_attr_keys, node_values, &pd, &nd, &bad);
  (void)c;
  return CHECKED(cook_offers_update(H(h), &d));
}
/* the counts of the last pod delta (cook_offers_update_info): info_out = direct buffer of one cook_pod_delta_info */
JNIEXPORT jint JNICALL Java_cook_hip_Native_offersUpdateInfo(JNIEnv* env, jclass c, jlong h, jobject info_out) {
  int bad = 0;
  cook_pod_delta_info* out = BUF(cook_pod_delta_info, info_out);
  (void)c;
  if (bad || !out) return COOK_E_INVALID;
  return cook_offers_update_info(H(h), out);
}
/* The pod table as it stands (cook_offers_fetch_pods).  cols: {node, cpus, mem, gpus, gpu_model, disk, disk_type, flags, id} direct
 * buffers with room for cap rows each (null: skipped); n_out: direct buffer of one jint that receives the row count (also when cap is
 * too small: COOK_E_INVALID, no column written) */
JNIEXPORT jint JNICALL Java_cook_hip_Native_offersFetchPods(JNIEnv* env, jclass c, jlong h, jint cap, jobjectArray cols, jobject n_out) {
  int bad = 0, rc;
  const jint cp = cap > 0 ? cap : 0;
  cook_pod_rows r;
  jint* n = BUF(jint, n_out);
  (void)c;
  r.cap = (uint32_t)cp;
  r.n = 0;
  r.node = EL(uint32_t, cols, 0, cp);
  r.cpus = EL(double, cols, 1, cp);
  r.mem = EL(double, cols, 2, cp);
  r.gpus = EL(int32_t, cols, 3, cp);
  r.gpu_model = EL(uint32_t, cols, 4, cp);
  r.disk = EL(double, cols, 5, cp);
  r.disk_type = EL(uint32_t, cols, 6, cp);
  r.flags = EL(uint8_t, cols, 7, cp);
  r.id = EL(uint32_t, cols, 8, cp);
  if (bad || cap < 0) return COOK_E_INVALID;
  rc = cook_offers_fetch_pods(H(h), &r);
  if (n) *n = (jint)r.n;
  return rc;
}
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleSetBuiltOffers(JNIEnv* env, jclass c, jlong h, jint with_task_limits) {
  (void)env, (void)c;
  return cook_cycle_set_built_offers(H(h), with_task_limits);
}
/* cycleRunQueueReserve of a pool whose offers are built from its pods (cook_cycle_run_queue_pods; defer != 0:
 * cook_cycle_run_queue_pods_multi for this one pool, the placement then runs in cycleMatchMulti): no host churn, the pod delta of
 * pod_delta_of in its place (has_pods = 0: none, a rebuild from the table as it stands); the step carries no offers. */
JNIEXPORT jint JNICALL Java_cook_hip_Native_cycleRunQueuePods(JNIEnv* env, jclass c, jlong h, jint num_considerable, jint remove_mode,
                                                              jint n_last_offers, jobject offer_skipped, jint n_groups, jobjectArray groups,
                                                              jint carry_usage, jint n_users, jobject tokens_left, jint n_finished,
                                                              jint n_fin_scalars, jobjectArray finished, jint release_usage, jint release_groups,
                                                              jint has_pods, jint n_remove, jobject remove_id, jint n_add, jobjectArray add,
                                                              jobject add_id, jint n_node_rows, jobject node_row, jint n_attr_keys,
                                                              jobjectArray node_values, jint release_matched, jint replace, jint n_reserve,
                                                              jobject rsv_pending, jobject rsv_host, jint with_task_limits, jint defer) {
  int bad = 0;
  cook_pods pd;
  cook_nodes nd;
  cook_groups g = groups_of(env, n_groups, groups, &bad);
  const cook_queue_step s = step_of(env, remove_mode, n_last_offers, offer_skipped, 0, groups ? &g : 0, &bad);
  const cook_queue_carry cy = carry_of(env, 0, carry_usage, n_users, tokens_left, &bad);
  const cook_finished f = finished_of(env, n_finished, n_fin_scalars, finished, 0, release_usage, release_groups, &bad);
  const cook_reservations rv = reservations_of(env, release_matched, replace, n_reserve, rsv_pending, rsv_host, &bad);
  const cook_pod_delta d = pod_delta_of(env, n_remove, remove_id, n_add, add, add_id, n_node_rows, node_row, n_attr_keys, node_values, &pd, &nd, &bad);
  cook_engine* e = H(h);
  const cook_queue_step* sp = &s;
  const uint32_t k = (uint32_t)num_considerable;
  const cook_queue_carry* cp = &cy;
  const cook_finished* fp = finished ? &f : 0;
  const cook_pod_delta* dp = has_pods ? &d : 0;
  const cook_reservations* rp = &rv;
  const int32_t wl = (int32_t)with_task_limits;
  (void)c;
  if (bad) return COOK_E_INVALID;
  return defer ? cook_cycle_run_queue_pods_multi(&e, 1, &sp, &cp, &fp, &dp, &rp, &wl, &k)
               : cook_cycle_run_queue_pods(e, sp, cp, fp, dp, rp, with_task_limits, k);
}
