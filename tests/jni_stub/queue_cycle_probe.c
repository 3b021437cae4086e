/* What the JNI shim hands to the queue-cycle entries of the C ABI (TEST INFRASTRUCTURE, host only, no GPU and no library).
 * The program includes bindings/jni/cookmatch_jni.c, gives it a JNIEnv over fake direct buffers and object arrays, and defines
 * the eleven cook_cycle_run_queue* entries and cook_cycle_set_reservations itself: each prints which entry was called, n,
 * num_considerable and every part's struct (null or not; every scalar; every pointer field null or its first and last element).
 * Built with -ffunction-sections and linked with -Wl,--gc-sections, so the shim's other exports and the cook_* functions they
 * call are dropped.  tests/test_jni_queue_abi.py compares the output with tests/golden/jni_queue_cycle_probe.txt, which was
 * recorded from the shim as it stood before its marshalling was folded into one helper per struct. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../bindings/jni/cookmatch_jni.c"

/* ---- the fake JVM: a "direct buffer" is {address, capacity}, an "object array" is {length, elements} --------------------------- */
typedef struct fake_buf {
  void* address;
  jlong capacity;
} fake_buf;
typedef struct fake_arr {
  jsize length;
  jobject* elements;
} fake_arr;

static void* env_address(JNIEnv* env, jobject b) {
  (void)env;
  return ((fake_buf*)b)->address;
}
static jlong env_capacity(JNIEnv* env, jobject b) {
  (void)env;
  return ((fake_buf*)b)->capacity;
}
static jsize env_length(JNIEnv* env, jobjectArray a) {
  (void)env;
  return ((fake_arr*)a)->length;
}
static jobject env_element(JNIEnv* env, jobjectArray a, jsize i) {
  (void)env;
  return ((fake_arr*)a)->elements[i];
}
static jstring env_string(JNIEnv* env, const char* s) {
  (void)env;
  return (jstring)(intptr_t)s;
}
static void env_delete_local(JNIEnv* env, jobject o) {
  (void)env;
  (void)o;
}
static jobject env_new_buffer(JNIEnv* env, void* p, jlong n) {
  fake_buf* b = (fake_buf*)malloc(sizeof *b);
  (void)env;
  b->address = p;
  b->capacity = n;
  return b;
}
static const struct JNINativeInterface_ g_table = {env_address, env_length, env_element, env_string, env_capacity, env_delete_local, env_new_buffer};
static JNIEnv g_env = &g_table;

/* a buffer of `count` elements of `size` bytes; element i holds base + i (doubles: base + i + 0.5); `cut` bytes short of that */
enum { T_U8, T_I32, T_U32, T_I64, T_F64 };
static jobject buf(int type, uint64_t count, int base, int cut) {
  static const size_t size_of[] = {1, 4, 4, 8, 8};
  const size_t size = size_of[type];
  unsigned char* p = (unsigned char*)calloc(count ? count : 1, size);
  uint64_t i;
  for (i = 0; i < count; ++i) switch (type) {
      case T_U8: ((uint8_t*)p)[i] = (uint8_t)(base + (int)i); break;
      case T_I32: ((int32_t*)p)[i] = base + (int)i; break;
      case T_U32: ((uint32_t*)p)[i] = (uint32_t)(base + (int)i); break;
      case T_I64: ((int64_t*)p)[i] = base + (int)i; break;
      default: ((double*)p)[i] = base + (int)i + 0.5; break;
    }
  return env_new_buffer(&g_env, p, (jlong)(count * size) - cut);
}
static jobjectArray arr(jsize n) {
  fake_arr* a = (fake_arr*)malloc(sizeof *a);
  a->length = n;
  a->elements = (jobject*)calloc((size_t)n, sizeof(jobject));
  return a;
}
#define SET(a, i, b) (((fake_arr*)(a))->elements[i] = (b))

/* ---- the recording cook_* entries ---------------------------------------------------------------------------------------------- */
static int g_calls = 0;
static uint32_t g_n_users = 0; /* the length of cook_queue_carry.tokens_left, which the struct does not carry */

#define SHOW(fmt, T, name, p, count)                                                         \
  do {                                                                                       \
    const T* q_ = (p);                                                                       \
    const uint64_t c_ = (count);                                                             \
    if (!q_) printf(" %s=null", name);                                                       \
    else if (!c_) printf(" %s=[]", name);                                                    \
    else printf(" %s=[" fmt ".." fmt "]x%" PRIu64, name, q_[0], q_[c_ - 1], c_);             \
  } while (0)
#define SHOW_U8(name, p, count) SHOW("%u", uint8_t, name, p, count)
#define SHOW_I32(name, p, count) SHOW("%" PRId32, int32_t, name, p, count)
#define SHOW_U32(name, p, count) SHOW("%" PRIu32, uint32_t, name, p, count)
#define SHOW_I64(name, p, count) SHOW("%" PRId64, int64_t, name, p, count)
#define SHOW_F64(name, p, count) SHOW("%.1f", double, name, p, count)

static void show_offers(const char* what, const cook_offers* o) {
  uint64_t n, gs, ds;
  if (!o) {
    printf("    %s=null\n", what);
    return;
  }
  n = o->n, gs = o->gpu_slots ? o->gpu_slots : 1u, ds = o->disk_slots ? o->disk_slots : 1u;
  printf("    %s: n=%u n_attr_keys=%u gpu_slots=%u disk_slots=%u n_scalars=%u reserved_=%u\n     ", what, o->n, o->n_attr_keys, o->gpu_slots,
         o->disk_slots, o->n_scalars, o->reserved_);
  SHOW_F64("cpus", o->cpus, n);
  SHOW_F64("mem", o->mem, n);
  SHOW_U32("host", o->host, n);
  SHOW_U8("k8s", o->k8s, n);
  SHOW_U32("gpu_model", o->gpu_model, n * gs);
  SHOW_F64("gpu_count", o->gpu_count, n * gs);
  SHOW_U32("disk_type", o->disk_type, n * ds);
  SHOW_F64("disk_space", o->disk_space, n * ds);
  SHOW_U32("attr", o->attr, n * o->n_attr_keys);
  printf("\n     ");
  SHOW_I32("max_tasks", o->max_tasks, n);
  SHOW_I32("num_tasks", o->num_tasks, n);
  SHOW_U32("location", o->location, n);
  SHOW_I64("host_start_s", o->host_start_s, n);
  SHOW_F64("run_cpus", o->run_cpus, n);
  SHOW_F64("run_mem", o->run_mem, n);
  SHOW_I32("run_count", o->run_count, n);
  SHOW_I32("ports", o->ports, n);
  SHOW_F64("scalars", o->scalars, n * o->n_scalars);
  printf("\n");
}
static void show_step(const cook_queue_step* s) {
  if (!s) {
    printf("  step=null\n");
    return;
  }
  printf("  step: remove_mode=%u n_offer_skipped=%u", s->remove_mode, s->n_offer_skipped);
  SHOW_U8("offer_skipped", s->offer_skipped, s->n_offer_skipped);
  printf("\n");
  show_offers("offers", s->offers);
  if (!s->groups) {
    printf("    groups=null\n");
  } else {
    const cook_groups* g = s->groups;
    const uint64_t nr = g->run_off ? g->run_off[g->n] : 0u;
    printf("    groups: n=%u", g->n);
    SHOW_U8("type", g->type, g->n);
    SHOW_U32("attr_key", g->attr_key, g->n);
    SHOW_I32("minimum", g->minimum, g->n);
    SHOW_U32("run_off", g->run_off, (uint64_t)g->n + 1u);
    SHOW_U32("run_host", g->run_host, nr);
    SHOW_U32("run_attr", g->run_attr, nr);
    printf("\n");
  }
}
static void show_carry(const cook_queue_carry* c) {
  if (!c) {
    printf("  carry=null\n");
    return;
  }
  printf("  carry: offers=%u usage=%u", c->offers, c->usage);
  SHOW_I64("tokens_left", c->tokens_left, g_n_users);
  printf("\n");
}
static void show_finished(const cook_finished* f) {
  if (!f) {
    printf("  finished=null\n");
    return;
  }
  printf("  finished: n=%u n_scalars=%u offers=%u usage=%u groups=%u\n   ", f->n, f->n_scalars, f->offers, f->usage, f->groups);
  SHOW_U32("host", f->host, f->n);
  SHOW_U32("user", f->user, f->n);
  SHOW_F64("cpus", f->cpus, f->n);
  SHOW_F64("mem", f->mem, f->n);
  SHOW_F64("gpus", f->gpus, f->n);
  SHOW_I32("ports", f->ports, f->n);
  SHOW_F64("scalars", f->scalars, (uint64_t)f->n * f->n_scalars);
  SHOW_U32("gpu_model", f->gpu_model, f->n);
  SHOW_F64("disk_request", f->disk_request, f->n);
  SHOW_U32("disk_type", f->disk_type, f->n);
  SHOW_U32("group", f->group, f->n);
  printf("\n");
}
static void show_hosts(const cook_host_churn* h) {
  if (!h) {
    printf("  hosts=null\n");
    return;
  }
  printf("  hosts: n_leave=%u", h->n_leave);
  SHOW_U32("leave_host", h->leave_host, h->n_leave);
  SHOW_U32("join_before", h->join_before, h->join ? h->join->n : 0u);
  printf("\n");
  show_offers("join", h->join);
}
static void show_reservations(const cook_reservations* r) {
  if (!r) {
    printf("  reservations=null\n");
    return;
  }
  printf("  reservations: release_matched=%u replace=%u n=%u", r->release_matched, r->replace, r->n);
  SHOW_U32("pending", r->pending, r->n);
  SHOW_U32("host", r->host, r->n);
  printf("\n");
}
/* every entry answers with a code of its own, so the probe also shows that the shim returns what the entry returned */
static int entry(const char* name, int code, cook_engine* e, uint32_t n, uint32_t k) {
  ++g_calls;
  printf("  -> %s engine=%#" PRIxPTR " n=%u num_considerable=%u\n", name, (uintptr_t)e, n, k);
  return code;
}
#define AT0(a) ((a) ? (a)[0] : 0)

int cook_cycle_run_queue(cook_engine* e, const cook_queue_step* s, uint32_t k) {
  const int rc = entry("cook_cycle_run_queue", 101, e, 1, k);
  show_step(s);
  return rc;
}
int cook_cycle_run_queue_rank(cook_engine* e, const cook_queue_step* s, uint32_t k) {
  const int rc = entry("cook_cycle_run_queue_rank", 102, e, 1, k);
  show_step(s);
  return rc;
}
int cook_cycle_run_queue_multi(cook_engine** es, uint32_t n, const cook_queue_step* const* ss, const uint32_t* ks) {
  const int rc = entry("cook_cycle_run_queue_multi", 103, es[0], n, ks[0]);
  show_step(AT0(ss));
  return rc;
}
int cook_cycle_run_queue_carry(cook_engine* e, const cook_queue_step* s, const cook_queue_carry* c, uint32_t k) {
  const int rc = entry("cook_cycle_run_queue_carry", 104, e, 1, k);
  show_step(s), show_carry(c);
  return rc;
}
int cook_cycle_run_queue_carry_multi(cook_engine** es, uint32_t n, const cook_queue_step* const* ss, const cook_queue_carry* const* cs,
                                     const uint32_t* ks) {
  const int rc = entry("cook_cycle_run_queue_carry_multi", 105, es[0], n, ks[0]);
  show_step(AT0(ss)), show_carry(AT0(cs));
  return rc;
}
int cook_cycle_run_queue_release(cook_engine* e, const cook_queue_step* s, const cook_queue_carry* c, const cook_finished* f, uint32_t k) {
  const int rc = entry("cook_cycle_run_queue_release", 106, e, 1, k);
  show_step(s), show_carry(c), show_finished(f);
  return rc;
}
int cook_cycle_run_queue_release_multi(cook_engine** es, uint32_t n, const cook_queue_step* const* ss, const cook_queue_carry* const* cs,
                                       const cook_finished* const* fs, const uint32_t* ks) {
  const int rc = entry("cook_cycle_run_queue_release_multi", 107, es[0], n, ks[0]);
  show_step(AT0(ss)), show_carry(AT0(cs)), show_finished(AT0(fs));
  return rc;
}
int cook_cycle_run_queue_hosts(cook_engine* e, const cook_queue_step* s, const cook_queue_carry* c, const cook_finished* f,
                               const cook_host_churn* h, uint32_t k) {
  const int rc = entry("cook_cycle_run_queue_hosts", 108, e, 1, k);
  show_step(s), show_carry(c), show_finished(f), show_hosts(h);
  return rc;
}
int cook_cycle_run_queue_hosts_multi(cook_engine** es, uint32_t n, const cook_queue_step* const* ss, const cook_queue_carry* const* cs,
                                     const cook_finished* const* fs, const cook_host_churn* const* hs, const uint32_t* ks) {
  const int rc = entry("cook_cycle_run_queue_hosts_multi", 109, es[0], n, ks[0]);
  show_step(AT0(ss)), show_carry(AT0(cs)), show_finished(AT0(fs)), show_hosts(AT0(hs));
  return rc;
}
int cook_cycle_run_queue_reserve(cook_engine* e, const cook_queue_step* s, const cook_queue_carry* c, const cook_finished* f,
                                 const cook_host_churn* h, const cook_reservations* r, uint32_t k) {
  const int rc = entry("cook_cycle_run_queue_reserve", 110, e, 1, k);
  show_step(s), show_carry(c), show_finished(f), show_hosts(h), show_reservations(r);
  return rc;
}
int cook_cycle_run_queue_reserve_multi(cook_engine** es, uint32_t n, const cook_queue_step* const* ss, const cook_queue_carry* const* cs,
                                       const cook_finished* const* fs, const cook_host_churn* const* hs, const cook_reservations* const* rs,
                                       const uint32_t* ks) {
  const int rc = entry("cook_cycle_run_queue_reserve_multi", 111, es[0], n, ks[0]);
  show_step(AT0(ss)), show_carry(AT0(cs)), show_finished(AT0(fs)), show_hosts(AT0(hs)), show_reservations(AT0(rs));
  return rc;
}
int cook_cycle_set_reservations(cook_engine* e, const cook_reservations* r) {
  const int rc = entry("cook_cycle_set_reservations", 112, e, 1, 0);
  show_reservations(r);
  return rc;
}

/* ---- the calls ----------------------------------------------------------------------------------------------------------------- */
/* the sizes of every case: distinct, so a count taken from the wrong argument shows in the x<count> of a column */
enum { K = 77, REMOVE_MODE = 1, N_LAST = 5, M = 3, N_GROUPS = 2, N_RUN = 3, N_USERS = 6, NF = 3, NS = 2, N_LEAVE = 4, M_JOIN = 2, N_RESERVE = 7 };
static const jlong HANDLE = 0x1234;

/* the objects of one call; a null member is a null argument.  `cut` names the one buffer that is a byte short (0: none). */
typedef struct objects {
  jobject offer_skipped, offer_dims, tokens_left, leave_host, join_dims, join_before, rsv_pending, rsv_host;
  jobjectArray offers, groups, finished, join;
} objects;
enum { CUT_NONE, CUT_SKIPPED, CUT_OFFER_COL, CUT_GROUP_RUN, CUT_TOKENS, CUT_FIN_SCALARS, CUT_FIN_GROUP, CUT_LEAVE, CUT_JOIN_BEFORE, CUT_JOIN_COL,
       CUT_RSV_PENDING, CUT_RSV_HOST };

/* an offers array of n rows at dims {n_attr_keys 2, gpu_slots 2, disk_slots 3, n_scalars 2}; column i starts at base + 100 * i */
static jobject dims_buf(void) {
  fake_buf* b = (fake_buf*)buf(T_I32, 4, 0, 0);
  jint* d = (jint*)b->address;
  d[0] = 2, d[1] = 2, d[2] = 3, d[3] = 2;
  return b;
}
static jobjectArray offers_arr(uint64_t n, int base, int cut_scalars) {
  static const int type[18] = {T_F64, T_F64, T_U32, T_U8, T_U32, T_F64, T_U32, T_F64, T_U32, T_I32, T_I32, T_U32, T_I64, T_F64, T_F64, T_I32, T_I32, T_F64};
  static const int width[18] = {1, 1, 1, 1, 2, 2, 3, 3, 2, 1, 1, 1, 1, 1, 1, 1, 1, 2};
  jobjectArray a = arr(18);
  int i;
  for (i = 0; i < 18; ++i) SET(a, i, buf(type[i], n * (uint64_t)width[i], type[i] == T_U8 ? 10 * i : base + 100 * i, i == 17 ? cut_scalars : 0));
  return a;
}
static objects all_present(int cut) {
  objects o;
  o.offer_skipped = buf(T_U8, N_LAST, 40, cut == CUT_SKIPPED);
  o.offer_dims = dims_buf();
  o.offers = offers_arr(M, 1000, cut == CUT_OFFER_COL);
  o.groups = arr(6);
  SET(o.groups, 0, buf(T_U8, N_GROUPS, 50, 0));
  SET(o.groups, 1, buf(T_U32, N_GROUPS, 5100, 0));
  SET(o.groups, 2, buf(T_I32, N_GROUPS, 5200, 0));
  SET(o.groups, 3, buf(T_U32, N_GROUPS + 1, 0, 0));
  ((uint32_t*)((fake_buf*)((fake_arr*)o.groups)->elements[3])->address)[1] = 1u;
  ((uint32_t*)((fake_buf*)((fake_arr*)o.groups)->elements[3])->address)[2] = N_RUN;
  SET(o.groups, 4, buf(T_U32, N_RUN, 5400, cut == CUT_GROUP_RUN));
  SET(o.groups, 5, buf(T_U32, N_RUN, 5500, 0));
  o.tokens_left = buf(T_I64, N_USERS, 6000, cut == CUT_TOKENS);
  {
    static const int type[11] = {T_U32, T_U32, T_F64, T_F64, T_F64, T_I32, T_F64, T_U32, T_F64, T_U32, T_U32};
    int i;
    o.finished = arr(11);
    for (i = 0; i < 11; ++i)
      SET(o.finished, i, buf(type[i], i == 6 ? NF * NS : NF, 7000 + 100 * i, (i == 6 && cut == CUT_FIN_SCALARS) || (i == 10 && cut == CUT_FIN_GROUP)));
  }
  o.leave_host = buf(T_U32, N_LEAVE, 8500, cut == CUT_LEAVE);
  o.join_dims = dims_buf();
  o.join = offers_arr(M_JOIN, 3000, cut == CUT_JOIN_COL);
  o.join_before = buf(T_U32, M_JOIN, 8600, cut == CUT_JOIN_BEFORE);
  o.rsv_pending = buf(T_U32, N_RESERVE, 9000, cut == CUT_RSV_PENDING);
  o.rsv_host = buf(T_U32, N_RESERVE, 9100, cut == CUT_RSV_HOST);
  return o;
}
static objects all_null(void) {
  objects o;
  memset(&o, 0, sizeof o);
  return o;
}

/* export 0..4 = cycleRunQueue, ..Carry, ..Release, ..Hosts, ..Reserve; the flags of the parts are distinct too */
static const char* const EXPORT[5] = {"cycleRunQueue", "cycleRunQueueCarry", "cycleRunQueueRelease", "cycleRunQueueHosts", "cycleRunQueueReserve"};
static jint call_export(int which, const objects* o, jint defer) {
  JNIEnv* env = &g_env;
  switch (which) {
    case 0:
      return Java_cook_hip_Native_cycleRunQueue(env, 0, HANDLE, K, REMOVE_MODE, N_LAST, o->offer_skipped, M, o->offer_dims, o->offers, N_GROUPS,
                                                o->groups, defer);
    case 1:
      return Java_cook_hip_Native_cycleRunQueueCarry(env, 0, HANDLE, K, REMOVE_MODE, N_LAST, o->offer_skipped, M, o->offer_dims, o->offers, N_GROUPS,
                                                     o->groups, 11, 12, N_USERS, o->tokens_left, defer);
    case 2:
      return Java_cook_hip_Native_cycleRunQueueRelease(env, 0, HANDLE, K, REMOVE_MODE, N_LAST, o->offer_skipped, M, o->offer_dims, o->offers, N_GROUPS,
                                                       o->groups, 11, 12, N_USERS, o->tokens_left, NF, NS, o->finished, 21, 22, 23, defer);
    case 3:
      return Java_cook_hip_Native_cycleRunQueueHosts(env, 0, HANDLE, K, REMOVE_MODE, N_LAST, o->offer_skipped, N_GROUPS, o->groups, 11, 12, N_USERS,
                                                     o->tokens_left, NF, NS, o->finished, 21, 22, 23, N_LEAVE, o->leave_host, M_JOIN, o->join_dims,
                                                     o->join, o->join_before, defer);
    default:
      return Java_cook_hip_Native_cycleRunQueueReserve(env, 0, HANDLE, K, REMOVE_MODE, N_LAST, o->offer_skipped, N_GROUPS, o->groups, 11, 12, N_USERS,
                                                       o->tokens_left, NF, NS, o->finished, 21, 22, 23, N_LEAVE, o->leave_host, M_JOIN, o->join_dims,
                                                       o->join, o->join_before, 31, 32, N_RESERVE, o->rsv_pending, o->rsv_host, defer);
  }
}

static int g_failures = 0;
static void short_case(const char* what, int which, int cut, jint defer) {
  const objects o = all_present(cut);
  const int before = g_calls;
  const jint rc = which < 5 ? call_export(which, &o, defer) : Java_cook_hip_Native_cycleSetReservations(&g_env, 0, HANDLE, N_RESERVE, o.rsv_pending, o.rsv_host);
  printf("%s defer=%d, %s a byte short: rc=%d entries called=%d\n", which < 5 ? EXPORT[which] : "cycleSetReservations", defer, what, rc,
         g_calls - before);
  if (rc != COOK_E_INVALID || g_calls != before) ++g_failures;
}

int main(void) {
  int which, i;
  jint defer, rc;
  g_n_users = N_USERS;

  printf("== full cases\n");
  for (which = 0; which < 5; ++which)
    for (defer = 0; defer < 2; ++defer) {
      objects o = all_null();
      printf("%s defer=%d, every object null\n", EXPORT[which], defer);
      rc = call_export(which, &o, defer);
      printf("  rc=%d\n", rc);
      o = all_present(CUT_NONE);
      printf("%s defer=%d, every object present\n", EXPORT[which], defer);
      rc = call_export(which, &o, defer);
      printf("  rc=%d\n", rc);
    }

  printf("== finished columns: n_finished=%d n_fin_scalars=%d, one column present at a time\n", NF, NS);
  for (i = 0; i < 11; ++i) {
    const objects full = all_present(CUT_NONE);
    objects o = all_null();
    o.finished = arr(11);
    SET(o.finished, i, ((fake_arr*)full.finished)->elements[i]);
    printf("cycleRunQueueRelease, finished element %d\n", i);
    rc = call_export(2, &o, 0);
    printf("  rc=%d\n", rc);
  }
  {
    objects o = all_null(); /* an array shorter than the struct: the missing columns are absent */
    o.finished = arr(3);
    SET(o.finished, 0, buf(T_U32, NF, 7000, 0));
    SET(o.finished, 2, buf(T_F64, NF, 7200, 0));
    printf("cycleRunQueueRelease, finished array of 3 elements\n");
    rc = call_export(2, &o, 1);
    printf("  rc=%d\n", rc);
  }

  printf("== short buffers\n");
  short_case("offer_skipped", 0, CUT_SKIPPED, 0);
  short_case("the offers' scalars", 0, CUT_OFFER_COL, 1);
  short_case("tokens_left", 1, CUT_TOKENS, 0);
  short_case("the groups' run_host", 1, CUT_GROUP_RUN, 1);
  short_case("the finished scalars", 2, CUT_FIN_SCALARS, 0);
  short_case("the finished groups", 2, CUT_FIN_GROUP, 1);
  short_case("join_before", 3, CUT_JOIN_BEFORE, 0);
  short_case("leave_host", 3, CUT_LEAVE, 1);
  short_case("the join's scalars", 3, CUT_JOIN_COL, 0);
  short_case("the finished scalars", 3, CUT_FIN_SCALARS, 1);
  short_case("rsv_host", 4, CUT_RSV_HOST, 0);
  short_case("rsv_pending", 4, CUT_RSV_PENDING, 1);
  short_case("tokens_left", 4, CUT_TOKENS, 0);
  short_case("rsv_pending", 5, CUT_RSV_PENDING, 0);
  short_case("rsv_host", 5, CUT_RSV_HOST, 0);

  printf("== cycleSetReservations\n");
  {
    const objects o = all_present(CUT_NONE);
    printf("cycleSetReservations with a list\n");
    rc = Java_cook_hip_Native_cycleSetReservations(&g_env, 0, HANDLE, N_RESERVE, o.rsv_pending, o.rsv_host);
    printf("  rc=%d\n", rc);
    printf("cycleSetReservations n_reserve=0, buffers present\n");
    rc = Java_cook_hip_Native_cycleSetReservations(&g_env, 0, HANDLE, 0, o.rsv_pending, o.rsv_host);
    printf("  rc=%d\n", rc);
    printf("cycleSetReservations n_reserve=0, buffers null\n");
    rc = Java_cook_hip_Native_cycleSetReservations(&g_env, 0, HANDLE, 0, 0, 0);
    printf("  rc=%d\n", rc);
  }
  printf("== %d entries called, %d short-buffer cases not refused\n", g_calls, g_failures);
  return g_failures ? 1 : 0;
}
