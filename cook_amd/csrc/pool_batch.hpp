// pool_batch.hpp — pool batches: the flows of several pools on ONE stream, the same kernel of all of them in ONE launch.  Included by
// engine.hip inside its anonymous namespace, behind launch.hpp (BatchOp, StageTimer, prof_collect, the synchronisation counters) and
// guarded(); defines recording / batch_new_op / batch_park, which launch.hpp declares, and batch_drain_before_free, which device_buf.hpp declares.
//
// cook_cycle_run_rank_multi runs the rank part of a cycle for every pool of a GPU.  Each pool's flow is the code a single pool runs
// (rank_run, the considerable filters, the set-up of the match), on a fiber of its own: while a flow runs, KM / KL / copy_async /
// memset_async RECORD what they would enqueue, and sync() — every point at which the host needs to read something back — parks the flow.
// When every flow is parked (or finished) the scheduler issues what was recorded: operations of the same kernel that stand at the front
// of several flows become one `cook_multi` launch (multi.hpp: blockIdx.y = pool), everything else is issued as recorded, each flow's
// order kept; then ONE stream synchronisation, and the flows go on.  The flows' decisions (radix digits, tie rounds, queue lengths)
// stay per pool: a pool that needs a pass the others do not simply has a record of its own at that point.
struct PoolFlow {
  cook_engine* e = nullptr;
  ucontext_t ctx;
  char* stack = nullptr;
  std::vector<BatchOp> ops;
  size_t cur = 0;
  int state = 0;  // 0 ready to run, 1 parked at a synchronisation, 2 finished
  int rc = COOK_OK;
  std::function<void()> body;
};
struct PoolBatch {
  cook_engine* lead = nullptr;
  hipStream_t stream = nullptr;
  std::vector<PoolFlow> flows;
  ucontext_t main_ctx;
  unsigned launches = 0, grouped = 0, singles = 0, syncs = 0;  // launches made, of them for more than one pool; operations issued alone
  bool closing_sync = true;  // synchronise once more when every flow has finished, even if nothing was issued since the last synchronisation
};
static thread_local PoolBatch* tl_batch = nullptr;
static thread_local PoolFlow* tl_flow = nullptr;  // the flow running on this thread (null: none, or the scheduler itself)
static inline bool recording() { return tl_flow != nullptr; }
static BatchOp& batch_new_op() {
  tl_flow->ops.emplace_back();
  return tl_flow->ops.back();
}
static void batch_park() {  // the running flow waits until everything recorded so far has run
  PoolFlow* f = tl_flow;
  f->state = 1;
  tl_flow = nullptr;
  swapcontext(&f->ctx, &tl_batch->main_ctx);
}
static void batch_drain_before_free() {
  if (recording() && !tl_flow->ops.empty()) batch_park();
}

// issues what the flows have recorded: operations without a key as they stand, the same kernel at the front of several flows as one launch
// COOK_BATCH_TRACE=1: every operation a pool batch issues, to stderr (name x pools; "alone" = issued on its own)
static const bool g_batch_trace = std::getenv("COOK_BATCH_TRACE") != nullptr;
static unsigned batch_flush(PoolBatch& b) {  // -> operations issued
  const unsigned P = (unsigned)b.flows.size();
  const unsigned before = b.launches + b.singles;
  const BatchOp* group[COOK_MULTI_MAX * 8];
  for (;;) {
    for (auto& f : b.flows)
      while (f.cur < f.ops.size() && !f.ops[f.cur].key) {
        if (g_batch_trace) std::fprintf(stderr, "batch: %s alone\n", f.ops[f.cur].name);
        f.ops[f.cur].generic(b.lead, b.stream);
        ++f.cur;
        ++b.singles;
      }
    const void* best = nullptr;
    unsigned best_n = 0;
    for (unsigned i = 0; i < P; ++i) {
      const PoolFlow& f = b.flows[i];
      if (f.cur >= f.ops.size()) continue;
      const void* k = f.ops[f.cur].key;
      unsigned c = 0;
      for (unsigned j = 0; j < P; ++j) c += (b.flows[j].cur < b.flows[j].ops.size() && b.flows[j].ops[b.flows[j].cur].key == k) ? 1u : 0u;
      if (c > best_n) best_n = c, best = k;
    }
    if (!best) break;
    unsigned n = 0;
    const BatchOp* first = nullptr;
    for (auto& f : b.flows)
      if (f.cur < f.ops.size() && f.ops[f.cur].key == best && n < COOK_MULTI_MAX * 8) {
        group[n++] = &f.ops[f.cur];
        if (!first) first = &f.ops[f.cur];
        ++f.cur;
      }
    if (g_batch_trace) std::fprintf(stderr, "batch: %s x %u (grid %u)\n", first->name, n, first->grid);
    first->launch(b.lead, b.stream, first->name, group, n);
    ++b.launches;
    if (n > 1) ++b.grouped;
  }
  for (auto& f : b.flows) f.ops.clear(), f.cur = 0;
  return b.launches + b.singles - before;
}

static void flow_entry() {
  PoolFlow* f = tl_flow;
  cook_engine* e = f->e;
  try {
    f->body();
    e->err.clear();
    f->rc = COOK_OK;
  } catch (const cook_error& ce) {
    e->err = ce.msg;
    f->rc = ce.code;
  } catch (const std::exception& ex) {
    e->err = ex.what();
    f->rc = COOK_E_NOMEM;
  } catch (...) {
    e->err = "unknown exception";
    f->rc = COOK_E_STATE;
  }
  f->state = 2;
  tl_flow = nullptr;
  swapcontext(&f->ctx, &tl_batch->main_ctx);  // (never resumed)
}
constexpr size_t FLOW_STACK_BYTES = 2u << 20;
constexpr size_t FLOW_GUARD_BYTES = 64u << 10;  // below the stack, no access: an overflow faults instead of writing into the heap
// a thread's flow stacks: kept for its next batch, unmapped when the thread ends (an executor's or a JVM's pool thread that once led a batch)
struct FlowStacks {
  std::vector<char*> maps;  // mapping = guard + stack
  ~FlowStacks() {
    for (char* m : maps) munmap(m, FLOW_GUARD_BYTES + FLOW_STACK_BYTES);
  }
  char* stack(size_t i) { return maps[i] + FLOW_GUARD_BYTES; }
};
static thread_local FlowStacks tl_flow_stacks;
// runs the flows to completion; returns the first flow's error code that is not COOK_OK (every engine keeps its own message)
static int batch_run(PoolBatch& b) {
  const unsigned P = (unsigned)b.flows.size();
  while (tl_flow_stacks.maps.size() < P) {
    void* m = mmap(nullptr, FLOW_GUARD_BYTES + FLOW_STACK_BYTES, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_STACK, -1, 0);
    if (m == MAP_FAILED) throw cook_error(COOK_E_NOMEM, "pool batch: no memory for a flow's stack");
    (void)mprotect(m, FLOW_GUARD_BYTES, PROT_NONE);
    tl_flow_stacks.maps.push_back((char*)m);
  }
  for (unsigned i = 0; i < P; ++i) {
    PoolFlow& f = b.flows[i];
    f.stack = tl_flow_stacks.stack(i);
    f.state = 0;
    getcontext(&f.ctx);
    f.ctx.uc_stack.ss_sp = f.stack;
    f.ctx.uc_stack.ss_size = FLOW_STACK_BYTES;
    f.ctx.uc_link = nullptr;
    makecontext(&f.ctx, flow_entry, 0);
  }
  struct Reset {
    ~Reset() { tl_batch = nullptr, tl_flow = nullptr; }
  } reset;
  tl_batch = &b;
  // an error on the scheduler's own side (a flush, the synchronisation): the parked flows are never resumed — every engine of the batch is left
  // failed, with the clean-up guarded() gives an engine whose own call threw
  auto abandon = [&](int code, const std::string& msg) {
    for (auto& f : b.flows) {
      if (f.state == 2 && f.rc != COOK_OK) continue;  // (keeps its own message)
      f.rc = code;
      f.e->err = msg;
      f.e->ev_pending.clear();
      f.e->ev_used = 0;
    }
  };
  try {
  for (;;) {
    for (auto& f : b.flows)
      if (f.state == 0) {
        tl_flow = &f;
        swapcontext(&b.main_ctx, &f.ctx);
        tl_flow = nullptr;
      }
    const unsigned issued = batch_flush(b);
    bool parked = false;
    for (auto& f : b.flows) parked = parked || f.state == 1;
    if (!parked && !issued && !b.closing_sync) break;  // every flow ended at its last synchronisation: the stream is idle
    const auto t0 = std::chrono::steady_clock::now();
    if (g_batch_trace) std::fprintf(stderr, "batch: synchronise\n");
    COOK_HIP(hipStreamSynchronize(b.stream));
    tl_sync_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ++tl_syncs;
    ++b.syncs;
    if (!parked) break;
    for (auto& f : b.flows)
      if (f.state == 1) f.state = 0;
  }
  } catch (const cook_error& ce) {
    abandon(ce.code, ce.msg);
    throw;
  } catch (const std::exception& ex) {
    abandon(COOK_E_NOMEM, ex.what());
    throw;
  }
  for (auto& f : b.flows)
    if (f.rc != COOK_OK) return f.rc;
  return COOK_OK;
}

// the rank part of a cycle for every pool of a GPU: one flow per pool in a pool batch
static const bool g_rank_batch = env_switch_on_unless_zero("COOK_RANK_BATCH");
// The pools of a GPU through one call: `one(i)` is the call for engine i alone (the fall-back: one engine, COOK_RANK_BATCH=0, engines of
// several devices, COOK_SYNC_TRACE, a call from inside a flow), `body(i)` what engine i's flow does inside the pool batch.  Returns the
// first engine's error that is not COOK_OK; every engine whose flow failed keeps its own message.  rank_part: the batch is the rank part of a
// cycle — timed as the rank stage of every engine, counted in the lead's batch statistics, its kernel timings collected.
// rc_out (optional, [n]): every engine's own code.
template <class One, class Body>
int run_pools_batched(cook_engine** engines, uint32_t n, One&& one, Body&& body, bool rank_part, int* rc_out = nullptr) {
  if (!engines_valid(engines, n, false)) return COOK_E_INVALID;
  cook_engine* lead = engines[0];
  bool same_device = true;
  for (uint32_t i = 1; i < n; ++i) same_device = same_device && engines[i]->device == lead->device;
  if (n == 1 || !g_rank_batch || !same_device || g_sync_trace || tl_flow) {
    int first = COOK_OK;
    for (uint32_t i = 0; i < n; ++i) {
      const int rc = one(i);
      if (rc_out) rc_out[i] = rc;
      if (rc != COOK_OK && first == COOK_OK) first = rc;
    }
    return first;
  }
  int flows_rc = COOK_OK;
  std::vector<std::pair<int, std::string>> flow_err(n, {COOK_OK, std::string()});  // (guarded() clears the lead's message on its way out)
  const int rc = guarded(lead, [&] {
    for (uint32_t i = 0; i < n; ++i) COOK_HIP(hipStreamSynchronize(engines[i]->stream));  // (whatever a call before this one left running)
    PoolBatch b;
    b.lead = lead;
    b.stream = lead->stream;
    b.closing_sync = rank_part;
    b.flows.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
      b.flows[i].e = engines[i];
      b.flows[i].body = [&body, i] { body(i); };
    }
    std::optional<StageTimer> tr;
    if (rank_part) tr.emplace(lead, 0, &lead->rank_ms);
    flows_rc = batch_run(b);
    for (uint32_t i = 0; i < n; ++i)
      if (b.flows[i].rc != COOK_OK) flow_err[i] = {b.flows[i].rc, engines[i]->err};
    lead->any_batch_stats[0] = n, lead->any_batch_stats[1] = b.launches, lead->any_batch_stats[2] = b.grouped,
    lead->any_batch_stats[3] = b.singles, lead->any_batch_stats[4] = b.syncs;
    if (!rank_part) {
      prof_collect(lead);
      return;
    }
    tr->stop();
    for (uint32_t i = 1; i < n; ++i) engines[i]->rank_ms = lead->rank_ms;  // one joint sequence of launches
    lead->batch_stats[0] = n, lead->batch_stats[1] = b.launches, lead->batch_stats[2] = b.grouped, lead->batch_stats[3] = b.singles,
    lead->batch_stats[4] = b.syncs;
    prof_collect(lead);
  });
  for (uint32_t i = 0; i < n; ++i)
    if (flow_err[i].first != COOK_OK) engines[i]->err = flow_err[i].second;  // every engine whose flow failed keeps its own message
  if (rc_out)
    for (uint32_t i = 0; i < n; ++i) rc_out[i] = rc != COOK_OK ? rc : flow_err[i].first;  // (the scheduler's own error: every engine of the batch failed)
  return rc != COOK_OK ? rc : flows_rc;
}
