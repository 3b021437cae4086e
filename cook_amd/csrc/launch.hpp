// launch.hpp — what every host flow is written in: kernel launches (KM, KL, KLS) with optional per-kernel HIP-event timing, copies and
// fills on the engine's stream, stream synchronisation, small read-backs, the stage timer.  Included by engine.hip inside its anonymous
// namespace, behind struct cook_engine; expects multi.hpp (ArgPack, MultiArgs, cook_multi).  Inside a pool batch these calls record
// instead of enqueueing: the record of one operation (BatchOp) is defined here, the batch itself in pool_batch.hpp, which also defines the
// three functions that are only declared here.

// ---- per-kernel HIP-event timing ----------------------------------------------------------------------------------
hipEvent_t take_event(cook_engine* e) {
  if (e->ev_used == e->ev_pool.size()) {
    hipEvent_t ev;
    COOK_HIP(hipEventCreate(&ev));
    e->ev_pool.push_back(ev);
  }
  return e->ev_pool[e->ev_used++];
}
struct ProfScope {
  cook_engine* e;
  hipEvent_t a = nullptr, b = nullptr;
  const char* name;
  hipStream_t stream;
  ProfScope(cook_engine* e_, const char* n, hipStream_t s = nullptr) : e(e_), name(n), stream(s ? s : e_->stream) {
    if (e->profiling) {
      a = take_event(e);
      b = take_event(e);
      (void)hipEventRecord(a, stream);
    }
  }
  ~ProfScope() {
    if (e->profiling) {
      (void)hipEventRecord(b, stream);
      e->ev_pending.push_back({name, a, b});
    }
  }
};
void prof_collect(cook_engine* e) {
  if (!e->profiling) return;
  for (auto& p : e->ev_pending) {
    float ms = 0;
    if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      auto& s = e->kstats[p.name];
      s.ms += ms;
      s.launches += 1;
    }
  }
  e->ev_pending.clear();
  e->ev_used = 0;
}

// ---- launches, copies, synchronisation: enqueued on the engine's stream, or recorded inside a pool batch ---------------------------
constexpr unsigned BATCH_ARG_BYTES = 496;
struct BatchOp {
  const void* key = nullptr;  // the group launcher of (kernel, block size); null: an operation issued on its own
  void (*launch)(cook_engine* lead, hipStream_t s, const char* name, const BatchOp* const* ops, unsigned n) = nullptr;
  const char* name = "";
  unsigned grid = 0;
  alignas(16) unsigned char args[BATCH_ARG_BYTES];
  std::function<void(cook_engine*, hipStream_t)> generic;
};
static inline bool recording();  // this thread is running a pool's flow inside a pool batch (pool_batch.hpp)
static BatchOp& batch_new_op();  // a fresh record at the end of the running flow
static void batch_park();        // the running flow waits until everything recorded so far has run

template <class Fp>
struct KernelSig;
template <class... A>
struct KernelSig<void (*)(A...)> {
  using Pack = ArgPack<A...>;
  using Args = MultiArgs<A...>;
  template <auto F, int B>
  static void launch_group(cook_engine* lead, hipStream_t s, const char* name, const BatchOp* const* ops, unsigned n) {
    for (unsigned i0 = 0; i0 < n; i0 += Args::PER) {
      const unsigned c = std::min<unsigned>(Args::PER, n - i0);
      Args m{};
      unsigned gmax = 0;
      for (unsigned i = 0; i < c; ++i) {
        m.grid[i] = ops[i0 + i]->grid;
        std::memcpy(&m.a[i], ops[i0 + i]->args, sizeof(Pack));
        gmax = std::max(gmax, m.grid[i]);
      }
      ProfScope _ps(lead, name, s);
      hipLaunchKernelGGL((cook_multi<F, B, A...>), dim3(gmax, c), dim3(B), 0, s, m);
    }
  }
};
// launch of a COOK_KERNEL (a 1-D grid of `grid` blocks of B threads) on the engine's stream — or its record, inside a pool batch
template <auto F, int B, class... X>
void KM(cook_engine* e, const char* name, unsigned grid, const X&... x) {
  using Sig = KernelSig<decltype(F)>;
  static_assert(sizeof(typename Sig::Pack) <= BATCH_ARG_BYTES, "a batched kernel's arguments: pass large structures by pointer");
  if (grid == 0) return;
  const typename Sig::Pack p = Sig::Pack::make(x...);
  BatchOp local;
  BatchOp& op = recording() ? batch_new_op() : local;
  op.key = (const void*)&Sig::template launch_group<F, B>;
  op.launch = &Sig::template launch_group<F, B>;
  op.name = name;
  op.grid = grid;
  std::memcpy(op.args, &p, sizeof(p));
  if (recording()) return;
  const BatchOp* one[1] = {&op};
  op.launch(e, e->stream, name, one, 1);
}

// a __global__ kernel of its own (arguments evaluated here and now; inside a pool batch the launch is recorded and issued alone)
#define KL(name_, kern, grid, block, ...)                                                                     \
  do {                                                                                                       \
    if (recording()) {                                                                                       \
      const auto _a = std::make_tuple(__VA_ARGS__);                                                          \
      const dim3 _g(grid), _b(block);                                                                        \
      const char* _n = name_;                                                                                 \
      BatchOp& _op = batch_new_op();                                                                         \
      _op.name = _n;                                                                                         \
      _op.generic = [=](cook_engine* lead_, hipStream_t s_) {                                                \
        ProfScope _ps(lead_, _n, s_);                                                                        \
        std::apply([&](const auto&... x_) { hipLaunchKernelGGL(kern, _g, _b, 0, s_, x_...); }, _a);          \
      };                                                                                                     \
    } else {                                                                                                 \
      ProfScope _ps(e, name_);                                                                               \
      hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, e->stream, __VA_ARGS__);                          \
    }                                                                                                        \
  } while (0)

// the same on a given stream (timed, when profiling, with events on THAT stream); never part of a pool batch
#define KLS(name, stream_, kern, grid, block, ...)                               \
  do {                                                                        \
    ProfScope _ps(e, name, stream_);                                          \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, stream_, __VA_ARGS__); \
  } while (0)

// copies and fills on the engine's stream (recorded inside a pool batch: a source in host memory must stay as it is until the flow's
// next synchronisation, which is what an asynchronous copy asks for anyway)
void copy_async(cook_engine* e, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (!bytes) return;
  if (recording()) {
    BatchOp& op = batch_new_op();
    op.name = "copy";
    op.generic = [=](cook_engine*, hipStream_t s_) { COOK_HIP(hipMemcpyAsync(dst, src, bytes, kind, s_)); };
    return;
  }
  COOK_HIP(hipMemcpyAsync(dst, src, bytes, kind, e->stream));
}
void memset_async(cook_engine* e, void* dst, int value, size_t bytes) {
  if (!bytes) return;
  if (recording()) {
    BatchOp& op = batch_new_op();
    op.name = "fill";
    op.generic = [=](cook_engine*, hipStream_t s_) { COOK_HIP(hipMemsetAsync(dst, value, bytes, s_)); };
    return;
  }
  COOK_HIP(hipMemsetAsync(dst, value, bytes, e->stream));
}

// a few words between device memory and PAGE-LOCKED host memory (read-backs of counters into h_scratch, a control block on its way in).
// Inside a pool batch they are moved by a kernel — the device reads and writes page-locked host memory over the link — so that the eight
// copies of eight pools are one launch and not eight calls of the runtime (COOK_BATCH_COPY_KERNEL=0: recorded copies, issued one by one)
COOK_KERNEL void copy_words_k(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, unsigned nwords) {
  for (unsigned i = threadIdx.x; i < nwords; i += blockDim.x) dst[i] = src[i];
}
// (a plain function: hipcc gave a second namespace-scope lambda initialiser in this anonymous namespace the body of the first — COOK_GUARD's —,
//  found in the disassembly of the library's static initialisers after the switch had read as "off" on the GPU box)
static bool env_switch_on_unless_zero(const char* name) {
  const char* s = std::getenv(name);
  return !(s && std::atoi(s) == 0);
}
static const bool g_batch_copy_kernel = env_switch_on_unless_zero("COOK_BATCH_COPY_KERNEL");
void pinned_copy(cook_engine* e, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (recording() && g_batch_copy_kernel && bytes % 4 == 0 && bytes <= 4096 && ((uintptr_t)dst | (uintptr_t)src) % 4 == 0) {
    KM<copy_words_k, COOK_WAVE>(e, "copy_words", 1, (uint32_t*)dst, (const uint32_t*)src, (unsigned)(bytes / 4));
    return;
  }
  copy_async(e, dst, src, bytes, kind);
}

template <class T>
void h2d(cook_engine* e, DArr<T>& d, const T* h, size_t n) {
  d.ensure(n);
  copy_async(e, d.ptr(), h, n * sizeof(T), hipMemcpyHostToDevice);
}
template <class T>
const T* h2d_opt(cook_engine* e, DArr<T>& d, const T* h, size_t n) {
  if (!h) return nullptr;
  h2d(e, d, h, n);
  return d.ptr();
}

// COOK_SYNC_TRACE=1: what the stream synchronisations of a call cost the host (stderr, per cook_rank_run)
static const bool g_sync_trace = std::getenv("COOK_SYNC_TRACE") != nullptr;
static thread_local double tl_sync_ms = 0.0;
static thread_local unsigned tl_syncs = 0;
void sync(cook_engine* e) {  // (always timed: two clock reads against a stream synchronisation)
  if (recording()) {  // inside a pool batch: the flow goes on once every pool's flow has come to such a point and the stream has drained
    batch_park();
    return;
  }
  const auto t0 = std::chrono::steady_clock::now();
  COOK_HIP(hipStreamSynchronize(e->stream));
  tl_sync_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  ++tl_syncs;
}

// read back `words` 64-bit words from d_scratch64 (synchronises the stream)
void readback64(cook_engine* e, unsigned words) {
  pinned_copy(e, e->h_scratch, e->d_scratch64.ptr(), words * 8, hipMemcpyDeviceToHost);
  sync(e);
}
void readback_counters(cook_engine* e, unsigned* out, unsigned words) {
  pinned_copy(e, e->h_scratch, e->d_counters.ptr(), words * 4, hipMemcpyDeviceToHost);
  sync(e);
  std::memcpy(out, e->h_scratch, words * 4);
}

// the device's time between here and stop(), in milliseconds, by two of the engine's four stage events (slot 0: rank, 2: match)
struct StageTimer {
  cook_engine* e;
  int slot;
  double* out;
  StageTimer(cook_engine* e_, int s, double* o) : e(e_), slot(s), out(o) { (void)hipEventRecord(e->ev_stage[slot], e->stream); }
  void stop() {
    (void)hipEventRecord(e->ev_stage[slot + 1], e->stream);
    (void)hipEventSynchronize(e->ev_stage[slot + 1]);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e->ev_stage[slot], e->ev_stage[slot + 1]);
    *out = ms;
  }
};
