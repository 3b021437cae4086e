// device_buf.hpp — the engine's grow-only device buffers (DBuf, DArr, ScanTmp) and their COOK_GUARD bands.  Included by engine.hip inside
// its anonymous namespace, ahead of struct cook_engine (whose members they are); expects <hip/hip_runtime.h>, common.hpp (COOK_HIP) and
// scan.hpp (SegAgg).  batch_drain_before_free is only declared here: pool_batch.hpp defines it.
// COOK_GUARD=1 (diagnostics; scripts/fuzz_sweep.py runs under it): every buffer is allocated at exactly the size asked for between two
// 4 KB bands of a pattern, and the bands are looked at when the buffer is freed or grown — a kernel that writes before or past a buffer
// is named on stderr ("COOK_GUARD") even when the write lands in mapped memory and faults nothing.
static const bool g_guard = [] {
  const char* s = std::getenv("COOK_GUARD");
  return s && std::atoi(s) != 0;
}();
static std::atomic<unsigned> g_guard_hits{0};
static thread_local unsigned tl_dbuf_allocs = 0;  // device allocations made by this thread (cook_match_stats_ex [28]: a call that grows a buffer pays hipFree + hipMalloc)
constexpr size_t GUARD_BYTES = 4096;
// a pool batch (pool_batch.hpp) holds launches back until its pools meet at a synchronisation: a buffer must not be freed under them
static void batch_drain_before_free();
// the guarded buffers alive in this process (COOK_GUARD=1 only): what cook_match_stats_ex looks at, with no list kept by hand
struct DBuf;
static std::mutex g_guard_mu;
static std::vector<DBuf*> g_guard_live;
struct DBuf {
  void* p = nullptr;
  size_t cap = 0;
  void check_guard() {
    if (!g_guard || !p) return;
    std::vector<unsigned char> h(2 * GUARD_BYTES);
    if (hipMemcpy(h.data(), (char*)p - GUARD_BYTES, GUARD_BYTES, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(h.data() + GUARD_BYTES, (char*)p + cap, GUARD_BYTES, hipMemcpyDeviceToHost) != hipSuccess)
      return;
    for (size_t x = 0; x < 2 * GUARD_BYTES; ++x)
      if (h[x] != 0xA5) {
        std::fprintf(stderr, "COOK_GUARD: a buffer of %zu bytes was written %s (guard byte %zu)\n", cap, x < GUARD_BYTES ? "BEFORE its start" : "PAST its end",
                     x < GUARD_BYTES ? x : x - GUARD_BYTES);
        g_guard_hits.fetch_add(1);
        (void)hipMemset((char*)p - GUARD_BYTES, 0xA5, GUARD_BYTES);  // re-armed: one report per overrun, not one per look
        (void)hipMemset((char*)p + cap, 0xA5, GUARD_BYTES);
        break;
      }
  }
  void free_now() {
    if (!p) return;
    batch_drain_before_free();
    if (g_guard) {
      std::lock_guard<std::mutex> l(g_guard_mu);
      g_guard_live.erase(std::find(g_guard_live.begin(), g_guard_live.end(), this));
    }
    check_guard();
    (void)hipFree(g_guard ? (void*)((char*)p - GUARD_BYTES) : p);
    p = nullptr;
    cap = 0;
  }
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    ++tl_dbuf_allocs;
    free_now();
    if (g_guard) {
      const size_t want = (bytes + 15) & ~(size_t)15;
      void* base = nullptr;
      COOK_HIP(hipMalloc(&base, want + 2 * GUARD_BYTES));
      COOK_HIP(hipMemset(base, 0xA5, GUARD_BYTES));
      COOK_HIP(hipMemset((char*)base + GUARD_BYTES + want, 0xA5, GUARD_BYTES));
      p = (char*)base + GUARD_BYTES;
      cap = want;
      std::lock_guard<std::mutex> l(g_guard_mu);
      g_guard_live.push_back(this);
      return;
    }
    size_t want = bytes + bytes / 4 + 256;
    COOK_HIP(hipMalloc(&p, want));
    cap = want;
  }
  void release() { free_now(); }
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() { release(); }
};
static void guard_check_live() {  // (blocking copies on the null stream: the caller has synchronised what may still write)
  std::lock_guard<std::mutex> l(g_guard_mu);
  for (DBuf* b : g_guard_live) b->check_guard();
}
template <class T>
struct DArr {
  DBuf b;
  T* ptr() { return (T*)b.p; }
  const T* ptr() const { return (const T*)b.p; }
  T* ensure(size_t n) {
    b.ensure((n ? n : 1) * sizeof(T));
    return ptr();
  }
  void release() { b.release(); }
};

template <class T>
struct ScanTmp {
  DArr<SegAgg<T>> agg, carry;
  DArr<unsigned> first_head;
};
