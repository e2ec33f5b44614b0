// Host side of libbgls_hip.so, part 1 of 4 (included by engine.hip, one translation unit): error reporting and the exception barrier,
// contexts and workspaces, the run-time switches, and Engine<C> -- the stages of a verification (duplicate scan, hashing, Miller
// product, reduce, final exponentiation, key sums) as launches on a context's stream.
// ======================================================================= host side
namespace {

thread_local std::string g_err;

int fail(int code, const char* what, hipError_t e = hipSuccess) noexcept {
  char buf[256];
  if (e != hipSuccess)
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(buf, sizeof buf, "%s", what);
  try { g_err = buf; } catch (...) {}      // the message is best effort, the code is the contract
  return code;
}
// the two refusals that many calls share
int too_large() noexcept { return fail(BGLS_ERR_ARG, "batch too large (n must be below 2^30)"); }
int in_flight() noexcept { return fail(BGLS_ERR_ARG, "a verification is already in flight on this context (collect it first)"); }

// The exception barrier of the C ABI ("no exceptions, no abort()": include/bgls_hip.h; the reference never panics and returns
// (nil, false): curves/curve.go:15-22).  Every extern "C" body below is a function-try-block ending in BGLS_ABI_GUARD: host
// containers sized by the caller (std::vector), std::string, std::thread and std::shared_ptr can throw, and an exception must
// not unwind into a cgo / ctypes frame.
int abi_catch() noexcept {
  try {
    throw;
  } catch (const std::bad_alloc&) {
    return fail(BGLS_ERR_NOMEM, "out of host memory");
  } catch (const std::length_error&) {
    return fail(BGLS_ERR_NOMEM, "host container size limit");
  } catch (const std::system_error& e) {
    return fail(BGLS_ERR_HIP, e.what());
  } catch (const std::exception& e) {
    return fail(BGLS_ERR_ARG, e.what());
  } catch (...) {
    return fail(BGLS_ERR_ARG, "unknown C++ exception");
  }
}
#define BGLS_ABI_GUARD catch (...) { return abi_catch(); }

// Error-path guard of a fork onto a context's side stream: kernels launched there read and write the context's workspaces, so
// an early return between the fork and the join must not leave them running into the next call on the same context.  Armed at
// the fork, disarmed once the main stream waits on the join event; an error return in between drains the side stream.
struct SideJoin {
  hipStream_t side;
  bool armed = false;
  ~SideJoin() {
    if (armed) (void)hipStreamSynchronize(side);
  }
};
// Error-path guard of a call that returns results to host memory: an error return between the first launch and the call's own
// synchronise leaves launches, and copies out of host staging vectors (Ctx::stage_tab), in flight.  Armed from the start, disarmed after
// that synchronise; an error return in between drains the stream.
struct Drain {
  hipStream_t st;
  bool armed = true;
  ~Drain() {
    if (armed) (void)hipStreamSynchronize(st);
  }
};

#define HIPCHK(expr)                                         \
  do {                                                       \
    hipError_t e_ = (expr);                                  \
    if (e_ != hipSuccess) return fail(BGLS_ERR_HIP, #expr, e_); \
  } while (0)

// Largest batch one call accepts: the duplicate table (2n rounded up to a power of two, u32 slots), the hashing work
// lists (u32 indices) and the grid computations all assume n < 2^30.
constexpr size_t MAX_BATCH = (size_t)1 << 30;
// keys per set of the batched HAE calls: the XOF length 16 n is a uint32 (blsHAE.go:81)
constexpr size_t HAE_MAX_SET = (size_t)1 << 28;
// batches up to this many pairings take the latency form of the Miller loop (one block per pairing, k_miller_lat)
constexpr size_t LAT_MAX = 128;

// The rules of a table of count + 1 host offsets, stated once (`name` is the table's name in the messages): from 0 where OFF_FROM_ZERO
// asks for it, monotone, no segment above max_seg, under OFF_HAE no segment of 2^28 entries or more, under OFF_TOTAL fewer than 2^30
// entries in all.  *largest (nullable): the largest segment.
enum { OFF_FROM_ZERO = 1, OFF_HAE = 2, OFF_TOTAL = 4 };
int offsets_ok(const char* name, const uint64_t* off, size_t count, unsigned rules, size_t max_seg = SIZE_MAX, size_t* largest = nullptr) {
  auto named = [name](const char* what) {
    char msg[64];
    snprintf(msg, sizeof msg, "%s %s", name, what);
    return fail(BGLS_ERR_ARG, msg);
  };
  size_t top = 0;
  if ((rules & OFF_FROM_ZERO) && off[0] != 0) return named("must start at 0");
  for (size_t b = 0; b < count; ++b) {
    if (off[b + 1] < off[b]) return named("not monotone");
    const size_t seg = off[b + 1] - off[b];
    if (seg > max_seg) return fail(BGLS_ERR_ARG, "a set is larger than max_set");
    if ((rules & OFF_HAE) && seg >= HAE_MAX_SET) return fail(BGLS_ERR_ARG, "XOF length 16 n must fit a uint32 (blsHAE.go:81)");
    if (seg > top) top = seg;
  }
  if ((rules & OFF_TOTAL) && count && off[count] - off[0] >= MAX_BATCH) return too_large();
  if (largest) *largest = top;
  return 0;
}

// workspace slots
enum { WS_G1S = 0, WS_F_A, WS_F_B, WS_FLAGS, WS_TABLE, WS_IN_A, WS_IN_B, WS_IN_C, WS_IN_D, WS_OUT, WS_JAC_A, WS_JAC_B, WS_PART, WS_TMP, WS_TMP2, WS_H2C_LIST, WS_H2C_CNT, WS_H2C_PTS, WS_H2C_KIND, WS_HAE_ROOT, WS_HAE_T, WS_HAE_KEYS, WS_HAE_APK, WS_HAE_SIGN, WS_FLAGS2, WS_GEN_TMP, WS_LINES, WS_SUMJ, WS_QP, WS_MSM_AFF, WS_MSM_CNT, WS_MSM_START, WS_MSM_LIST, WS_SEG_OFF, WS_SEG_KEYS, WS_EPI, WS_TREE_S, WS_TREE_T,
       WS_BATCH_IDX, WS_BATCH_G1, WS_BATCH_KEYS, WS_BATCH_SIGS, WS_BATCH_EPI, WS_BATCH_RES, WS_HAE_NODES, WS_AMS_SIGNERS, WS_AMS_OFF, WS_AMS_BLOB, WS_AMS_PTS,
       WS_AMS_SUMS, WS_AMS_AGG, WS_RLC_SIGS, WS_RLC_SUMS, WS_RLC_OFF, WS_KEYED_BLOB, WS_KEYED_OFF, WS_NUM };

struct Ctx {
  std::mutex mu;
  int device = 0;
  bool ready = false;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;                // a lone verification's independent stages run beside each other (fork / join with the two events)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  std::vector<std::pair<void*, size_t>> ws;  // cached device workspaces by slot
  uint32_t* h_res = nullptr;                 // pinned host words {verdict, final-stage flags, caller flags} of the verification in flight
  bool res_pending = false;
  hipStream_t res_stream = nullptr;
  // optional per-stage timing with HIP events on the launch stream (bench.py roofline leg)
  bool prof = false;
  struct Pending { hipEvent_t a, b; int stage; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> ev_pool;
  double stage_ms[16] = {0};
  unsigned long long stage_cnt[16] = {0};
  std::vector<uint64_t> stage_tab;           // host tables of a batch verification (offsets, reduce passes) on their way to WS_BATCH_IDX
  uint32_t msm_last[6] = {0};                // what the last weighted sum did: path, c, S, W, largest bucket, listed pairs (bgls_selftest_msm_last)
  hipEvent_t ev() {
    if (!ev_pool.empty()) { hipEvent_t e = ev_pool.back(); ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  void collect() {
    for (auto& p : pending) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { stage_ms[p.stage] += ms; stage_cnt[p.stage] += 1; }
      ev_pool.push_back(p.a);
      ev_pool.push_back(p.b);
    }
    pending.clear();
  }

  // makes this context's device current for the calling thread and creates the stream on first use
  int enter() {
    if (!ready) {
      int cnt = 0;
      hipError_t e = hipGetDeviceCount(&cnt);
      if (e != hipSuccess || cnt <= 0) return fail(BGLS_ERR_NO_DEVICE, "no HIP device available", e);
      if (device < 0 || device >= cnt) return fail(BGLS_ERR_NO_DEVICE, "device index out of range");
    }
    HIPCHK(hipSetDevice(device));
    if (ready) return 0;
    HIPCHK(hipStreamCreate(&stream));
    HIPCHK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    HIPCHK(hipHostMalloc((void**)&h_res, 64));
    ws.assign(WS_NUM + 8, {nullptr, 0});
    ready = true;
    return 0;
  }
  int get(int slot, size_t bytes, void** out) {
    if (bytes == 0) bytes = 16;
    if (ws[slot].second < bytes) {
      if (ws[slot].first) HIPCHK(hipFree(ws[slot].first));
      ws[slot] = {nullptr, 0};
      size_t cap = bytes + bytes / 4;
      HIPCHK(hipMalloc(&ws[slot].first, cap));
      ws[slot].second = cap;
    }
    *out = ws[slot].first;
    return 0;
  }
  // slot sized for bytes (+ spare), filled with `bytes` of host memory by a copy on st (no copy of nothing)
  int put(hipStream_t st, int slot, const void* src, size_t bytes, void** out, size_t spare = 0) {
    int rc;
    if ((rc = get(slot, bytes + spare, out))) return rc;
    if (bytes) HIPCHK(hipMemcpyAsync(*out, src, bytes, hipMemcpyHostToDevice, st));
    return 0;
  }
};

// Contexts: each owns a stream, its workspaces and its stage timers.  A host thread works on context (device, index) =
// (bgls_init's device or bgls_select_device's, bgls_select_context's index, default 0): several contexts of one device
// let one thread keep several verifications in flight, so the serial, latency-bound stages of one (hashing rounds,
// reduction tail, final exponentiation) overlap the Miller launch of another; contexts of different devices are what
// the multi-GPU entry points drive from their worker threads.
constexpr int NCTX = 16;
constexpr int MAX_DEVICES = 16;
std::atomic<int> g_default_device{0};
thread_local int g_sel = 0;
thread_local int g_dev = -1;           // -1: the process default
// The calling thread's device / context selection, put back on EVERY way out of a scope that rebinds it to a key set's device
// (advice r5: trailing assignments were skipped by a caught std::bad_alloc, and the thread stayed bound to the key set's root device).
struct SelectionGuard {
  const int dev, sel;
  SelectionGuard() : dev(g_dev), sel(g_sel) {}
  ~SelectionGuard() { g_dev = dev; g_sel = sel; }
  SelectionGuard(const SelectionGuard&) = delete;
  SelectionGuard& operator=(const SelectionGuard&) = delete;
};
Ctx* ctx_pool() {
  static Ctx c[MAX_DEVICES][NCTX];
  static std::once_flag once;
  std::call_once(once, [] {
    for (int d = 0; d < MAX_DEVICES; ++d)
      for (int k = 0; k < NCTX; ++k) c[d][k].device = d;
  });
  return &c[0][0];
}
int cur_device() { return g_dev >= 0 ? g_dev : g_default_device.load(); }
Ctx& ctx_of(int device, int index) { return ctx_pool()[(size_t)device * NCTX + index]; }
Ctx& ctx() { return ctx_of(cur_device(), g_sel); }

// The opening of a call body: the calling thread's context with its lock held for the body, the device made current, and the stream
// the call works on -- the caller's where it gave one, else the context's.  rc != 0: Ctx::enter's code, to be returned before anything else.
struct Call {
  Ctx& c;
  std::lock_guard<std::mutex> lk;
  const int rc;
  const hipStream_t st;
  explicit Call(void* stream = nullptr) : c(ctx()), lk(c.mu), rc(c.enter()), st(stream ? (hipStream_t)stream : c.stream) {}
};

// Per-device tables built once: the fixed-argument line coefficients of the generator g2 (k_gen_lines), one per curve,
// and the window multiples d 2^(8j) g of both generators for batch key generation (k_fb_build).
// Built under the device's lock on a private stream and published only after the build has completed, so every stream
// of every context of that device may read them without further ordering.
struct DeviceTables {
  std::mutex mu;
  void* gen_lines[2] = {nullptr, nullptr};
  void* fixed_base[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};      // [curve][group - 1]: window multiples of the generator (k_fb_build)
};
DeviceTables& tables_of(int device) {
  static DeviceTables t[MAX_DEVICES];
  return t[device];
}

// Throughput mode (bgls_set_throughput_mode / BGLS_THROUGHPUT=1): the caller keeps several verifications in flight, so a
// verification neither forks onto the side stream nor takes the block form / priorities meant for a lone launch.
std::atomic<int> g_throughput{-1};
bool throughput_mode() {
  int v = g_throughput.load();
  if (v < 0) {
    const char* e = getenv("BGLS_THROUGHPUT");
    v = (e && e[0] == '1') ? 1 : 0;
    g_throughput.store(v);
  }
  return v == 1;
}
// bgls_set_throughput_mode(2): one stream per verification as in throughput mode, but the grids of a verification that has the machine to itself
// -- what a stage-by-stage timing of ONE verification wants (bench.py's exclusive stage times)
bool side_fork_allowed() {
  (void)throughput_mode();
  return g_throughput.load() == 0;
}

// Miller shape (bgls_set_miller_shape / BGLS_MILLER_SHAPE): 0 = automatic -- k_miller_latx up to 128 pairings, k_miller_x60 (carry-free
// limbs, both curves) above; 4 = k_miller_x60 for every batch size (the second argument is then its role / priority / block-form
// mode word); 5 = the 32-bit fused kernel k_miller_ab64 for every batch size (the legacy-path matrix of the tests).
// items per Engine::sum_sets pass of the batched accountable-subgroup check (bgls_set_ams_sum_cut; tests lower it to reach a second pass)
std::atomic<size_t> g_ams_sum_cut{(size_t)1 << 16};
std::atomic<int> g_shape{-1}, g_x60_rot{-1};      // x60 mode -1: automatic (see Engine::miller)
int miller_shape() {
  // the environment preset is read exactly once (thread-safe static initialiser), before any setter's value can be overwritten
  static const bool env_once = [] {
    const char* e = getenv("BGLS_MILLER_SHAPE");
    int v = e ? atoi(e) : 0;
#ifdef BGLS_LEGACY_KERNELS
    if (v != 4 && v != 5) v = 0;
#else
    if (v != 4) v = 0;                    // shape 5 (k_miller_ab64) exists in LEGACY=1 builds only
#endif
    int expect = -1;
    g_shape.compare_exchange_strong(expect, v);
    return true;
  }();
  (void)env_once;
  const int v = g_shape.load();
  return v < 0 ? 0 : v;
}

// BGLS_LEGACY=<bit mask>, read once per process: the ONE 32-bit-limb fallback kept per stage, for A/B measurements and the
// legacy-path matrix of the tests (tests/test_gpu_legacy_paths.py).  Since round 6 the kernels that ONLY these switches reach --
// k_final36, k_miller_lat, k_cofactor_epilogue, the G2 forms of k_sum_main, and k_miller_ab64 behind BGLS_MILLER_SHAPE=5 -- are compiled
// only by `make LEGACY=1` (-DBGLS_LEGACY_KERNELS, bgls_amd/libbgls_hip_legacy.so: what those tests load); in the shipped library the
// bits that select them and shape 5 are ignored.  Bits 16, 32 and 64 choose between kernels that every build has.
//    1  final exponentiation on k_final36 (finalexp.hpp) instead of k_finalx                                   [LEGACY=1 builds]
//    2  latency Miller loop on k_miller_lat instead of k_miller_latx                                           [LEGACY=1 builds]
//    4  epilogue on k_cofactor_epilogue instead of k_epilogue_ax / _bx (and no early signature pair)           [LEGACY=1 builds]
//    8  G2 key sums on k_sum_main (32-bit limbs, one lane per partial) instead of the lane-pair kernel         [LEGACY=1 builds]
//   16  the key-sum tree as one launch per level (k_sum_coop) instead of the ticket-climbing k_sum_tree_x
//   32  BLS12-381 G1 scalar multiplications on the 32-bit kernels instead of k_g1x.hip
//   64  every reduce pass on k_reduce_coop (none on k_reduce_fx)
enum { LG_FINAL = 1, LG_LAT = 2, LG_EPI = 4, LG_SUM = 8, LG_TREE = 16, LG_G1 = 32, LG_REDUCE = 64 };
#ifdef BGLS_LEGACY_KERNELS
constexpr int LG_BUILT = LG_FINAL | LG_LAT | LG_EPI | LG_SUM | LG_TREE | LG_G1 | LG_REDUCE;
#else
constexpr int LG_BUILT = LG_TREE | LG_G1 | LG_REDUCE;
#endif
bool legacy(int bit) {
  static const int mask = [] { const char* e = getenv("BGLS_LEGACY"); return (e ? atoi(e) : 0) & LG_BUILT; }();
  return (mask & bit) != 0;
}
bool g1x() { return !legacy(LG_G1); }
// G2 key sums: true = one partial per LANE PAIR on the carry-free limbs (k_sumpair.hip, rx_jacpair.hpp), false = k_sum_main
bool sum_pairs() { return !legacy(LG_SUM); }

// ST_SUM is opened ONCE per key sum (main pass + tree + conversion); ST_SUM_MAIN brackets the main-pass kernel alone, inside it
// ST_SCATTER and ST_EPI are opened by the batch of independent verifications only (Engine::miller_product_batch): the padded layout
// of its pairs and its batched epilogue; ST_BB_KEYS by the batched Boneh-Boyen verification only (Engine::miller_bb: its Q_b = m_b g2 + U_b + r_b V_b)
// ST_HAE_KEYS by the batched HAE multi-signatures only (bgls_verify_multi_hae_sets: the roots, the XOF expansion and the weighted main pass)
// ST_AMS_MSGS by the batched accountable-subgroup multisignatures only (Engine::miller_ams: the assembly of the hash inputs)
// ST_RLC by the combined multi-signature check only (verify_sets_combined_run: the coefficients, k_rlc_pair, the per-group signature sums)
// ST_KEY_MSGS by the distinct-message and authentication checks only (Engine::key_msgs: the hash inputs built from the keys on the device)
// ST_GROUP by the grouping of messages only (Engine::group_messages: table, numbering, index list, work items, compaction)
enum { ST_DUP = 0, ST_H2C, ST_MILLER, ST_REDUCE, ST_FINAL, ST_SUM, ST_SUM_MAIN, ST_SCATTER, ST_EPI, ST_BB_KEYS, ST_HAE_KEYS, ST_AMS_MSGS, ST_KEY_MSGS, ST_RLC,
       ST_GROUP, ST_NUM };
const char* const STAGE_NAMES[ST_NUM] = {"dup_check", "h2c", "miller", "reduce", "final_exp", "sum_points", "sum_main", "scatter", "epilogue", "bb_keys",
                                         "hae_keys", "ams_msgs", "key_msgs", "rlc", "group"};

// roctx ranges around the stages (SURVEY section 5: "roctx ranges around H2C / Miller / reduce / final-exp"), behind bgls_profile_enable like
// the event timers: `rocprofv3 --marker-trace` then shows bgls:h2c, bgls:miller, ... on the host timeline next to the kernels.  The
// marker library is looked up at run time (dlopen, as librccl is): no link-time dependency, nothing happens where it is absent.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
      void* so = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (!so) continue;
      push = (int (*)(const char*))dlsym(so, "roctxRangePushA");
      pop = (int (*)())dlsym(so, "roctxRangePop");
      if (push && pop) return;
      push = nullptr;
      pop = nullptr;
    }
  }
};
Roctx& roctx() {
  static Roctx r;
  return r;
}
const char* const STAGE_RANGES[ST_NUM] = {"bgls:dup_check", "bgls:h2c", "bgls:miller", "bgls:reduce", "bgls:final_exp", "bgls:sum_points", "bgls:sum_main",
                                          "bgls:scatter", "bgls:epilogue", "bgls:bb_keys", "bgls:hae_keys", "bgls:ams_msgs", "bgls:key_msgs", "bgls:rlc",
                                          "bgls:group"};

struct Scope {  // brackets the launches of one stage with events (and a roctx range) when profiling is on; on = false: part of the caller's stage
  Ctx& c; hipStream_t st; int stage; hipEvent_t a = nullptr; bool ranged = false;
  Scope(Ctx& c_, hipStream_t st_, int stage_, bool on = true) : c(c_), st(st_), stage(stage_) {
    if (c.prof && on) {
      a = c.ev(); (void)hipEventRecord(a, st);
      if (roctx().push) { (void)roctx().push(STAGE_RANGES[stage]); ranged = true; }
    }
  }
  ~Scope() {
    if (ranged) (void)roctx().pop();
    if (c.prof && a) { hipEvent_t b = c.ev(); (void)hipEventRecord(b, st); c.pending.push_back({a, b, stage}); }
  }
};

// the duplicate scan's hash seed: unpredictable per process, different per call (k_dup_check)
inline uint64_t dup_seed() {
  static const uint64_t base = [] {
    std::random_device rd;
    return ((uint64_t)rd() << 32) ^ (uint64_t)rd() ^ (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
  }();
  static std::atomic<uint64_t> calls{0};
  uint64_t x = base + 0x9e3779b97f4a7c15ull * (calls.fetch_add(1, std::memory_order_relaxed) + 1);
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27;
  return x;
}

// window multiples of a generator for this device (engine_verify.inc), built on first use
template <class C> int fixed_base_table(Ctx& c, int group, const void** out);

template <class C>
struct Engine {
  typedef F1<C> G1F;
  typedef F2<C> G2F;
  static constexpr size_t FB = C::FP_BYTES, G1B = 2 * FB, G2B = 4 * FB, GTB = 12 * FB;

  // n_buckets > 1: the scan of ONE bucket of the records (first byte mod n_buckets, see k_dup_check) -- the table is sized for twice
  // the bucket's fair share plus slack, and a table that fills up is reported as a hit
  // packed (round 6): the records are what an all-to-all by bucket delivered -- this bucket's digests and padding of other buckets -- so the
  // table is sized for ALL of them (it cannot fill up: the scan is exact and probes without a bound), the bucket filter only skips the padding.
  static int dup_scan(Ctx& c, hipStream_t st, MsgView mv, size_t n, uint32_t* d_flags, uint32_t bucket = 0, uint32_t n_buckets = 1, bool packed = false) {
    if (n < 2) return 0;
    if (n >= MAX_BATCH) return too_large();
    const size_t share = n_buckets > 1 && !packed ? 2 * (n / n_buckets) + 4096 : n;
    size_t cap = 1;
    while (cap < 2 * (share < n ? share : n)) cap <<= 1;
    void* tab;
    int rc;
    if ((rc = c.get(WS_TABLE, cap * 4, &tab))) return rc;
    Scope sc(c, st, ST_DUP);
    HIPCHK(hipMemsetAsync(tab, 0, cap * 4, st));
    kl::dup_check(st, mv, n, (uint32_t*)tab, (uint32_t)(cap - 1), d_flags, bucket, n_buckets, dup_seed(), packed);
    HIPCHK(hipGetLastError());
    return 0;
  }

  // The hash inputs of n (key, message) pairs whose message is derived from the key, built from keys that are on the device already
  // (kl::key_msgs, k_keymsgs.hip): BGLS_KEYED_PREFIX -- key i's wire bytes || message i of mv (msg_bytes: the bytes of the n messages together;
  // DistinctMsg*, bgls/blsDistinctMessage.go:51), BGLS_KEYED_POP -- the compressed key i alone (CheckAuthentication, bgls/blsKosk.go:66; mv
  // unused, a key that does not compress sets FLAG_ENC).  *out: the view the call hashes in place of mv.
  static int key_msgs(Ctx& c, hipStream_t st, int mode, const uint8_t* d_keys, MsgView mv, size_t msg_bytes, size_t n, uint32_t* d_flags, MsgView* out) {
    if (n >= MAX_BATCH) return too_large();
    const bool pop = mode == BGLS_KEYED_POP;
    const size_t cap = pop ? n * (G2B / 2) : msg_bytes + n * G2B;
    void *blob, *ooff = nullptr;
    int rc;
    if ((rc = c.get(WS_KEYED_BLOB, cap, &blob))) return rc;
    if (!pop && mv.off && (rc = c.get(WS_KEYED_OFF, (n + 1) * 8, &ooff))) return rc;
    if (pop) *out = {(const uint8_t*)blob, nullptr, G2B / 2, G2B / 2};
    else if (mv.off) *out = {(const uint8_t*)blob, (const uint64_t*)ooff, 0, 0};
    else *out = {(const uint8_t*)blob, nullptr, G2B + mv.len, G2B + mv.len};
    Scope sc(c, st, ST_KEY_MSGS);
    kl::key_msgs(st, C::CURVE_ID, mode, d_keys, n, mv, (uint8_t*)blob, cap, (uint64_t*)ooff, d_flags);
    HIPCHK(hipGetLastError());
    return 0;
  }

  // The groups of n >= 1 messages by exact bytes (k_msggroup.hip; bgls_group_messages, bgls_verify_aggregate_grouped).  d = the number of
  // distinct messages; group_of[i] = the group of message i, numbered in the order of first occurrence (written to d_group_of where the
  // caller gives a device array, else to the workspace).  plan = true adds what the verification needs: the index list idx sorted by group
  // (group g: start[g] .. start[g + 1]), the n_items work items {lo, hi} of the indexed key sum with item_start (d + 1 offsets: the
  // partials of group g), the n_multi groups of several items (multi) with their runs of partials as the work items of the second pass
  // (joins), and reps: the d representative messages as an ordinary view
  // (msg_bytes: an upper bound of the bytes of all n messages).  Workspaces (DESIGN.md section 5): the table and the first occurrences in
  // WS_TABLE, every array of 32-bit words in WS_MSM_LIST, of 64-bit words in WS_SEG_OFF, the compacted messages in WS_KEYED_BLOB /
  // WS_KEYED_OFF.  Table, counters, cursors and the size word are reset here; everything else is written before it is read.  The host
  // waits once for d and, with plan, once more for the item count: the launches that follow are sized by them.
  struct Groups {
    size_t d = 0, n_items = 0, n_multi = 0;
    const uint32_t *group_of = nullptr, *idx = nullptr, *start = nullptr, *multi = nullptr;
    const void *items = nullptr, *joins = nullptr;
    const uint64_t* item_start = nullptr;
    MsgView reps = {nullptr, nullptr, 0, 0};
  };
  // small (grpkeys.hpp): groups of at most that many keys get no work item -- their sums come from k_sumpairgrp_main (sum_groups); 0, what
  // every caller but the key-set form passes, is the plan of msggroup.hpp.
  static int group_messages(Ctx& c, hipStream_t st, MsgView mv, size_t msg_bytes, size_t n, uint32_t* d_group_of, bool plan, Groups* out, uint32_t small = 0) {
    if (n >= MAX_BATCH) return too_large();
    if (c.res_pending) return in_flight();                  // the pinned result words carry d and the item count to the host
    size_t cap = 2;
    while (cap < 2 * n) cap <<= 1;
    const size_t tiles = kl::scan_tiles(n + 1);
    const uint32_t chunk = msggroup_chunk(n);
    const size_t most_multi = n / chunk + 1;                // a group of several items has more than `chunk` keys
    size_t w32 = 0, w64 = 0;
    auto take = [](size_t& at, size_t words) { const size_t r = at; at += (words + 63) & ~(size_t)63; return r; };
    const size_t o_slot = take(w32, n), o_rep = take(w32, n), o_rank = take(w32, n + 1), o_group = take(w32, d_group_of ? 0 : n), o_idx = take(w32, n),
                 o_repidx = take(w32, n), o_count = take(w32, n), o_cursor = take(w32, n), o_start = take(w32, n + 1), o_nitems = take(w32, n),
                 o_items = take(w32, 2 * (msggroup_max_items(n, n, chunk) + 1)), o_joins = take(w32, 2 * most_multi), o_multi = take(w32, most_multi),
                 o_bsum = take(w32, tiles + 1), o_meta = take(w32, 8);
    const size_t o_istart = take(w64, n + 1), o_lens = take(w64, n), o_bsum64 = take(w64, tiles + 1);
    void *tab, *a32, *a64, *blob = nullptr, *ooff = nullptr;
    int rc;
    if ((rc = c.get(WS_TABLE, cap * 8, &tab))) return rc;
    if ((rc = c.get(WS_MSM_LIST, w32 * 4, &a32))) return rc;
    if ((rc = c.get(WS_SEG_OFF, w64 * 8, &a64))) return rc;
    if (plan && (rc = c.get(WS_KEYED_BLOB, mv.off ? msg_bytes : n * mv.len, &blob))) return rc;
    if (plan && mv.off && (rc = c.get(WS_KEYED_OFF, (n + 1) * 8, &ooff))) return rc;
    uint32_t *table = (uint32_t*)tab, *first = table + cap, *u = (uint32_t*)a32;
    uint64_t* v = (uint64_t*)a64;
    uint32_t* group_of = d_group_of ? d_group_of : u + o_group;
    Scope sc(c, st, ST_GROUP);
    HIPCHK(hipMemsetAsync(table, 0, cap * 4, st));
    HIPCHK(hipMemsetAsync(first, 0xFF, cap * 4, st));
    kl::grp_resolve(st, mv, n, table, (uint32_t)(cap - 1), first, u + o_slot, dup_seed());
    kl::grp_mark(st, n, u + o_slot, first, u + o_rep);
    kl::scan_excl<uint32_t, uint32_t>(st, u + o_rep, n, u + o_bsum, u + o_rank);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&c.h_res[4], u + o_rank + n, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const size_t d = c.h_res[4];
    if (d == 0 || d > n) return fail(BGLS_ERR_HIP, "message grouping: inconsistent group count");
    HIPCHK(hipMemsetAsync(u + o_count, 0, d * 4, st));
    kl::grp_assign(st, n, u + o_rep, u + o_rank, u + o_slot, table, u + o_repidx);
    kl::grp_groups(st, n, u + o_slot, table, group_of, u + o_count);
    kl::scan_excl<uint32_t, uint32_t>(st, u + o_count, d, u + o_bsum, u + o_start);
    HIPCHK(hipGetLastError());
    out->d = d;
    out->group_of = group_of;
    if (!plan) return 0;
    HIPCHK(hipMemsetAsync(u + o_cursor, 0, d * 4, st));
    HIPCHK(hipMemsetAsync(u + o_meta, 0, 8 * 4, st));
    kl::grp_scatter(st, n, group_of, u + o_start, u + o_cursor, u + o_idx);
    kl::grp_nitems(st, d, u + o_start, chunk, small, u + o_nitems, u + o_meta);
    kl::scan_excl<uint32_t, uint64_t>(st, u + o_nitems, d, v + o_bsum64, v + o_istart);
    kl::grp_items(st, d, u + o_start, v + o_istart, chunk, u + o_items, u + o_joins, u + o_multi, u + o_meta);
    HIPCHK(hipMemcpyAsync(&c.h_res[8], u + o_meta, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&c.h_res[6], v + o_istart + d, 8, hipMemcpyDeviceToHost, st));
    if (mv.off) {
      kl::grp_lens(st, mv, d, u + o_repidx, v + o_lens);
      kl::scan_excl<uint64_t, uint64_t>(st, v + o_lens, d, v + o_bsum64, (uint64_t*)ooff);
      kl::grp_compact(st, mv, d, u + o_repidx, (const uint64_t*)ooff, 0, (uint8_t*)blob);
      out->reps = {(const uint8_t*)blob, (const uint64_t*)ooff, 0, 0};
    } else {
      kl::grp_compact(st, mv, d, u + o_repidx, nullptr, mv.len, (uint8_t*)blob);
      out->reps = {(const uint8_t*)blob, nullptr, mv.len, mv.len};
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    uint64_t n_items;
    memcpy(&n_items, &c.h_res[6], 8);
    const size_t largest = c.h_res[8], n_multi = c.h_res[9];
    if ((small == 0 && n_items < d) || n_items > grpkeys_max_items(n, d, chunk, small) || largest == 0 || largest > n || n_multi >= most_multi || (n_multi != 0) != (largest > chunk))
      return fail(BGLS_ERR_HIP, "message grouping: inconsistent work plan");
    out->n_items = (size_t)n_items;
    out->n_multi = n_multi;
    out->multi = u + o_multi;
    out->joins = u + o_joins;
    out->idx = u + o_idx;
    out->start = u + o_start;
    out->items = u + o_items;
    out->item_start = v + o_istart;
    return 0;
  }

  // The d key sums of the groups as wire bytes at *d_sums (WS_SEG_KEYS): the indexed main pass, one block and one partial per work item
  // (k_sumpairidx_main), the partials to wire bytes, and each group's sum to its place -- the partial itself where the group has one item,
  // else the sum of its partials (contiguous by construction) from a second pass of the same kernel, one block per such group, over the
  // partials' wire bytes.  There are fewer than n / chunk + 1 such groups.  A bad key anywhere sets FLAG_ENC.
  // Layout of WS_SEG_KEYS: d + 1 key sums | n_items partials | n_multi joined sums; WS_JAC_A: n_items partials, WS_JAC_B: n_multi.
  // recs = true (bgls_verify_aggregate_grouped_h): d_keys are a key set's sum-ready records, g.idx holds ranks among the selected keys sel
  // (nullptr: every key, the ranks are the keys), and the plan was made with the threshold `small` -- the groups it left without an item
  // are summed by one lane pair each (k_sumpairgrp_main: d Jacobian sums behind the partials in WS_JAC_A, infinity where a group has
  // items), and k_jac_to_bytes puts all d of them in place before k_grp_pick / k_grp_place overwrite those of the groups with items.
  static int sum_groups(Ctx& c, hipStream_t st, const uint8_t* d_keys, const Groups& g, const uint8_t** d_sums, uint32_t* d_flags, bool recs = false,
                        const uint32_t* sel = nullptr, uint32_t small = 0) {
    const size_t JB = kl::jac_bytes<C>(BGLS_G2);
    if (g.n_items > ((size_t)1 << 30)) return fail(BGLS_ERR_ARG, "too many work items for one call");
    void *ja, *jb, *ks;
    int rc;
    Scope sc(c, st, ST_SUM);
    if ((rc = c.get(WS_JAC_A, (g.n_items + 1 + (small ? g.d : 0)) * JB, &ja))) return rc;
    if ((rc = c.get(WS_JAC_B, (g.n_multi + 1) * JB, &jb))) return rc;
    if ((rc = c.get(WS_SEG_KEYS, (g.d + 1 + g.n_items + g.n_multi) * G2B, &ks))) return rc;
    uint8_t *sums = (uint8_t*)ks, *parts = sums + (g.d + 1) * G2B, *joined = parts + g.n_items * G2B;
    {
      Scope scm(c, st, ST_SUM_MAIN);
      if (!recs) kl::sumpairidx_main<C>(st, d_keys, g.idx, g.items, g.n_items, ja, d_flags);
      else {
        if (g.n_items) kl::sumpairidx_recs<C>(st, d_keys, g.idx, sel, g.items, g.n_items, ja, d_flags);
        if (small) kl::sumpairgrp_main<C>(st, d_keys, g.idx, sel, g.start, g.d, small, (uint8_t*)ja + g.n_items * JB);
      }
    }
    if (small) kl::jac_to_bytes<C>(st, BGLS_G2, (uint8_t*)ja + g.n_items * JB, g.d, sums);
    if (g.n_items) kl::jac_to_bytes<C>(st, BGLS_G2, ja, g.n_items, parts);
    kl::grp_pick(st, g.d, g.item_start, parts, G2B, sums);
    if (g.n_multi) {
      kl::sumpairidx_main<C>(st, parts, nullptr, g.joins, g.n_multi, jb, d_flags);
      kl::jac_to_bytes<C>(st, BGLS_G2, jb, g.n_multi, joined);
      kl::grp_place(st, g.n_multi, g.multi, joined, G2B, sums);
    }
    HIPCHK(hipGetLastError());
    *d_sums = sums;
    return 0;
  }

  // d_flags: device u32 (already zeroed by caller).  Writes the product of the n (+1) Miller values to d_partial (GT
  // bytes, no final exponentiation).
  // d_w16 != nullptr: pair i is (w_i H(m_i), pk_i) with 16-byte big-endian weights (hashed aggregation exponents).
  static int miller_product(Ctx& c, hipStream_t st, const uint8_t* d_sig, const uint8_t* d_keys, MsgView mv, size_t n,
                            int check_dups, uint8_t* d_partial, uint32_t* d_flags, const uint8_t* d_w16 = nullptr) {
    if (n >= MAX_BATCH) return too_large();
    const bool raw = C::CURVE_ID == 1 && n > 0;           // BLS12-381: uncleared hash points, cofactor applied once in GT (any batch size:
                                                          // clearing it per message is a 126-bit scalar multiplication on a lone lane, 4.8 ms)
    void* g1s;
    int rc;
    if ((rc = c.get(WS_G1S, (n + 2) * sizeof(Aff<G1F>), &g1s))) return rc;
    // The signature pair (-sigma, g2) depends on nothing but sigma.  A verification with the machine to itself (one stream, not
    // throughput mode) walks it on the context's side stream WHILE THE MESSAGES ARE HASHED, and joins before the Miller launch:
    // the epilogue behind the reduce stage is then only rest^h and one product (0.4 ms off the serial tail on alt-bn128).  The join
    // is early on purpose: a block still running beside a launch that fills the chip exactly would displace one of its blocks
    // into a second round (measured: Miller stage 4.9 -> 6.0 ms at 2^16).
    const bool sig_early = d_sig != nullptr && !legacy(LG_EPI) && !throughput_mode() && n > LAT_MAX && (miller_shape() == 0 || miller_shape() == 4);
    Fp2<C>* sig_half = nullptr;
    SideJoin sj{c.side};
    if (d_sig && sig_early) {
      const LineCoeffs<C>* gl = nullptr;
      void* tmp;
      if ((rc = gen_lines(c, &gl))) return rc;
      if ((rc = c.get(WS_EPI, 12 * sizeof(Fp2<C>), &tmp))) return rc;
      kl::g1_parse<C>(st, d_sig, 1, 1, (Aff<G1F>*)g1s + n, d_flags);
      HIPCHK(hipEventRecord(c.ev_fork, st));
      HIPCHK(hipStreamWaitEvent(c.side, c.ev_fork, 0));
      sj.armed = true;
      kl::cofactor_epiloguex_part<C>(c.side, 1, nullptr, (const Aff<G1F>*)g1s + n, gl, (Fp2<C>*)tmp, nullptr);
      HIPCHK(hipEventRecord(c.ev_join, c.side));
      sig_half = (Fp2<C>*)tmp;
    }
    if (check_dups && (rc = dup_scan(c, st, mv, n, d_flags))) return rc;
    if (n) {
      Scope sc(c, st, ST_H2C);
      if ((rc = hash_to_g1(c, st, mv, n, (Aff<G1F>*)g1s, d_flags, raw))) return rc;
      if (d_w16) kl::scale_g1_inplace<C>(st, (Aff<G1F>*)g1s, d_w16, n);
    }
    if (d_sig && !sig_early) kl::g1_parse<C>(st, d_sig, 1, 1, (Aff<G1F>*)g1s + n, d_flags);
    if (sig_half) HIPCHK(hipStreamWaitEvent(st, c.ev_join, 0));
    sj.armed = false;
    return miller(c, st, (const Aff<G1F>*)g1s, d_keys, n, d_sig ? (const Aff<G1F>*)g1s + n : nullptr, d_partial, d_flags, raw, sig_half);
  }

  // The same product against a PREPARED key range (prepared.hpp): no point steps, the hash points only scale the resident
  // line ratios.  BLS12-381 hash points stay uncleared as on the unprepared path: the cofactor is applied once in GT.
  static int miller_product_prepared(Ctx& c, hipStream_t st, const uint8_t* d_sig, const uint32_t* d_prep, const uint8_t* d_kinf, size_t n_pad, int ng,
                                     MsgView mv, size_t n, uint8_t* d_partial, uint32_t* d_flags) {
    if (n >= MAX_BATCH) return too_large();
    void *g1s, *ptab, *pa, *pb;
    int rc;
    if ((rc = c.get(WS_G1S, (n + 2) * sizeof(Aff<G1F>), &g1s))) return rc;
    const bool raw = C::CURVE_ID == 1 && n > 0;
    if (n) {
      Scope sc(c, st, ST_H2C);
      if ((rc = hash_to_g1(c, st, mv, n, (Aff<G1F>*)g1s, d_flags, raw))) return rc;
    }
    const Aff<G1F>* sig = nullptr;
    const LineCoeffs<C>* gl = nullptr;
    if (d_sig) {
      kl::g1_parse<C>(st, d_sig, 1, 1, (Aff<G1F>*)g1s + n, d_flags);
      sig = (const Aff<G1F>*)g1s + n;
      if ((rc = gen_lines(c, &gl))) return rc;
    }
    if (n == 0) return miller(c, st, (const Aff<G1F>*)g1s, nullptr, 0, sig, d_partial, d_flags, false);
    // ng = pairings per group and squaring, fixed when the key set was uploaded (engine_keys.inc prep_ng: one round of resident waves)
    if (ng < 1 || n_pad % ((size_t)10 * ng) != 0) return fail(BGLS_ERR_ARG, "prepared key set: inconsistent padding");
    const kl::PrepSizes ps = kl::prep_sizes<C>();
    const size_t groups = n_pad / ng;
    if ((rc = c.get(WS_LINES, n_pad * ps.point_bytes, &ptab))) return rc;
    if ((rc = c.get(WS_F_A, (groups + 1) * 6 * sizeof(Fp2<C>), &pa))) return rc;
    if ((rc = c.get(WS_F_B, (groups / REDUCE_R + 2) * 6 * sizeof(Fp2<C>), &pb))) return rc;
    {
      Scope sc(c, st, ST_MILLER);
      kl::prep_points<C>(st, (const Aff<G1F>*)g1s, d_kinf, n, n_pad, (uint32_t*)ptab);
      kl::fold_prep<C>(st, d_prep, (const uint32_t*)ptab, n_pad, ng, (Fp2<C>*)pa);
      HIPCHK(hipGetLastError());
    }
    Fp2<C>* red = nullptr;
    if ((rc = reduce(c, st, (Fp2<C>*)pa, (Fp2<C>*)pb, groups, &red))) return rc;
    return emit_partial(c, st, red, raw || sig != nullptr, sig, gl, d_partial);
  }

  // A batch of n_inst independent aggregate verifications (bgls_verify_aggregate_batch): instance b is the signature d_sigs[b]
  // (wire bytes) and the pairs inst_off[b] .. inst_off[b + 1] of the flat keys / messages (inst_off: n_inst + 1 HOST offsets from 0, monotone).
  // Every stage runs once for the whole batch: one duplicate scan (a duplicate within instance b sets d_iflags[b]), one hashing pass
  // over all messages, a scatter of the pairs to padded positions (each instance a run of whole six-pairing groups), one k_miller_x60
  // launch sequence in its 60-pairing form (the 64-form's last four pairings join groups 0..3 of their block, so a group could straddle
  // two instances), a segmented reduce to one partial per instance, the batched epilogue (rest^h and the signature pair).  Writes
  // n_inst GT partials (bytes, no final exponentiation) to d_partials; d_iflags: n_inst words, zeroed by the caller.
  // d_w16 != nullptr: pair i is (w_i H(m_i), pk_i) with 16-byte big-endian weights, as in miller_product.
  // pre != nullptr (the combined multi-signature check): nothing is hashed or parsed here -- pre->g1s are the n resident G1 points of the
  // pairs (already scaled; uncleared on BLS12-381) and pre->sigs the n_inst resident affine points that take the place of the -sigma_b;
  // d_sigs, mv and d_w16 are not read.  pre->cleared (the combined Boneh-Boyen check): the pre->g1s are G1 points, and the epilogue folds the
  // signature-slot pair in without raising an instance's rest to the cofactor.
  struct PreScaled { const Aff<G1F>* g1s; const Aff<G1F>* sigs; bool cleared = false; };
  static int miller_product_batch(Ctx& c, hipStream_t st, const uint8_t* d_sigs, const uint8_t* d_keys, MsgView mv, const uint64_t* inst_off, size_t n_inst,
                                  int check_dups, uint8_t* d_partials, uint32_t* d_iflags, uint32_t* d_flags, const uint8_t* d_w16 = nullptr,
                                  const PreScaled* pre = nullptr) {
    const size_t n = inst_off[n_inst];
    if (n >= MAX_BATCH || n_inst >= MAX_BATCH) return too_large();
    constexpr bool raw = C::CURVE_ID == 1;                // BLS12-381: uncleared hash points, the cofactor applied per instance in the epilogue
    // host tables, uploaded in one copy: inst_off, pad_off, then the segment tables of the reduce passes ({start, count} words)
    std::vector<uint64_t>& tab = c.stage_tab;
    tab.assign(2 * (n_inst + 1), 0);
    for (size_t b = 0; b <= n_inst; ++b) tab[b] = inst_off[b];
    for (size_t b = 0; b < n_inst; ++b) tab[n_inst + 2 + b] = tab[n_inst + 1 + b] + (inst_off[b + 1] - inst_off[b] + 5) / 6 * 6;
    const size_t n_pad = tab[2 * n_inst + 1];
    if (n_pad >= MAX_BATCH) return too_large();
    const size_t nb = (n_pad + 59) / 60, groups = nb * 10;
    // reduce passes, planned on the host: segment b holds cnt[b] partials from pos[b]; a pass leaves ceil(cnt / R) of them (one for an
    // empty segment), until every instance has exactly one.  Kernel per pass as in Engine::reduce: k_reduce_fx (R = 10) once at most
    // REDUCE_FX_MAX partials are left, k_reduce_coop (R = REDUCE_R) above.
    struct Pass { size_t at, nout; bool fx; int R; };
    std::vector<Pass> passes;
    std::vector<size_t> pos(n_inst), cnt(n_inst);
    size_t total = 0, max_out = 1;
    bool done = true;
    for (size_t b = 0; b < n_inst; ++b) {
      pos[b] = tab[n_inst + 1 + b] / 6;
      cnt[b] = (tab[n_inst + 2 + b] - tab[n_inst + 1 + b]) / 6;
      total += cnt[b];
      done = done && cnt[b] == 1;
    }
    while (!done) {
      const bool fx = !legacy(LG_REDUCE) && total <= REDUCE_FX_MAX;
      const int R = fx ? 10 : REDUCE_R;
      const size_t at = tab.size();
      size_t nout = 0;
      done = true;
      for (size_t b = 0; b < n_inst; ++b) {
        const size_t k = cnt[b] == 0 ? 1 : (cnt[b] + R - 1) / R;
        for (size_t j = 0; j < k; ++j) {
          const size_t lo = pos[b] + j * R, m = cnt[b] - j * R < (size_t)R ? cnt[b] - j * R : (size_t)R;
          tab.push_back((uint64_t)(cnt[b] ? lo : 0) | ((uint64_t)(cnt[b] ? m : 0) << 32));
        }
        pos[b] = nout;
        cnt[b] = k;
        nout += k;
        done = done && k == 1;
      }
      passes.push_back({at, nout, fx, R});
      total = nout;
      if (nout > max_out) max_out = nout;
    }
    void *d_tab, *g1s, *g1p, *keyp, *sigs, *epi;
    int rc;
    if ((rc = c.get(WS_BATCH_IDX, tab.size() * 8, &d_tab))) return rc;
    if (pre) {
      g1s = (void*)pre->g1s;
      sigs = (void*)pre->sigs;
    } else {
      if ((rc = c.get(WS_G1S, (n + 1) * sizeof(Aff<G1F>), &g1s))) return rc;
      if ((rc = c.get(WS_BATCH_SIGS, (n_inst + 1) * sizeof(Aff<G1F>), &sigs))) return rc;
    }
    if ((rc = c.get(WS_BATCH_EPI, (n_inst + 1) * 12 * sizeof(Fp2<C>), &epi))) return rc;
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
    const uint64_t* d_inst_off = (const uint64_t*)d_tab;
    const uint64_t* d_pad_off = d_inst_off + n_inst + 1;
    if (check_dups && n >= 2) {
      size_t cap = 1;
      while (cap < 2 * n) cap <<= 1;
      void* table;
      if ((rc = c.get(WS_TABLE, cap * 4, &table))) return rc;
      Scope sc(c, st, ST_DUP);
      HIPCHK(hipMemsetAsync(table, 0, cap * 4, st));
      kl::dup_check_seg(st, mv, n, d_inst_off, (uint32_t)n_inst, (uint32_t*)table, (uint32_t)(cap - 1), d_iflags, dup_seed());
      HIPCHK(hipGetLastError());
    }
    if (n && !pre) {
      Scope sc(c, st, ST_H2C);
      if ((rc = hash_to_g1(c, st, mv, n, (Aff<G1F>*)g1s, d_flags, raw))) return rc;
      if (d_w16) kl::scale_g1_inplace<C>(st, (Aff<G1F>*)g1s, d_w16, n);
    }
    if (!pre) kl::g1_parse<C>(st, d_sigs, n_inst, 1, (Aff<G1F>*)sigs, d_flags);               // -sigma_b
    void *pa, *pb;
    if ((rc = c.get(WS_F_A, (groups + max_out + 1) * 6 * sizeof(Fp2<C>), &pa))) return rc;
    if ((rc = c.get(WS_F_B, (max_out + 1) * 6 * sizeof(Fp2<C>), &pb))) return rc;
    if (n_pad) {
      if ((rc = c.get(WS_BATCH_G1, n_pad * sizeof(Aff<G1F>), &g1p))) return rc;
      if ((rc = c.get(WS_BATCH_KEYS, n_pad * G2B, &keyp))) return rc;
      {
        Scope sc(c, st, ST_SCATTER);
        kl::batch_scatter<C>(st, (const Aff<G1F>*)g1s, d_keys, d_inst_off, d_pad_off, n_inst, n_pad, (Aff<G1F>*)g1p, (uint8_t*)keyp);
        HIPCHK(hipGetLastError());
      }
      constexpr size_t RES = 1024, XB = 32768;            // resident blocks, blocks per launch (as in Engine::miller)
      const int xmode = g_x60_rot.load() >= 0 ? (g_x60_rot.load() & 15) : ((nb <= RES && !throughput_mode()) ? 8 : 0);
      void* park;
      if ((rc = c.get(WS_QP, kl::miller_x_park_bytes<C, 60>(nb < XB ? nb : XB), &park))) return rc;
      Scope sc(c, st, ST_MILLER);
      for (size_t blk0 = 0; blk0 < nb; blk0 += XB) {
        const size_t nblocks = nb - blk0 < XB ? nb - blk0 : XB;
        const size_t p0 = blk0 * 60;
        kl::miller_x<C, 60>(st, (unsigned)nblocks, (const Aff<G1F>*)g1p + p0, (const uint8_t*)keyp + p0 * G2B, n_pad - p0, (Fp2<C>*)pa + blk0 * 60, d_flags,
                            (uint32_t*)park, xmode);
      }
      HIPCHK(hipGetLastError());
    }
    Fp2<C>* red = (Fp2<C>*)pa;
    {
      Scope sc(c, st, ST_REDUCE);
      Fp2<C>* a = (Fp2<C>*)pa;
      Fp2<C>* b = (Fp2<C>*)pb;
      for (const Pass& p : passes) {
        const uint32_t* seg = (const uint32_t*)(d_inst_off + p.at);
        if (p.fx) kl::reduce_fx_seg<C>(st, a, seg, p.nout, b);
        else kl::reduce_coop_seg<C>(st, a, seg, p.nout, p.R, b);
        std::swap(a, b);
      }
      HIPCHK(hipGetLastError());
      red = a;
    }
    const LineCoeffs<C>* gl = nullptr;
    if ((rc = gen_lines(c, &gl))) return rc;
    Scope sc(c, st, ST_EPI);
    kl::epiloguex_seg<C>(st, n_inst, red, (const Aff<G1F>*)sigs, gl, (Fp2<C>*)epi, d_partials, d_flags, !(pre && pre->cleared));
    HIPCHK(hipGetLastError());
    return 0;
  }

  // The k_miller_sets launch sequence (ST_MILLER) of Engine::miller_multi_sets and Engine::miller_bb: m accumulators, accumulator b over the
  // pair (g1s[b], d_q[b] as wire bytes) and, where sigs[b] is not at infinity, (sigs[b], g2) on the generator lines gl.  BLS12-381: the
  // w-basis values to rest (6 Fp2 each, for the caller's epilogue); alt-bn128: GT bytes to d_partials.
  static int miller_sets(Ctx& c, hipStream_t st, const Aff<G1F>* g1s, const uint8_t* d_q, const Aff<G1F>* sigs, const LineCoeffs<C>* gl, size_t m, Fp2<C>* rest,
                         uint8_t* d_partials, uint32_t* d_flags) {
    constexpr bool bls = C::CURVE_ID == 1;
    constexpr size_t XB = 32768;                          // blocks per launch (as in Engine::miller)
    const size_t spb = kl::miller_sets_per_block<C>(), nb = (m + spb - 1) / spb;
    void* park;
    int rc;
    if ((rc = c.get(WS_QP, kl::miller_sets_park_bytes<C>(nb < XB ? nb : XB), &park))) return rc;
    Scope sc(c, st, ST_MILLER);
    for (size_t blk0 = 0; blk0 < nb; blk0 += XB) {
      const size_t nblocks = nb - blk0 < XB ? nb - blk0 : XB;
      const size_t s0 = blk0 * spb;
      kl::miller_sets<C>(st, (unsigned)nblocks, g1s + s0, d_q + s0 * G2B, sigs + s0, gl, m - s0, bls ? rest + s0 * 6 : nullptr,
                         bls ? nullptr : d_partials + s0 * GTB, d_flags, (uint32_t*)park);
    }
    HIPCHK(hipGetLastError());
    return 0;
  }

  // A batch of n_sets independent multi-signature verifications (bgls_verify_multi_sets): set b is the signature d_sigs[b] (wire
  // bytes), the key sum d_apks[b] (wire bytes, Engine::sum_sets) and message b of mv.  Every stage runs once for the batch: one
  // hashing pass, the parse of the -sigma_b, one k_miller_sets launch sequence (one accumulator per set: the hash pair and, on
  // alt-bn128, the signature pair on the generator lines), on BLS12-381 the batched epilogue (rest^h, then the signature pair: the
  // single path's order for uncleared hash points).  Writes n_sets GT partials (bytes, no final exponentiation) to d_partials.
  static int miller_multi_sets(Ctx& c, hipStream_t st, const uint8_t* d_sigs, const uint8_t* d_apks, MsgView mv, size_t n_sets, uint8_t* d_partials,
                               uint32_t* d_flags) {
    if (n_sets >= MAX_BATCH) return too_large();
    constexpr bool bls = C::CURVE_ID == 1;                // uncleared hash points, the cofactor applied per set in the epilogue
    void *g1s, *sigs, *rest = nullptr, *epi = nullptr;
    int rc;
    if ((rc = c.get(WS_G1S, (n_sets + 1) * sizeof(Aff<G1F>), &g1s))) return rc;
    if ((rc = c.get(WS_BATCH_SIGS, (n_sets + 1) * sizeof(Aff<G1F>), &sigs))) return rc;
    if (bls) {
      if ((rc = c.get(WS_F_A, (n_sets + 1) * 6 * sizeof(Fp2<C>), &rest))) return rc;
      if ((rc = c.get(WS_BATCH_EPI, (n_sets + 1) * 12 * sizeof(Fp2<C>), &epi))) return rc;
    }
    const LineCoeffs<C>* gl = nullptr;
    if ((rc = gen_lines(c, &gl))) return rc;
    {
      Scope sc(c, st, ST_H2C);
      if ((rc = hash_to_g1(c, st, mv, n_sets, (Aff<G1F>*)g1s, d_flags, bls))) return rc;
    }
    kl::g1_parse<C>(st, d_sigs, n_sets, 1, (Aff<G1F>*)sigs, d_flags);                         // -sigma_b
    if ((rc = miller_sets(c, st, (const Aff<G1F>*)g1s, d_apks, (const Aff<G1F>*)sigs, gl, n_sets, (Fp2<C>*)rest, d_partials, d_flags))) return rc;
    if (bls) {
      Scope sc(c, st, ST_EPI);
      kl::epiloguex_seg<C>(st, n_sets, (const Fp2<C>*)rest, (const Aff<G1F>*)sigs, gl, (Fp2<C>*)epi, d_partials, d_flags);
      HIPCHK(hipGetLastError());
    }
    return 0;
  }

  // A batch of n accountable-subgroup multisignature checks (bgls_ams_verify_batch, bgls/blsAsmSigs.go:48-59): item b is the group key
  // d_apks[b], the signers' key sum d_agg_keys[b] (G2 wire bytes), the signature d_sigs[b] (G1 wire bytes), the indices
  // d_signers[d_soff[b] .. d_soff[b + 1]) (d_soff: n + 1 device offsets from 0, total = d_soff[n], max_signers = the longest list) and
  // message b of mv.  d_hoff: the n + total + 1 offsets of the hash inputs (hbytes in all), a prefix of their exact lengths made by the
  // caller.  Every stage runs once for the batch: k_ams_msgs (the hash inputs; an empty list sets d_iflags[b]), ONE hashing pass over the
  // n + total inputs, the hash points of the signers as wire bytes through Engine::sum_sets (aggMsg_b; exact for a repeated index), the
  // parse of the sums and of the -sigma_b, one k_miller_ams launch sequence (one accumulator per item over both walked pairs and, on
  // alt-bn128, the signature pair), on BLS12-381 the batched epilogue: every hash point there is uncleared, so the product of the two
  // walked pairs is raised to the cofactor (a sum of uncleared points is cleared by the same power), then the signature pair.  Writes n
  // GT partials (bytes, no final exponentiation) to d_partials.
  static int miller_ams(Ctx& c, hipStream_t st, const uint8_t* d_apks, const uint8_t* d_agg_keys, const uint8_t* d_sigs, const uint32_t* d_signers,
                        const uint64_t* d_soff, size_t n, size_t total, size_t max_signers, MsgView mv, const uint64_t* d_hoff, size_t hbytes,
                        uint8_t* d_partials, uint32_t* d_iflags, uint32_t* d_flags) {
    const size_t nh = n + total;
    if (n >= MAX_BATCH || nh >= MAX_BATCH) return too_large();
    constexpr bool bls = C::CURVE_ID == 1;
    void *blob, *g1s, *pts, *sums, *agg, *sigs, *rest = nullptr, *epi = nullptr;
    int rc;
    if ((rc = c.get(WS_AMS_BLOB, hbytes + 16, &blob))) return rc;
    if ((rc = c.get(WS_G1S, (nh + 1) * sizeof(Aff<G1F>), &g1s))) return rc;
    if ((rc = c.get(WS_AMS_PTS, (total + 1) * G1B, &pts))) return rc;
    if ((rc = c.get(WS_AMS_SUMS, (n + 1) * G1B, &sums))) return rc;
    if ((rc = c.get(WS_AMS_AGG, (n + 1) * sizeof(Aff<G1F>), &agg))) return rc;
    if ((rc = c.get(WS_BATCH_SIGS, (n + 1) * sizeof(Aff<G1F>), &sigs))) return rc;
    if (bls) {
      if ((rc = c.get(WS_F_A, (n + 1) * 6 * sizeof(Fp2<C>), &rest))) return rc;
      if ((rc = c.get(WS_BATCH_EPI, (n + 1) * 12 * sizeof(Fp2<C>), &epi))) return rc;
    }
    const LineCoeffs<C>* gl = nullptr;
    if ((rc = gen_lines(c, &gl))) return rc;
    {
      Scope sc(c, st, ST_AMS_MSGS);
      kl::ams_msgs(st, d_apks, d_signers, d_soff, n, total, mv, (unsigned)G2B, d_hoff, (uint8_t*)blob, d_iflags);
      HIPCHK(hipGetLastError());
    }
    {
      Scope sc(c, st, ST_H2C);
      const MsgView hv = {(const uint8_t*)blob, d_hoff, 0, 0};
      if ((rc = hash_to_g1(c, st, hv, nh, (Aff<G1F>*)g1s, d_flags, bls))) return rc;
      // the segmented sum takes wire bytes: the signers' hash points leave the stage in that form
      if (total) kl::g1_to_bytes<C>(st, (const Aff<G1F>*)g1s + n, total, (uint8_t*)pts);
    }
    // aggMsg_b = sum of the item's H2 points.  Engine::sum_sets keeps 64 Jacobian partials per set on G1, so the items go through it
    // 2^16 at a time (0.6 GB of partials on BLS12-381; bgls_set_ams_sum_cut): the offsets index the one array of points, whichever items
    // a pass covers.  Each pass is a key sum of its own in the stage timers (sum_points).
    const size_t SUM_CUT = g_ams_sum_cut.load();
    for (size_t b0 = 0; b0 < n; b0 += SUM_CUT) {
      const size_t cnt = n - b0 < SUM_CUT ? n - b0 : SUM_CUT;
      if ((rc = sum_sets(c, st, BGLS_G1, (const uint8_t*)pts, d_soff + b0, cnt, max_signers, (uint8_t*)sums + b0 * G1B, d_flags))) return rc;
    }
    {
      constexpr size_t XB = 32768;                          // blocks per launch (as in Engine::miller)
      const size_t ipb = kl::miller_ams_per_block<C>(), nb = (n + ipb - 1) / ipb;
      void* park;
      if ((rc = c.get(WS_QP, kl::miller_ams_park_bytes<C>(nb < XB ? nb : XB), &park))) return rc;
      Scope sc(c, st, ST_MILLER);
      kl::g1_parse<C>(st, (const uint8_t*)sums, n, 0, (Aff<G1F>*)agg, d_flags);
      kl::g1_parse<C>(st, d_sigs, n, 1, (Aff<G1F>*)sigs, d_flags);                           // -sigma_b
      for (size_t blk0 = 0; blk0 < nb; blk0 += XB) {
        const size_t nblocks = nb - blk0 < XB ? nb - blk0 : XB;
        const size_t s0 = blk0 * ipb;
        kl::miller_ams<C>(st, (unsigned)nblocks, (const Aff<G1F>*)g1s + s0, d_agg_keys + s0 * G2B, (const Aff<G1F>*)agg + s0, d_apks + s0 * G2B,
                          (const Aff<G1F>*)sigs + s0, gl, n - s0, bls ? (Fp2<C>*)rest + s0 * 6 : nullptr, bls ? nullptr : d_partials + s0 * GTB, d_flags,
                          (uint32_t*)park);
      }
      HIPCHK(hipGetLastError());
    }
    if (bls) {
      Scope sc(c, st, ST_EPI);
      kl::epiloguex_seg<C>(st, n, (const Fp2<C>*)rest, (const Aff<G1F>*)sigs, gl, (Fp2<C>*)epi, d_partials, d_flags);
      HIPCHK(hipGetLastError());
    }
    return 0;
  }

  // A batch of n independent Boneh-Boyen verifications (bgls_bb_verify_batch): item b is sigma_b (d_sigmas, wire bytes) against
  // Q_b = m_b g2 + U_b + r_b V_b (d_keys: U_b || V_b, d_rs / d_ms: 32-byte big-endian scalars).  Every stage runs once for the batch:
  // the parse of the sigma_b, k_bb_keys (Q_b as wire bytes; item n is the reference pair (g1, g2)), one k_miller_sets launch sequence
  // with sigma_b in the hash-point slot and Q_b in the key-sum slot (alt-bn128: no generator pair, every signature slot at infinity;
  // BLS12-381: the w-basis value straight to bytes -- no cofactor power, sigma is a G1 point), writing n + 1 GT partials (bytes, no
  // final exponentiation) to d_partials.
  static int miller_bb(Ctx& c, hipStream_t st, const uint8_t* d_sigmas, const uint8_t* d_rs, const uint8_t* d_keys, const uint8_t* d_ms, size_t n,
                       uint8_t* d_partials, uint32_t* d_flags) {
    if (n >= MAX_BATCH) return too_large();
    constexpr bool bls = C::CURVE_ID == 1;
    const size_t m = n + 1;                               // the items and the reference pair
    void *g1s, *qs, *nosig, *rest = nullptr;
    const void* fb;
    int rc;
    if ((rc = c.get(WS_G1S, (m + 1) * sizeof(Aff<G1F>), &g1s))) return rc;
    if ((rc = c.get(WS_SEG_KEYS, (m + 1) * G2B, &qs))) return rc;
    if ((rc = c.get(WS_BATCH_SIGS, (m + 1) * sizeof(Aff<G1F>), &nosig))) return rc;
    if (bls && (rc = c.get(WS_F_A, (m + 1) * 6 * sizeof(Fp2<C>), &rest))) return rc;
    const LineCoeffs<C>* gl = nullptr;
    if ((rc = gen_lines(c, &gl))) return rc;
    if ((rc = fixed_base_table<C>(c, BGLS_G2, &fb))) return rc;
    kl::g1_parse<C>(st, d_sigmas, n, 0, (Aff<G1F>*)g1s, d_flags);
    {
      Scope sc(c, st, ST_BB_KEYS);
      kl::bb_keys<C>(st, d_keys, d_rs, d_ms, fb, n, (uint8_t*)qs, (Aff<G1F>*)g1s, bls ? nullptr : (Aff<G1F>*)nosig, d_flags);
      HIPCHK(hipGetLastError());
    }
    if ((rc = miller_sets(c, st, (const Aff<G1F>*)g1s, (const uint8_t*)qs, (const Aff<G1F>*)nosig, gl, m, (Fp2<C>*)rest, d_partials, d_flags))) return rc;
    if (bls) {
      Scope sc(c, st, ST_EPI);
      kl::bb_w_bytes<C>(st, (const Fp2<C>*)rest, m, d_partials);
      HIPCHK(hipGetLastError());
    }
    return 0;
  }

  // A batch of n independent pairings (bgls_pair_batch): item b is (P_b, Q_b) = (d_g1s[b], d_g2s[b]) as wire bytes.  Engine::miller_bb's
  // Miller stage without its keys and its reference pair: the parse of the P_b, one k_miller_sets launch sequence with P_b in the
  // hash-point slot and Q_b in the key-sum slot (alt-bn128: every signature slot at infinity; BLS12-381: the w-basis value straight to
  // bytes, no cofactor power), writing n GT partials (bytes, no final exponentiation) to d_partials.
  static int miller_pairs(Ctx& c, hipStream_t st, const uint8_t* d_g1s, const uint8_t* d_g2s, size_t n, uint8_t* d_partials, uint32_t* d_flags) {
    if (n >= MAX_BATCH) return too_large();
    constexpr bool bls = C::CURVE_ID == 1;
    void *g1s, *nosig, *rest = nullptr;
    int rc;
    if ((rc = c.get(WS_G1S, (n + 1) * sizeof(Aff<G1F>), &g1s))) return rc;
    if ((rc = c.get(WS_BATCH_SIGS, (n + 1) * sizeof(Aff<G1F>), &nosig))) return rc;
    if (bls && (rc = c.get(WS_F_A, (n + 1) * 6 * sizeof(Fp2<C>), &rest))) return rc;
    const LineCoeffs<C>* gl = nullptr;
    if ((rc = gen_lines(c, &gl))) return rc;
    kl::g1_parse<C>(st, d_g1s, n, 0, (Aff<G1F>*)g1s, d_flags);
    if (!bls) kl::g1_inf_fill<C>(st, (Aff<G1F>*)nosig, n);
    if ((rc = miller_sets(c, st, (const Aff<G1F>*)g1s, d_g2s, (const Aff<G1F>*)nosig, gl, n, (Fp2<C>*)rest, d_partials, d_flags))) return rc;
    if (bls) {
      Scope sc(c, st, ST_EPI);
      kl::bb_w_bytes<C>(st, (const Fp2<C>*)rest, n, d_partials);
      HIPCHK(hipGetLastError());
    }
    return 0;
  }

  // H(m_i) as affine Montgomery points.  raw (BLS12-381 only): points before cofactor clearing, for the cofactor-in-GT
  // verification path (DESIGN.md section 3).
  static int hash_to_g1(Ctx& c, hipStream_t st, MsgView mv, size_t n, Aff<G1F>* out, uint32_t* d_flags, bool raw = false) {
    if (n >= MAX_BATCH) return too_large();
    int rc;
    void *lists = nullptr, *cnts = nullptr;
    if constexpr (C::CURVE_ID == 0) {
      if (n >= 256) {
        if ((rc = c.get(WS_H2C_LIST, 2 * n * 4, &lists))) return rc;
        if ((rc = c.get(WS_H2C_CNT, 64, &cnts))) return rc;
        HIPCHK(hipMemsetAsync(cnts, 0, 64, st));
      }
      kl::h2c_bn(st, mv, n, (uint32_t*)lists, (uint32_t*)cnts, out, d_flags, throughput_mode());
    } else {
      void *pts, *kinds;
      if ((rc = c.get(WS_H2C_PTS, 2 * n * sizeof(Jac<G1F>), &pts))) return rc;
      if ((rc = c.get(WS_H2C_KIND, 2 * n * 4, &kinds))) return rc;
      kl::h2c_bls(st, mv, n, (Jac<G1F>*)pts, (uint32_t*)kinds, out, raw);
    }
    HIPCHK(hipGetLastError());
    return 0;
  }

  // fixed-argument lines of g2 for this device (DeviceTables)
  static int gen_lines(Ctx& c, const LineCoeffs<C>** out) {
    DeviceTables& t = tables_of(c.device);
    std::lock_guard<std::mutex> lk(t.mu);
    if (!t.gen_lines[C::CURVE_ID]) {
      void *tab = nullptr, *cnt = nullptr;
      hipStream_t bs = nullptr;
      HIPCHK(hipMalloc(&tab, 160 * sizeof(LineCoeffs<C>)));
      hipError_t e = hipMalloc(&cnt, 16);
      if (e == hipSuccess) e = hipStreamCreate(&bs);
      if (e == hipSuccess) {
        kl::gen_lines<C>(bs, (LineCoeffs<C>*)tab, (int*)cnt);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(bs);
      }
      if (bs) (void)hipStreamDestroy(bs);
      if (cnt) (void)hipFree(cnt);
      if (e != hipSuccess) {
        (void)hipFree(tab);
        return fail(BGLS_ERR_HIP, "building the generator line table", e);
      }
      t.gen_lines[C::CURVE_ID] = tab;
    }
    *out = (const LineCoeffs<C>*)t.gen_lines[C::CURVE_ID];
    return 0;
  }

  // product of the per-group partial products (w-basis Fp12 arrays, 6 Fp2 each) down to one.  Fan-in REDUCE_R per pass: a pass
  // costs a launch boundary plus R - 1 dependent products (~11 us each on six lanes); three per pass is the shortest chain at
  // the sizes that matter (65 partials of an n = 64 verification: 4 passes x 2 products instead of 4 x 3, 1.73 -> 1.69 ms;
  // 10 240 of a 2^16 batch: 0.24 -> 0.22 ms).  The second buffer (b) must hold count / REDUCE_R + 1 products.
  static constexpr int REDUCE_R = 3;
  static constexpr size_t REDUCE_FX_MAX = 12288;
  static int reduce(Ctx& c, hipStream_t st, Fp2<C>* a, Fp2<C>* b, size_t cnt, Fp2<C>** out) {
    Scope sc(c, st, ST_REDUCE);
    const int R = REDUCE_R;
    // passes with at most REDUCE_FX_MAX products left run one product per BLOCK on the carry-free 36-lane form (k_reduce_fx:
    // ~2-3 us per dependent product instead of 11 / 22 us); BGLS_LEGACY bit 64 keeps k_reduce_coop everywhere
    const bool rfx = !legacy(LG_REDUCE);
    constexpr int rfx_r = 10;                                 // >= REDUCE_R: the second buffer is sized for that (3 .. 12 measured, tools/exp/reduce_r.sh: 10)
    while (cnt > 1) {
      const bool fx = rfx && cnt <= REDUCE_FX_MAX;
      const int Rp = fx ? rfx_r : R;                          // operands converted side by side into LDS slots (at most 12), then a bare chain of ~1.5 us products: fewer, longer passes
      const size_t nout = (cnt + Rp - 1) / Rp;
      if (fx) kl::reduce_fx<C>(st, a, cnt, Rp, b);
      else kl::reduce_coop<C>(st, a, cnt, Rp, b);
      Fp2<C>* t = a;
      a = b;
      b = t;
      cnt = nout;
    }
    HIPCHK(hipGetLastError());
    *out = a;
    return 0;
  }

  // Miller product of npairs (g1s[i], g2s[i]) pairs and, when sig != nullptr, of (*sig, g2) on the generator's
  // pre-computed lines; GT bytes (no final exponentiation) to d_partial.  sig must be an element of the g1s array
  // (verification stores -sigma behind the hash points).  cofactor: the g1s are uncleared BLS12-381 hash points, the
  // product of their Miller values is raised to the G1 cofactor before the signature pair is folded in.
  // sig_half != nullptr: the signature pair's Miller value is already there (12 Fp2 of scratch, the first six filled by
  // cofactor_epiloguex_part 1): the x60 shape's epilogue is then rest^h and the product only.
  static int miller(Ctx& c, hipStream_t st, const Aff<G1F>* g1s, const uint8_t* g2s, size_t npairs, const Aff<G1F>* sig,
                    uint8_t* d_partial, uint32_t* d_flags, bool cofactor = false, Fp2<C>* sig_half = nullptr) {
    if (npairs == 0 && !sig) {
      HIPCHK(hipMemsetAsync(d_partial, 0, GTB, st));
      HIPCHK(hipMemsetAsync(d_partial + GTB - 1, 1, 1, st));
      return 0;
    }
    int rc;
    // BLS12-381 G1 points with a signature pair (the combined Boneh-Boyen check): the k_miller_x60 shape folds the pair in with its
    // epilogue's cofactor power switched off.  The legacy epilogue and the 32-bit fallback shape always raise the product to the
    // cofactor, and cleared points would come out as prod^h * e(sig, g2) there: refused rather than answered with a wrong GT value.
    if (C::CURVE_ID == 1 && sig && !cofactor && npairs > LAT_MAX && (legacy(LG_EPI) || !(miller_shape() == 4 || miller_shape() == 0)))
      return fail(BGLS_ERR_ARG, "BLS12-381: a signature pair with G1 points above 128 pairings is served by the k_miller_x60 shape and its epilogue only");
    const LineCoeffs<C>* gl = nullptr;
    if (sig && (rc = gen_lines(c, &gl))) return rc;
    void *pa, *pb;
    Fp2<C>* red = nullptr;
    bool epilogue = cofactor;
    if ((npairs <= LAT_MAX && miller_shape() == 0) || npairs == 0) {
      // a handful of pairings: one block per pairing (k_miller_latx), the signature pair as one more block -- or, with uncleared
      // BLS12-381 hash points, in the epilogue that raises the other pairs' product to the cofactor.  The signature pair alone
      // (npairs = 0) comes here under every shape: the throughput kernels need at least one pairing
      const bool sig_block = sig && !cofactor;
      const size_t blocks = npairs + (sig_block ? 1 : 0);
      if ((rc = c.get(WS_F_A, (blocks + 1) * 6 * sizeof(Fp2<C>), &pa))) return rc;
      if ((rc = c.get(WS_F_B, (blocks / REDUCE_R + 2) * 6 * sizeof(Fp2<C>), &pb))) return rc;
      {
        Scope sc(c, st, ST_MILLER);
        // k_miller_latx: the same two-wave block on the carry-free limbs (BGLS_LEGACY bit 2 keeps k_miller_lat)
#ifdef BGLS_LEGACY_KERNELS
        if (legacy(LG_LAT)) kl::miller_lat<C>(st, g1s, g2s, npairs, sig_block ? (long long)(sig - g1s) : -1LL, gl, (Fp2<C>*)pa, d_flags);
        else
#endif
        kl::miller_latx<C>(st, g1s, g2s, npairs, sig_block ? (long long)(sig - g1s) : -1LL, gl, (Fp2<C>*)pa, d_flags);
        HIPCHK(hipGetLastError());
      }
      if ((rc = reduce(c, st, (Fp2<C>*)pa, (Fp2<C>*)pb, blocks, &red))) return rc;
      return emit_partial(c, st, red, cofactor, cofactor ? sig : nullptr, gl, d_partial);
    }
    // k_miller_x60 (both roles on carry-free 28-bit limbs; the signature pair goes to the epilogue kernel) is the default above
    // the latency shape.  1024 blocks are resident at a time.  Its 60-pairing block is the faster one per pairing; the
    // 64-pairing block (a seventh line in four of a block's ten groups: the consumer's step is a fold longer) needs fewer
    // blocks, and a verification with the machine to itself takes it where that saves a nearly empty last round of blocks --
    // 61 441 .. 65 536 pairings (exactly 2^16: BASELINE configs 2 / 3) are ONE round instead of two.  (Round 3 fell back to
    // the 32-bit k_miller_ab64 there.)  In throughput mode the neighbours' blocks fill the last round and the 60-form stays.
    const bool x60_auto = miller_shape() == 0 && npairs > LAT_MAX;
    if ((miller_shape() == 4 || x60_auto) && npairs >= 1) {
      constexpr size_t RES = 1024;                      // resident blocks: 256 CUs x 4
      const size_t nb60 = (npairs + 59) / 60, nb64 = (npairs + 63) / 64;
      const size_t r60 = (nb60 + RES - 1) / RES, r64 = (nb64 + RES - 1) / RES;
      // A/B runs and tests: bgls_set_miller_shape(4, mode) with mode bit 16 = the 64-form (clear = the 60-form)
      const int force_np = miller_shape() == 4 && g_x60_rot.load() >= 0 ? ((g_x60_rot.load() & 16) ? 64 : 60) : 0;
      const bool np64 = force_np == 64 || (force_np != 60 && !throughput_mode() && r64 < r60 && r64 <= 2);
      // role / priority mode: consumers placed by SIMD; the producers get issue priority only when the whole batch is one round of
      // resident blocks with the machine to itself (there the slowest block is the launch: 5.5 instead of 7.2 ms for 61 440
      // BLS12-381 pairings), in steady state it costs 3-6 % (measured at 2^20, four verifications in flight)
      const size_t nb = np64 ? nb64 : nb60, NPB = np64 ? 64 : 60, groups = nb * 10;
      const int xmode = g_x60_rot.load() >= 0 ? (g_x60_rot.load() & 15) : ((nb <= RES && !throughput_mode()) ? 8 : 0);
      constexpr size_t XB = 32768;                      // blocks per launch (the lanes' parked operands take up to 57 / 49 KB per block)
      void* park;
      const size_t pblocks = nb < XB ? nb : XB;
      if ((rc = c.get(WS_QP, np64 ? kl::miller_x_park_bytes<C, 64>(pblocks) : kl::miller_x_park_bytes<C, 60>(pblocks), &park))) return rc;
      if ((rc = c.get(WS_F_A, (groups + 1) * 6 * sizeof(Fp2<C>), &pa))) return rc;
      if ((rc = c.get(WS_F_B, (groups / REDUCE_R + 2) * 6 * sizeof(Fp2<C>), &pb))) return rc;
      {
        Scope sc(c, st, ST_MILLER);
        for (size_t blk0 = 0; blk0 < nb; blk0 += XB) {
          const size_t nblocks = nb - blk0 < XB ? nb - blk0 : XB;
          const size_t p0 = blk0 * NPB;
          if (np64) kl::miller_x<C, 64>(st, (unsigned)nblocks, g1s + p0, g2s + p0 * G2B, npairs - p0, (Fp2<C>*)pa + blk0 * 60, d_flags, (uint32_t*)park, xmode);
          else kl::miller_x<C, 60>(st, (unsigned)nblocks, g1s + p0, g2s + p0 * G2B, npairs - p0, (Fp2<C>*)pa + blk0 * 60, d_flags, (uint32_t*)park, xmode);
        }
        HIPCHK(hipGetLastError());
      }
      if ((rc = reduce(c, st, (Fp2<C>*)pa, (Fp2<C>*)pb, groups, &red))) return rc;
      if (sig_half) {
        kl::cofactor_epiloguex_part<C>(st, 2, red, sig, gl, sig_half, d_partial);
        HIPCHK(hipGetLastError());
        return 0;
      }
      return emit_partial(c, st, red, cofactor || sig != nullptr, sig, gl, d_partial, cofactor);
    }
#ifdef BGLS_LEGACY_KERNELS
    // shape 5, the 32-bit fallback (k_miller_ab64): 64 pairings per block at 256 registers: one 2^16 batch is exactly 1024 resident blocks; larger batches run as
    // launches of up to 16384 blocks (one launch drains once: 5 % faster alone than sixteen launches of 1024).  Block 0 of the first launch also scales the generator lines for the
    // signature pair (unless the epilogue kernel does: cofactor path).
    const size_t nb64 = npairs ? (npairs + 63) / 64 : 1, groups = nb64 * 10;
    void* qp;
    constexpr size_t AB = 16384;                        // blocks per launch: 2^20 pairings; the parked operands of a launch take 200 / 300 MB
    if ((rc = c.get(WS_QP, kl::miller_qp_bytes<C>(nb64 < AB ? nb64 : AB), &qp))) return rc;
    if ((rc = c.get(WS_F_A, (groups + 1) * 6 * sizeof(Fp2<C>), &pa))) return rc;
    if ((rc = c.get(WS_F_B, (groups / REDUCE_R + 2) * 6 * sizeof(Fp2<C>), &pb))) return rc;
    {
      Scope sc(c, st, ST_MILLER);
      for (size_t blk0 = 0; blk0 < nb64; blk0 += AB) {
        const size_t nblocks = nb64 - blk0 < AB ? nb64 - blk0 : AB;
        const size_t p0 = blk0 * 64;
        const size_t np = npairs - p0 < nblocks * 64 ? npairs - p0 : nblocks * 64;
        const long long sig_at = (blk0 == 0 && sig && !cofactor) ? (long long)(sig - (g1s + p0)) : -1LL;
        kl::miller_ab64<C>(st, (unsigned)nblocks, g1s + p0, g2s + p0 * G2B, np, sig_at, gl, (Fp2<C>*)pa + blk0 * 10 * 6, d_flags, (uint32_t*)qp);
      }
      HIPCHK(hipGetLastError());
    }
    if ((rc = reduce(c, st, (Fp2<C>*)pa, (Fp2<C>*)pb, groups, &red))) return rc;
    return emit_partial(c, st, red, cofactor, cofactor ? sig : nullptr, gl, d_partial);
#else
    return fail(BGLS_ERR_ARG, "Miller shape 5 (k_miller_ab64) is compiled by `make LEGACY=1` only");
#endif
  }

  // serialise the reduced product; with `epilogue`: raise it to the G1 cofactor (BLS12-381 raw hash points; a no-op
  // exponent on alt-bn128; not at all with power = false, k_epilogue_ax only) and fold the signature pair in on the 36-lane arithmetic
  static int emit_partial(Ctx& c, hipStream_t st, const Fp2<C>* w, bool epilogue, const Aff<G1F>* sig, const LineCoeffs<C>* gl,
                          uint8_t* d_partial, bool power = true) {
    if (!epilogue) {
      kl::w_to_bytes<C>(st, w, d_partial);
    } else {
      // k_epilogue_ax / _bx: the two chains on the carry-free limbs, side by side as two blocks (BGLS_LEGACY bit 4 keeps k_cofactor_epilogue)
      const bool epix = !legacy(LG_EPI);
      void* tmp = nullptr;
      int rc;
      if (epix && (rc = c.get(WS_EPI, 12 * sizeof(Fp2<C>), &tmp))) return rc;
#ifdef BGLS_LEGACY_KERNELS
      if (!epix) kl::cofactor_epilogue<C>(st, w, sig, gl, d_partial);
      else
#endif
      kl::cofactor_epiloguex<C>(st, w, sig, gl, (Fp2<C>*)tmp, d_partial, nullptr, power);
    }
    HIPCHK(hipGetLastError());
    return 0;
  }

  // enqueue product-of-partials + final exponentiation + compare; the verdict lands in the context's pinned words
  static int finalize_submit(Ctx& c, hipStream_t st, const uint8_t* d_partials, size_t count, int do_final_exp, const uint32_t* d_flags_in,
                             uint8_t* h_gt_out) {
    void *tmp, *fl;
    int rc;
    if (c.res_pending) return in_flight();
    if ((rc = c.get(WS_TMP, GTB + 16, &tmp))) return rc;
    if ((rc = c.get(WS_OUT, 16, &fl))) return rc;
    uint8_t* d_gt = (uint8_t*)tmp;
    uint32_t* d_verdict = (uint32_t*)(d_gt + GTB);        // three words: {verdict, final-stage flags, caller flags} on the finalx path
    uint32_t* d_fl2 = (uint32_t*)fl;
    // finalx.hpp: the same 36-lane split on the carry-free limbs (BGLS_LEGACY bit 1 keeps the 32-bit form of finalexp.hpp)
    const bool finalx = !legacy(LG_FINAL);
    if (!finalx) HIPCHK(hipMemsetAsync(d_fl2, 0, 4, st));
    {
      Scope sc(c, st, ST_FINAL);
#ifdef BGLS_LEGACY_KERNELS
      if (!finalx) kl::final36<C>(st, d_partials, count, do_final_exp, d_gt, d_verdict, d_fl2);
      else
#endif
      kl::finalx_res<C>(st, d_partials, count, do_final_exp, d_gt, d_verdict, d_flags_in);
    }
    HIPCHK(hipGetLastError());
    c.h_res[0] = c.h_res[1] = c.h_res[2] = 0;
    if (finalx) {
      HIPCHK(hipMemcpyAsync(&c.h_res[0], d_verdict, 12, hipMemcpyDeviceToHost, st));      // one copy: the kernel gathered the three words
    } else {
      HIPCHK(hipMemcpyAsync(&c.h_res[0], d_verdict, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(&c.h_res[1], d_fl2, 4, hipMemcpyDeviceToHost, st));
      if (d_flags_in) HIPCHK(hipMemcpyAsync(&c.h_res[2], d_flags_in, 4, hipMemcpyDeviceToHost, st));
    }
    if (h_gt_out) HIPCHK(hipMemcpyAsync(h_gt_out, d_gt, GTB, hipMemcpyDeviceToHost, st));
    c.res_pending = true;
    c.res_stream = st;
    return 0;
  }
  // wait for the verification in flight; returns 1/0 or <0
  static int finalize_collect(Ctx& c) {
    if (!c.res_pending) return fail(BGLS_ERR_ARG, "no verification in flight on this context");
    c.res_pending = false;
    HIPCHK(hipStreamSynchronize(c.res_stream));
    c.collect();
    uint32_t f = c.h_res[1] | c.h_res[2];
    if (f & FLAG_ENC) return fail(BGLS_ERR_ENCODING, "non-canonical coordinate or point not on curve");
    if (f & FLAG_SUBGROUP) return fail(BGLS_ERR_ENCODING, "G2 point outside the order-r subgroup");
    if (f & FLAG_DEGENERATE) return fail(BGLS_ERR_ENCODING, "degenerate point step (small-order key)");
    if (f & FLAG_HASH) return fail(BGLS_ERR_HASH, "try-and-increment exhausted");
    if (f & FLAG_DUP) return 0;
    return c.h_res[0] ? 1 : 0;
  }
  // returns 1/0 or <0; optionally copies the GT bytes out
  static int finalize(Ctx& c, hipStream_t st, const uint8_t* d_partials, size_t count, int do_final_exp, const uint32_t* d_flags_in,
                      uint8_t* h_gt_out) {
    int rc;
    if ((rc = finalize_submit(c, st, d_partials, count, do_final_exp, d_flags_in, h_gt_out))) return rc;
    return finalize_collect(c);
  }

  // AggregatePoints (curves/curve.go:73-121): affine bytes of the sum of n points to d_out.
  // src: 0 = wire bytes; 1 = the Montgomery affine points of a key set; 2 = its sum-ready records (lane-pair kernel only)
  static int sum_points(Ctx& c, hipStream_t st, int group, const uint8_t* d_pts, size_t n, uint8_t* d_out, uint32_t* d_flags,
                        int src = 0) {
    const size_t PTB = group == BGLS_G1 ? G1B : G2B;
    if (n == 0) {
      HIPCHK(hipMemsetAsync(d_out, 0, PTB, st));
      return 0;
    }
    void* jac;
    int rc;
    if ((rc = c.get(WS_SUMJ, 4 * kl::jac_bytes<C>(group), &jac))) return rc;
    Scope sc(c, st, ST_SUM);                                   // one scope per key sum: the stage count equals the number of sums
    bool bytes_done = false;
    if ((rc = sum_points_jac(c, st, group, d_pts, n, jac, d_flags, src, false, d_out, &bytes_done))) return rc;
    if (!bytes_done) kl::jac_to_bytes<C>(st, group, jac, 1, d_out);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // nsets sums in one pass: set b = points d_off[b] .. d_off[b+1] (d_off: nsets + 1 offsets on the device, max_set = the
  // largest set); wire bytes of the nsets sums to d_out.  One main launch for all sets (P partials per set), then the
  // usual tree levels over the flat array of nsets * P partials -- P is a power of two, so no level pairs two sets.
  // own_scope = false: the launches count towards the stage the caller has open.
  static int sum_sets(Ctx& c, hipStream_t st, int group, const uint8_t* d_pts, const uint64_t* d_off, size_t nsets, size_t max_set,
                      uint8_t* d_out, uint32_t* d_flags, bool own_scope = true) {
    if (nsets == 0) return 0;
    // P partials (lane pairs / lanes) per set, a power of two.  The lane-pair kernel adds the 32 sums of a block itself and
    // leaves ONE partial per block, so a set of a few keys needs one block (P = 32) and no tree; the other kernels write one
    // partial per lane of at least one wave (P = 64).  Workspaces are sized by what the selected kernel writes.
    const bool pairs = group == BGLS_G2 && sum_pairs();
    size_t P = pairs ? 32 : 64;
    while (P < 8192 && P * 4 <= max_set && nsets * P * 2 <= (size_t)131072) P *= 2;     // >= 4 points per partial, <= 2048 waves in all
    const size_t written = pairs ? nsets * (P / 32) : nsets * P;                         // partial sums the main pass leaves
    const size_t blocks = pairs ? nsets * (P / 32) : nsets * (P / 64);
    const size_t JB = kl::jac_bytes<C>(group);
    // bounds of one call: the grid of the main pass and the partials' workspace (the caller can cut a larger job into calls)
    if (blocks > ((size_t)1 << 30) || (written + 1) * JB > ((size_t)8 << 30))
      return fail(BGLS_ERR_ARG, "too many key sets for one call (cut the batch: at most 2^30 blocks / 8 GiB of partial sums)");
    void *ja, *jb;
    int rc;
    Scope sc(c, st, ST_SUM, own_scope);
    if ((rc = c.get(WS_JAC_A, (written + 1) * JB, &ja))) return rc;
    if ((rc = c.get(WS_JAC_B, (written / 2 + 2) * JB, &jb))) return rc;
    if (group == BGLS_G2 && sum_pairs()) kl::sumpairseg_main<C>(st, d_pts, d_off, nsets, (unsigned)P, ja, d_flags);
    else kl::sumseg_main<C>(st, group, d_pts, d_off, nsets, (unsigned)P, ja, d_flags);
    sum_sets_tree(st, group, ja, jb, pairs ? P / 32 : P, nsets, d_out);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // The levels above a segmented main pass (sum_sets, the weighted sums of bgls_verify_multi_hae_sets): a holds nsets * p Jacobian
  // partials, set-major, p a power of two -- so no level pairs two sets; b has room for half of them.  The nsets sums to d_out as wire bytes.
  static void sum_sets_tree(hipStream_t st, int group, void* a, void* b, size_t p, size_t nsets, uint8_t* d_out) {
    size_t cnt = nsets * p;
    while (p > 1) {
      if (group == BGLS_G2 && cnt <= 8192) {
        kl::sum_coop<C>(st, a, cnt, b);
        p /= 2; cnt /= 2;
      } else if (cnt > 4096 || p < 64) {
        kl::sum_pair<C>(st, group, a, cnt, b);
        p /= 2; cnt /= 2;
      } else {
        kl::sum_wave<C>(st, group, a, cnt, b);
        p /= 64; cnt /= 64;
      }
      std::swap(a, b);
    }
    kl::jac_to_bytes<C>(st, group, a, nsets, d_out);
  }
  // the same sum left in Jacobian form at d_jac (multi-device key sums exchange projective partials, SURVEY 8e);
  // n == 0 gives the point at infinity (all-zero record: Z = 0)
  // d_bytes != nullptr: the caller wants the affine wire bytes as well; where the one-launch tree (k_sumtree.hip) serves the
  // sum it writes them itself and *bytes_done is set (no separate conversion launch)
  static int sum_points_jac(Ctx& c, hipStream_t st, int group, const uint8_t* d_pts, size_t n, void* d_jac, uint32_t* d_flags,
                            int src = 0, bool own_scope = true, uint8_t* d_bytes = nullptr, bool* bytes_done = nullptr) {
    if (n == 0) {
      HIPCHK(hipMemsetAsync(d_jac, 0, kl::jac_bytes<C>(group), st));
      return 0;
    }
    // main pass: at most two waves per SIMD (2048 waves), at least ~4 points per lane; then the per-thread partials
    // are folded 64 at a time
    size_t waves = (n + 255) / 256;
    if (waves > 2048) waves = 2048;
    const bool pairs = group == BGLS_G2 && sum_pairs();
    if (pairs) {                      // one running sum per lane pair, >= ~4 keys per pair;
      waves = (n + 127) / 128;        // a block (one wave) adds its 32 sums itself and leaves ONE partial
      // Waves of the main pass (round 6, re-measured through bench.py at 2^20 keys, wire bytes / key set).  A check with the machine to itself:
      // two per SIMD -- main pass 0.46 / 0.36 ms at 2048 waves, 0.48 / 0.37 at 3072 (the cap of rounds 4-5), 0.50 / 0.38 at 1792, 0.52 / 0.37 at
      // 1024.  Several checks in flight (throughput mode): ONE per SIMD -- a main pass that fills every wave slot keeps the other checks'
      // latency-bound tails (tree, hash, two-pairing Miller, final exponentiation) waiting for its last wave; at one wave per SIMD three
      // main passes and the tails share the machine: 1.75 / 2.10 G signers/s at 1024 against 1.66 / 1.98 at 2048 and 1.51 / 1.76 at 3072.
      const size_t cap = throughput_mode() ? 1024 : 2048;
      if (waves > cap) waves = cap;
    }
    const size_t partials = pairs ? waves : waves * 64;
    void *ja, *jb;
    int rc;
    std::optional<Scope> sc;
    if (own_scope) sc.emplace(c, st, ST_SUM);
    const size_t JB = kl::jac_bytes<C>(group);
    if ((rc = c.get(WS_JAC_A, (partials + 1) * JB, &ja))) return rc;
    if ((rc = c.get(WS_JAC_B, (partials / 2 + 2) * JB, &jb))) return rc;
    std::optional<Scope> scm;
    scm.emplace(c, st, ST_SUM_MAIN);
    if (src == 2 && !pairs) return fail(BGLS_ERR_ARG, "sum-ready records need the lane-pair key-sum kernel");
    if (pairs) kl::sumpair_main<C>(st, src, d_pts, n, (unsigned)(waves * 32), ja, d_flags);                                     // lane pairs, carry-free limbs (rx_jacpair.hpp)
    else kl::sum_main<C>(st, group, src == 1, d_pts, n, (unsigned)waves, ja, d_flags);
    scm.reset();
    void *a = ja, *b = jb;
    size_t cnt = partials;
    const bool one_launch_tree = !legacy(LG_TREE);
    while (cnt > 1) {
      if (group == BGLS_G2 && cnt <= 8192 && one_launch_tree) {
        // the whole tree in ONE launch: a wave per pair of leaves climbs by tickets (k_sumtree.hip); the root's wave writes the
        // Jacobian record and, if asked, the affine bytes
        void *store, *tick;
        if ((rc = c.get(WS_TREE_S, std::max((cnt + 64) * JB, kl::sum_tree_store_bytes<C>(cnt)), &store))) return rc;
        if ((rc = c.get(WS_TREE_T, (size_t)(8192 + 64) * 4, &tick))) return rc;
        // The tickets of THIS tree are zeroed in front of every launch (cnt + 64 words: the levels' offsets sum below cnt + 64).  The
        // kernel also leaves them at zero, but a launch that was aborted -- or a second sum submitted on the same context through a
        // user stream while the first was in flight -- would leave ones behind, every later tree would then take its waves for
        // "first arrivals", the root would never be written and a STALE key sum would be verified against.
        HIPCHK(hipMemsetAsync(tick, 0, (cnt + 64) * 4, st));
        kl::sum_tree<C>(st, a, cnt, store, (uint32_t*)tick, d_bytes, d_jac);
        HIPCHK(hipGetLastError());
        if (bytes_done) *bytes_done = d_bytes != nullptr;
        return 0;
      }
      // halving launches while there is parallelism to speak of, then 64 -> 1 per wave with lane shuffles
      if (group == BGLS_G2 && cnt <= 8192) {
        kl::sum_coop<C>(st, a, cnt, b);                    // few additions left: one wave per addition, ~12 us a level
        cnt = (cnt + 1) / 2;
      } else if (cnt > 4096) {
        kl::sum_pair<C>(st, group, a, cnt, b);
        cnt = (cnt + 1) / 2;
      } else {
        kl::sum_wave<C>(st, group, a, cnt, b);
        cnt = (cnt + 63) / 64;
      }
      void* t = a;
      a = b;
      b = t;
    }
    HIPCHK(hipMemcpyAsync(d_jac, a, JB, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipGetLastError());
    return 0;
  }
};

