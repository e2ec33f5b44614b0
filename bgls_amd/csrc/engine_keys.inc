// Host side, part 3 of 4 (included by engine.hip): resident key sets (bgls_keys_t), their shards on one or several devices, the RCCL /
// peer-copy exchange of partial products, and the verifications against a key set.
// ======================================================================= key sets and multi-device verification
// RCCL is loaded at run time (dlopen) so that the library has no link-time dependency on it: the exchange of the
// per-device partials falls back to peer copies whenever RCCL is missing, a device id repeats, or a call fails.
struct Rccl {
  void* so = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  bool ok = false;
  Rccl() {
    if (const char* e = getenv("BGLS_NO_RCCL")) { if (e[0] == '1') return; }
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      so = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (so) break;
    }
    if (!so) return;
    CommInitAll = (decltype(CommInitAll))dlsym(so, "ncclCommInitAll");
    CommDestroy = (decltype(CommDestroy))dlsym(so, "ncclCommDestroy");
    AllGather = (decltype(AllGather))dlsym(so, "ncclAllGather");
    GroupStart = (decltype(GroupStart))dlsym(so, "ncclGroupStart");
    GroupEnd = (decltype(GroupEnd))dlsym(so, "ncclGroupEnd");
    ok = CommInitAll && CommDestroy && AllGather && GroupStart && GroupEnd;
  }
};
Rccl& rccl() {
  static Rccl r;
  return r;
}

struct KeyShard {
  int device = 0;
  size_t lo = 0, hi = 0;
  void* d_wire = nullptr;    // (hi - lo) wire-format keys
  void* d_mont = nullptr;    // the same keys as Aff<F2<C>> (Montgomery form): prepared lines, weighted sums, the one-lane key sums
  void* d_sumr = nullptr;    // the same keys as sum-ready records (k_g2_sumready): what the lane-pair key sum reads
  void* d_rec = nullptr;     // this shard's exchange record: GT partial + status word (send buffer)
  void* d_all = nullptr;     // every shard's record (receive buffer)
  // prepared sets (BGLS_KEYS_PREPARE, prepared.hpp): normalised line ratios of every key and step, [step][n_pad] rows
  void* d_prep = nullptr;
  void* d_kinf = nullptr;    // n_pad bytes: 1 = key at infinity / padding
  size_t n_pad = 0;          // hi - lo rounded up to whole waves of the fold (10 groups x ng pairings)
  int ng = 0;                // pairings per group and squaring (prep_ng)
};
struct KeySet {
  int curve = 0;
  size_t n = 0;
  std::vector<KeyShard> shards;
  bool prepared = false;
  std::vector<ncclComm_t> comms;     // one per shard when the RCCL exchange is usable, else empty
  std::mutex mu;                     // one verification at a time per key set (the shards' buffers are part of it)
  int base_ctx = 0;                  // context of shard 0 in the verification in flight (the caller's bgls_select_context)
  void* d_total = nullptr;           // one-shard sets: the sum of ALL keys as one sum-ready record (keyset_total: made by the first subset call)
  ~KeySet() {
    for (auto cm : comms) if (cm) (void)rccl().CommDestroy(cm);
    for (auto& sh : shards) {
      if (hipSetDevice(sh.device) != hipSuccess) continue;
      for (void* q : {sh.d_wire, sh.d_mont, sh.d_sumr, sh.d_rec, sh.d_all, sh.d_prep, sh.d_kinf}) if (q) (void)hipFree(q);
    }
    if (d_total && !shards.empty() && hipSetDevice(shards[0].device) == hipSuccess) (void)hipFree(d_total);
  }
};
std::mutex g_keys_mu;
std::unordered_map<uint64_t, std::shared_ptr<KeySet>> g_keys;
uint64_t g_keys_next = 1;
thread_local int g_last_exchange = 0;

std::shared_ptr<KeySet> keyset(bgls_keys_t h) {
  std::lock_guard<std::mutex> lk(g_keys_mu);
  auto it = g_keys.find(h);
  return it == g_keys.end() ? nullptr : it->second;
}

constexpr size_t REC_PAD = 16;     // status word + padding behind the GT bytes of an exchange record
// Prepared sets: pairings per group and squaring (NG) of the fold, chosen at upload so that the whole set is ONE round of resident waves --
// round 6: a 2^20-key alt-bn128 set at NG = 38 is 2 760 waves on 2 816 wave slots, all resident from the first clock, and the accumulator is squared
// once per 38 lines instead of 24 (rounds 2-5: NG = 6 / 12 / 24 by size).  The set is padded to whole waves
// of 10 groups x NG pairings (padding keys are lines of 1).
constexpr int PREP_CUS = 256;
template <class C>
inline int prep_ng(size_t cnt) {
  // k_fold_prep (prepared.hpp): eleven waves per CU on alt-bn128 (13.3 KB of LDS per wave are handed out in 2 KB steps: measured, a lone 2^20-key
  // launch takes 31.5 ms cut for eleven and 37.2 ms cut for twelve), eight on BLS12-381 (two waves per SIMD)
  const size_t slots = (size_t)PREP_CUS * (C::CURVE_ID == 0 ? 11 : 8);
  size_t ng = (cnt + 10 * slots - 1) / (10 * slots);
  if (ng < 6) ng = 6;
  if (ng > 96) ng = 96;                                                         // beyond 96 x 30 720 keys per device: several rounds
  return (int)ng;
}
// bgls_set_prepare_shape: NG forced for the key sets uploaded afterwards (0 = prep_ng) and the keys per k_prepare launch (0 = 2^17), packed
// as {ng, chunk} so that an upload reads both from one setting.  The results do not depend on it (tests and A/B runs).
constexpr int PREP_NG_MIN = 6, PREP_NG_MAX = 96;                                 // what prep_ng can return
constexpr size_t PREP_CHUNK = (size_t)1 << 17;
struct PrepShape { size_t ng = 0, chunk = 0; };
std::mutex g_prep_shape_mu;
PrepShape g_prep_shape;

// compressed: `keys` holds Point.Marshal encodings (E::G2B / 2 bytes each); each shard decodes its range with the one-pass kernel of
// k_wirex.hip, which validates every key and writes d_wire and d_mont itself (bgls_keys_upload_compressed).  *first_bad: the smallest
// refused index -- the shards are walked in index order and the walk stops at the first that refuses a key.
template <class C>
int keys_upload_t(const uint8_t* keys, size_t n, const int* devices, int n_devices, unsigned flags, bgls_keys_t* out, bool compressed = false,
                  size_t* first_bad = nullptr) {
  typedef Engine<C> E;
  if (n >= MAX_BATCH) return fail(BGLS_ERR_ARG, "key set too large (n must be below 2^30)");
  auto ks = std::make_shared<KeySet>();
  ks->curve = C::CURVE_ID;
  ks->n = n;
  ks->prepared = (flags & BGLS_KEYS_PREPARE) != 0;
  const size_t REC = E::GTB + REC_PAD;
  PrepShape shape;                       // read once: every shard of this set is prepared under the same setting
  {
    std::lock_guard<std::mutex> lk(g_prep_shape_mu);
    shape = g_prep_shape;
  }
  bool distinct = true;
  for (int s = 0; s < n_devices; ++s) {
    KeyShard sh;
    sh.device = devices ? devices[s] : s;
    if (sh.device < 0 || sh.device >= MAX_DEVICES) return fail(BGLS_ERR_NO_DEVICE, "device index out of range");
    for (int t = 0; t < s; ++t) distinct = distinct && ks->shards[t].device != sh.device;
    sh.lo = n * (size_t)s / n_devices;
    sh.hi = n * (size_t)(s + 1) / n_devices;
    ks->shards.push_back(sh);
  }
  SelectionGuard keep_selection;
  int rc = 0;
  for (int s = 0; s < n_devices && rc == 0; ++s) {
    KeyShard& sh = ks->shards[s];
    const size_t cnt = sh.hi - sh.lo;
    g_dev = sh.device;
    g_sel = 0;
    Ctx& c = ctx();
    std::lock_guard<std::mutex> lk(c.mu);
    rc = [&]() -> int {
      int r;
      if ((r = c.enter())) return r;
      HIPCHK(hipMalloc(&sh.d_wire, cnt ? cnt * E::G2B : 16));
      HIPCHK(hipMalloc(&sh.d_mont, cnt ? cnt * kl::g2_parsed_bytes<C>() : 16));
      HIPCHK(hipMalloc(&sh.d_sumr, cnt ? cnt * kl::g2_sumready_bytes<C>() : 16));
      HIPCHK(hipMalloc(&sh.d_rec, REC));
      HIPCHK(hipMalloc(&sh.d_all, REC * n_devices));
      void* d_flags;
      if ((r = c.get(WS_FLAGS, 16, &d_flags))) return r;
      HIPCHK(hipMemsetAsync(d_flags, 0, 4, c.stream));
      uint32_t* d_bad = (uint32_t*)d_flags + 1;             // compressed: the smallest refused index of this shard (atomicMin)
      if (cnt && compressed) {
        const size_t CB = E::G2B / 2;
        void* d_comp;
        if ((r = c.get(WS_IN_B, cnt * CB, &d_comp))) return r;
        HIPCHK(hipMemsetAsync(d_bad, 0xFF, 4, c.stream));
        HIPCHK(hipMemcpyAsync(d_comp, keys + sh.lo * CB, cnt * CB, hipMemcpyHostToDevice, c.stream));
        kl::wirex_decode<C>(c.stream, BGLS_G2, (const uint8_t*)d_comp, cnt, (uint8_t*)sh.d_wire, nullptr, sh.d_mont, d_bad);
        kl::g2_sumready<C>(c.stream, sh.d_mont, cnt, sh.d_sumr);
        HIPCHK(hipGetLastError());
      } else if (cnt) {
        HIPCHK(hipMemcpyAsync(sh.d_wire, keys + sh.lo * E::G2B, cnt * E::G2B, hipMemcpyHostToDevice, c.stream));
        kl::g2_parse<C>(c.stream, (const uint8_t*)sh.d_wire, cnt, (flags & BGLS_KEYS_CHECK) ? 1 : 0, sh.d_mont, (uint32_t*)d_flags);
        kl::g2_sumready<C>(c.stream, sh.d_mont, cnt, sh.d_sumr);
        HIPCHK(hipGetLastError());
      }
      uint32_t f = 0, bad = 0xFFFFFFFFu;
      HIPCHK(hipMemcpyAsync(&f, d_flags, 4, hipMemcpyDeviceToHost, c.stream));
      if (cnt && compressed) HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c.stream));
      HIPCHK(hipStreamSynchronize(c.stream));
      if (bad != 0xFFFFFFFFu) {
        if (first_bad) *first_bad = sh.lo + bad;
        return fail(BGLS_ERR_ENCODING, "key set: a compressed key was refused (encoding, not on the twist, or outside the order-r subgroup)");
      }
      if (f & FLAG_ENC) return fail(BGLS_ERR_ENCODING, "key set: non-canonical coordinate or key not on the twist");
      if (f & FLAG_SUBGROUP) return fail(BGLS_ERR_ENCODING, "key set: key outside the order-r subgroup");
      if (flags & BGLS_KEYS_PREPARE) {
        // line ratios of every key (k_prepare), in chunks so that the scratch stays a few GB
        const kl::PrepSizes ps = kl::prep_sizes<C>();
        sh.ng = shape.ng ? (int)shape.ng : prep_ng<C>(cnt);
        const size_t pad = (size_t)10 * sh.ng;
        sh.n_pad = (cnt + pad - 1) / pad * pad;
        if (sh.n_pad == 0) sh.n_pad = pad;
        HIPCHK(hipMalloc(&sh.d_prep, sh.n_pad * ps.line_bytes_per_key));
        HIPCHK(hipMalloc(&sh.d_kinf, sh.n_pad));
        const size_t chunk = shape.chunk ? shape.chunk : PREP_CHUNK;
        void* tmp = nullptr;
        HIPCHK(hipMalloc(&tmp, (sh.n_pad < chunk ? sh.n_pad : chunk) * ps.tmp_bytes_per_key));
        HIPCHK(hipMemsetAsync(d_flags, 0, 4, c.stream));
        for (size_t i0 = 0; i0 < sh.n_pad; i0 += chunk) {
          const size_t count = sh.n_pad - i0 < chunk ? sh.n_pad - i0 : chunk;
          kl::prepare_keys<C>(c.stream, sh.d_mont, cnt, sh.n_pad, i0, count, (uint32_t*)sh.d_prep, (uint8_t*)sh.d_kinf, (uint32_t*)tmp, (uint32_t*)d_flags);
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&f, d_flags, 4, hipMemcpyDeviceToHost, c.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
        (void)hipFree(tmp);
        if (e != hipSuccess) return fail(BGLS_ERR_HIP, "preparing the key set", e);
        if (f & FLAG_DEGENERATE) return fail(BGLS_ERR_ENCODING, "key set: a key has a degenerate Miller step and cannot be prepared (upload it without BGLS_KEYS_PREPARE)");
      }
      return 0;
    }();
  }
  if (rc) return rc;                  // ~KeySet frees what was allocated
  if (n_devices > 1 && distinct && rccl().ok) {
    std::vector<int> devs;
    for (auto& sh : ks->shards) devs.push_back(sh.device);
    ks->comms.assign(n_devices, nullptr);
    if (rccl().CommInitAll(ks->comms.data(), n_devices, devs.data()) != ncclSuccess) ks->comms.clear();
  }
  std::lock_guard<std::mutex> lk(g_keys_mu);
  const uint64_t h = g_keys_next++;
  g_keys[h] = ks;
  *out = h;
  return 0;
}

// Gather every shard's exchange record on shard 0 (sh[0].d_all, shard order).  Each shard's record is complete on its
// context-`s` stream.  RCCL: one all-gather enqueued on every device's stream; else peer / device copies.
template <class C>
int exchange_records(KeySet& ks) {
  typedef Engine<C> E;
  const size_t REC = E::GTB + REC_PAD;
  const int S = (int)ks.shards.size();
  g_last_exchange = S > 1 ? 1 : 0;
  if (!ks.comms.empty()) {
    bool good = rccl().GroupStart() == ncclSuccess;
    for (int s = 0; s < S && good; ++s) {
      KeyShard& sh = ks.shards[s];
      good = hipSetDevice(sh.device) == hipSuccess &&
             rccl().AllGather(sh.d_rec, sh.d_all, REC, ncclUint8, ks.comms[s], ctx_of(sh.device, (ks.base_ctx + s) % NCTX).stream) == ncclSuccess;
    }
    good = (rccl().GroupEnd() == ncclSuccess) && good;
    if (good) {
      g_last_exchange = 2;
      return 0;
    }
  }
  KeyShard& root = ks.shards[0];
  for (int s = 0; s < S; ++s) {
    KeyShard& sh = ks.shards[s];
    hipStream_t st = ctx_of(sh.device, (ks.base_ctx + s) % NCTX).stream;
    HIPCHK(hipSetDevice(sh.device));
    uint8_t* dst = (uint8_t*)root.d_all + (size_t)s * REC;
    if (sh.device == root.device) HIPCHK(hipMemcpyAsync(dst, sh.d_rec, REC, hipMemcpyDeviceToDevice, st));
    else HIPCHK(hipMemcpyPeerAsync(dst, root.device, sh.d_rec, sh.device, REC, st));
    if (s) HIPCHK(hipStreamSynchronize(st));         // shard 0 continues on its own stream
  }
  return 0;
}

// runs fn(shard index) on one host thread per shard, each bound to its shard's device and to context `s`
template <class Fn>
int for_each_shard(KeySet& ks, Fn&& fn) {
  const int S = (int)ks.shards.size();
  std::vector<int> rcs(S, 0);
  std::vector<std::string> errs(S);
  const int base = g_sel;                 // the context the caller selected (bgls_select_context): shard s takes (base + s) mod NCTX,
  ks.base_ctx = base;                     // so a one-shard key set runs on the caller's context and threads on distinct contexts do not serialise
  auto body = [&](int s) noexcept {        // runs on a thread of its own: nothing may leave it
    g_dev = ks.shards[s].device;
    g_sel = (base + s) % NCTX;
    try {
      rcs[s] = fn(s);
    } catch (...) {
      rcs[s] = abi_catch();
    }
    try {
      if (rcs[s] < 0) errs[s] = g_err;
    } catch (...) {}
  };
  if (S == 1) {
    SelectionGuard keep_selection;
    body(0);
  } else {
    std::vector<std::thread> th;
    th.reserve(S);
    int started = 0;
    try {
      for (; started < S; ++started) th.emplace_back(body, started);
    } catch (...) {                        // a thread could not be created: the shards without one fail, the others are joined below
      for (int s = started; s < S; ++s) {
        rcs[s] = fail(BGLS_ERR_NOMEM, "could not start a shard's host thread");       // a resource failure (advice r5), and its message must survive the loop below
        try { errs[s] = g_err; } catch (...) {}
      }
    }
    for (auto& t : th) t.join();
  }
  for (int s = 0; s < S; ++s)
    if (rcs[s] < 0) {
      if (!errs[s].empty()) g_err = errs[s];
      return rcs[s];
    }
  return 0;
}

int merged_flags_rc(uint32_t f) {
  if (f & FLAG_ENC) return fail(BGLS_ERR_ENCODING, "non-canonical coordinate or point not on curve");
  if (f & FLAG_SUBGROUP) return fail(BGLS_ERR_ENCODING, "point outside the order-r subgroup");
  if (f & FLAG_DEGENERATE) return fail(BGLS_ERR_ENCODING, "degenerate point step (small-order key)");
  if (f & FLAG_HASH) return fail(BGLS_ERR_HASH, "try-and-increment exhausted");
  return 0;
}

// distinct (bgls_verify_aggregate_distinct_h): message i is hashed behind key i's wire bytes, which every shard takes from its own d_wire
// (Engine::key_msgs); there is no duplicate rule, so every shard, shard 0 included, uploads its own range of messages only.
template <class C>
int verify_aggregate_h_t(KeySet& ks, const uint8_t* sig, const uint8_t* blob, const uint64_t* off, size_t n, int allow_dups, uint8_t* gt_out,
                         bool distinct = false) {
  typedef Engine<C> E;
  if (n != ks.n) return fail(BGLS_ERR_ARG, "message count differs from the key set's size");
  if (int bad = offsets_ok("msg_off", off, n, 0)) return bad;
  std::lock_guard<std::mutex> lk_set(ks.mu);
  const size_t REC = E::GTB + REC_PAD;
  const int S = (int)ks.shards.size();
  int rc = for_each_shard(ks, [&](int s) -> int {
    KeyShard& sh = ks.shards[s];
    Ctx& c = ctx();
    std::lock_guard<std::mutex> lk(c.mu);
    int r;
    if ((r = c.enter())) return r;
    hipStream_t st = c.stream;
    const size_t cnt = sh.hi - sh.lo;
    // shard 0 holds ALL messages: the duplicate rule is a property of the whole list (two equal messages may sit in
    // different shards); the other shards upload their own range only
    const size_t mlo = s == 0 && !distinct ? 0 : sh.lo, mhi = s == 0 && !distinct ? n : sh.hi;
    const size_t bytes = off[mhi] - off[mlo];
    void *d_sig, *d_blob, *d_off, *d_flags;
    if ((r = c.get(WS_IN_A, E::G1B, &d_sig))) return r;
    if ((r = c.get(WS_FLAGS, 16, &d_flags))) return r;
    HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
    if (s == 0) HIPCHK(hipMemcpyAsync(d_sig, sig, E::G1B, hipMemcpyHostToDevice, st));
    MsgView mine;
    if (distinct) {
      Keyed keyed;
      if ((r = upload_keyed_msgs(c, st, BGLS_KEYED_PREFIX, blob, off, mlo, mhi, &mine, &keyed))) return r;
      if ((r = E::key_msgs(c, st, keyed.mode, (const uint8_t*)sh.d_wire, mine, keyed.msg_bytes, cnt, (uint32_t*)d_flags, &mine))) return r;
    } else {
      if ((r = c.get(WS_IN_C, bytes, &d_blob))) return r;
      if ((r = c.get(WS_IN_D, (mhi - mlo + 1) * 8, &d_off))) return r;
      if (bytes) HIPCHK(hipMemcpyAsync(d_blob, blob + off[mlo], bytes, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_off, off + mlo, (mhi - mlo + 1) * 8, hipMemcpyHostToDevice, st));
      // offsets keep their global values: the view's base is shifted instead (never dereferenced below d_blob)
      MsgView all = {(const uint8_t*)d_blob - off[mlo], (const uint64_t*)d_off, 0, 0};
      if (s == 0 && !allow_dups && (r = E::dup_scan(c, st, all, n, (uint32_t*)d_flags))) return r;
      mine = all;
      if (s == 0) mine.off = (const uint64_t*)d_off + sh.lo;      // sh.lo == 0; kept for clarity
    }
    if (ks.prepared) {
      if ((r = E::miller_product_prepared(c, st, s == 0 ? (const uint8_t*)d_sig : nullptr, (const uint32_t*)sh.d_prep, (const uint8_t*)sh.d_kinf, sh.n_pad, sh.ng,
                                          mine, cnt, (uint8_t*)sh.d_rec, (uint32_t*)d_flags)))
        return r;
    } else if ((r = E::miller_product(c, st, s == 0 ? (const uint8_t*)d_sig : nullptr, (const uint8_t*)sh.d_wire, mine, cnt, 0,
                                      (uint8_t*)sh.d_rec, (uint32_t*)d_flags)))
      return r;
    HIPCHK(hipMemcpyAsync((uint8_t*)sh.d_rec + E::GTB, d_flags, 4, hipMemcpyDeviceToDevice, st));
    if (s) HIPCHK(hipStreamSynchronize(st));       // record complete before the exchange reads it (shard 0: stream order)
    return 0;
  });
  if (rc) return rc;
  if ((rc = exchange_records<C>(ks))) return rc;
  // shard 0: product of the S partials, one final exponentiation, compare with 1; status words OR-ed on the host
  KeyShard& root = ks.shards[0];
  SelectionGuard keep_selection;
  g_dev = root.device;
  g_sel = ks.base_ctx % NCTX;             // shard 0's context
  Ctx& c = ctx();
  std::lock_guard<std::mutex> lk(c.mu);
  rc = [&]() -> int {
    int r;
    if ((r = c.enter())) return r;
    void* d_parts;
    if ((r = c.get(WS_HAE_KEYS, (size_t)S * E::GTB, &d_parts))) return r;
    std::vector<uint8_t> recs((size_t)S * REC);
    HIPCHK(hipMemcpyAsync(recs.data(), root.d_all, recs.size(), hipMemcpyDeviceToHost, c.stream));
    for (int s = 0; s < S; ++s)
      HIPCHK(hipMemcpyAsync((uint8_t*)d_parts + (size_t)s * E::GTB, (uint8_t*)root.d_all + (size_t)s * REC, E::GTB, hipMemcpyDeviceToDevice, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    uint32_t f = 0;
    for (int s = 0; s < S; ++s) {
      uint32_t w;
      memcpy(&w, recs.data() + (size_t)s * REC + E::GTB, 4);
      f |= w;
    }
    if ((r = merged_flags_rc(f))) return r;
    r = E::finalize(c, c.stream, (const uint8_t*)d_parts, (size_t)S, 1, nullptr, gt_out);
    if (r < 0) return r;
    return (f & FLAG_DUP) ? 0 : r;
  }();
  return rc;
}

template <class C>
int verify_multi_h_t(KeySet& ks, const uint8_t* sig, const uint8_t* msg, size_t msg_len) {
  typedef Engine<C> E;
  std::lock_guard<std::mutex> lk_set(ks.mu);
  const int S = (int)ks.shards.size();
  const size_t JB = kl::jac_bytes<C>(BGLS_G2);
  const size_t REC = E::GTB + REC_PAD;
  static_assert(E::GTB >= 3 * 2 * C::L * 4, "a projective G2 partial fits an exchange record");
  // per-device partial key sums (projective): the exchange record carries the Jacobian point instead of a GT partial
  int rc = for_each_shard(ks, [&](int s) -> int {
    KeyShard& sh = ks.shards[s];
    Ctx& c = ctx();
    std::lock_guard<std::mutex> lk(c.mu);
    int r;
    if ((r = c.enter())) return r;
    void* d_flags;
    if ((r = c.get(WS_FLAGS, 16, &d_flags))) return r;
    HIPCHK(hipMemsetAsync(d_flags, 0, 4, c.stream));
    HIPCHK(hipMemsetAsync(sh.d_rec, 0, REC, c.stream));
    const bool ready = sum_pairs();       // the lane-pair kernel reads the sum-ready records, the others the Montgomery points
    if ((r = E::sum_points_jac(c, c.stream, BGLS_G2, (const uint8_t*)(ready ? sh.d_sumr : sh.d_mont), sh.hi - sh.lo, sh.d_rec, (uint32_t*)d_flags, ready ? 2 : 1))) return r;
    if (s) HIPCHK(hipStreamSynchronize(c.stream));
    return 0;
  });
  if (rc) return rc;
  if ((rc = exchange_records<C>(ks))) return rc;
  KeyShard& root = ks.shards[0];
  SelectionGuard keep_selection;
  g_dev = root.device;
  g_sel = ks.base_ctx % NCTX;
  Ctx& c = ctx();
  std::lock_guard<std::mutex> lk(c.mu);
  rc = [&]() -> int {
    int r;
    if ((r = c.enter())) return r;
    hipStream_t st = c.stream;
    void *d_jacs, *d_tmp, *d_apk, *d_sig, *d_msg;
    if ((r = c.get(WS_JAC_A, (size_t)(S + 64) * JB, &d_jacs))) return r;
    if ((r = c.get(WS_JAC_B, 4 * JB, &d_tmp))) return r;
    if ((r = c.get(WS_HAE_APK, E::G2B, &d_apk))) return r;
    if ((r = c.get(WS_IN_A, E::G1B, &d_sig))) return r;
    if ((r = c.get(WS_IN_C, msg_len, &d_msg))) return r;
    for (int s = 0; s < S; ++s)
      HIPCHK(hipMemcpyAsync((uint8_t*)d_jacs + (size_t)s * JB, (uint8_t*)root.d_all + (size_t)s * REC, JB, hipMemcpyDeviceToDevice, st));
    void* cur = d_jacs;
    if (S > 1) {
      kl::sum_wave<C>(st, BGLS_G2, d_jacs, (size_t)S, d_tmp);       // S <= 16 partials: one wave
      cur = d_tmp;
    }
    kl::jac_to_bytes<C>(st, BGLS_G2, cur, 1, (uint8_t*)d_apk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d_sig, sig, E::G1B, hipMemcpyHostToDevice, st));
    if (msg_len) HIPCHK(hipMemcpyAsync(d_msg, msg, msg_len, hipMemcpyHostToDevice, st));
    return verify_multi_dev_t<C>(c, st, (const uint8_t*)d_sig, (const uint8_t*)d_apk, 1, (const uint8_t*)d_msg, msg_len);
  }();
  return rc;
}

// ---- multi-signatures by signer bitmap against a one-shard key set (bgls_verify_multi_subsets_h / _keys_dev, bgls_aggregate_subsets_h) ----
// bgls_set_subset_complement: 0 = per set (the shorter side of the row), 1 = never, 2 = always.  The sums do not depend on it.
std::atomic<int> g_subset_complement{0};

// What a subset call must find before any device work: a one-shard set, the lane-pair key sum (the only reader of sum-ready records), a
// row stride that covers the set, and a batch within the bounds of one main-pass launch (those of Engine::sum_sets).
template <class C>
int subsets_args_ok(const KeySet& ks, size_t stride, size_t n_sets) {
  if (ks.shards.size() != 1) return fail(BGLS_ERR_ARG, "subset entry point: the key set must live on one device");
  if (!sum_pairs()) return fail(BGLS_ERR_ARG, "subset entry point: needs the lane-pair key sum (BGLS_LEGACY bit 8 is set)");
  if (stride < (ks.n + 7) / 8) return fail(BGLS_ERR_ARG, "bitmap stride is shorter than ceil(n / 8) bytes");
  if (n_sets >= MAX_BATCH) return too_large();
  const size_t blocks = n_sets * (sumsel_pairs_per_set(ks.n, n_sets) / 32);
  if (blocks > ((size_t)1 << 30) || (blocks + 1) * kl::jac_bytes<C>(BGLS_G2) > ((size_t)8 << 30))
    return fail(BGLS_ERR_ARG, "too many key sets for one call (cut the batch: at most 2^30 blocks / 8 GiB of partial sums)");
  return 0;
}

// a host row has no bit at a position >= n, anywhere in its `stride` bytes
bool subset_rows_clean(const uint8_t* bitmaps, size_t stride, size_t n_sets, size_t n) {
  const size_t full = n / 8;
  for (size_t b = 0; b < n_sets; ++b) {
    const uint8_t* row = bitmaps + b * stride;
    if (full < stride && (n & 7) && (row[full] >> (n & 7))) return false;
    for (size_t i = (n + 7) / 8; i < stride; ++i)
      if (row[i]) return false;
  }
  return true;
}

// The whole-set sum of a one-shard key set as ONE sum-ready record: Engine::sum_points over the resident records, the wire bytes parsed and
// converted like a key at upload.  Made once, by the first subset call, under the set's mutex; it belongs to the key set (freed with it,
// not a workspace).  Runs on the calling thread's context of the set's device.
template <class C>
int keyset_total(KeySet& ks) {
  typedef Engine<C> E;
  std::lock_guard<std::mutex> lk_set(ks.mu);
  if (ks.d_total) return 0;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const KeyShard& sh = ks.shards[0];
  const size_t rec = (kl::g2_sumready_bytes<C>() + 15) & ~(size_t)15, mont = (kl::g2_parsed_bytes<C>() + 15) & ~(size_t)15;
  void *buf = nullptr, *d_flags;
  int rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMalloc(&buf, rec + mont + E::G2B));
  uint8_t* d_rec = (uint8_t*)buf;
  uint8_t* d_mont = d_rec + rec;
  uint8_t* d_wire = d_mont + mont;
  rc = [&]() -> int {
    int r;
    HIPCHK(hipMemsetAsync(d_flags, 0, 4, k.st));
    if ((r = E::sum_points(c, k.st, BGLS_G2, (const uint8_t*)sh.d_sumr, ks.n, d_wire, (uint32_t*)d_flags, 2))) return r;
    kl::g2_parse<C>(k.st, d_wire, 1, 0, d_mont, (uint32_t*)d_flags);
    kl::g2_sumready<C>(k.st, d_mont, 1, d_rec);
    HIPCHK(hipGetLastError());
    return read_flags(c, k.st, d_flags, true);
  }();
  if (rc) {
    (void)hipStreamSynchronize(k.st);
    (void)hipFree(buf);
    return rc;
  }
  ks.d_total = buf;
  return 0;
}

// The n_sets key sums selected by the rows at d_rows (stride_w 32-bit words each) as wire bytes at d_out: the planning pass (popcount and
// mode per set in WS_SEG_OFF, FLAG_SUBSET_STRAY in d_flags), k_sumsel_main over the set's sum-ready records, then Engine::sum_sets_tree.
template <class C>
int sum_subsets(Ctx& c, hipStream_t st, const KeySet& ks, const uint32_t* d_rows, size_t stride_w, size_t n_sets, uint8_t* d_out, uint32_t* d_flags) {
  typedef Engine<C> E;
  if (n_sets == 0) return 0;
  const size_t P = sumsel_pairs_per_set(ks.n, n_sets), written = n_sets * (P / 32), JB = kl::jac_bytes<C>(BGLS_G2);
  void *ja, *jb, *plan;
  int rc;
  Scope sc(c, st, ST_SUM);
  if ((rc = c.get(WS_JAC_A, (written + 1) * JB, &ja))) return rc;
  if ((rc = c.get(WS_JAC_B, (written / 2 + 2) * JB, &jb))) return rc;
  if ((rc = c.get(WS_SEG_OFF, n_sets * 8, &plan))) return rc;
  {
    Scope scm(c, st, ST_SUM_MAIN);
    kl::sumsel_plan(st, d_rows, stride_w, ks.n, n_sets, g_subset_complement.load(), (uint32_t*)plan, d_flags);
    kl::sumsel_main<C>(st, (const uint8_t*)ks.shards[0].d_sumr, ks.n, d_rows, stride_w, (const uint32_t*)plan, (const uint8_t*)ks.d_total, n_sets, (unsigned)P, ja);
  }
  E::sum_sets_tree(st, BGLS_G2, ja, jb, P / 32, n_sets, d_out);
  HIPCHK(hipGetLastError());
  return 0;
}

// host rows (stride bytes each, checked) repacked to whole 32-bit words per row and staged in WS_IN_B; packed is the copy's source
template <class C>
int upload_subset_rows(Ctx& c, hipStream_t st, const KeySet& ks, const uint8_t* bitmaps, size_t stride, size_t n_sets, std::vector<uint32_t>& packed, void** d_rows,
                       size_t* stride_w) {
  const size_t nb = (ks.n + 7) / 8, sw = (ks.n + 31) / 32;
  packed.assign(n_sets * sw, 0u);
  for (size_t b = 0; b < n_sets && nb; ++b) memcpy((uint8_t*)packed.data() + b * sw * 4, bitmaps + b * stride, nb);
  *stride_w = sw;
  return c.put(st, WS_IN_B, packed.data(), packed.size() * 4, d_rows);
}

template <class C>
int aggregate_subsets_t(KeySet& ks, const uint8_t* bitmaps, size_t stride, size_t n_sets, uint8_t* out) {
  typedef Engine<C> E;
  int rc;
  SelectionGuard keep_selection;
  g_dev = ks.shards[0].device;
  if ((rc = keyset_total<C>(ks))) return rc;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  void *d_rows, *d_out, *d_flags;
  size_t sw;
  std::vector<uint32_t> packed;                           // alive until read_flags has synchronised
  Drain drain{k.st};
  if ((rc = c.get(WS_SEG_KEYS, (n_sets + 1) * E::G2B, &d_out))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, k.st));
  if ((rc = upload_subset_rows<C>(c, k.st, ks, bitmaps, stride, n_sets, packed, &d_rows, &sw))) return rc;
  if ((rc = sum_subsets<C>(c, k.st, ks, (const uint32_t*)d_rows, sw, n_sets, (uint8_t*)d_out, (uint32_t*)d_flags))) return rc;
  return read_flags(c, k.st, d_flags, true, out, d_out, n_sets * E::G2B);
}

template <class C>
int verify_multi_subsets_t(KeySet& ks, const uint8_t* sigs, const uint8_t* bitmaps, size_t stride, size_t n_sets, const uint8_t* blob, const uint64_t* off,
                           uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out) {
  typedef Engine<C> E;
  int rc;
  SelectionGuard keep_selection;
  g_dev = ks.shards[0].device;
  if ((rc = keyset_total<C>(ks))) return rc;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  MsgView mv;
  void *d_sigs, *d_rows;
  size_t sw;
  std::vector<uint32_t> packed;
  if ((rc = upload_msgs(c, k.st, blob, off, n_sets, &mv))) return rc;
  if ((rc = c.put(k.st, WS_IN_A, sigs, n_sets * E::G1B, &d_sigs))) return rc;
  if ((rc = upload_subset_rows<C>(c, k.st, ks, bitmaps, stride, n_sets, packed, &d_rows, &sw))) return rc;
  HIPCHK(hipStreamSynchronize(k.st));                     // packed may go out of scope on an error path below
  return verify_sets_run<C>(c, k.st, (const uint8_t*)d_sigs, n_sets, mv, verdicts, apk_out, gt_out, [&](uint8_t* d_apks, uint32_t* d_flags) {
    return sum_subsets<C>(c, k.st, ks, (const uint32_t*)d_rows, sw, n_sets, d_apks, d_flags);
  });
}

template <class C>
int verify_multi_subsets_dev_t(KeySet& ks, const void* d_sigs, const void* d_bitmaps, size_t stride, size_t n_sets, const void* d_msgs, size_t msg_len,
                               size_t msg_stride, uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out, void* stream) {
  int rc;
  SelectionGuard keep_selection;
  g_dev = ks.shards[0].device;
  if ((rc = keyset_total<C>(ks))) return rc;
  Call k(stream);
  if (k.rc) return k.rc;
  const MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return verify_sets_run<C>(k.c, k.st, (const uint8_t*)d_sigs, n_sets, mv, verdicts, apk_out, gt_out, [&](uint8_t* d_apks, uint32_t* d_flags) {
    return sum_subsets<C>(k.c, k.st, ks, (const uint32_t*)d_bitmaps, stride / 4, n_sets, d_apks, d_flags);
  });
}

// ---- grouped aggregate verification over a one-shard key set by signer bitmap (bgls_verify_aggregate_grouped_h / _keys_dev) ----
// bgls_set_group_small: groups of at most min(k, 128) keys are summed by one lane pair each (k_sumpairgrp_main); 0 = none.  The results do
// not depend on it.  Default 32, by measurement (DESIGN.md section 6): at groups of 1, 4 and 16 keys every threshold from 32 up runs the
// same kernels, at groups of 128 the serial chain of one lane pair loses to the block pass by 2x.
std::atomic<size_t> g_group_small{32};

// what the handle must be: a one-shard set, and the lane-pair key sum (the only reader of sum-ready records)
int grouped_keys_args_ok(const KeySet& ks) {
  if (ks.shards.size() != 1) return fail(BGLS_ERR_ARG, "grouped verification over a key set: the key set must live on one device");
  if (!sum_pairs()) return fail(BGLS_ERR_ARG, "grouped verification over a key set: needs the lane-pair key sum (BGLS_LEGACY bit 8 is set)");
  return 0;
}

// selected keys of a host row over n keys (its bytes below ceil(n / 8); the positions >= n are checked by subset_rows_clean)
size_t subset_row_popcount(const uint8_t* row, size_t n) {
  size_t k = 0;
  for (size_t i = 0; i < (n + 7) / 8; ++i) k += (size_t)__builtin_popcount(row[i]);
  return k;
}

// The selection pass (grpkeys.hpp; under ST_GROUP), the grouping of the k = n_msgs messages with the small / large plan, the key sums of
// the d groups from the set's sum-ready records -- key sel[idx[p]], or idx[p] where everybody signs (d_row == nullptr) -- and the
// sibling's tail: the product over the d (key sum, representative message) pairs and ONE final exponentiation.
// d_row: row_words 32-bit words, of which the first grpkeys_words(n) hold the keys; a bit at a position >= n or a popcount other than
// n_msgs fails the call here, whatever the host checked before.  The selection lives in WS_AMS_SIGNERS, which nothing else in this call
// touches: sel (n_msgs) | cnt (words) | rank (words + 1) | the scan's block sums; all of it is written before it is read.
template <class C>
int verify_aggregate_grouped_keys_run(Ctx& c, hipStream_t st, const KeySet& ks, const uint8_t* d_sig, const uint32_t* d_row, size_t row_words, MsgView mv,
                                      size_t msg_bytes, size_t n_msgs, size_t* n_groups, uint8_t* gt_out) {
  typedef Engine<C> E;
  if (c.res_pending) return in_flight();
  int rc;
  void *d_flags, *d_part, *d_none;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  if ((rc = c.get(WS_PART, E::GTB, &d_part))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  const uint32_t* sel = nullptr;
  if (d_row) {
    const size_t nw = grpkeys_words(ks.n), tiles = kl::scan_tiles(nw + 1);
    size_t w32 = 0;
    auto take = [](size_t& at, size_t words) { const size_t r = at; at += (words + 63) & ~(size_t)63; return r; };
    const size_t o_sel = take(w32, n_msgs), o_cnt = take(w32, nw), o_rank = take(w32, nw + 1), o_bsum = take(w32, tiles + 1);
    void* arena;
    if ((rc = c.get(WS_AMS_SIGNERS, w32 * 4, &arena))) return rc;
    uint32_t* u = (uint32_t*)arena;
    c.h_res[10] = c.h_res[11] = 0;
    {
      Scope sc(c, st, ST_GROUP);
      if (row_words) kl::sel_count(st, d_row, row_words, ks.n, u + o_cnt, (uint32_t*)d_flags);
      if (nw) {
        kl::scan_excl<uint32_t, uint32_t>(st, u + o_cnt, nw, u + o_bsum, u + o_rank);
        kl::sel_scatter(st, d_row, ks.n, u + o_rank, (uint32_t)n_msgs, u + o_sel);
      }
    }
    HIPCHK(hipGetLastError());
    if (nw) HIPCHK(hipMemcpyAsync(&c.h_res[10], u + o_rank + nw, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&c.h_res[11], d_flags, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (c.h_res[11] & FLAG_SUBSET_STRAY) return fail(BGLS_ERR_ARG, "a signer bitmap has a bit at a position beyond the key set");
    if (c.h_res[10] != n_msgs) return fail(BGLS_ERR_ARG, "the signer bitmap does not select as many keys as there are messages");
    sel = u + o_sel;
  } else if (n_msgs != ks.n) {
    return fail(BGLS_ERR_ARG, "message count differs from the key set's size");
  }
  typename E::Groups g;
  if ((rc = c.get(WS_SEG_KEYS, 16, &d_none))) return rc;
  const uint8_t* d_sums = (const uint8_t*)d_none;                // no signer: nothing of it is read
  if (n_msgs) {
    const uint32_t small = grpkeys_small(g_group_small.load());
    if ((rc = E::group_messages(c, st, mv, msg_bytes, n_msgs, nullptr, true, &g, small))) return rc;
    if ((rc = E::sum_groups(c, st, (const uint8_t*)ks.shards[0].d_sumr, g, &d_sums, (uint32_t*)d_flags, true, sel, small))) return rc;
    mv = g.reps;
  }
  if ((rc = E::miller_product(c, st, d_sig, d_sums, mv, g.d, 0, (uint8_t*)d_part, (uint32_t*)d_flags))) return rc;
  if (n_groups) *n_groups = g.d;
  return E::finalize(c, st, (const uint8_t*)d_part, 1, 1, (const uint32_t*)d_flags, gt_out);
}

// host form: the row (checked by the caller: no stray bit, popcount = n_msgs) repacked to whole 32-bit words and staged in WS_IN_B
template <class C>
int verify_aggregate_grouped_keys_t(KeySet& ks, const uint8_t* sig, const uint8_t* bitmap, const uint8_t* blob, const uint64_t* off, size_t n_msgs,
                                    size_t* n_groups, uint8_t* gt_out) {
  typedef Engine<C> E;
  SelectionGuard keep_selection;
  g_dev = ks.shards[0].device;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  int rc;
  MsgView mv;
  void *d_sig, *d_row = nullptr;
  const size_t nw = grpkeys_words(ks.n);
  std::vector<uint32_t> packed;                             // the source of an asynchronous copy: alive until the stream is drained
  Drain drain{k.st};
  if ((rc = upload_msgs(c, k.st, blob, off, n_msgs, &mv))) return rc;
  if ((rc = c.put(k.st, WS_IN_A, sig, E::G1B, &d_sig))) return rc;
  if (bitmap) {
    packed.assign(nw, 0u);
    if (nw) memcpy(packed.data(), bitmap, (ks.n + 7) / 8);
    if ((rc = c.put(k.st, WS_IN_B, packed.data(), nw * 4, &d_row))) return rc;
  }
  return verify_aggregate_grouped_keys_run<C>(c, k.st, ks, (const uint8_t*)d_sig, (const uint32_t*)d_row, nw, mv, n_msgs ? off[n_msgs] : 0, n_msgs, n_groups,
                                              gt_out);
}

template <class C>
int verify_aggregate_grouped_keys_dev_t(KeySet& ks, const void* d_sig, const void* d_bitmap, size_t bitmap_len, const void* d_msgs, size_t msg_len,
                                        size_t msg_stride, size_t n_msgs, size_t* n_groups, uint8_t* gt_out, void* stream) {
  SelectionGuard keep_selection;
  g_dev = ks.shards[0].device;
  Call k(stream);
  if (k.rc) return k.rc;
  const MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return verify_aggregate_grouped_keys_run<C>(k.c, k.st, ks, (const uint8_t*)d_sig, (const uint32_t*)d_bitmap, bitmap_len / 4, mv, n_msgs * msg_len, n_msgs,
                                              n_groups, gt_out);
}

// bgls_keys_read: the wire bytes of keys [first, first + count), each shard's part from its own d_wire
template <class C>
int keys_read_t(KeySet& ks, size_t first, size_t count, uint8_t* out) {
  typedef Engine<C> E;
  std::lock_guard<std::mutex> lk_set(ks.mu);
  SelectionGuard keep_selection;
  for (KeyShard& sh : ks.shards) {
    const size_t a = first > sh.lo ? first : sh.lo, b = first + count < sh.hi ? first + count : sh.hi;
    if (a >= b) continue;
    g_dev = sh.device;
    g_sel = 0;
    Ctx& c = ctx();
    std::lock_guard<std::mutex> lk(c.mu);
    int r;
    if ((r = c.enter())) return r;
    HIPCHK(hipMemcpyAsync(out + (a - first) * E::G2B, (const uint8_t*)sh.d_wire + (a - sh.lo) * E::G2B, (b - a) * E::G2B, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
  }
  return 0;
}

// bgls_decompress_points_dev: the one-pass kernel of k_wirex.hip over resident input; nothing is read back, nothing is awaited
template <class C>
int decompress_points_dev_t(int group, const void* d_in, size_t n, void* d_out, void* d_ok, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  kl::wirex_decode<C>(k.st, group, (const uint8_t*)d_in, n, (uint8_t*)d_out, (uint8_t*)d_ok, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  return 0;
}

bool group_ok(int g) { return g == BGLS_G1 || g == BGLS_G2; }

}  // namespace

