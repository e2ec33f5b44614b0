// Host side, part 2 of 4 (included by engine.hip): the per-call bodies behind the C ABI -- VerifyAggregateSignature / VerifyMultiSignature
// and their batch, device-buffer and weighted (multiplicity / HAE) forms, point operations, wire formats, key generation and signing.
int flags_to_rc(uint32_t f) {
  if (f & FLAG_SUBSET_STRAY) return fail(BGLS_ERR_ARG, "a signer bitmap has a bit at a position beyond the key set");
  if (f & FLAG_ENC) return fail(BGLS_ERR_ENCODING, "non-canonical coordinate or point not on curve");
  if (f & FLAG_SUBGROUP) return fail(BGLS_ERR_ENCODING, "point outside the order-r subgroup");
  if (f & FLAG_DEGENERATE) return fail(BGLS_ERR_ENCODING, "degenerate point step (small-order key)");
  if (f & FLAG_HASH) return fail(BGLS_ERR_HASH, "try-and-increment exhausted");
  return 0;
}

// The close of a call that answers with its flag word: `bytes` of result from d_src to dst where there are any, the word itself, the stream
// drained, the stage timers collected where the call does that, and the word's meaning as the return code.
int read_flags(Ctx& c, hipStream_t st, const void* d_flags, bool collect, void* dst = nullptr, const void* d_src = nullptr, size_t bytes = 0) {
  uint32_t f = 0;
  if (bytes) HIPCHK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&f, d_flags, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (collect) c.collect();
  return flags_to_rc(f);
}

// The messages of a host-pointer call on the device: the n + 1 offsets, checked here and before anything of the call is enqueued, to
// WS_IN_D, the blob to WS_IN_C.
int upload_msgs(Ctx& c, hipStream_t st, const uint8_t* blob, const uint64_t* off, size_t n, MsgView* mv) {
  int rc;
  void *d_blob, *d_off;
  if ((rc = offsets_ok("msg_off", off, n, 0))) return rc;
  if ((rc = c.put(st, WS_IN_C, blob, n ? off[n] : 0, &d_blob))) return rc;
  if ((rc = c.put(st, WS_IN_D, off, (n + 1) * 8, &d_off))) return rc;
  *mv = {(const uint8_t*)d_blob, (const uint64_t*)d_off, 0, 0};
  return 0;
}

// Messages lo .. hi of a host-pointer call whose hash inputs are built on the device (Engine::key_msgs), offsets already checked: the
// blob range to WS_IN_C; messages of ONE length become the fixed-stride view and no offsets travel, else the hi - lo + 1 offsets go to
// WS_IN_D with their caller's values and the view's base is shifted instead (never dereferenced below the blob).  *bytes: the bytes of
// the messages together.  keyed.mode == BGLS_KEYED_POP: no messages, nothing is read or uploaded.
struct Keyed { int mode; size_t msg_bytes; };
int upload_keyed_msgs(Ctx& c, hipStream_t st, int mode, const uint8_t* blob, const uint64_t* off, size_t lo, size_t hi, MsgView* mv, Keyed* keyed) {
  *keyed = {mode, 0};
  *mv = {nullptr, nullptr, 0, 0};
  if (mode == BGLS_KEYED_POP || hi == lo) return 0;
  const size_t n = hi - lo, bytes = off[hi] - off[lo], len = off[lo + 1] - off[lo];
  bool one_len = true;
  for (size_t i = lo; i < hi && one_len; ++i) one_len = off[i + 1] - off[i] == len;
  int rc;
  void *d_blob, *d_off;
  if ((rc = c.put(st, WS_IN_C, bytes ? blob + off[lo] : nullptr, bytes, &d_blob))) return rc;
  keyed->msg_bytes = bytes;
  if (one_len) {
    *mv = {(const uint8_t*)d_blob, nullptr, len, len};
    return 0;
  }
  if ((rc = c.put(st, WS_IN_D, off + lo, (n + 1) * 8, &d_off))) return rc;
  *mv = {(const uint8_t*)d_blob - off[lo], (const uint64_t*)d_off, 0, 0};
  return 0;
}

// The points of the sets of a host-pointer call on the device (PB bytes each): points off[0] .. off[n_sets] to *d_pts (WS_IN_B), the offsets
// relative to off[0] to *d_off (WS_SEG_OFF) and to rel.  rel is the source of an asynchronous copy: the caller keeps it until it has
// synchronised the stream.  Nothing of off is read when n_sets == 0.
int upload_key_sets(Ctx& c, hipStream_t st, size_t PB, const uint8_t* pts, const uint64_t* off, size_t n_sets, void** d_pts, void** d_off,
                std::vector<uint64_t>& rel) {
  const size_t k0 = n_sets ? off[0] : 0;
  int rc;
  rel.assign(n_sets + 1, 0);
  for (size_t i = 1; i <= n_sets; ++i) rel[i] = off[i] - k0;
  if ((rc = c.put(st, WS_IN_B, rel[n_sets] ? pts + k0 * PB : nullptr, rel[n_sets] * PB, d_pts, PB))) return rc;
  return c.put(st, WS_SEG_OFF, rel.data(), (n_sets + 1) * 8, d_off);
}

#define DISPATCH(curve, CALL)                                    \
  do {                                                           \
    if ((curve) == BGLS_CURVE_ALTBN128) {                        \
      typedef BN254 CV;                                          \
      return CALL;                                               \
    } else if ((curve) == BGLS_CURVE_BLS12_381) {                \
      typedef BLS381 CV;                                         \
      return CALL;                                               \
    }                                                            \
    return fail(BGLS_ERR_ARG, "unknown curve id");               \
  } while (0)

// distinct (DistinctMsgVerifyAggregateSignature, bgls/blsDistinctMessage.go:45-57): message i is hashed behind key i's wire bytes, put
// there on the device, and there is no duplicate rule
template <class C>
int verify_aggregate_t(const uint8_t* sig, const uint8_t* keys, const uint8_t* blob, const uint64_t* off, size_t n, int allow_dups, bool distinct = false) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  MsgView mv;
  Keyed keyed;
  void *d_sig, *d_keys, *d_flags, *d_part;
  if (distinct) {
    if ((rc = offsets_ok("msg_off", off, n, 0))) return rc;
    if ((rc = upload_keyed_msgs(c, st, BGLS_KEYED_PREFIX, blob, off, 0, n, &mv, &keyed))) return rc;
  } else if ((rc = upload_msgs(c, st, blob, off, n, &mv))) return rc;
  if ((rc = c.put(st, WS_IN_A, sig, E::G1B, &d_sig))) return rc;
  if ((rc = c.put(st, WS_IN_B, keys, n * E::G2B, &d_keys))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  if ((rc = c.get(WS_PART, E::GTB, &d_part))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if (distinct && (rc = E::key_msgs(c, st, keyed.mode, (const uint8_t*)d_keys, mv, keyed.msg_bytes, n, (uint32_t*)d_flags, &mv))) return rc;
  if ((rc = E::miller_product(c, st, (const uint8_t*)d_sig, (const uint8_t*)d_keys, mv, n, !allow_dups, (uint8_t*)d_part,
                              (uint32_t*)d_flags)))
    return rc;
  return E::finalize(c, st, (const uint8_t*)d_part, 1, 1, (const uint32_t*)d_flags, nullptr);
}

// ---- aggregate verification that pairs once per distinct message (bgls_group_messages, bgls_verify_aggregate_grouped) ----
// the grouping alone: group_of to the host (h_group_of) or left in the caller's device array (d_group_of)
int group_messages_run(Ctx& c, hipStream_t st, MsgView mv, size_t n, uint32_t* h_group_of, uint32_t* d_group_of, size_t* n_groups) {
  typedef Engine<BN254> E;                                 // curve-independent
  E::Groups g;
  int rc;
  if ((rc = E::group_messages(c, st, mv, 0, n, d_group_of, false, &g))) return rc;
  if (h_group_of) HIPCHK(hipMemcpyAsync(h_group_of, g.group_of, n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c.collect();
  if (n_groups) *n_groups = g.d;
  return 0;
}
int group_messages_t(const uint8_t* blob, const uint64_t* off, size_t n, uint32_t* group_of, size_t* n_groups) {
  Call k;
  if (k.rc) return k.rc;
  int rc;
  MsgView mv;
  if ((rc = upload_msgs(k.c, k.st, blob, off, n, &mv))) return rc;
  return group_messages_run(k.c, k.st, mv, n, group_of, nullptr, n_groups);
}
int group_messages_dev_t(const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n, void* d_group_of, size_t* n_groups, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return group_messages_run(k.c, k.st, mv, n, nullptr, (uint32_t*)d_group_of, n_groups);
}

// the grouping, the indexed key sum into d key sums, then the sibling's product over the d (key sum, representative message) pairs
// (no duplicate rule) and ONE final exponentiation.  msg_bytes: an upper bound of the bytes of the n messages.
template <class C>
int verify_aggregate_grouped_run(Ctx& c, hipStream_t st, const uint8_t* d_sig, const uint8_t* d_keys, MsgView mv, size_t msg_bytes, size_t n,
                                 size_t* n_groups, uint8_t* gt_out) {
  typedef Engine<C> E;
  if (c.res_pending) return in_flight();
  int rc;
  void *d_flags, *d_part;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  if ((rc = c.get(WS_PART, E::GTB, &d_part))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  typename E::Groups g;
  const uint8_t* d_sums = d_keys;
  if (n) {
    if ((rc = E::group_messages(c, st, mv, msg_bytes, n, nullptr, true, &g))) return rc;
    if ((rc = E::sum_groups(c, st, d_keys, g, &d_sums, (uint32_t*)d_flags))) return rc;
    mv = g.reps;
  }
  if ((rc = E::miller_product(c, st, d_sig, d_sums, mv, g.d, 0, (uint8_t*)d_part, (uint32_t*)d_flags))) return rc;
  if (n_groups) *n_groups = g.d;
  return E::finalize(c, st, (const uint8_t*)d_part, 1, 1, (const uint32_t*)d_flags, gt_out);
}
template <class C>
int verify_aggregate_grouped_t(const uint8_t* sig, const uint8_t* keys, const uint8_t* blob, const uint64_t* off, size_t n, size_t* n_groups,
                               uint8_t* gt_out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  int rc;
  MsgView mv;
  void *d_sig, *d_keys;
  if ((rc = upload_msgs(c, k.st, blob, off, n, &mv))) return rc;
  if ((rc = c.put(k.st, WS_IN_A, sig, E::G1B, &d_sig))) return rc;
  if ((rc = c.put(k.st, WS_IN_B, keys, n * E::G2B, &d_keys))) return rc;
  return verify_aggregate_grouped_run<C>(c, k.st, (const uint8_t*)d_sig, (const uint8_t*)d_keys, mv, n ? off[n] : 0, n, n_groups, gt_out);
}
template <class C>
int verify_aggregate_grouped_dev_t(const void* d_sig, const void* d_keys, const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n,
                                   size_t* n_groups, uint8_t* gt_out, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return verify_aggregate_grouped_run<C>(k.c, k.st, (const uint8_t*)d_sig, (const uint8_t*)d_keys, mv, n * msg_len, n, n_groups, gt_out);
}

// What a call with one verdict per item hands back, and the two things in which the Boneh-Boyen form differs from the others.
struct BatchOut {
  uint8_t* verdicts;                 // n bytes, 1 / 0
  uint8_t* gt = nullptr;             // nullable: the n GT elements
  uint8_t* apks = nullptr;           // nullable: the n key sums of a batch of sets, wire bytes, from d_apks
  const uint8_t* d_apks = nullptr;
  bool bb = false;                   // Boneh-Boyen: item n is the reference pair (g1, g2), verdict b = (GT element b == GT element n)
};

// The common tail of the calls with one verdict per item (aggregate instances, multi-signature sets with plain or hashed key sums,
// Boneh-Boyen signatures): stage(d_part, d_iflags, d_flags) runs the call's own launches up to one GT partial per item at d_part (no
// final exponentiation; per-item refusals in d_iflags, encoding and hashing failures in d_flags, all zeroed here), then one final
// exponentiation per item in ONE launch.  out.verdicts[b] = 1 / 0, returns the number of accepted items.  An encoding or hashing failure
// anywhere fails the whole call with the single call's code.
template <class C, class Stage>
int batch_verdicts_run(Ctx& c, hipStream_t st, size_t n, const BatchOut& out, Stage&& stage) {
  typedef Engine<C> E;
  if (c.res_pending) return in_flight();
  const size_t m = out.bb ? n + 1 : n;                    // items through the final exponentiation
  // words: m per-item flags, m verdicts of the final exponentiation, (Boneh-Boyen: whose verdicts against one are unused, then m words for
  // the n verdicts of the comparison,) the call's flag word -- right behind the n verdicts, so that one copy fetches both
  const size_t n_words = (out.bb ? 3 : 2) * m + 1;
  const bool dev_gt = out.gt || out.bb;
  void *d_res, *d_part;
  int rc;
  if ((rc = c.get(WS_BATCH_RES, n_words * 4, &d_res))) return rc;
  if ((rc = c.get(WS_PART, m * E::GTB * (dev_gt ? 2 : 1), &d_part))) return rc;
  uint32_t* d_iflags = (uint32_t*)d_res;
  uint32_t* d_fx = d_iflags + m;
  uint32_t* d_verdicts = out.bb ? d_fx + m : d_fx;
  uint32_t* d_flags = d_verdicts + n;
  uint8_t* d_gt = dev_gt ? (uint8_t*)d_part + m * E::GTB : nullptr;
  Drain drain{st};
  HIPCHK(hipMemsetAsync(d_res, 0, n_words * 4, st));
  if ((rc = stage((uint8_t*)d_part, d_iflags, d_flags))) return rc;
  {
    Scope sc(c, st, ST_FINAL);
    kl::finalx_batch<C>(st, (const uint8_t*)d_part, m, d_gt, d_fx, d_iflags, d_flags);
    if (out.bb) kl::bb_verdicts<C>(st, d_gt, n, d_verdicts);
  }
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> words(n + 1);
  HIPCHK(hipMemcpyAsync(words.data(), d_verdicts, (n + 1) * 4, hipMemcpyDeviceToHost, st));
  if (out.gt) HIPCHK(hipMemcpyAsync(out.gt, d_gt, n * E::GTB, hipMemcpyDeviceToHost, st));
  if (out.apks) HIPCHK(hipMemcpyAsync(out.apks, out.d_apks, n * E::G2B, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  drain.armed = false;
  c.collect();
  if ((rc = flags_to_rc(words[n]))) return rc;
  int accepted = 0;
  for (size_t b = 0; b < n; ++b) {
    out.verdicts[b] = words[b] ? 1 : 0;
    accepted += words[b] ? 1 : 0;
  }
  return accepted;
}

// n_inst independent VerifyAggregateSignature calls (bgls/bgls.go:94-119) in one set of launches (Engine::miller_product_batch, which sets
// d_iflags[b] for a duplicate message within instance b), then batch_verdicts_run's tail.
// keyed != nullptr (the distinct-message batch): every message is hashed behind its key's wire bytes (Engine::key_msgs).
template <class C>
int verify_aggregate_batch_run(Ctx& c, hipStream_t st, const uint8_t* d_sigs, const uint8_t* d_keys, MsgView mv, const uint64_t* inst_off, size_t n_inst,
                               int allow_dups, uint8_t* verdicts, uint8_t* gt_out, const Keyed* keyed = nullptr) {
  return batch_verdicts_run<C>(c, st, n_inst, {verdicts, gt_out}, [&](uint8_t* d_part, uint32_t* d_iflags, uint32_t* d_flags) {
    MsgView hv = mv;
    int r;
    if (keyed && (r = Engine<C>::key_msgs(c, st, keyed->mode, d_keys, mv, keyed->msg_bytes, inst_off[n_inst], d_flags, &hv))) return r;
    return Engine<C>::miller_product_batch(c, st, d_sigs, d_keys, hv, inst_off, n_inst, !allow_dups, d_part, d_iflags, d_flags);
  });
}

template <class C>
int verify_aggregate_batch_t(const uint8_t* sigs, const uint8_t* keys, const uint64_t* inst_off, size_t n_inst, const uint8_t* blob, const uint64_t* off,
                             int allow_dups, uint8_t* verdicts, uint8_t* gt_out, bool distinct = false) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  const size_t n = inst_off[n_inst];
  MsgView mv;
  Keyed keyed;
  void *d_sigs, *d_keys;
  if (distinct) {
    if ((rc = offsets_ok("msg_off", off, n, 0))) return rc;
    if ((rc = upload_keyed_msgs(c, st, BGLS_KEYED_PREFIX, blob, off, 0, n, &mv, &keyed))) return rc;
  } else if ((rc = upload_msgs(c, st, blob, off, n, &mv))) return rc;
  if ((rc = c.put(st, WS_IN_A, sigs, n_inst * E::G1B, &d_sigs))) return rc;
  if ((rc = c.put(st, WS_IN_B, keys, n * E::G2B, &d_keys))) return rc;
  return verify_aggregate_batch_run<C>(c, st, (const uint8_t*)d_sigs, (const uint8_t*)d_keys, mv, inst_off, n_inst, allow_dups, verdicts, gt_out,
                                       distinct ? &keyed : nullptr);
}

template <class C>
int verify_aggregate_batch_dev_t(const void* d_sigs, const void* d_keys, const uint64_t* inst_off, size_t n_inst, const void* d_msgs, size_t msg_len,
                                 size_t msg_stride, int allow_dups, uint8_t* verdicts, uint8_t* gt_out, void* stream, bool distinct = false) {
  Call k(stream);
  if (k.rc) return k.rc;
  MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  const Keyed keyed = {BGLS_KEYED_PREFIX, (size_t)inst_off[n_inst] * msg_len};
  return verify_aggregate_batch_run<C>(k.c, k.st, (const uint8_t*)d_sigs, (const uint8_t*)d_keys, mv, inst_off, n_inst, allow_dups, verdicts, gt_out,
                                       distinct ? &keyed : nullptr);
}

template <class C>
int verify_multi_dev_t(Ctx& c, hipStream_t st, const uint8_t* d_sig, const uint8_t* d_keys, size_t n, const uint8_t* d_msg,
                       size_t msg_len, bool submit_only = false, int key_src = 0) {
  typedef Engine<C> E;
  int rc;
  void *d_flags, *d_g2s, *d_g1s, *d_part;
  if (n >= MAX_BATCH) return too_large();
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  if ((rc = c.get(WS_TMP2, 2 * E::G2B, &d_g2s))) return rc;
  if ((rc = c.get(WS_G1S, 4 * sizeof(Aff<F1<C>>), &d_g1s))) return rc;
  if ((rc = c.get(WS_PART, E::GTB, &d_part))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  // pairs (H(msg), apk) and (-sig, g2) -- the reference's e(sig, g2) = e(H(msg), apk) (bgls/bgls.go:59-70) as a product that
  // must be 1: one message through the batch hashing path, then the two-pairing product on the cooperative Miller kernel
  // with the (-sig, g2) pair on the pre-computed generator lines.
  // H(m) and -sig do not depend on the key sum: a verification with the machine to itself hashes on the context's side stream
  // while the keys are added (0.3 ms off its latency); with several in flight (throughput mode) the neighbours fill the machine
  // and one stream per verification is what the hardware queues are budgeted for.
  MsgView mv = {d_msg, nullptr, msg_len, msg_len};
  Aff<F1<C>>* g1s = (Aff<F1<C>>*)d_g1s;
  constexpr bool raw = C::CURVE_ID == 1;        // BLS12-381: H(m) before cofactor clearing, the cofactor applied in GT (DESIGN.md section 3)
  const bool fork = side_fork_allowed() && n >= 4096;
  hipStream_t hs = fork ? c.side : st;
  SideJoin sj{c.side};
  if (fork) {
    HIPCHK(hipEventRecord(c.ev_fork, st));
    HIPCHK(hipStreamWaitEvent(c.side, c.ev_fork, 0));
    sj.armed = true;
  } else {
    // apk = sum(keys)  (AggregatePoints)
    if ((rc = E::sum_points(c, st, BGLS_G2, d_keys, n, (uint8_t*)d_g2s, (uint32_t*)d_flags, key_src))) return rc;
  }
  if ((rc = E::hash_to_g1(c, hs, mv, 1, g1s, (uint32_t*)d_flags, raw))) return rc;          // H(m)
  kl::g1_parse<C>(hs, d_sig, 1, 1, g1s + 1, (uint32_t*)d_flags);                            // -sig
  if (fork) {
    HIPCHK(hipEventRecord(c.ev_join, c.side));
    if ((rc = E::sum_points(c, st, BGLS_G2, d_keys, n, (uint8_t*)d_g2s, (uint32_t*)d_flags, key_src))) return rc;
    HIPCHK(hipStreamWaitEvent(st, c.ev_join, 0));
    sj.armed = false;
  }
  if ((rc = E::miller(c, st, g1s, (const uint8_t*)d_g2s, 1, g1s + 1, (uint8_t*)d_part, (uint32_t*)d_flags, raw))) return rc;
  if (submit_only) return E::finalize_submit(c, st, (const uint8_t*)d_part, 1, 1, (const uint32_t*)d_flags, nullptr);
  return E::finalize(c, st, (const uint8_t*)d_part, 1, 1, (const uint32_t*)d_flags, nullptr);
}

// KoskVerifyBatchMultiSignature's body (bgls/blsKosk.go:126-133): aggsig = sum(sigs), key_b = sum(set b), then ONE aggregate
// verification over the nsets pairs (key_b, msg_b) -- one Miller launch, one final exponentiation for all the sets.
template <class C>
int verify_multi_batch_dev_t(Ctx& c, hipStream_t st, const uint8_t* d_sigs, const uint8_t* d_keys, const uint64_t* d_key_off, size_t nsets,
                             size_t max_set, MsgView mv, int allow_dups, bool submit_only) {
  typedef Engine<C> E;
  int rc;
  void *d_flags, *d_akeys, *d_sig, *d_part;
  if (nsets >= MAX_BATCH) return too_large();
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  if ((rc = c.get(WS_SEG_KEYS, (nsets + 1) * E::G2B, &d_akeys))) return rc;
  if ((rc = c.get(WS_TMP2, 2 * E::G2B, &d_sig))) return rc;
  if ((rc = c.get(WS_PART, E::GTB, &d_part))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if ((rc = E::sum_sets(c, st, BGLS_G2, d_keys, d_key_off, nsets, max_set, (uint8_t*)d_akeys, (uint32_t*)d_flags))) return rc;   // AggregateKeys x nsets
  if ((rc = E::sum_points(c, st, BGLS_G1, d_sigs, nsets, (uint8_t*)d_sig, (uint32_t*)d_flags))) return rc;                          // AggregateSignatures
  if ((rc = E::miller_product(c, st, (const uint8_t*)d_sig, (const uint8_t*)d_akeys, mv, nsets, !allow_dups, (uint8_t*)d_part, (uint32_t*)d_flags)))
    return rc;
  if (submit_only) return E::finalize_submit(c, st, (const uint8_t*)d_part, 1, 1, (const uint32_t*)d_flags, nullptr);
  return E::finalize(c, st, (const uint8_t*)d_part, 1, 1, (const uint32_t*)d_flags, nullptr);
}

template <class C>
int verify_multi_batch_t(const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t nsets, const uint8_t* blob, const uint64_t* off,
                         int allow_dups) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  size_t max_set = 0;
  MsgView mv;
  void *d_sigs, *d_keys, *d_koff;
  std::vector<uint64_t> rel;
  if ((rc = upload_msgs(c, st, blob, off, nsets, &mv))) return rc;
  if ((rc = offsets_ok("key_off", key_off, nsets, OFF_TOTAL, SIZE_MAX, &max_set))) return rc;
  if ((rc = c.put(st, WS_IN_A, sigs, nsets * E::G1B, &d_sigs, E::G1B))) return rc;
  if ((rc = upload_key_sets(c, st, E::G2B, keys, key_off, nsets, &d_keys, &d_koff, rel))) return rc;
  HIPCHK(hipStreamSynchronize(st));                       // rel goes out of scope
  return verify_multi_batch_dev_t<C>(c, st, (const uint8_t*)d_sigs, (const uint8_t*)d_keys, (const uint64_t*)d_koff, nsets, max_set, mv, allow_dups, false);
}

// AggregatePoints over nsets sets in one pass (host buffers): out = nsets points
template <class C>
int aggregate_sets_t(int group, const uint8_t* pts, const uint64_t* set_off, size_t nsets, uint8_t* out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  const size_t PB = group == BGLS_G1 ? E::G1B : E::G2B;
  size_t max_set = 0;
  if ((rc = offsets_ok("set_off", set_off, nsets, 0, SIZE_MAX, &max_set))) return rc;
  if (nsets == 0) return 0;
  if (set_off[nsets] - set_off[0] >= MAX_BATCH || nsets >= MAX_BATCH) return too_large();
  void *d_pts, *d_off, *d_out, *d_flags;
  std::vector<uint64_t> rel;                              // alive until read_flags has synchronised
  if ((rc = c.get(WS_SEG_KEYS, (nsets + 1) * PB, &d_out))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if ((rc = upload_key_sets(c, st, PB, pts, set_off, nsets, &d_pts, &d_off, rel))) return rc;
  if ((rc = E::sum_sets(c, st, group, (const uint8_t*)d_pts, (const uint64_t*)d_off, nsets, max_set, (uint8_t*)d_out, (uint32_t*)d_flags))) return rc;
  return read_flags(c, st, d_flags, true, out, d_out, nsets * PB);
}

// A batch of n_sets multi-signature sets with one verdict per set: sum_keys(d_apks, d_flags) leaves the n_sets key sums apk_b as wire bytes
// at d_apks (encoding failures in d_flags); then Engine::miller_multi_sets and batch_verdicts_run's tail.  apk_out / gt_out (nullable): the
// key sums / GT elements.
template <class C, class SumKeys>
int verify_sets_run(Ctx& c, hipStream_t st, const uint8_t* d_sigs, size_t n_sets, MsgView mv, uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out,
                    SumKeys&& sum_keys) {
  void* d_apks;
  int rc;
  if ((rc = c.get(WS_SEG_KEYS, (n_sets + 1) * Engine<C>::G2B, &d_apks))) return rc;
  return batch_verdicts_run<C>(c, st, n_sets, {verdicts, gt_out, apk_out, (const uint8_t*)d_apks}, [&](uint8_t* d_part, uint32_t*, uint32_t* d_flags) {
    int r = sum_keys((uint8_t*)d_apks, d_flags);
    return r ? r : Engine<C>::miller_multi_sets(c, st, d_sigs, (const uint8_t*)d_apks, mv, n_sets, d_part, d_flags);
  });
}

// n_sets independent verifyMultiSignature calls (bgls/bgls.go:89-92) in one set of launches: every key sum in one pass
// (Engine::sum_sets), then verify_sets_run.  d_key_off: n_sets + 1 device offsets, already checked (monotone, no set above max_set).
template <class C>
int verify_multi_sets_run(Ctx& c, hipStream_t st, const uint8_t* d_sigs, const uint8_t* d_keys, const uint64_t* d_key_off, size_t n_sets, size_t max_set,
                          MsgView mv, uint8_t* verdicts, uint8_t* gt_out) {
  return verify_sets_run<C>(c, st, d_sigs, n_sets, mv, verdicts, nullptr, gt_out, [&](uint8_t* d_apks, uint32_t* d_flags) {
    return Engine<C>::sum_sets(c, st, BGLS_G2, d_keys, d_key_off, n_sets, max_set, d_apks, d_flags);     // apk_b = AggregateKeys(set b)
  });
}

template <class C>
int verify_multi_sets_t(const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t n_sets, const uint8_t* blob, const uint64_t* off,
                        uint8_t* verdicts, uint8_t* gt_out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  size_t max_set = 0;
  MsgView mv;
  void *d_sigs, *d_keys, *d_koff;
  std::vector<uint64_t> rel;
  if ((rc = offsets_ok("key_off", key_off, n_sets, 0, SIZE_MAX, &max_set))) return rc;
  if ((rc = c.put(st, WS_IN_A, sigs, n_sets * E::G1B, &d_sigs))) return rc;
  if ((rc = upload_key_sets(c, st, E::G2B, keys, key_off, n_sets, &d_keys, &d_koff, rel))) return rc;
  if ((rc = upload_msgs(c, st, blob, off, n_sets, &mv))) return rc;
  HIPCHK(hipStreamSynchronize(st));                       // rel goes out of scope
  return verify_multi_sets_run<C>(c, st, (const uint8_t*)d_sigs, (const uint8_t*)d_keys, (const uint64_t*)d_koff, n_sets, max_set, mv, verdicts, gt_out);
}

// The n_sets + 1 key offsets of a device-pointer call are the caller's device words: copied back to koff and checked here (from 0,
// monotone, no set above max_set, hae: every set below 2^28 keys, below 2^30 keys in all, keys non-NULL), so that no launch reads past the keys.
int fetch_key_off(hipStream_t st, const void* d_key_off, size_t n_sets, size_t max_set, bool hae, const void* d_keys, std::vector<uint64_t>& koff) {
  int rc;
  koff.resize(n_sets + 1);
  HIPCHK(hipMemcpyAsync(koff.data(), d_key_off, (n_sets + 1) * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if ((rc = offsets_ok("key_off", koff.data(), n_sets, OFF_FROM_ZERO | OFF_TOTAL | (hae ? OFF_HAE : 0), max_set))) return rc;
  if (koff[n_sets] && !d_keys) return fail(BGLS_ERR_ARG, "NULL argument");
  return 0;
}

template <class C>
int verify_multi_sets_dev_t(const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets, size_t max_set, const void* d_msgs, size_t msg_len,
                            size_t msg_stride, uint8_t* verdicts, uint8_t* gt_out, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  int rc;
  std::vector<uint64_t> koff;
  if ((rc = fetch_key_off(k.st, d_key_off, n_sets, max_set, false, d_keys, koff))) return rc;
  MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return verify_multi_sets_run<C>(k.c, k.st, (const uint8_t*)d_sigs, (const uint8_t*)d_keys, (const uint64_t*)d_key_off, n_sets, max_set, mv, verdicts, gt_out);
}

// n single-signature checks whose message is derived from the key (DistinctMsgVerifySingleSignature, bgls/blsDistinctMessage.go:37-40;
// CheckAuthentication, bgls/blsKosk.go:59-69): item b is the signature d_sigs[b], the key d_keys[b] and, under BGLS_KEYED_PREFIX, message b
// of mv.  The hash inputs are built on the device (Engine::key_msgs), then Engine::miller_multi_sets with the keys themselves as the
// per-set key sums and batch_verdicts_run's tail.
template <class C>
int verify_single_keyed_run(Ctx& c, hipStream_t st, const uint8_t* d_sigs, const uint8_t* d_keys, MsgView mv, const Keyed& keyed, size_t n, uint8_t* verdicts,
                            uint8_t* gt_out) {
  return batch_verdicts_run<C>(c, st, n, {verdicts, gt_out}, [&](uint8_t* d_part, uint32_t*, uint32_t* d_flags) {
    MsgView hv;
    int r = Engine<C>::key_msgs(c, st, keyed.mode, d_keys, mv, keyed.msg_bytes, n, d_flags, &hv);
    return r ? r : Engine<C>::miller_multi_sets(c, st, d_sigs, d_keys, hv, n, d_part, d_flags);
  });
}

template <class C>
int verify_single_keyed_t(int mode, const uint8_t* sigs, const uint8_t* keys, const uint8_t* blob, const uint64_t* off, size_t n, uint8_t* verdicts,
                          uint8_t* gt_out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  MsgView mv;
  Keyed keyed;
  void *d_sigs, *d_keys;
  if ((rc = upload_keyed_msgs(c, st, mode, blob, off, 0, n, &mv, &keyed))) return rc;
  if ((rc = c.put(st, WS_IN_A, sigs, n * E::G1B, &d_sigs))) return rc;
  if ((rc = c.put(st, WS_IN_B, keys, n * E::G2B, &d_keys))) return rc;
  return verify_single_keyed_run<C>(c, st, (const uint8_t*)d_sigs, (const uint8_t*)d_keys, mv, keyed, n, verdicts, gt_out);
}

template <class C>
int verify_single_distinct_dev_t(const void* d_sigs, const void* d_keys, size_t n, const void* d_msgs, size_t msg_len, size_t msg_stride, uint8_t* verdicts,
                                 uint8_t* gt_out, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  const MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return verify_single_keyed_run<C>(k.c, k.st, (const uint8_t*)d_sigs, (const uint8_t*)d_keys, mv, {BGLS_KEYED_PREFIX, n * msg_len}, n, verdicts, gt_out);
}

// HashToG1 of the n inputs Engine::key_msgs builds from host keys (and messages): the hash of DistinctMsgSign / Authenticate.
template <class C>
int hash_to_g1_keyed_t(int mode, const uint8_t* keys, const uint8_t* blob, const uint64_t* off, size_t n, uint8_t* out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  if (n == 0) return 0;
  MsgView mv;
  Keyed keyed;
  void *d_keys, *d_g1s, *d_out, *d_flags;
  if ((rc = upload_keyed_msgs(c, st, mode, blob, off, 0, n, &mv, &keyed))) return rc;
  if ((rc = c.put(st, WS_IN_B, keys, n * E::G2B, &d_keys))) return rc;
  if ((rc = c.get(WS_G1S, n * sizeof(Aff<F1<C>>), &d_g1s))) return rc;
  if ((rc = c.get(WS_IN_A, n * E::G1B, &d_out))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if ((rc = E::key_msgs(c, st, mode, (const uint8_t*)d_keys, mv, keyed.msg_bytes, n, (uint32_t*)d_flags, &mv))) return rc;
  if ((rc = E::hash_to_g1(c, st, mv, n, (Aff<F1<C>>*)d_g1s, (uint32_t*)d_flags))) return rc;
  kl::g1_to_bytes<C>(st, (const Aff<F1<C>>*)d_g1s, n, (uint8_t*)d_out);
  HIPCHK(hipGetLastError());
  return read_flags(c, st, d_flags, true, out, d_out, n * E::G1B);
}

// ---- the combined check: many multi-signatures under one random linear combination per group (bgls_verify_multi_sets_combined) ----
namespace host_blake2 { void xb_root(const uint8_t* data, size_t len, uint32_t xof_len, uint64_t h[8]); }

// The rules of the groups of a combined call, checked before any device work: group_off == NULL means ONE group over all sets (n_groups
// must be 1), else n_groups + 1 offsets into the sets, from 0, monotone, ending at n_sets.  The coefficients' XOF length 16 n_sets is a uint32.
int rlc_args_ok(const uint64_t* group_off, size_t n_groups, size_t n_sets, const uint8_t* seed) {
  if (n_sets >= MAX_BATCH || n_groups >= MAX_BATCH) return too_large();
  if (n_sets >= HAE_MAX_SET) return fail(BGLS_ERR_ARG, "XOF length 16 n_sets must fit a uint32 (fewer than 2^28 sets)");
  if (!seed) return fail(BGLS_ERR_ARG, "NULL seed");
  if (!group_off) return n_groups == 1 ? 0 : fail(BGLS_ERR_ARG, "group_off == NULL means one group (n_groups must be 1)");
  int rc;
  if ((rc = offsets_ok("group_off", group_off, n_groups, OFF_FROM_ZERO))) return rc;
  if (group_off[n_groups] != n_sets) return fail(BGLS_ERR_ARG, "group_off must end at n_sets");
  return 0;
}

// root <- the BLAKE2Xb root of "bgls-rlc-v1" || seed || u64le(n) for an XOF of 16 n bytes (include/bgls_hip.h: bgls_rlc_coefficients)
void rlc_root(const uint8_t* seed, size_t n, uint64_t root[8]) {
  uint8_t in[11 + 32 + 8];
  memcpy(in, "bgls-rlc-v1", 11);
  memcpy(in + 11, seed, 32);
  for (int j = 0; j < 8; ++j) in[43 + j] = (uint8_t)((uint64_t)n >> (8 * j));
  host_blake2::xb_root(in, sizeof in, (uint32_t)(16 * n), root);
}

int rlc_coefficients_t(const uint8_t* seed, size_t n, uint8_t* r_out) {
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  int rc;
  void *d_root, *d_r;
  uint64_t root[8];
  rlc_root(seed, n, root);
  if ((rc = c.put(k.st, WS_HAE_ROOT, root, 64, &d_root))) return rc;
  if ((rc = c.get(WS_HAE_T, n * 16, &d_r))) return rc;
  kl::blake2x_expand(k.st, (const uint64_t*)d_root, (uint32_t)(16 * n), (uint8_t*)d_r);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(r_out, d_r, n * 16, hipMemcpyDeviceToHost, k.st));
  HIPCHK(hipStreamSynchronize(k.st));                        // root[] is a stack buffer
  for (size_t b = 0; b < n; ++b) r_out[16 * b + 15] |= 1;    // the lowest bit set: what k_rlc_pair multiplies by (rlc_scalar)
  return 0;
}

// n_sets multi-signature sets under ONE check per group of consecutive sets: with r_b the coefficients of bgls_rlc_coefficients,
// verdict g = [ e(-sum_b r_b sigma_b, g2) * prod_b e(r_b H(m_b), apk_b) == 1 ] over the sets b of group g.  Each stage once per call:
// the key sums apk_b (Engine::sum_sets, wire bytes), one hashing pass, then under ST_RLC the coefficients (root on the host,
// k_blake2x_expand), k_rlc_pair (r_b H_b in place, r_b sigma_b as wire bytes) and the segmented G1 sum per group with its negation;
// Engine::miller_product_batch over the groups as instances on the pre-scaled points -- or, with one group, Engine::miller on the same
// resident points, so that a single big group takes the unpadded 64-form -- and batch_verdicts_run's tail over n_groups items.
// group_off: n_groups + 1 HOST offsets or nullptr (one group), already checked (rlc_args_ok); d_key_off: already checked.
template <class C>
int verify_sets_combined_run(Ctx& c, hipStream_t st, const uint8_t* d_sigs, const uint8_t* d_keys, const uint64_t* d_key_off, size_t n_sets, size_t max_set,
                             MsgView mv, const uint64_t* group_off, size_t n_groups, const uint8_t* seed, uint8_t* verdicts, uint8_t* gt_out) {
  typedef Engine<C> E;
  typedef Aff<F1<C>> A1;
  constexpr bool raw = C::CURVE_ID == 1;                     // BLS12-381: uncleared hash points, the cofactor applied per group in the epilogue
  // host words on their way to WS_RLC_OFF in one copy: the XOF root, then the n_groups + 1 group offsets (alive until the tail has synchronised)
  std::vector<uint64_t> tab(8 + n_groups + 1, 0);
  rlc_root(seed, n_sets, tab.data());
  uint64_t* goff = tab.data() + 8;
  size_t max_group = 0;
  for (size_t g = 0; g <= n_groups; ++g) goff[g] = group_off ? group_off[g] : (g ? n_sets : 0);
  for (size_t g = 0; g < n_groups; ++g) max_group = goff[g + 1] - goff[g] > max_group ? goff[g + 1] - goff[g] : max_group;
  return batch_verdicts_run<C>(c, st, n_groups, {verdicts, gt_out}, [&](uint8_t* d_part, uint32_t* d_iflags, uint32_t* d_flags) {
    int rc;
    void *d_apks, *g1s, *d_tab, *d_r, *d_rs, *d_sums, *sigs;
    if ((rc = c.get(WS_SEG_KEYS, (n_sets + 1) * E::G2B, &d_apks))) return rc;
    if ((rc = c.get(WS_G1S, (n_sets + 2) * sizeof(A1), &g1s))) return rc;
    if ((rc = c.get(WS_HAE_T, n_sets * 16, &d_r))) return rc;
    if ((rc = c.get(WS_RLC_SIGS, n_sets * E::G1B, &d_rs))) return rc;
    if ((rc = c.get(WS_RLC_SUMS, (n_groups + 1) * E::G1B, &d_sums))) return rc;
    if ((rc = c.get(WS_BATCH_SIGS, (n_groups + 1) * sizeof(A1), &sigs))) return rc;
    if (n_groups == 1) sigs = (A1*)g1s + n_sets;             // Engine::miller wants the signature point behind the hash points
    if ((rc = E::sum_sets(c, st, BGLS_G2, d_keys, d_key_off, n_sets, max_set, (uint8_t*)d_apks, d_flags))) return rc;     // apk_b = AggregateKeys(set b)
    {
      Scope sc(c, st, ST_H2C);
      if ((rc = E::hash_to_g1(c, st, mv, n_sets, (A1*)g1s, d_flags, raw))) return rc;
    }
    {
      Scope sc(c, st, ST_RLC);
      if ((rc = c.put(st, WS_RLC_OFF, tab.data(), tab.size() * 8, &d_tab))) return rc;
      kl::blake2x_expand(st, (const uint64_t*)d_tab, (uint32_t)(16 * n_sets), (uint8_t*)d_r);
      kl::rlc_pair<C>(st, (A1*)g1s, d_sigs, (const uint8_t*)d_r, n_sets, (uint8_t*)d_rs, d_flags);
      HIPCHK(hipGetLastError());
      if ((rc = E::sum_sets(c, st, BGLS_G1, (const uint8_t*)d_rs, (const uint64_t*)d_tab + 8, n_groups, max_group, (uint8_t*)d_sums, d_flags, false))) return rc;
      kl::g1_parse<C>(st, (const uint8_t*)d_sums, n_groups, 1, (A1*)sigs, d_flags);                  // -sum_b r_b sigma_b
      HIPCHK(hipGetLastError());
    }
    if (n_groups == 1) return E::miller(c, st, (const A1*)g1s, (const uint8_t*)d_apks, n_sets, (const A1*)sigs, d_part, d_flags, raw);
    const typename E::PreScaled pre = {(const A1*)g1s, (const A1*)sigs};
    return E::miller_product_batch(c, st, nullptr, (const uint8_t*)d_apks, MsgView{}, goff, n_groups, 0, d_part, d_iflags, d_flags, nullptr, &pre);
  });
}

template <class C>
int verify_multi_sets_combined_t(const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t n_sets, const uint8_t* blob, const uint64_t* off,
                                 const uint64_t* group_off, size_t n_groups, const uint8_t* seed, uint8_t* verdicts, uint8_t* gt_out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  size_t max_set = 0;
  MsgView mv;
  void *d_sigs, *d_keys, *d_koff;
  std::vector<uint64_t> rel;
  if ((rc = offsets_ok("key_off", key_off, n_sets, 0, SIZE_MAX, &max_set))) return rc;
  if ((rc = c.put(st, WS_IN_A, sigs, n_sets * E::G1B, &d_sigs))) return rc;
  if ((rc = upload_key_sets(c, st, E::G2B, keys, key_off, n_sets, &d_keys, &d_koff, rel))) return rc;
  if ((rc = upload_msgs(c, st, blob, off, n_sets, &mv))) return rc;
  HIPCHK(hipStreamSynchronize(st));                       // rel goes out of scope
  return verify_sets_combined_run<C>(c, st, (const uint8_t*)d_sigs, (const uint8_t*)d_keys, (const uint64_t*)d_koff, n_sets, max_set, mv, group_off, n_groups,
                                     seed, verdicts, gt_out);
}

template <class C>
int verify_multi_sets_combined_dev_t(const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets, size_t max_set, const void* d_msgs,
                                     size_t msg_len, size_t msg_stride, const uint64_t* group_off, size_t n_groups, const uint8_t* seed, uint8_t* verdicts,
                                     uint8_t* gt_out, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  int rc;
  std::vector<uint64_t> koff;
  if ((rc = fetch_key_off(k.st, d_key_off, n_sets, max_set, false, d_keys, koff))) return rc;
  MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return verify_sets_combined_run<C>(k.c, k.st, (const uint8_t*)d_sigs, (const uint8_t*)d_keys, (const uint64_t*)d_key_off, n_sets, max_set, mv, group_off,
                                     n_groups, seed, verdicts, gt_out);
}

// n independent bbsigs.Verify calls (bbsigs/bbsigs.go:68-73) in one set of launches: Engine::miller_bb (item n is the reference pair
// (g1, g2)), then batch_verdicts_run's tail in its Boneh-Boyen form: verdicts[b] = (e(sigma_b, Q_b) == e(g1, g2)) byte for byte on the
// device.  gt_out (nullable): the n GT elements.  An encoding failure anywhere (sigma, U, V) or a degenerate point step fails the whole call.
template <class C>
int bb_verify_run(Ctx& c, hipStream_t st, const uint8_t* d_sigmas, const uint8_t* d_rs, const uint8_t* d_keys, const uint8_t* d_ms, size_t n,
                  uint8_t* verdicts, uint8_t* gt_out) {
  return batch_verdicts_run<C>(c, st, n, {verdicts, gt_out, nullptr, nullptr, true}, [&](uint8_t* d_part, uint32_t*, uint32_t* d_flags) {
    return Engine<C>::miller_bb(c, st, d_sigmas, d_rs, d_keys, d_ms, n, d_part, d_flags);
  });
}

template <class C>
int bb_verify_t(const uint8_t* sigmas, const uint8_t* rs, const uint8_t* keys, const uint8_t* ms, size_t n, uint8_t* verdicts, uint8_t* gt_out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void *d_sigmas, *d_rs, *d_keys, *d_ms;
  if ((rc = c.put(st, WS_IN_A, sigmas, n * E::G1B, &d_sigmas))) return rc;
  if ((rc = c.put(st, WS_IN_B, rs, n * 32, &d_rs))) return rc;
  if ((rc = c.put(st, WS_IN_C, keys, n * 2 * E::G2B, &d_keys))) return rc;
  if ((rc = c.put(st, WS_IN_D, ms, n * 32, &d_ms))) return rc;
  return bb_verify_run<C>(c, st, (const uint8_t*)d_sigmas, (const uint8_t*)d_rs, (const uint8_t*)d_keys, (const uint8_t*)d_ms, n, verdicts, gt_out);
}

template <class C>
int bb_verify_dev_t(const void* d_sigmas, const void* d_rs, const void* d_keys, const void* d_ms, size_t n, uint8_t* verdicts, uint8_t* gt_out, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  return bb_verify_run<C>(k.c, k.st, (const uint8_t*)d_sigmas, (const uint8_t*)d_rs, (const uint8_t*)d_keys, (const uint8_t*)d_ms, n, verdicts, gt_out);
}

// ---- one GT element per item: n final exponentiations, n pairings (bgls_final_exp_batch, bgls_pair_batch) ----
// Where the n GT elements and the n "is one" marks of gt_values_run go: device pointers (dev: the caller's, written by the launches) or
// host pointers (copied out only after the call's flag word has come back clear, so a failed call leaves them as they were).
struct GtOut {
  uint8_t* gt;                       // nullable (not both)
  uint8_t* is_one;                   // nullable
  bool dev;
};

// stage(d_part, d_flags) leaves one GT partial per item at d_part (WS_PART, n GT elements; encoding failures in d_flags, zeroed here), or
// nothing where d_in is the caller's own n partials; then one final exponentiation per item in ONE launch of the throughput kernel
// k_finalxt_batch (ST_FINAL; ten items per wave, finalxt.hpp -- batch_verdicts_run above still finishes on k_finalx_batch).
// Words at WS_BATCH_RES: n per-item flags (zero: nothing refuses an item here), n marks of the final exponentiation, the call's flag word.
// Synchronises st.  Returns 0 or the code of the flag word.
template <class C, class Stage>
int gt_values_run(Ctx& c, hipStream_t st, size_t n, const uint8_t* d_in, const GtOut& out, Stage&& stage) {
  typedef Engine<C> E;
  if (c.res_pending) return in_flight();
  const bool host_gt = out.gt && !out.dev;
  void *d_res, *d_part = nullptr, *d_gt = out.dev ? out.gt : nullptr;
  int rc;
  if ((rc = c.get(WS_BATCH_RES, (2 * n + 1) * 4, &d_res))) return rc;
  if (!d_in && (rc = c.get(WS_PART, n * E::GTB, &d_part))) return rc;
  if (host_gt && (rc = c.get(WS_OUT, n * E::GTB, &d_gt))) return rc;
  uint32_t* d_iflags = (uint32_t*)d_res;
  uint32_t* d_one = d_iflags + n;
  uint32_t* d_flags = d_one + n;
  Drain drain{st};
  HIPCHK(hipMemsetAsync(d_res, 0, (2 * n + 1) * 4, st));
  if ((rc = stage((uint8_t*)d_part, d_flags))) return rc;
  {
    Scope sc(c, st, ST_FINAL);
    kl::finalxt_batch<C>(st, d_in ? d_in : (const uint8_t*)d_part, n, (uint8_t*)d_gt, d_one, d_iflags, d_flags);
  }
  if (out.dev && out.is_one) kl::is_one_bytes(st, d_one, n, out.is_one);
  HIPCHK(hipGetLastError());
  uint32_t flags = 0;
  HIPCHK(hipMemcpyAsync(&flags, d_flags, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c.collect();
  if ((rc = flags_to_rc(flags))) return rc;
  if (out.dev) {
    drain.armed = false;
    return 0;
  }
  std::vector<uint32_t> ones(out.is_one ? n : 0);
  if (out.is_one) HIPCHK(hipMemcpyAsync(ones.data(), d_one, n * 4, hipMemcpyDeviceToHost, st));
  if (host_gt) HIPCHK(hipMemcpyAsync(out.gt, d_gt, n * E::GTB, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  drain.armed = false;
  for (size_t b = 0; b < ones.size(); ++b) out.is_one[b] = ones[b] ? 1 : 0;
  return 0;
}

template <class C>
int final_exp_batch_t(const uint8_t* gt_in, size_t n, uint8_t* gt_out, uint8_t* is_one) {
  Call k;
  if (k.rc) return k.rc;
  int rc;
  void* d_in;
  if ((rc = k.c.put(k.st, WS_IN_A, gt_in, n * Engine<C>::GTB, &d_in))) return rc;
  return gt_values_run<C>(k.c, k.st, n, (const uint8_t*)d_in, {gt_out, is_one, false}, [](uint8_t*, uint32_t*) { return 0; });
}

template <class C>
int final_exp_batch_dev_t(const void* d_gt_in, size_t n, void* d_gt_out, void* d_is_one, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  return gt_values_run<C>(k.c, k.st, n, (const uint8_t*)d_gt_in, {(uint8_t*)d_gt_out, (uint8_t*)d_is_one, true}, [](uint8_t*, uint32_t*) { return 0; });
}

// n independent CurveSystem.Pair calls in one set of launches: Engine::miller_pairs, then gt_values_run's tail
template <class C>
int pair_batch_t(const uint8_t* g1s, const uint8_t* g2s, size_t n, uint8_t* gt_out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void *d_g1s, *d_g2s;
  if ((rc = c.put(st, WS_IN_A, g1s, n * E::G1B, &d_g1s))) return rc;
  if ((rc = c.put(st, WS_IN_B, g2s, n * E::G2B, &d_g2s))) return rc;
  return gt_values_run<C>(c, st, n, nullptr, {gt_out, nullptr, false}, [&](uint8_t* d_part, uint32_t* d_flags) {
    return E::miller_pairs(c, st, (const uint8_t*)d_g1s, (const uint8_t*)d_g2s, n, d_part, d_flags);
  });
}

template <class C>
int pair_batch_dev_t(const void* d_g1s, const void* d_g2s, size_t n, void* d_gt_out, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  return gt_values_run<C>(c, st, n, nullptr, {(uint8_t*)d_gt_out, nullptr, true}, [&](uint8_t* d_part, uint32_t* d_flags) {
    return Engine<C>::miller_pairs(c, st, (const uint8_t*)d_g1s, (const uint8_t*)d_g2s, n, d_part, d_flags);
  });
}

// ---- the combined check for Boneh-Boyen signatures: one random linear combination per group (bgls_bb_verify_batch_combined) ----
// n Boneh-Boyen items under ONE check per group of consecutive items: with rho_b the coefficients of bgls_rlc_coefficients and
// s_g = sum of rho_b over group g as a plain integer, verdict g = [ prod_b e(rho_b sigma_b, Q_b) * e(-s_g g1, g2) == 1 ] over the items b of
// group g, Q_b = m_b g2 + U_b + r_b V_b.  Each stage once per call: the parse of the sigma_b; k_bb_keys (ST_BB_KEYS: Q_b as wire bytes, no
// reference pair); then under ST_RLC the coefficients (root on the host, k_blake2x_expand, k_bb_rlc_odd), rho_b sigma_b in place
// (k_scale_g1_inplace), the sums s_g (k_bb_rlc_sums), s_g g1 from the fixed-base table of g1 (k_fb_scale) and its parse with negation
// into the signature slots; Engine::miller_product_batch over the groups as instances on the pre-scaled points -- or, with one group,
// Engine::miller on the same resident points, so that a single big group takes the unpadded 64-form -- both WITHOUT the cofactor power of
// their BLS12-381 epilogues (sigma_b is a G1 point, not an uncleared hash point); batch_verdicts_run's tail over n_groups items.
// Slots (one live buffer each): WS_G1S n + 2 points (sigma_b, then rho_b sigma_b; one group: -s g1 at index n), WS_SEG_KEYS the Q_b,
// WS_RLC_OFF the XOF root and the n_groups + 1 group offsets, WS_HAE_T the coefficients, WS_RLC_SUMS the n_groups magnitudes s_g,
// WS_RLC_SIGS the n_groups points s_g g1 as wire bytes, WS_BATCH_SIGS the n_groups signature-slot points; beside them the slots of
// batch_verdicts_run (WS_BATCH_RES, WS_PART) and of the Miller stage called.
// group_off: n_groups + 1 HOST offsets or nullptr (one group), already checked (rlc_args_ok).
template <class C>
int bb_verify_combined_run(Ctx& c, hipStream_t st, const uint8_t* d_sigmas, const uint8_t* d_rs, const uint8_t* d_keys, const uint8_t* d_ms, size_t n,
                           const uint64_t* group_off, size_t n_groups, const uint8_t* seed, uint8_t* verdicts, uint8_t* gt_out) {
  typedef Engine<C> E;
  typedef Aff<F1<C>> A1;
  // host words on their way to WS_RLC_OFF in one copy: the XOF root, then the n_groups + 1 group offsets (alive until the tail has synchronised)
  std::vector<uint64_t> tab(8 + n_groups + 1, 0);
  rlc_root(seed, n, tab.data());
  uint64_t* goff = tab.data() + 8;
  for (size_t g = 0; g <= n_groups; ++g) goff[g] = group_off ? group_off[g] : (g ? n : 0);
  return batch_verdicts_run<C>(c, st, n_groups, {verdicts, gt_out}, [&](uint8_t* d_part, uint32_t* d_iflags, uint32_t* d_flags) {
    int rc;
    void *g1s, *qs, *d_tab, *d_r, *d_sums, *d_sg, *sigs;
    const void *fb1, *fb2;
    if ((rc = c.get(WS_G1S, (n + 2) * sizeof(A1), &g1s))) return rc;
    if ((rc = c.get(WS_SEG_KEYS, (n + 1) * E::G2B, &qs))) return rc;
    if ((rc = c.get(WS_HAE_T, n * 16, &d_r))) return rc;
    if ((rc = c.get(WS_RLC_SUMS, (n_groups + 1) * 32, &d_sums))) return rc;
    if ((rc = c.get(WS_RLC_SIGS, (n_groups + 1) * E::G1B, &d_sg))) return rc;
    if ((rc = c.get(WS_BATCH_SIGS, (n_groups + 1) * sizeof(A1), &sigs))) return rc;
    if (n_groups == 1) sigs = (A1*)g1s + n;                  // Engine::miller wants the signature-slot point behind the pairs' points
    if ((rc = fixed_base_table<C>(c, BGLS_G1, &fb1))) return rc;
    if ((rc = fixed_base_table<C>(c, BGLS_G2, &fb2))) return rc;
    kl::g1_parse<C>(st, d_sigmas, n, 0, (A1*)g1s, d_flags);
    {
      Scope sc(c, st, ST_BB_KEYS);
      kl::bb_keys<C>(st, d_keys, d_rs, d_ms, fb2, n, (uint8_t*)qs, (A1*)g1s, nullptr, d_flags, false);
      HIPCHK(hipGetLastError());
    }
    {
      Scope sc(c, st, ST_RLC);
      if ((rc = c.put(st, WS_RLC_OFF, tab.data(), tab.size() * 8, &d_tab))) return rc;
      kl::blake2x_expand(st, (const uint64_t*)d_tab, (uint32_t)(16 * n), (uint8_t*)d_r);
      kl::bb_rlc_odd(st, (uint8_t*)d_r, n);
      kl::scale_g1_inplace<C>(st, (A1*)g1s, (const uint8_t*)d_r, n);                               // rho_b sigma_b
      kl::bb_rlc_sums(st, (const uint8_t*)d_r, (const uint64_t*)d_tab + 8, n_groups, (uint8_t*)d_sums);
      kl::fb_scale<C>(st, BGLS_G1, fb1, (const uint8_t*)d_sums, n_groups, (uint8_t*)d_sg);       // s_g g1
      kl::g1_parse<C>(st, (const uint8_t*)d_sg, n_groups, 1, (A1*)sigs, d_flags);                  // -s_g g1
      HIPCHK(hipGetLastError());
    }
    if (n_groups == 1) return E::miller(c, st, (const A1*)g1s, (const uint8_t*)qs, n, (const A1*)sigs, d_part, d_flags, false);
    const typename E::PreScaled pre = {(const A1*)g1s, (const A1*)sigs, true};
    return E::miller_product_batch(c, st, nullptr, (const uint8_t*)qs, MsgView{}, goff, n_groups, 0, d_part, d_iflags, d_flags, nullptr, &pre);
  });
}

template <class C>
int bb_verify_combined_t(const uint8_t* sigmas, const uint8_t* rs, const uint8_t* keys, const uint8_t* ms, size_t n, const uint64_t* group_off,
                         size_t n_groups, const uint8_t* seed, uint8_t* verdicts, uint8_t* gt_out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void *d_sigmas, *d_rs, *d_keys, *d_ms;
  if ((rc = c.put(st, WS_IN_A, sigmas, n * E::G1B, &d_sigmas))) return rc;
  if ((rc = c.put(st, WS_IN_B, rs, n * 32, &d_rs))) return rc;
  if ((rc = c.put(st, WS_IN_C, keys, n * 2 * E::G2B, &d_keys))) return rc;
  if ((rc = c.put(st, WS_IN_D, ms, n * 32, &d_ms))) return rc;
  return bb_verify_combined_run<C>(c, st, (const uint8_t*)d_sigmas, (const uint8_t*)d_rs, (const uint8_t*)d_keys, (const uint8_t*)d_ms, n, group_off,
                                   n_groups, seed, verdicts, gt_out);
}

template <class C>
int bb_verify_combined_dev_t(const void* d_sigmas, const void* d_rs, const void* d_keys, const void* d_ms, size_t n, const uint64_t* group_off,
                             size_t n_groups, const uint8_t* seed, uint8_t* verdicts, uint8_t* gt_out, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  return bb_verify_combined_run<C>(k.c, k.st, (const uint8_t*)d_sigmas, (const uint8_t*)d_rs, (const uint8_t*)d_keys, (const uint8_t*)d_ms, n,
                                   group_off, n_groups, seed, verdicts, gt_out);
}

template <class C>
int verify_multi_t(const uint8_t* sig, const uint8_t* keys, size_t n, const uint8_t* msg, size_t msg_len) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void *d_sig, *d_keys, *d_msg;
  if ((rc = c.put(st, WS_IN_A, sig, E::G1B, &d_sig))) return rc;
  if ((rc = c.put(st, WS_IN_B, keys, n * E::G2B, &d_keys))) return rc;
  if ((rc = c.put(st, WS_IN_C, msg, msg_len, &d_msg))) return rc;
  return verify_multi_dev_t<C>(c, st, (const uint8_t*)d_sig, (const uint8_t*)d_keys, n, (const uint8_t*)d_msg, msg_len);
}

template <class C>
int pairing_product_t(const uint8_t* g1s, const uint8_t* g2s, size_t n, uint8_t* gt_out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  if (n >= MAX_BATCH) return too_large();
  void *d_g1b, *d_g2b, *d_g1s, *d_flags, *d_part;
  if ((rc = c.get(WS_IN_A, n * E::G1B, &d_g1b))) return rc;
  if ((rc = c.get(WS_IN_B, n * E::G2B, &d_g2b))) return rc;
  if ((rc = c.get(WS_G1S, (n + 1) * sizeof(Aff<F1<C>>), &d_g1s))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  if ((rc = c.get(WS_PART, E::GTB, &d_part))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if (n == 0) {
    memset(gt_out, 0, E::GTB);
    gt_out[E::GTB - 1] = 1;
    return 0;
  }
  HIPCHK(hipMemcpyAsync(d_g1b, g1s, n * E::G1B, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_g2b, g2s, n * E::G2B, hipMemcpyHostToDevice, st));
  kl::g1_parse<C>(st, (const uint8_t*)d_g1b, n, 0, (Aff<F1<C>>*)d_g1s, (uint32_t*)d_flags);
  if ((rc = E::miller(c, st, (const Aff<F1<C>>*)d_g1s, (const uint8_t*)d_g2b, n, nullptr, (uint8_t*)d_part, (uint32_t*)d_flags))) return rc;
  rc = E::finalize(c, st, (const uint8_t*)d_part, 1, 1, (const uint32_t*)d_flags, gt_out);
  return rc < 0 ? rc : 0;
}

template <class C>
int hash_to_g1_t(const uint8_t* blob, const uint64_t* off, size_t n, uint8_t* out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  if (n == 0) return 0;
  MsgView mv;
  void *d_g1s, *d_out, *d_flags;
  if ((rc = upload_msgs(c, st, blob, off, n, &mv))) return rc;
  if ((rc = c.get(WS_G1S, n * sizeof(Aff<F1<C>>), &d_g1s))) return rc;
  if ((rc = c.get(WS_IN_A, n * E::G1B, &d_out))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if ((rc = E::hash_to_g1(c, st, mv, n, (Aff<F1<C>>*)d_g1s, (uint32_t*)d_flags))) return rc;
  kl::g1_to_bytes<C>(st, (const Aff<F1<C>>*)d_g1s, n, (uint8_t*)d_out);
  HIPCHK(hipGetLastError());
  return read_flags(c, st, d_flags, false, out, d_out, n * E::G1B);
}

template <class C>
int aggregate_points_t(int group, const uint8_t* pts, size_t n, uint8_t* out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  const size_t PB = group == BGLS_G1 ? E::G1B : E::G2B;
  void *d_in, *d_out, *d_flags;
  if ((rc = c.get(WS_IN_B, n * PB, &d_in))) return rc;
  if ((rc = c.get(WS_OUT, PB, &d_out))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if (n) HIPCHK(hipMemcpyAsync(d_in, pts, n * PB, hipMemcpyHostToDevice, st));
  if ((rc = E::sum_points(c, st, group, (const uint8_t*)d_in, n, (uint8_t*)d_out, (uint32_t*)d_flags))) return rc;
  return read_flags(c, st, d_flags, false, out, d_out, PB);
}

template <class C>
int scale_points_t(int group, const uint8_t* pts, const uint8_t* scalars, const uint8_t* signs, size_t n, uint8_t* out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  if (n == 0) return 0;
  const size_t PB = group == BGLS_G1 ? E::G1B : E::G2B;
  void *d_in, *d_sc, *d_sg, *d_out, *d_flags;
  if ((rc = c.get(WS_IN_B, n * PB, &d_in))) return rc;
  if ((rc = c.get(WS_IN_C, n * 32, &d_sc))) return rc;
  if ((rc = c.get(WS_IN_D, n, &d_sg))) return rc;
  if ((rc = c.get(WS_IN_A, n * PB, &d_out))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  HIPCHK(hipMemcpyAsync(d_in, pts, n * PB, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_sc, scalars, n * 32, hipMemcpyHostToDevice, st));
  if (signs) HIPCHK(hipMemcpyAsync(d_sg, signs, n, hipMemcpyHostToDevice, st));
  const uint8_t* sg = signs ? (const uint8_t*)d_sg : nullptr;
  if (group == BGLS_G1 && C::CURVE_ID == 1 && g1x()) kl::scale_g1x<C>(st, (const uint8_t*)d_in, (const uint8_t*)d_sc, sg, n, (uint8_t*)d_out, (uint32_t*)d_flags, 32);
  else kl::scale<C>(st, group, (const uint8_t*)d_in, (const uint8_t*)d_sc, sg, n, (uint8_t*)d_out, (uint32_t*)d_flags, 32);
  HIPCHK(hipGetLastError());
  return read_flags(c, st, d_flags, false, out, d_out, n * PB);
}

template <class C>
int point_check_t(int group, const uint8_t* a) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  const size_t PB = group == BGLS_G1 ? E::G1B : E::G2B;
  void *d_in, *d_flags;
  if ((rc = c.get(WS_IN_B, PB, &d_in))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  HIPCHK(hipMemcpyAsync(d_in, a, PB, hipMemcpyHostToDevice, st));
  kl::check<C>(st, group, (const uint8_t*)d_in, 1, (uint32_t*)d_flags, nullptr);
  uint32_t f = 0;
  HIPCHK(hipMemcpyAsync(&f, d_flags, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return f ? 0 : 1;
}

template <class C>
int check_points_t(int group, const uint8_t* pts, size_t n, uint8_t* ok_out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  if (n == 0) return 0;
  if (n >= MAX_BATCH) return too_large();
  const size_t PB = group == BGLS_G1 ? E::G1B : E::G2B;
  void *d_in, *d_ok, *d_flags;
  if ((rc = c.get(WS_IN_B, n * PB, &d_in))) return rc;
  if ((rc = c.get(WS_IN_D, n, &d_ok))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  HIPCHK(hipMemcpyAsync(d_in, pts, n * PB, hipMemcpyHostToDevice, st));
  kl::check<C>(st, group, (const uint8_t*)d_in, n, (uint32_t*)d_flags, (uint8_t*)d_ok);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ok_out, d_ok, n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

template <class C>
int generator_t(int group, uint8_t* out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  const size_t PB = group == BGLS_G1 ? E::G1B : E::G2B;
  void* d_out;
  if ((rc = c.get(WS_OUT, PB, &d_out))) return rc;
  kl::generator<C>(st, group, (uint8_t*)d_out);
  HIPCHK(hipMemcpyAsync(out, d_out, PB, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

template <class C>
int gt_mul_t(const uint8_t* a, const uint8_t* b, uint8_t* out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void* d_in;
  if ((rc = c.get(WS_IN_A, 2 * E::GTB, &d_in))) return rc;
  HIPCHK(hipMemcpyAsync(d_in, a, E::GTB, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync((uint8_t*)d_in + E::GTB, b, E::GTB, hipMemcpyHostToDevice, st));
  rc = E::finalize(c, st, (const uint8_t*)d_in, 2, 0, nullptr, out);
  return rc < 0 ? rc : 0;
}

template <class C>
int gt_pow_t(const uint8_t* gt, const uint8_t* k_be32, int negate, uint8_t* out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void *d_in, *d_flags;
  if ((rc = c.get(WS_IN_A, 2 * E::GTB + 32, &d_in))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  uint8_t* d = (uint8_t*)d_in;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  HIPCHK(hipMemcpyAsync(d, gt, E::GTB, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d + E::GTB, k_be32, 32, hipMemcpyHostToDevice, st));
  kl::gt_pow<C>(st, d, d + E::GTB, negate, d + E::GTB + 32, (uint32_t*)d_flags);
  HIPCHK(hipGetLastError());
  return read_flags(c, st, d_flags, false, out, d + E::GTB + 32, E::GTB);
}

template <class C>
int miller_product_dev_t(const void* d_sig, const void* d_keys, const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n,
                         int check_dups, void* d_partial, void* d_flags, void* stream) {
  typedef Engine<C> E;
  Call k(stream);
  if (k.rc) return k.rc;
  MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return E::miller_product(k.c, k.st, (const uint8_t*)d_sig, (const uint8_t*)d_keys, mv, n, check_dups, (uint8_t*)d_partial,
                           (uint32_t*)d_flags);
}

// containsDuplicateMessage (bgls/bgls.go:139-150) over device-resident fixed-stride messages: exact byte comparison
int duplicate_scan_dev(const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n, void* d_flags, void* stream, uint32_t bucket = 0, uint32_t n_buckets = 1,
                       bool packed = false) {
  Call k(stream);
  if (k.rc) return k.rc;
  MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return Engine<BN254>::dup_scan(k.c, k.st, mv, n, (uint32_t*)d_flags, bucket, n_buckets, packed);      // curve-independent
}

// the sending half of the digest exchange: n 16-byte digests into n_buckets slots of `cap` records (k_digest_pack)
int digest_pack_dev(const void* d_dig, size_t n, unsigned n_buckets, size_t cap, void* d_out, void* d_flags, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void* counts;
  if ((rc = c.get(WS_TABLE, 256 * 4, &counts))) return rc;          // the scan's table workspace: the scan of this verification comes after the exchange, in stream order
  HIPCHK(hipMemsetAsync(counts, 0, 256 * 4, st));
  kl::digest_pack(st, (const uint8_t*)d_dig, n, (uint8_t*)d_out, cap, n_buckets, (uint32_t*)counts, (uint32_t*)d_flags);
  HIPCHK(hipGetLastError());
  return 0;
}

template <class C>
int final_verify_dev_t(const void* d_partials, size_t count, const void* d_flags, void* stream) {
  typedef Engine<C> E;
  Call k(stream);
  if (k.rc) return k.rc;
  return E::finalize(k.c, k.st, (const uint8_t*)d_partials, count, 1, (const uint32_t*)d_flags, nullptr);
}

template <class C>
int final_verify_submit_dev_t(const void* d_partials, size_t count, const void* d_flags, void* stream) {
  typedef Engine<C> E;
  Call k(stream);
  if (k.rc) return k.rc;
  return E::finalize_submit(k.c, k.st, (const uint8_t*)d_partials, count, 1, (const uint32_t*)d_flags, nullptr);
}

template <class C>
int aggregate_points_dev_t(int group, const void* d_pts, size_t n, void* d_out, void* stream) {
  typedef Engine<C> E;
  Call k(stream);
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void* d_flags;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if ((rc = E::sum_points(c, st, group, (const uint8_t*)d_pts, n, (uint8_t*)d_out, (uint32_t*)d_flags))) return rc;
  return read_flags(c, st, d_flags, false);
}

template <class C>
int verify_multi_dev_entry_t(const void* d_sig, const void* d_keys, size_t n, const void* d_msg, size_t msg_len, void* stream,
                             bool submit_only = false) {
  Call k(stream);
  if (k.rc) return k.rc;
  return verify_multi_dev_t<C>(k.c, k.st, (const uint8_t*)d_sig, (const uint8_t*)d_keys, n, (const uint8_t*)d_msg, msg_len, submit_only);
}

template <class C>
int verify_multi_batch_sub_t(const void* d_sigs, const void* d_keys, const void* d_key_off, size_t nsets, size_t max_set, const void* d_msgs,
                             size_t msg_len, size_t msg_stride, int allow_dups, void* stream, bool submit_only) {
  Call k(stream);
  if (k.rc) return k.rc;
  MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return verify_multi_batch_dev_t<C>(k.c, k.st, (const uint8_t*)d_sigs, (const uint8_t*)d_keys, (const uint64_t*)d_key_off, nsets, max_set, mv, allow_dups,
                                     submit_only);
}

// ---- hashed aggregation exponents / weighted sums: host flows -------------------------------------------------
// Root digest of BLAKE2Xb (hashes.hpp has the device-side tables; these are the host's own copies).  One sequential
// compression chain over all key bytes -- by construction not parallel -- computed while the keys travel to the device.
namespace host_blake2 {
const uint64_t IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                        0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
const uint8_t SIGMA[12][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
inline uint64_t ror(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
inline void compress(uint64_t h[8], const uint8_t* block, uint64_t t, bool last) {
  uint64_t m[16], v[16];
  memcpy(m, block, 128);                                     // little-endian host
  for (int i = 0; i < 8; ++i) { v[i] = h[i]; v[i + 8] = IV[i]; }
  v[12] ^= t;
  if (last) v[14] = ~v[14];
#define BGLS_G(a, b, c, d, x, y)                                                    \
  v[a] += v[b] + (x); v[d] = ror(v[d] ^ v[a], 32); v[c] += v[d]; v[b] = ror(v[b] ^ v[c], 24); \
  v[a] += v[b] + (y); v[d] = ror(v[d] ^ v[a], 16); v[c] += v[d]; v[b] = ror(v[b] ^ v[c], 63);
  for (int r = 0; r < 12; ++r) {
    const uint8_t* s = SIGMA[r];
    BGLS_G(0, 4, 8, 12, m[s[0]], m[s[1]]) BGLS_G(1, 5, 9, 13, m[s[2]], m[s[3]])
    BGLS_G(2, 6, 10, 14, m[s[4]], m[s[5]]) BGLS_G(3, 7, 11, 15, m[s[6]], m[s[7]])
    BGLS_G(0, 5, 10, 15, m[s[8]], m[s[9]]) BGLS_G(1, 6, 11, 12, m[s[10]], m[s[11]])
    BGLS_G(2, 7, 8, 13, m[s[12]], m[s[13]]) BGLS_G(3, 4, 9, 14, m[s[14]], m[s[15]])
  }
#undef BGLS_G
  for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}
// h <- BLAKE2Xb root of data[0..len) for an XOF of xof_len bytes (x/crypto/blake2b/blake2x.go Reset + Write + finalize)
void xb_root(const uint8_t* data, size_t len, uint32_t xof_len, uint64_t h[8]) {
  for (int i = 0; i < 8; ++i) h[i] = IV[i];
  h[0] ^= 0x01010040ull;
  h[1] ^= (uint64_t)xof_len << 32;
  size_t off = 0;
  while (len - off > 128) {
    compress(h, data + off, (uint64_t)off + 128, false);
    off += 128;
  }
  uint8_t lastb[128];
  memset(lastb, 0, 128);
  if (len > off) memcpy(lastb, data + off, len - off);
  compress(h, lastb, (uint64_t)len, true);
}
}  // namespace host_blake2

// d_t (WS_HAE_T) <- the n 16-byte exponents of hashPubKeysToExponents (blsHAE.go:80-93) for the keys' wire bytes
template <class C>
int hae_exponents_dev(Ctx& c, hipStream_t st, const uint8_t* h_keys, size_t n, void** d_t) {
  typedef Engine<C> E;
  if (n >= (1ull << 28)) return fail(BGLS_ERR_ARG, "XOF length 16 n must fit a uint32 (blsHAE.go:81)");
  int rc;
  void* d_root;
  if ((rc = c.get(WS_HAE_ROOT, 64, &d_root))) return rc;
  if ((rc = c.get(WS_HAE_T, n * 16, d_t))) return rc;
  if (n == 0) return 0;
  uint64_t root[8];
  const uint32_t xof_len = (uint32_t)(16 * n);
  host_blake2::xb_root(h_keys, n * E::G2B, xof_len, root);
  HIPCHK(hipMemcpyAsync(d_root, root, 64, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));                          // root[] is a stack buffer
  kl::blake2x_expand(st, (const uint64_t*)d_root, xof_len, (uint8_t*)*d_t);
  HIPCHK(hipGetLastError());
  return 0;
}

template <class C>
int hae_exponents_t(const uint8_t* keys, size_t n, uint8_t* t_out) {
  Call k;
  if (k.rc) return k.rc;
  int rc;
  void* d_t;
  if ((rc = hae_exponents_dev<C>(k.c, k.st, keys, n, &d_t))) return rc;
  if (n) HIPCHK(hipMemcpyAsync(t_out, d_t, n * 16, hipMemcpyDeviceToHost, k.st));
  HIPCHK(hipStreamSynchronize(k.st));
  return 0;
}

// Weighted sums below this many points keep one double-and-add per point (bgls_set_msm_min; tests pin both paths)
std::atomic<size_t> g_msm_min{32};
// bgls_set_msm_plan: window bits << 8 | threads per bucket forced on every weighted sum (0 = by size each); tests walk every plan with it
std::atomic<int> g_msm_plan{0};

// d_out (affine bytes) <- sum_i w_i P_i over device-resident points and 16-byte weights, one scalar multiplication per
// point (k_wsum_first) followed by the addition tree
template <class C>
int weighted_sum_naive(Ctx& c, hipStream_t st, int group, const uint8_t* d_pts, const uint8_t* d_w16, const uint8_t* d_signs, size_t n,
                       uint8_t* d_out, uint32_t* d_flags) {
  void *ja, *jb;
  int rc;
  const size_t JB = kl::jac_bytes<C>(group);
  if ((rc = c.get(WS_JAC_A, (n + 1) * JB, &ja))) return rc;
  if ((rc = c.get(WS_JAC_B, (n / 2 + 2) * JB, &jb))) return rc;
  kl::wsum_first<C>(st, group, d_pts, d_w16, d_signs, n, ja, d_flags);
  void *a = ja, *b = jb;
  size_t cnt = n;
  while (cnt > 1) {
    size_t r16 = (cnt + 131071) / 131072;                 // same fan-in rule as Engine::sum_points
    const int R = (int)(r16 < 2 ? 2 : r16 > 16 ? 16 : r16);
    size_t nout = (cnt + R - 1) / R;
    kl::sum_next<C>(st, group, a, cnt, R, b);
    void* t = a;
    a = b;
    b = t;
    cnt = nout;
  }
  kl::jac_to_bytes<C>(st, group, a, 1, d_out);
  HIPCHK(hipGetLastError());
  return 0;
}

// The same sum by the bucket method (k_msm.hip): n W mixed additions instead of n (128 doublings + 64 additions).
// Bucket populations are only balanced for weights that look random (hashed exponents do); when the largest bucket is
// far above the mean -- small multiplicities, repeated weights -- the per-point form is the faster one and is used.
// The top window holds only 128 - c (W - 1) bits (two at c = 6, 7 and 9; seven or eight at c = 11 and 12), so with uniform 128-bit
// weights its buckets alone exceed the bound at the sizes that choose these widths, and such sums take the per-point form: measured
// the faster one there (a thread per bucket walks the top window's long lists alone).
template <class C>
int weighted_sum_dev(Ctx& c, hipStream_t st, int group, const uint8_t* d_pts, const uint8_t* d_w16, const uint8_t* d_signs, size_t n,
                     uint8_t* d_out, uint32_t* d_flags) {
  const size_t PTB = group == BGLS_G1 ? Engine<C>::G1B : Engine<C>::G2B;
  if (n == 0) {
    HIPCHK(hipMemsetAsync(d_out, 0, PTB, st));
    return 0;
  }
  if (n >= MAX_BATCH) return too_large();
  Scope sc(c, st, ST_SUM);
  const int forced = g_msm_plan.load();
  const kl::MsmPlan p = kl::msm_plan(n, forced >> 8, forced & 255);
  uint32_t* last = c.msm_last;                                                          // path, c, S, W, largest bucket, listed pairs
  last[0] = 0; last[1] = (uint32_t)p.c; last[2] = (uint32_t)p.S; last[3] = (uint32_t)p.W; last[4] = last[5] = 0;
  if (n < g_msm_min.load() || (uint64_t)n * (uint64_t)p.W >= (1ull << 32))            // list positions are 32-bit
    return weighted_sum_naive<C>(c, st, group, d_pts, d_w16, d_signs, n, d_out, d_flags);
  const size_t JB = kl::jac_bytes<C>(group);
  void *aff, *cnt, *start, *list, *buckets, *tail;
  int rc;
  if ((rc = c.get(WS_MSM_AFF, n * kl::msm_aff_bytes<C>(group), &aff))) return rc;
  if ((rc = c.get(WS_MSM_CNT, ((size_t)p.NB + 2) * 4, &cnt))) return rc;
  if ((rc = c.get(WS_MSM_START, ((size_t)p.NB + 1) * 4, &start))) return rc;
  if ((rc = c.get(WS_MSM_LIST, n * (size_t)p.W * 4, &list))) return rc;
  if ((rc = c.get(WS_JAC_A, (size_t)p.NB * p.S * JB, &buckets))) return rc;
  const size_t half = p.S > 1 ? (size_t)p.NB * p.S / 2 : 0;                  // second buffer of the partials' pairwise folds
  if ((rc = c.get(WS_JAC_B, (half + kl::msm_tail_points(p)) * JB, &tail))) return rc;
  uint32_t* d_meta = (uint32_t*)cnt + p.NB;
  HIPCHK(hipMemsetAsync(cnt, 0, ((size_t)p.NB + 2) * 4, st));
  kl::msm_parse<C>(st, group, d_pts, d_w16, d_signs, n, p, aff, (uint32_t*)cnt, d_flags);
  kl::msm_scan(st, (uint32_t*)cnt, p.NB, (uint32_t*)start, d_meta);
  HIPCHK(hipGetLastError());
  uint32_t meta[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(meta, d_meta, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const size_t mean = n >> p.c;
  last[4] = meta[0];
  last[5] = meta[1];
  last[0] = meta[0] > (mean * 8 > 64 ? mean * 8 : 64) ? 2 : 1;
  if (last[0] == 2) return weighted_sum_naive<C>(c, st, group, d_pts, d_w16, d_signs, n, d_out, d_flags);
  void* res = nullptr;
  kl::msm_scatter<C>(st, group, aff, d_w16, n, p, (uint32_t*)cnt, (uint32_t*)list);
  kl::msm_buckets<C>(st, group, aff, (const uint32_t*)list, (const uint32_t*)start, p, buckets);
  void *a = buckets, *b = tail;
  for (size_t cntp = (size_t)p.NB * p.S; cntp > p.NB; cntp /= 2) {            // S partials per bucket -> one, halving
    kl::sum_pair<C>(st, group, a, cntp, b);
    std::swap(a, b);
  }
  kl::msm_tail<C>(st, group, a, p, (uint8_t*)tail + half * JB, &res);
  kl::jac_to_bytes<C>(st, group, res, 1, d_out);
  HIPCHK(hipGetLastError());
  return 0;
}

// verify_multi with apk = sum w_i pk_i: VerifyMultiSignatureWithHAE (blsHAE.go:56-58; weights hashed from the keys) when
// mult == nullptr, the core of KoskVerifyMultiSignatureWithMultiplicity (blsKosk.go:137-150) otherwise.
template <class C>
int verify_multi_weighted_t(const uint8_t* sig, const uint8_t* keys, const int64_t* mult, size_t n, const uint8_t* msg, size_t msg_len) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void *d_sig, *d_keys, *d_msg, *d_apk, *d_fl2, *d_t = nullptr, *d_sg = nullptr;
  if ((rc = c.get(WS_IN_A, E::G1B, &d_sig))) return rc;
  if ((rc = c.get(WS_IN_B, n * E::G2B, &d_keys))) return rc;
  if ((rc = c.get(WS_IN_C, msg_len, &d_msg))) return rc;
  if ((rc = c.get(WS_HAE_APK, E::G2B, &d_apk))) return rc;
  if ((rc = c.get(WS_FLAGS2, 16, &d_fl2))) return rc;
  HIPCHK(hipMemsetAsync(d_fl2, 0, 4, st));
  HIPCHK(hipMemcpyAsync(d_sig, sig, E::G1B, hipMemcpyHostToDevice, st));
  if (n) HIPCHK(hipMemcpyAsync(d_keys, keys, n * E::G2B, hipMemcpyHostToDevice, st));
  if (msg_len) HIPCHK(hipMemcpyAsync(d_msg, msg, msg_len, hipMemcpyHostToDevice, st));
  if (!mult) {
    if ((rc = hae_exponents_dev<C>(c, st, keys, n, &d_t))) return rc;
  } else {
    std::vector<uint8_t> w(n * 16, 0), sg(n, 0);
    for (size_t i = 0; i < n; ++i) {
      const int64_t m = mult[i];
      uint64_t mag = m < 0 ? (uint64_t)0 - (uint64_t)m : (uint64_t)m;
      sg[i] = m < 0 ? 1 : 0;
      for (int b = 0; b < 8; ++b) w[i * 16 + 15 - b] = (uint8_t)(mag >> (8 * b));
    }
    if ((rc = c.get(WS_HAE_T, n * 16, &d_t))) return rc;
    if ((rc = c.get(WS_HAE_SIGN, n, &d_sg))) return rc;
    if (n) {
      HIPCHK(hipMemcpyAsync(d_t, w.data(), n * 16, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_sg, sg.data(), n, hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));                      // w, sg are locals
    }
  }
  if ((rc = weighted_sum_dev<C>(c, st, BGLS_G2, (const uint8_t*)d_keys, (const uint8_t*)d_t, (const uint8_t*)d_sg, n,
                                                   (uint8_t*)d_apk, (uint32_t*)d_fl2)))
    return rc;
  if ((rc = read_flags(c, st, d_fl2, false))) return rc;
  return verify_multi_dev_t<C>(c, st, (const uint8_t*)d_sig, (const uint8_t*)d_apk, 1, (const uint8_t*)d_msg, msg_len);
}

// getAggregatePubKey over device-resident points and weights (blsHAE.go:74-77): d_out <- sum_i w_i P_i as affine bytes
template <class C>
int weighted_sum_dev_t(int group, const void* d_pts, const void* d_w16, size_t n, void* d_out, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void* d_flags;
  if ((rc = c.get(WS_FLAGS2, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if ((rc = weighted_sum_dev<C>(c, st, group, (const uint8_t*)d_pts, (const uint8_t*)d_w16, nullptr, n, (uint8_t*)d_out, (uint32_t*)d_flags)))
    return rc;
  return read_flags(c, st, d_flags, true);
}

// VerifyAggregateSignatureWithHAE (blsHAE.go:49-53): keys scaled by their exponents, then verifyAggSig with duplicates allowed
template <class C>
int verify_aggregate_hae_t(const uint8_t* sig, const uint8_t* keys, const uint8_t* blob, const uint64_t* off, size_t n) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  MsgView mv;
  void *d_sig, *d_keys, *d_flags, *d_part, *d_t;
  if ((rc = upload_msgs(c, st, blob, off, n, &mv))) return rc;
  if ((rc = c.put(st, WS_IN_A, sig, E::G1B, &d_sig))) return rc;
  if ((rc = c.put(st, WS_IN_B, keys, n * E::G2B, &d_keys))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  if ((rc = c.get(WS_PART, E::GTB, &d_part))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if ((rc = hae_exponents_dev<C>(c, st, keys, n, &d_t))) return rc;
  // e(H(m_i), t_i pk_i) = e(t_i H(m_i), pk_i): the exponent goes to the G1 side (a third of the G2 work, same GT value)
  if ((rc = E::miller_product(c, st, (const uint8_t*)d_sig, (const uint8_t*)d_keys, mv, n, 0, (uint8_t*)d_part, (uint32_t*)d_flags,
                              (const uint8_t*)d_t)))
    return rc;
  return E::finalize(c, st, (const uint8_t*)d_part, 1, 1, (const uint32_t*)d_flags, nullptr);
}

// AggregateSignaturesWithHAE (blsHAE.go:39-46): sum_i t_i sigma_i
template <class C>
int aggregate_signatures_hae_t(const uint8_t* sigs, const uint8_t* keys, size_t n, uint8_t* out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void *d_sigs, *d_out, *d_flags, *d_t;
  if ((rc = c.get(WS_IN_B, n * E::G1B, &d_sigs))) return rc;
  if ((rc = c.get(WS_OUT, E::G1B, &d_out))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if (n) HIPCHK(hipMemcpyAsync(d_sigs, sigs, n * E::G1B, hipMemcpyHostToDevice, st));
  if ((rc = hae_exponents_dev<C>(c, st, keys, n, &d_t))) return rc;
  if ((rc = weighted_sum_dev<C>(c, st, BGLS_G1, (const uint8_t*)d_sigs, (const uint8_t*)d_t, nullptr, n, (uint8_t*)d_out,
                                                   (uint32_t*)d_flags)))
    return rc;
  return read_flags(c, st, d_flags, false, out, d_out, E::G1B);
}

// ---- n_sets VerifyMultiSignatureWithHAE calls in one set of launches (bgls_verify_multi_hae_sets) -------------------------------
// Sets with more keys than this have their BLAKE2Xb root computed on the host by the host-pointer entries (bgls_set_hae_root_host_min;
// tests pin both paths).  A root is one sequential compression chain, much slower on one GPU lane than on the host: the host takes the
// few sets whose lone chain would hold up the batch (DESIGN.md, batched HAE multi-signatures).
std::atomic<size_t> g_hae_root_host_min{2048};

// The exponents of n_sets key sets (hashPubKeysToExponents per set, blsHAE.go:80-93), staged on the host: the node table of the XOF
// expansion and the roots of the sets above host_min when the keys' host bytes are given (h_keys), else none.  koff: the n_sets + 1
// offsets from 0, checked.  stage() returns with the stream synchronised (its tables, and the caller's offsets, have landed).  launch() then runs k_hae_root_seg and k_hae_expand_seg: set b's exponents at d_t + 16 koff[b].
template <class C>
struct HaeSets {
  const uint8_t* d_keys;
  const uint64_t* d_koff;
  size_t n_sets, n_host = 0, n_nodes = 0, host_min = SIZE_MAX;
  uint64_t* d_roots = nullptr;
  uint32_t* d_nodes = nullptr;
  uint8_t* d_t = nullptr;
  int stage(Ctx& c, hipStream_t st, const uint64_t* koff, const uint8_t* h_keys, size_t host_min_) {
    constexpr size_t G2B = Engine<C>::G2B;
    if (h_keys) host_min = host_min_;
    std::vector<uint64_t> host;                            // records of nine words: set index, root
    std::vector<uint32_t> nodes;                           // (set, node index) per 64-byte XOF node
    nodes.reserve(2 * (koff[n_sets] / 4 + n_sets));
    for (size_t b = 0; b < n_sets; ++b) {
      const size_t nk = koff[b + 1] - koff[b];
      const uint32_t xof_len = (uint32_t)(16 * nk);
      for (uint32_t i = 0; 64ull * i < xof_len; ++i) {
        nodes.push_back((uint32_t)b);
        nodes.push_back(i);
      }
      if (nk > host_min) {
        host.push_back(b);
        host.resize(host.size() + 8);
        host_blake2::xb_root(h_keys + koff[b] * G2B, nk * G2B, xof_len, host.data() + host.size() - 8);
      }
    }
    n_host = host.size() / 9;
    n_nodes = nodes.size() / 2;
    void *roots, *nd, *t;
    int rc;
    if ((rc = c.get(WS_HAE_ROOT, (n_sets * 8 + host.size()) * 8, &roots))) return rc;
    if ((rc = c.get(WS_HAE_NODES, (nodes.size() + 2) * 4, &nd))) return rc;
    if ((rc = c.get(WS_HAE_T, (koff[n_sets] + 1) * 16, &t))) return rc;
    d_roots = (uint64_t*)roots;
    d_nodes = (uint32_t*)nd;
    d_t = (uint8_t*)t;
    if (n_host) HIPCHK(hipMemcpyAsync(d_roots + n_sets * 8, host.data(), host.size() * 8, hipMemcpyHostToDevice, st));
    if (n_nodes) HIPCHK(hipMemcpyAsync(d_nodes, nodes.data(), nodes.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                       // host, nodes are locals
    return 0;
  }
  void launch(hipStream_t st) const {
    kl::hae_root_seg(st, d_keys, d_koff, n_sets, (unsigned)Engine<C>::G2B, host_min, d_roots + n_sets * 8, n_host, d_roots);
    kl::hae_expand_seg(st, d_roots, d_nodes, n_nodes, d_koff, d_t);
  }
};

// the key sums apk_b = sum_i t_i pk_i of the staged sets, as wire bytes to d_apks: k_hae_wsum_main (P partials per set), then the tree
// levels of Engine::sum_sets.  A 128-bit multiplication costs about as much as 200 mixed additions, so P is planned for lanes rather
// than for keys per lane: up to 2^18 lanes (four rounds of one wave per SIMD), a power of two no larger than the largest set.
template <class C>
int hae_sets_sum(Ctx& c, hipStream_t st, const HaeSets<C>& hs, size_t max_set, uint8_t* d_apks, uint32_t* d_flags) {
  const size_t n_sets = hs.n_sets;
  size_t P = 1;
  while (2 * P <= max_set && n_sets * 2 * P <= ((size_t)1 << 18)) P *= 2;
  const size_t written = n_sets * P, JB = kl::jac_bytes<C>(BGLS_G2);
  if ((written + 1) * JB > ((size_t)8 << 30)) return fail(BGLS_ERR_ARG, "too many key sets for one call (cut the batch: at most 8 GiB of partial sums)");
  void *ja, *jb;
  int rc;
  if ((rc = c.get(WS_JAC_A, (written + 1) * JB, &ja))) return rc;
  if ((rc = c.get(WS_JAC_B, (written / 2 + 2) * JB, &jb))) return rc;
  {
    Scope sc(c, st, ST_HAE_KEYS);
    hs.launch(st);
    kl::hae_wsum_main<C>(st, hs.d_keys, hs.d_koff, hs.d_t, n_sets, (unsigned)P, ja, d_flags);
  }
  {
    Scope sc(c, st, ST_SUM);
    Engine<C>::sum_sets_tree(st, BGLS_G2, ja, jb, P, n_sets, d_apks);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

template <class C>
int hae_exponents_sets_t(const uint8_t* keys, const uint64_t* key_off, size_t n_sets, uint8_t* t_out) {
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void *d_keys, *d_koff;
  std::vector<uint64_t> rel;
  if ((rc = upload_key_sets(c, st, Engine<C>::G2B, keys, key_off, n_sets, &d_keys, &d_koff, rel))) return rc;
  HaeSets<C> hs{(const uint8_t*)d_keys, (const uint64_t*)d_koff, n_sets};
  if ((rc = hs.stage(c, st, rel.data(), keys + key_off[0] * Engine<C>::G2B, g_hae_root_host_min.load()))) return rc;   // synchronises: rel has landed
  hs.launch(st);
  HIPCHK(hipGetLastError());
  if (rel[n_sets]) HIPCHK(hipMemcpyAsync(t_out + 16 * key_off[0], hs.d_t, rel[n_sets] * 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

template <class C>
int verify_multi_hae_sets_t(const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t n_sets, const uint8_t* blob, const uint64_t* off,
                            uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  if (c.res_pending) return in_flight();                  // before the staging below overwrites the exponents' workspaces
  size_t max_set = 0;
  MsgView mv;
  void *d_sigs, *d_keys, *d_koff;
  std::vector<uint64_t> rel;
  if ((rc = offsets_ok("key_off", key_off, n_sets, 0, SIZE_MAX, &max_set))) return rc;
  if ((rc = upload_key_sets(c, st, E::G2B, keys, key_off, n_sets, &d_keys, &d_koff, rel))) return rc;
  if ((rc = c.put(st, WS_IN_A, sigs, n_sets * E::G1B, &d_sigs))) return rc;
  if ((rc = upload_msgs(c, st, blob, off, n_sets, &mv))) return rc;
  HaeSets<C> hs{(const uint8_t*)d_keys, (const uint64_t*)d_koff, n_sets};
  if ((rc = hs.stage(c, st, rel.data(), keys + key_off[0] * E::G2B, g_hae_root_host_min.load()))) return rc;   // synchronises: rel has landed
  return verify_sets_run<C>(c, st, (const uint8_t*)d_sigs, n_sets, mv, verdicts, apk_out, gt_out,
                            [&](uint8_t* d_apks, uint32_t* d_flags) { return hae_sets_sum<C>(c, st, hs, max_set, d_apks, d_flags); });
}

template <class C>
int verify_multi_hae_sets_dev_t(const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets, size_t max_set, const void* d_msgs,
                                size_t msg_len, size_t msg_stride, uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out, void* stream) {
  Call k(stream);
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  if (c.res_pending) return in_flight();
  std::vector<uint64_t> koff;                             // the node table of the expansion is built from this copy
  if ((rc = fetch_key_off(st, d_key_off, n_sets, max_set, true, d_keys, koff))) return rc;
  HaeSets<C> hs{(const uint8_t*)d_keys, (const uint64_t*)d_key_off, n_sets};
  if ((rc = hs.stage(c, st, koff.data(), nullptr, 0))) return rc;
  MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return verify_sets_run<C>(c, st, (const uint8_t*)d_sigs, n_sets, mv, verdicts, apk_out, gt_out,
                            [&](uint8_t* d_apks, uint32_t* d_flags) { return hae_sets_sum<C>(c, st, hs, max_set, d_apks, d_flags); });
}

// ---- n AmsVerifySignature calls in one set of launches (bgls_ams_verify_batch, bgls/blsAsmSigs.go:48-59) ------------------------
// The offsets of the n + total hash inputs of a batch, appended to tab: input b < n is 0x00 || m_b (msg_off, or msg_len where it is
// NULL), input n + s is 0x01 || apk || strconv.Itoa(signers[s]) -- g2b key bytes and 1 to 10 digits.
void ams_hash_offsets(std::vector<uint64_t>& tab, const uint32_t* signers, size_t n, size_t total, const uint64_t* msg_off, size_t msg_len, size_t g2b) {
  uint64_t at = 0;
  tab.reserve(tab.size() + n + total + 1);
  for (size_t b = 0; b < n; ++b) {
    tab.push_back(at);
    at += 1 + (msg_off ? msg_off[b + 1] - msg_off[b] : msg_len);
  }
  for (size_t s = 0; s < total; ++s) {
    tab.push_back(at);
    unsigned digits = 1;
    for (uint32_t v = signers[s]; v >= 10; v /= 10) ++digits;
    at += 1 + g2b + digits;
  }
  tab.push_back(at);
}

// Engine::miller_ams and batch_verdicts_run's tail.  d_tab: the n + 1 signer offsets from 0, then the n + total + 1 offsets of the hash
// inputs (ams_hash_offsets; hbytes in all), on the device.
template <class C>
int ams_verify_run(Ctx& c, hipStream_t st, const uint8_t* d_apks, const uint8_t* d_agg_keys, const uint8_t* d_sigs, const uint32_t* d_signers,
                   const uint64_t* d_soff, const uint64_t* d_hoff, size_t n, size_t total, size_t max_signers, size_t hbytes, MsgView mv, uint8_t* verdicts,
                   uint8_t* gt_out) {
  return batch_verdicts_run<C>(c, st, n, {verdicts, gt_out}, [&](uint8_t* d_part, uint32_t* d_iflags, uint32_t* d_flags) {
    return Engine<C>::miller_ams(c, st, d_apks, d_agg_keys, d_sigs, d_signers, d_soff, n, total, max_signers, mv, d_hoff, hbytes, d_part, d_iflags, d_flags);
  });
}

template <class C>
int ams_verify_t(const uint8_t* apks, const uint8_t* agg_keys, const uint8_t* agg_sigs, const uint32_t* signers, const uint64_t* signer_off, size_t n,
                 const uint8_t* blob, const uint64_t* off, uint8_t* verdicts, uint8_t* gt_out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  if (c.res_pending) return in_flight();
  size_t max_signers = 0;
  if ((rc = offsets_ok("signer_off", signer_off, n, 0, SIZE_MAX, &max_signers))) return rc;
  const size_t s0 = signer_off[0], total = signer_off[n] - s0;
  std::vector<uint64_t> tab(n + 1);                       // alive until the stream has been synchronised below
  for (size_t b = 0; b <= n; ++b) tab[b] = signer_off[b] - s0;
  ams_hash_offsets(tab, total ? signers + s0 : nullptr, n, total, off, 0, E::G2B);
  MsgView mv;
  void *d_apks, *d_agg, *d_sigs, *d_signers, *d_tab;
  if ((rc = c.put(st, WS_IN_A, agg_sigs, n * E::G1B, &d_sigs))) return rc;
  if ((rc = c.put(st, WS_IN_B, apks, n * E::G2B, &d_apks))) return rc;
  if ((rc = c.put(st, WS_SEG_KEYS, agg_keys, n * E::G2B, &d_agg))) return rc;
  if ((rc = c.put(st, WS_AMS_SIGNERS, total ? signers + s0 : nullptr, total * 4, &d_signers))) return rc;
  if ((rc = c.put(st, WS_AMS_OFF, tab.data(), tab.size() * 8, &d_tab))) return rc;
  if ((rc = upload_msgs(c, st, blob, off, n, &mv))) return rc;
  HIPCHK(hipStreamSynchronize(st));                       // tab has landed
  return ams_verify_run<C>(c, st, (const uint8_t*)d_apks, (const uint8_t*)d_agg, (const uint8_t*)d_sigs, (const uint32_t*)d_signers, (const uint64_t*)d_tab,
                           (const uint64_t*)d_tab + n + 1, n, total, max_signers, tab.back(), mv, verdicts, gt_out);
}

// The n + 1 signer offsets of the device form, checked: from 0, monotone, no list above max_signers, n + total below 2^30, indices non-NULL.
int ams_offsets_ok(const std::vector<uint64_t>& soff, size_t n, size_t max_signers, const void* d_signers) {
  int rc;
  if ((rc = offsets_ok("signer_off", soff.data(), n, OFF_FROM_ZERO, max_signers))) return rc;
  if (n + soff[n] >= MAX_BATCH) return too_large();
  if (soff[n] && !d_signers) return fail(BGLS_ERR_ARG, "NULL argument");
  return 0;
}

// The signer offsets are the caller's device words, copied back and checked before any launch (as fetch_key_off).  A process without a
// device has no device memory: there the words are read where they lie, so that a bad argument is still BGLS_ERR_ARG, and everything
// else BGLS_ERR_NO_DEVICE.
template <class C>
int ams_verify_dev_t(const void* d_apks, const void* d_agg_keys, const void* d_sigs, const void* d_signers, const void* d_signer_off, size_t n,
                     size_t max_signers, const void* d_msgs, size_t msg_len, size_t msg_stride, uint8_t* verdicts, uint8_t* gt_out, void* stream) {
  typedef Engine<C> E;
  Call k(stream);
  std::vector<uint64_t> soff(n + 1);
  int rc;
  if (k.rc == BGLS_ERR_NO_DEVICE) {
    const std::string why = g_err;
    memcpy(soff.data(), d_signer_off, (n + 1) * 8);
    if ((rc = ams_offsets_ok(soff, n, max_signers, d_signers))) return rc;
    return fail(BGLS_ERR_NO_DEVICE, why.c_str());
  }
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  if (c.res_pending) return in_flight();
  HIPCHK(hipMemcpyAsync(soff.data(), d_signer_off, (n + 1) * 8, hipMemcpyDefault, st));
  HIPCHK(hipStreamSynchronize(st));
  if ((rc = ams_offsets_ok(soff, n, max_signers, d_signers))) return rc;
  const size_t total = soff[n];
  // the digits of an index set the length of its hash input: the indices come back once for the offsets of the inputs
  std::vector<uint32_t> idx(total);
  if (total) HIPCHK(hipMemcpyAsync(idx.data(), d_signers, total * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<uint64_t> tab;
  ams_hash_offsets(tab, idx.data(), n, total, nullptr, msg_len, E::G2B);
  void* d_tab;
  if ((rc = c.put(st, WS_AMS_OFF, tab.data(), tab.size() * 8, &d_tab))) return rc;
  HIPCHK(hipStreamSynchronize(st));                       // tab has landed
  MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  return ams_verify_run<C>(c, st, (const uint8_t*)d_apks, (const uint8_t*)d_agg_keys, (const uint8_t*)d_sigs, (const uint32_t*)d_signers,
                           (const uint64_t*)d_signer_off, (const uint64_t*)d_tab, n, total, max_signers, tab.back(), mv, verdicts, gt_out);
}

// Marshal / Unmarshal* compressed branch over a batch.  alt-bn128: the reference's own 32 / 64-byte forms
// (curves/altbn128.go:81-89,203-221,296-376).  BLS12-381: 48 / 96 bytes in the ebfull/pairing layout the reference names as
// its target (curves/bls12_381.go:54-62,115-123,242-264; wire.hpp) -- unpinned against the un-vendored dis2/bls12.
int wire_points(int curve, int group, bool compress, const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok) {
  if (curve != BGLS_CURVE_ALTBN128 && curve != BGLS_CURVE_BLS12_381) return fail(BGLS_ERR_ARG, "unknown curve id");
  const bool bls = curve == BGLS_CURVE_BLS12_381;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  if (n == 0) return 0;
  const size_t CB = (bls ? 48 : 32) * (group == BGLS_G1 ? 1 : 2), UB = 2 * CB;
  const size_t in_b = compress ? UB : CB, out_b = compress ? CB : UB;
  void *d_in, *d_out, *d_ok, *d_flags;
  if ((rc = c.get(WS_IN_B, n * in_b, &d_in))) return rc;
  if ((rc = c.get(WS_IN_A, n * out_b, &d_out))) return rc;
  if ((rc = c.get(WS_IN_D, n, &d_ok))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  HIPCHK(hipMemcpyAsync(d_in, in, n * in_b, hipMemcpyHostToDevice, st));
  {
    Scope sc(c, st, ST_SUM);
    if (compress) {
      if (bls) kl::compress_bls(st, group, (const uint8_t*)d_in, n, (uint8_t*)d_out, (uint32_t*)d_flags);
      else kl::compress_bn(st, group, (const uint8_t*)d_in, n, (uint8_t*)d_out, (uint32_t*)d_flags);
    } else {
      if (bls) kl::decompress_bls(st, group, (const uint8_t*)d_in, n, (uint8_t*)d_out, (uint8_t*)d_ok);
      else kl::decompress_bn(st, group, (const uint8_t*)d_in, n, (uint8_t*)d_out, (uint8_t*)d_ok);
    }
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d_out, n * out_b, hipMemcpyDeviceToHost, st));
  if (!compress) HIPCHK(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, st));
  return read_flags(c, st, d_flags, true);
}

// window multiples of a generator for this device (DeviceTables), built on first use
template <class C>
int fixed_base_table(Ctx& c, int group, const void** out) {
  DeviceTables& t = tables_of(c.device);
  std::lock_guard<std::mutex> lk(t.mu);
  void*& slot = t.fixed_base[C::CURVE_ID][group - 1];
  if (!slot) {
    void* tab = nullptr;
    hipStream_t bs = nullptr;
    HIPCHK(hipMalloc(&tab, kl::fb_table_bytes<C>(group)));
    hipError_t e = hipStreamCreate(&bs);
    if (e == hipSuccess) {
      kl::fb_build<C>(bs, group, tab);
      e = hipGetLastError();
      if (e == hipSuccess) e = hipStreamSynchronize(bs);
    }
    if (bs) (void)hipStreamDestroy(bs);
    if (e != hipSuccess) {
      (void)hipFree(tab);
      return fail(BGLS_ERR_HIP, "building the fixed-base table", e);
    }
    slot = tab;
  }
  *out = slot;
  return 0;
}

// LoadPublicKey over a batch (bgls/bgls.go:40-43): out[i] = sk_i * g2 (group = BGLS_G2) or sk_i * g1, one mixed addition
// per scalar byte from the resident table of window multiples
template <class C>
int scale_generator_t(int group, const uint8_t* sks, size_t n, uint8_t* out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  if (n == 0) return 0;
  const size_t PB = group == BGLS_G1 ? E::G1B : E::G2B;
  void *d_sc, *d_out;
  const void* tab;
  if ((rc = fixed_base_table<C>(c, group, &tab))) return rc;
  if ((rc = c.get(WS_IN_C, n * 32, &d_sc))) return rc;
  if ((rc = c.get(WS_IN_A, n * PB, &d_out))) return rc;
  HIPCHK(hipMemcpyAsync(d_sc, sks, n * 32, hipMemcpyHostToDevice, st));
  kl::fb_scale<C>(st, group, tab, (const uint8_t*)d_sc, n, (uint8_t*)d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d_out, n * PB, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// Sign over a batch (bgls/bgls.go:46-56): out[i] = sk_i * HashToG1(msg_i); the hash points never leave the device
template <class C>
int sign_batch_t(const uint8_t* sks, const uint8_t* blob, const uint64_t* off, size_t n, uint8_t* out) {
  typedef Engine<C> E;
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  if (n == 0) return 0;
  MsgView mv;
  void *d_g1s, *d_out, *d_flags, *d_sc;
  if ((rc = upload_msgs(c, st, blob, off, n, &mv))) return rc;
  if ((rc = c.get(WS_G1S, n * sizeof(Aff<F1<C>>), &d_g1s))) return rc;
  if ((rc = c.get(WS_IN_A, n * E::G1B, &d_out))) return rc;
  if ((rc = c.get(WS_FLAGS, 16, &d_flags))) return rc;
  HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
  if ((rc = c.put(st, WS_IN_B, sks, n * 32, &d_sc))) return rc;
  if ((rc = E::hash_to_g1(c, st, mv, n, (Aff<F1<C>>*)d_g1s, (uint32_t*)d_flags))) return rc;
  if (C::CURVE_ID == 1 && g1x()) kl::scale_aff_g1x<C>(st, (const Aff<F1<C>>*)d_g1s, (const uint8_t*)d_sc, n, (uint8_t*)d_out);
  else kl::scale_aff<C>(st, BGLS_G1, (const Aff<F1<C>>*)d_g1s, (const uint8_t*)d_sc, n, (uint8_t*)d_out);
  HIPCHK(hipGetLastError());
  return read_flags(c, st, d_flags, false, out, d_out, n * E::G1B);
}


