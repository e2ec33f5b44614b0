// Host side, part 4 of 4 (included by engine.hip): the extern "C" entry points of include/bgls_hip.h.  Every body is a function-try-block
// closed by BGLS_ABI_GUARD (engine_core.inc): no C++ exception leaves the library.
// ======================================================================= C ABI
extern "C" {

int bgls_abi_version(void) { return 2; }

const char* bgls_last_error(void) { return g_err.c_str(); }

int bgls_init(int device) try {
  if (device < 0 || device >= MAX_DEVICES) return fail(BGLS_ERR_NO_DEVICE, "device index out of range");
  g_default_device.store(device);
  g_dev = -1;
  Ctx& c = ctx();
  std::lock_guard<std::mutex> lk(c.mu);
  return c.enter();
} BGLS_ABI_GUARD

size_t bgls_fp_size(int curve) { return curve == BGLS_CURVE_ALTBN128 ? 32 : curve == BGLS_CURVE_BLS12_381 ? 48 : 0; }
size_t bgls_g1_size(int curve) { return 2 * bgls_fp_size(curve); }
size_t bgls_g2_size(int curve) { return 4 * bgls_fp_size(curve); }
size_t bgls_gt_size(int curve) { return 12 * bgls_fp_size(curve); }

int bgls_verify_aggregate(int curve, const uint8_t* sig, const uint8_t* keys, const uint8_t* msg_blob, const uint64_t* msg_off,
                          size_t n, int allow_duplicates) try {
  if (n >= MAX_BATCH) return too_large();
  if (!sig || !msg_off || (n && !keys)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_aggregate_t<CV>(sig, keys, msg_blob, msg_off, n, allow_duplicates));
} BGLS_ABI_GUARD

int bgls_verify_aggregate_batch(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* inst_off, size_t n_inst, const uint8_t* msg_blob,
                                const uint64_t* msg_off, int allow_duplicates, uint8_t* verdicts, uint8_t* gt_out) try {
  if (n_inst >= MAX_BATCH) return too_large();
  if (!inst_off) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("inst_off", inst_off, n_inst, OFF_FROM_ZERO | OFF_TOTAL))) return rc;
  if (n_inst == 0) return 0;
  if (!sigs || !verdicts || !msg_off || (inst_off[n_inst] && !keys)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_aggregate_batch_t<CV>(sigs, keys, inst_off, n_inst, msg_blob, msg_off, allow_duplicates, verdicts, gt_out));
} BGLS_ABI_GUARD

int bgls_verify_aggregate_batch_dev(int curve, const void* d_sigs, const void* d_keys, const uint64_t* inst_off, size_t n_inst, const void* d_msgs,
                                    size_t msg_len, size_t msg_stride, int allow_duplicates, uint8_t* verdicts, uint8_t* gt_out, void* stream) try {
  if (n_inst >= MAX_BATCH) return too_large();
  if (!inst_off) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("inst_off", inst_off, n_inst, OFF_FROM_ZERO | OFF_TOTAL))) return rc;
  if (n_inst == 0) return 0;
  if (!d_sigs || !verdicts || (inst_off[n_inst] && (!d_keys || (msg_len && !d_msgs)))) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_aggregate_batch_dev_t<CV>(d_sigs, d_keys, inst_off, n_inst, d_msgs, msg_len, msg_stride, allow_duplicates, verdicts, gt_out, stream));
} BGLS_ABI_GUARD

// ---- aggregate verification that pairs once per distinct message: the grouping by exact bytes, and the verification on top of it
int bgls_group_messages(const uint8_t* msg_blob, const uint64_t* msg_off, size_t n, uint32_t* group_of, size_t* n_groups) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) {
    if (n_groups) *n_groups = 0;
    return 0;
  }
  if (!msg_off || !group_of) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("msg_off", msg_off, n, 0))) return rc;
  if (msg_off[n] > msg_off[0] && !msg_blob) return fail(BGLS_ERR_ARG, "NULL argument");
  return group_messages_t(msg_blob, msg_off, n, group_of, n_groups);
} BGLS_ABI_GUARD

int bgls_group_messages_dev(const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n, void* d_group_of, size_t* n_groups,
                            void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) {
    if (n_groups) *n_groups = 0;
    return 0;
  }
  if (!d_group_of || (msg_len && !d_msgs)) return fail(BGLS_ERR_ARG, "NULL argument");
  if (msg_stride < msg_len) return fail(BGLS_ERR_ARG, "msg_stride below msg_len");
  return group_messages_dev_t(d_msgs, msg_len, msg_stride, n, d_group_of, n_groups, stream);
} BGLS_ABI_GUARD

int bgls_verify_aggregate_grouped(int curve, const uint8_t* sig, const uint8_t* keys, const uint8_t* msg_blob, const uint64_t* msg_off,
                                  size_t n, size_t* n_groups, uint8_t* gt_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (!sig || !msg_off || (n && !keys)) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("msg_off", msg_off, n, 0))) return rc;
  if (msg_off[n] > msg_off[0] && !msg_blob) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n_groups) *n_groups = 0;
  DISPATCH(curve, verify_aggregate_grouped_t<CV>(sig, keys, msg_blob, msg_off, n, n_groups, gt_out));
} BGLS_ABI_GUARD

int bgls_verify_aggregate_grouped_dev(int curve, const void* d_sig, const void* d_keys, const void* d_msgs, size_t msg_len,
                                      size_t msg_stride, size_t n, size_t* n_groups, uint8_t* gt_out, void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (!d_sig || (n && (!d_keys || (msg_len && !d_msgs)))) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n && msg_stride < msg_len) return fail(BGLS_ERR_ARG, "msg_stride below msg_len");
  if (n_groups) *n_groups = 0;
  DISPATCH(curve, verify_aggregate_grouped_dev_t<CV>(d_sig, d_keys, d_msgs, msg_len, msg_stride, n, n_groups, gt_out, stream));
} BGLS_ABI_GUARD

// ---- distinct messages (bgls/blsDistinctMessage.go) and proofs of possession (bgls/blsKosk.go:59-69): the hash inputs are built on the device
int bgls_verify_aggregate_distinct(int curve, const uint8_t* sig, const uint8_t* keys, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n) try {
  if (n >= MAX_BATCH) return too_large();
  if (!sig || !msg_off || (n && !keys)) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("msg_off", msg_off, n, 0))) return rc;
  if (msg_off[n] > msg_off[0] && !msg_blob) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_aggregate_t<CV>(sig, keys, msg_blob, msg_off, n, 1, true));
} BGLS_ABI_GUARD

int bgls_verify_aggregate_distinct_batch(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* inst_off, size_t n_inst, const uint8_t* msg_blob,
                                         const uint64_t* msg_off, uint8_t* verdicts, uint8_t* gt_out) try {
  if (n_inst >= MAX_BATCH) return too_large();
  if (!inst_off) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("inst_off", inst_off, n_inst, OFF_FROM_ZERO | OFF_TOTAL))) return rc;
  if (n_inst == 0) return 0;
  if (!sigs || !verdicts || !msg_off || (inst_off[n_inst] && !keys)) return fail(BGLS_ERR_ARG, "NULL argument");
  if ((rc = offsets_ok("msg_off", msg_off, inst_off[n_inst], 0))) return rc;
  if (msg_off[inst_off[n_inst]] > msg_off[0] && !msg_blob) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_aggregate_batch_t<CV>(sigs, keys, inst_off, n_inst, msg_blob, msg_off, 1, verdicts, gt_out, true));
} BGLS_ABI_GUARD

int bgls_verify_aggregate_distinct_batch_dev(int curve, const void* d_sigs, const void* d_keys, const uint64_t* inst_off, size_t n_inst, const void* d_msgs,
                                             size_t msg_len, size_t msg_stride, uint8_t* verdicts, uint8_t* gt_out, void* stream) try {
  if (n_inst >= MAX_BATCH) return too_large();
  if (!inst_off) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("inst_off", inst_off, n_inst, OFF_FROM_ZERO | OFF_TOTAL))) return rc;
  if (n_inst == 0) return 0;
  if (!d_sigs || !verdicts || (inst_off[n_inst] && (!d_keys || (msg_len && !d_msgs)))) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_aggregate_batch_dev_t<CV>(d_sigs, d_keys, inst_off, n_inst, d_msgs, msg_len, msg_stride, 1, verdicts, gt_out, stream, true));
} BGLS_ABI_GUARD

int bgls_verify_single_distinct_batch(int curve, const uint8_t* sigs, const uint8_t* keys, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n,
                                      uint8_t* verdicts, uint8_t* gt_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (!msg_off) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("msg_off", msg_off, n, 0))) return rc;
  if (n == 0) return 0;
  if (!sigs || !keys || !verdicts || (msg_off[n] > msg_off[0] && !msg_blob)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_single_keyed_t<CV>(BGLS_KEYED_PREFIX, sigs, keys, msg_blob, msg_off, n, verdicts, gt_out));
} BGLS_ABI_GUARD

int bgls_verify_single_distinct_batch_dev(int curve, const void* d_sigs, const void* d_keys, size_t n, const void* d_msgs, size_t msg_len, size_t msg_stride,
                                          uint8_t* verdicts, uint8_t* gt_out, void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) return 0;
  if (!d_sigs || !d_keys || !verdicts || (msg_len && !d_msgs)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_single_distinct_dev_t<CV>(d_sigs, d_keys, n, d_msgs, msg_len, msg_stride, verdicts, gt_out, stream));
} BGLS_ABI_GUARD

int bgls_check_authentication_batch(int curve, const uint8_t* keys, const uint8_t* auths, size_t n, uint8_t* verdicts, uint8_t* gt_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) return 0;
  if (!keys || !auths || !verdicts) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_single_keyed_t<CV>(BGLS_KEYED_POP, auths, keys, nullptr, nullptr, n, verdicts, gt_out));
} BGLS_ABI_GUARD

int bgls_hash_to_g1_keyed(int curve, int mode, const uint8_t* keys, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n, uint8_t* g1_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (mode != BGLS_KEYED_PREFIX && mode != BGLS_KEYED_POP) return fail(BGLS_ERR_ARG, "mode must be BGLS_KEYED_PREFIX or BGLS_KEYED_POP");
  if (n && (!keys || !g1_out || (mode == BGLS_KEYED_PREFIX && !msg_off))) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n && mode == BGLS_KEYED_PREFIX) {
    int rc;
    if ((rc = offsets_ok("msg_off", msg_off, n, 0))) return rc;
    if (msg_off[n] > msg_off[0] && !msg_blob) return fail(BGLS_ERR_ARG, "NULL argument");
  }
  DISPATCH(curve, hash_to_g1_keyed_t<CV>(mode, keys, msg_blob, msg_off, n, g1_out));
} BGLS_ABI_GUARD

int bgls_verify_multi(int curve, const uint8_t* sig, const uint8_t* keys, size_t n, const uint8_t* msg, size_t msg_len) try {
  if (n >= MAX_BATCH) return too_large();
  if (!sig || (n && !keys) || (msg_len && !msg)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_t<CV>(sig, keys, n, msg, msg_len));
} BGLS_ABI_GUARD

int bgls_verify_multi_batch(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t n_sets, const uint8_t* msg_blob,
                            const uint64_t* msg_off, int allow_duplicates) try {
  if (n_sets >= MAX_BATCH) return too_large();
  if (!key_off || !msg_off || (n_sets && (!sigs || !msg_blob)) || (n_sets && key_off[n_sets] > key_off[0] && !keys)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_batch_t<CV>(sigs, keys, key_off, n_sets, msg_blob, msg_off, allow_duplicates));
} BGLS_ABI_GUARD

int bgls_aggregate_sets(int curve, int group, const uint8_t* pts, const uint64_t* set_off, size_t n_sets, uint8_t* out) try {
  if (!group_ok(group) || !set_off || (n_sets && !out) || (n_sets && set_off[n_sets] > set_off[0] && !pts)) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  DISPATCH(curve, aggregate_sets_t<CV>(group, pts, set_off, n_sets, out));
} BGLS_ABI_GUARD

int bgls_verify_multi_batch_dev(int curve, const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets, size_t max_set,
                                const void* d_msgs, size_t msg_len, size_t msg_stride, int allow_duplicates, void* stream) try {
  if (n_sets >= MAX_BATCH) return too_large();
  if (n_sets && (!d_sigs || !d_keys || !d_key_off || !d_msgs)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_batch_sub_t<CV>(d_sigs, d_keys, d_key_off, n_sets, max_set, d_msgs, msg_len, msg_stride, allow_duplicates, stream, false));
} BGLS_ABI_GUARD
int bgls_verify_multi_batch_submit_dev(int curve, const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets, size_t max_set,
                                       const void* d_msgs, size_t msg_len, size_t msg_stride, int allow_duplicates, void* stream) try {
  if (n_sets >= MAX_BATCH) return too_large();
  if (n_sets && (!d_sigs || !d_keys || !d_key_off || !d_msgs)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_batch_sub_t<CV>(d_sigs, d_keys, d_key_off, n_sets, max_set, d_msgs, msg_len, msg_stride, allow_duplicates, stream, true));
} BGLS_ABI_GUARD

int bgls_verify_multi_sets(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t n_sets, const uint8_t* msg_blob,
                           const uint64_t* msg_off, uint8_t* verdicts, uint8_t* gt_out) try {
  if (n_sets >= MAX_BATCH) return too_large();
  if (!key_off || !msg_off) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("key_off", key_off, n_sets, OFF_TOTAL))) return rc;
  if ((rc = offsets_ok("msg_off", msg_off, n_sets, 0))) return rc;
  if (n_sets == 0) return 0;
  if (!sigs || !verdicts || (msg_off[n_sets] && !msg_blob) || (key_off[n_sets] > key_off[0] && !keys)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_sets_t<CV>(sigs, keys, key_off, n_sets, msg_blob, msg_off, verdicts, gt_out));
} BGLS_ABI_GUARD

int bgls_verify_multi_sets_dev(int curve, const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets, size_t max_set, const void* d_msgs,
                               size_t msg_len, size_t msg_stride, uint8_t* verdicts, uint8_t* gt_out, void* stream) try {
  if (n_sets >= MAX_BATCH) return too_large();
  if (n_sets == 0) return 0;
  if (!d_sigs || !d_key_off || !verdicts || (msg_len && !d_msgs)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_sets_dev_t<CV>(d_sigs, d_keys, d_key_off, n_sets, max_set, d_msgs, msg_len, msg_stride, verdicts, gt_out, stream));
} BGLS_ABI_GUARD

int bgls_verify_multi_sets_combined(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t n_sets, const uint8_t* msg_blob,
                                    const uint64_t* msg_off, const uint64_t* group_off, size_t n_groups, const uint8_t* seed, uint8_t* verdicts,
                                    uint8_t* gt_out) try {
  if (n_sets >= MAX_BATCH) return too_large();
  if (!key_off || !msg_off) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("key_off", key_off, n_sets, OFF_TOTAL))) return rc;
  if ((rc = offsets_ok("msg_off", msg_off, n_sets, 0))) return rc;
  if ((rc = rlc_args_ok(group_off, n_groups, n_sets, seed))) return rc;
  if (n_sets == 0) return 0;
  if (!sigs || !verdicts || (msg_off[n_sets] && !msg_blob) || (key_off[n_sets] > key_off[0] && !keys)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_sets_combined_t<CV>(sigs, keys, key_off, n_sets, msg_blob, msg_off, group_off, n_groups, seed, verdicts, gt_out));
} BGLS_ABI_GUARD

int bgls_verify_multi_sets_combined_dev(int curve, const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets, size_t max_set,
                                        const void* d_msgs, size_t msg_len, size_t msg_stride, const uint64_t* group_off, size_t n_groups,
                                        const uint8_t* seed, uint8_t* verdicts, uint8_t* gt_out, void* stream) try {
  int rc;
  if ((rc = rlc_args_ok(group_off, n_groups, n_sets, seed))) return rc;
  if (n_sets == 0) return 0;
  if (!d_sigs || !d_key_off || !verdicts || (msg_len && !d_msgs)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_sets_combined_dev_t<CV>(d_sigs, d_keys, d_key_off, n_sets, max_set, d_msgs, msg_len, msg_stride, group_off, n_groups, seed,
                                                       verdicts, gt_out, stream));
} BGLS_ABI_GUARD

int bgls_rlc_coefficients(const uint8_t* seed, size_t n, uint8_t* r_out) try {
  if (n >= HAE_MAX_SET) return fail(BGLS_ERR_ARG, "XOF length 16 n must fit a uint32 (fewer than 2^28 coefficients)");
  if (!seed || (n && !r_out)) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n == 0) return 0;
  return rlc_coefficients_t(seed, n, r_out);
} BGLS_ABI_GUARD

int bgls_verify_multi_hae_sets(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t n_sets, const uint8_t* msg_blob,
                               const uint64_t* msg_off, uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out) try {
  if (n_sets >= MAX_BATCH) return too_large();
  if (!key_off || !msg_off) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("msg_off", msg_off, n_sets, 0))) return rc;
  if ((rc = offsets_ok("key_off", key_off, n_sets, OFF_HAE | OFF_TOTAL))) return rc;
  if (n_sets == 0) return 0;
  if (!sigs || !verdicts || (msg_off[n_sets] && !msg_blob) || (key_off[n_sets] > key_off[0] && !keys)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_hae_sets_t<CV>(sigs, keys, key_off, n_sets, msg_blob, msg_off, verdicts, apk_out, gt_out));
} BGLS_ABI_GUARD

int bgls_verify_multi_hae_sets_dev(int curve, const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets, size_t max_set,
                                   const void* d_msgs, size_t msg_len, size_t msg_stride, uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out,
                                   void* stream) try {
  if (n_sets >= MAX_BATCH) return too_large();
  if (n_sets == 0) return 0;
  if (!d_sigs || !d_key_off || !verdicts || (msg_len && !d_msgs)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_hae_sets_dev_t<CV>(d_sigs, d_keys, d_key_off, n_sets, max_set, d_msgs, msg_len, msg_stride, verdicts, apk_out, gt_out,
                                                  stream));
} BGLS_ABI_GUARD

int bgls_ams_verify_batch(int curve, const uint8_t* apks, const uint8_t* agg_keys, const uint8_t* agg_sigs, const uint32_t* signers,
                          const uint64_t* signer_off, size_t n, const uint8_t* msg_blob, const uint64_t* msg_off, uint8_t* verdicts, uint8_t* gt_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) return 0;
  if (!signer_off || !msg_off) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("signer_off", signer_off, n, 0))) return rc;
  if ((rc = offsets_ok("msg_off", msg_off, n, 0))) return rc;
  if (n + (signer_off[n] - signer_off[0]) >= MAX_BATCH) return too_large();
  if (!apks || !agg_keys || !agg_sigs || !verdicts || (msg_off[n] > msg_off[0] && !msg_blob) || (signer_off[n] > signer_off[0] && !signers))
    return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, ams_verify_t<CV>(apks, agg_keys, agg_sigs, signers, signer_off, n, msg_blob, msg_off, verdicts, gt_out));
} BGLS_ABI_GUARD

int bgls_ams_verify_batch_dev(int curve, const void* d_apks, const void* d_agg_keys, const void* d_agg_sigs, const void* d_signers, const void* d_signer_off,
                              size_t n, size_t max_signers, const void* d_msgs, size_t msg_len, size_t msg_stride, uint8_t* verdicts, uint8_t* gt_out,
                              void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) return 0;
  if (!d_apks || !d_agg_keys || !d_agg_sigs || !d_signer_off || !verdicts || (msg_len && !d_msgs)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, ams_verify_dev_t<CV>(d_apks, d_agg_keys, d_agg_sigs, d_signers, d_signer_off, n, max_signers, d_msgs, msg_len, msg_stride, verdicts, gt_out,
                                       stream));
} BGLS_ABI_GUARD

int bgls_set_ams_sum_cut(size_t n) try {
  if (n == 0) return fail(BGLS_ERR_ARG, "the cut must be at least one item");
  g_ams_sum_cut.store(n);
  return 0;
} BGLS_ABI_GUARD

int bgls_hae_exponents_sets(int curve, const uint8_t* keys, const uint64_t* key_off, size_t n_sets, uint8_t* t_out) try {
  if (n_sets >= MAX_BATCH) return too_large();
  if (!key_off) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("key_off", key_off, n_sets, OFF_HAE | OFF_TOTAL))) return rc;
  if (n_sets == 0) return 0;
  if (key_off[n_sets] > key_off[0] && (!keys || !t_out)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, hae_exponents_sets_t<CV>(keys, key_off, n_sets, t_out));
} BGLS_ABI_GUARD

int bgls_set_hae_root_host_min(size_t n) try {
  g_hae_root_host_min.store(n);
  return 0;
} BGLS_ABI_GUARD

int bgls_bb_verify_batch(int curve, const uint8_t* sigmas, const uint8_t* rs, const uint8_t* keys, const uint8_t* ms, size_t n, uint8_t* verdicts,
                         uint8_t* gt_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) return 0;
  if (!sigmas || !rs || !keys || !ms || !verdicts) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, bb_verify_t<CV>(sigmas, rs, keys, ms, n, verdicts, gt_out));
} BGLS_ABI_GUARD

int bgls_bb_verify_batch_dev(int curve, const void* d_sigmas, const void* d_rs, const void* d_keys, const void* d_ms, size_t n, uint8_t* verdicts,
                             uint8_t* gt_out, void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) return 0;
  if (!d_sigmas || !d_rs || !d_keys || !d_ms || !verdicts) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, bb_verify_dev_t<CV>(d_sigmas, d_rs, d_keys, d_ms, n, verdicts, gt_out, stream));
} BGLS_ABI_GUARD

int bgls_bb_verify_batch_combined(int curve, const uint8_t* sigmas, const uint8_t* rs, const uint8_t* keys, const uint8_t* ms, size_t n,
                                  const uint64_t* group_off, size_t n_groups, const uint8_t* seed, uint8_t* verdicts, uint8_t* gt_out) try {
  if (n == 0) return 0;                                   // before any pointer is looked at, as bgls_bb_verify_batch
  int rc;
  if ((rc = rlc_args_ok(group_off, n_groups, n, seed))) return rc;
  if (!sigmas || !rs || !keys || !ms || !verdicts) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, bb_verify_combined_t<CV>(sigmas, rs, keys, ms, n, group_off, n_groups, seed, verdicts, gt_out));
} BGLS_ABI_GUARD

int bgls_bb_verify_batch_combined_dev(int curve, const void* d_sigmas, const void* d_rs, const void* d_keys, const void* d_ms, size_t n,
                                      const uint64_t* group_off, size_t n_groups, const uint8_t* seed, uint8_t* verdicts, uint8_t* gt_out,
                                      void* stream) try {
  if (n == 0) return 0;                                   // before any pointer is looked at, as bgls_bb_verify_batch
  int rc;
  if ((rc = rlc_args_ok(group_off, n_groups, n, seed))) return rc;
  if (!d_sigmas || !d_rs || !d_keys || !d_ms || !verdicts) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, bb_verify_combined_dev_t<CV>(d_sigmas, d_rs, d_keys, d_ms, n, group_off, n_groups, seed, verdicts, gt_out, stream));
} BGLS_ABI_GUARD

int bgls_final_exp_batch(int curve, const uint8_t* gt_in, size_t n, uint8_t* gt_out, uint8_t* is_one) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) return 0;
  if (!gt_in || (!gt_out && !is_one)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, final_exp_batch_t<CV>(gt_in, n, gt_out, is_one));
} BGLS_ABI_GUARD

int bgls_final_exp_batch_dev(int curve, const void* d_gt_in, size_t n, void* d_gt_out, void* d_is_one, void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) return 0;
  if (!d_gt_in || (!d_gt_out && !d_is_one)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, final_exp_batch_dev_t<CV>(d_gt_in, n, d_gt_out, d_is_one, stream));
} BGLS_ABI_GUARD

int bgls_pair_batch(int curve, const uint8_t* g1s, const uint8_t* g2s, size_t n, uint8_t* gt_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) return 0;
  if (!g1s || !g2s || !gt_out) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, pair_batch_t<CV>(g1s, g2s, n, gt_out));
} BGLS_ABI_GUARD

int bgls_pair_batch_dev(int curve, const void* d_g1s, const void* d_g2s, size_t n, void* d_gt_out, void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) return 0;
  if (!d_g1s || !d_g2s || !d_gt_out) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, pair_batch_dev_t<CV>(d_g1s, d_g2s, n, d_gt_out, stream));
} BGLS_ABI_GUARD

int bgls_pairing_product(int curve, const uint8_t* g1s, const uint8_t* g2s, size_t n, uint8_t* gt_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (!gt_out || (n && (!g1s || !g2s))) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, pairing_product_t<CV>(g1s, g2s, n, gt_out));
} BGLS_ABI_GUARD

int bgls_hash_to_g1(int curve, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n, uint8_t* g1_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (n && (!msg_off || !g1_out)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, hash_to_g1_t<CV>(msg_blob, msg_off, n, g1_out));
} BGLS_ABI_GUARD

int bgls_aggregate_points(int curve, int group, const uint8_t* pts, size_t n, uint8_t* out) try {
  if (n >= MAX_BATCH) return too_large();
  if (!group_ok(group) || !out || (n && !pts)) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  DISPATCH(curve, aggregate_points_t<CV>(group, pts, n, out));
} BGLS_ABI_GUARD

int bgls_scale_points(int curve, int group, const uint8_t* pts, const uint8_t* scalars, const uint8_t* signs, size_t n,
                      uint8_t* out) try {
  if (n >= MAX_BATCH) return too_large();
  if (!group_ok(group) || (n && (!pts || !scalars || !out))) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  DISPATCH(curve, scale_points_t<CV>(group, pts, scalars, signs, n, out));
} BGLS_ABI_GUARD

int bgls_point_add(int curve, int group, const uint8_t* a, const uint8_t* b, uint8_t* out) try {
  if (!group_ok(group) || !a || !b || !out) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  size_t pb = group == BGLS_G1 ? bgls_g1_size(curve) : bgls_g2_size(curve);
  if (!pb) return fail(BGLS_ERR_ARG, "unknown curve id");
  std::vector<uint8_t> two(2 * pb);
  memcpy(two.data(), a, pb);
  memcpy(two.data() + pb, b, pb);
  return bgls_aggregate_points(curve, group, two.data(), 2, out);
} BGLS_ABI_GUARD

int bgls_point_check(int curve, int group, const uint8_t* a) try {
  if (!group_ok(group) || !a) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  DISPATCH(curve, point_check_t<CV>(group, a));
} BGLS_ABI_GUARD

int bgls_check_points(int curve, int group, const uint8_t* pts, size_t n, uint8_t* ok_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (!group_ok(group) || (n && (!pts || !ok_out))) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  DISPATCH(curve, check_points_t<CV>(group, pts, n, ok_out));
} BGLS_ABI_GUARD

int bgls_select_device(int device) try {
  if (device < -1 || device >= MAX_DEVICES) return fail(BGLS_ERR_NO_DEVICE, "device index out of range");
  g_dev = device;
  return 0;
} BGLS_ABI_GUARD

int bgls_keys_upload(int curve, const uint8_t* keys, size_t n, const int* devices, int n_devices, unsigned flags, bgls_keys_t* handle_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (!handle_out || (n && !keys)) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n_devices < 1 || n_devices > NCTX) return fail(BGLS_ERR_ARG, "n_devices out of range (1..16)");
  int dflt = cur_device();
  if (!devices && n_devices == 1) devices = &dflt;
  DISPATCH(curve, keys_upload_t<CV>(keys, n, devices, n_devices, flags, handle_out));
} BGLS_ABI_GUARD

int bgls_keys_upload_compressed(int curve, const uint8_t* keys_c, size_t n, const int* devices, int n_devices, unsigned flags, bgls_keys_t* handle_out,
                                size_t* first_bad) try {
  if (n >= MAX_BATCH) return too_large();
  if (!handle_out || (n && !keys_c)) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n_devices < 1 || n_devices > NCTX) return fail(BGLS_ERR_ARG, "n_devices out of range (1..16)");
  int dflt = cur_device();
  if (!devices && n_devices == 1) devices = &dflt;
  DISPATCH(curve, keys_upload_t<CV>(keys_c, n, devices, n_devices, flags | BGLS_KEYS_CHECK, handle_out, true, first_bad));
} BGLS_ABI_GUARD

int bgls_keys_read(bgls_keys_t handle, size_t first, size_t count, uint8_t* out) try {
  auto ks = keyset(handle);
  if (!ks) return fail(BGLS_ERR_ARG, "unknown key-set handle");
  if (first > ks->n || count > ks->n - first) return fail(BGLS_ERR_ARG, "key range beyond the set");
  if (count && !out) return fail(BGLS_ERR_ARG, "NULL argument");
  if (count == 0) return 0;
  DISPATCH(ks->curve, keys_read_t<CV>(*ks, first, count, out));
} BGLS_ABI_GUARD

int bgls_keys_free(bgls_keys_t handle) try {
  std::shared_ptr<KeySet> ks;
  {
    std::lock_guard<std::mutex> lk(g_keys_mu);
    auto it = g_keys.find(handle);
    if (it == g_keys.end()) return fail(BGLS_ERR_ARG, "unknown key-set handle");
    ks = it->second;
    g_keys.erase(it);
  }
  std::lock_guard<std::mutex> lk(ks->mu);      // wait for a verification in progress
  return 0;
} BGLS_ABI_GUARD

int bgls_keys_info(bgls_keys_t handle, int* curve, size_t* n, int* n_devices) try {
  auto ks = keyset(handle);
  if (!ks) return fail(BGLS_ERR_ARG, "unknown key-set handle");
  if (curve) *curve = ks->curve;
  if (n) *n = ks->n;
  if (n_devices) *n_devices = (int)ks->shards.size();
  return 0;
} BGLS_ABI_GUARD

int bgls_verify_aggregate_h(bgls_keys_t handle, const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n,
                            int allow_duplicates) try {
  if (n >= MAX_BATCH) return too_large();
  auto ks = keyset(handle);
  if (!ks) return fail(BGLS_ERR_ARG, "unknown key-set handle");
  if (!sig || !msg_off) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(ks->curve, verify_aggregate_h_t<CV>(*ks, sig, msg_blob, msg_off, n, allow_duplicates, nullptr));
} BGLS_ABI_GUARD

int bgls_verify_aggregate_h_gt(bgls_keys_t handle, const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n,
                               int allow_duplicates, uint8_t* gt_out) try {
  if (n >= MAX_BATCH) return too_large();
  auto ks = keyset(handle);
  if (!ks) return fail(BGLS_ERR_ARG, "unknown key-set handle");
  if (!sig || !msg_off || !gt_out) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(ks->curve, verify_aggregate_h_t<CV>(*ks, sig, msg_blob, msg_off, n, allow_duplicates, gt_out));
} BGLS_ABI_GUARD

int bgls_verify_aggregate_distinct_h(bgls_keys_t handle, const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n, uint8_t* gt_out) try {
  if (n >= MAX_BATCH) return too_large();
  auto ks = keyset(handle);
  if (!ks) return fail(BGLS_ERR_ARG, "unknown key-set handle");
  if (!sig || !msg_off) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n != ks->n) return fail(BGLS_ERR_ARG, "message count differs from the key set's size");
  int rc;
  if ((rc = offsets_ok("msg_off", msg_off, n, 0))) return rc;
  if (msg_off[n] > msg_off[0] && !msg_blob) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(ks->curve, verify_aggregate_h_t<CV>(*ks, sig, msg_blob, msg_off, n, 1, gt_out, true));
} BGLS_ABI_GUARD

int bgls_rccl_available(void) try { return rccl().ok ? 1 : 0; } BGLS_ABI_GUARD

// device-resident messages against a one-device key set, on the calling thread's context (several verifications in flight
// on several contexts: the handle's resident arrays are read-only)
int bgls_miller_product_keys_dev(bgls_keys_t handle, const void* d_sig, const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n,
                                 int check_duplicates, void* d_partial_out, void* d_flags, void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  auto ks = keyset(handle);
  if (!ks) return fail(BGLS_ERR_ARG, "unknown key-set handle");
  if (ks->shards.size() != 1) return fail(BGLS_ERR_ARG, "device entry point: the key set must live on one device");
  if (n != ks->n) return fail(BGLS_ERR_ARG, "message count differs from the key set's size");
  if (!d_partial_out || !d_flags || (n && !d_msgs && msg_len)) return fail(BGLS_ERR_ARG, "NULL argument");
  SelectionGuard keep_selection;
  g_dev = ks->shards[0].device;
  Ctx& c = ctx();
  int rc;
  {
    std::lock_guard<std::mutex> lk(c.mu);
    rc = [&]() -> int {
      int r;
      if ((r = c.enter())) return r;
      hipStream_t st = stream ? (hipStream_t)stream : c.stream;
      const KeyShard& sh = ks->shards[0];
      MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
      if (ks->curve == BGLS_CURVE_ALTBN128) {
        typedef Engine<BN254> E;
        if (check_duplicates && (r = E::dup_scan(c, st, mv, n, (uint32_t*)d_flags))) return r;
        if (ks->prepared) return E::miller_product_prepared(c, st, (const uint8_t*)d_sig, (const uint32_t*)sh.d_prep, (const uint8_t*)sh.d_kinf, sh.n_pad, sh.ng, mv, n, (uint8_t*)d_partial_out, (uint32_t*)d_flags);
        return E::miller_product(c, st, (const uint8_t*)d_sig, (const uint8_t*)sh.d_wire, mv, n, 0, (uint8_t*)d_partial_out, (uint32_t*)d_flags);
      }
      typedef Engine<BLS381> E;
      if (check_duplicates && (r = E::dup_scan(c, st, mv, n, (uint32_t*)d_flags))) return r;
      if (ks->prepared) return E::miller_product_prepared(c, st, (const uint8_t*)d_sig, (const uint32_t*)sh.d_prep, (const uint8_t*)sh.d_kinf, sh.n_pad, sh.ng, mv, n, (uint8_t*)d_partial_out, (uint32_t*)d_flags);
      return E::miller_product(c, st, (const uint8_t*)d_sig, (const uint8_t*)sh.d_wire, mv, n, 0, (uint8_t*)d_partial_out, (uint32_t*)d_flags);
    }();
  }
  return rc;
} BGLS_ABI_GUARD

// verifyMultiSignature against a one-device key set with signature and message already on the device, on the calling thread's
// context (several checks in flight on several contexts: the handle's resident arrays are read-only)
static int verify_multi_keys_dev(bgls_keys_t handle, const void* d_sig, const void* d_msg, size_t msg_len, void* stream, bool submit_only) {
  auto ks = keyset(handle);
  if (!ks) return fail(BGLS_ERR_ARG, "unknown key-set handle");
  if (ks->shards.size() != 1) return fail(BGLS_ERR_ARG, "device entry point: the key set must live on one device");
  if (!d_sig || (msg_len && !d_msg)) return fail(BGLS_ERR_ARG, "NULL argument");
  SelectionGuard keep_selection;
  g_dev = ks->shards[0].device;
  Ctx& c = ctx();
  int rc;
  {
    std::lock_guard<std::mutex> lk(c.mu);
    rc = [&]() -> int {
      int r;
      if ((r = c.enter())) return r;
      hipStream_t st = stream ? (hipStream_t)stream : c.stream;
      const KeyShard& sh = ks->shards[0];
      if (ks->curve == BGLS_CURVE_ALTBN128) {
        const bool ready = sum_pairs();
        return verify_multi_dev_t<BN254>(c, st, (const uint8_t*)d_sig, (const uint8_t*)(ready ? sh.d_sumr : sh.d_mont), ks->n, (const uint8_t*)d_msg, msg_len, submit_only, ready ? 2 : 1);
      }
      const bool ready = sum_pairs();
      return verify_multi_dev_t<BLS381>(c, st, (const uint8_t*)d_sig, (const uint8_t*)(ready ? sh.d_sumr : sh.d_mont), ks->n, (const uint8_t*)d_msg, msg_len, submit_only, ready ? 2 : 1);
    }();
  }
  return rc;
}
int bgls_verify_multi_keys_dev(bgls_keys_t handle, const void* d_sig, const void* d_msg, size_t msg_len, void* stream) try {
  return verify_multi_keys_dev(handle, d_sig, d_msg, msg_len, stream, false);
} BGLS_ABI_GUARD
int bgls_verify_multi_keys_submit_dev(bgls_keys_t handle, const void* d_sig, const void* d_msg, size_t msg_len, void* stream) try {
  return verify_multi_keys_dev(handle, d_sig, d_msg, msg_len, stream, true);
} BGLS_ABI_GUARD

int bgls_verify_multi_h(bgls_keys_t handle, const uint8_t* sig, const uint8_t* msg, size_t msg_len) try {
  auto ks = keyset(handle);
  if (!ks) return fail(BGLS_ERR_ARG, "unknown key-set handle");
  if (!sig || (msg_len && !msg)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(ks->curve, verify_multi_h_t<CV>(*ks, sig, msg, msg_len));
} BGLS_ABI_GUARD

// Multi-signatures by signer bitmap against a one-device key set.  Order of the refusals: what the arguments alone decide (NULL arrays,
// alignment), then the machine (no device: a handle can only come from an upload to one), then what the handle decides -- all before any
// device work.  n_sets == 0 returns 0 first of all.
static int subsets_no_device() {
  int cnt = 0;
  const hipError_t e0 = hipGetDeviceCount(&cnt);
  return (e0 != hipSuccess || cnt <= 0) ? fail(BGLS_ERR_NO_DEVICE, "no HIP device available", e0) : 0;
}
static int subsets_keyset(bgls_keys_t handle, size_t stride, size_t n_sets, std::shared_ptr<KeySet>* ks) {
  int rc;
  if ((rc = subsets_no_device())) return rc;
  if (!(*ks = keyset(handle))) return fail(BGLS_ERR_ARG, "unknown key-set handle");
  DISPATCH((*ks)->curve, subsets_args_ok<CV>(**ks, stride, n_sets));
}

int bgls_aggregate_subsets_h(bgls_keys_t handle, const uint8_t* bitmaps, size_t stride, size_t n_sets, uint8_t* out) try {
  if (n_sets == 0) return 0;
  if (n_sets >= MAX_BATCH) return too_large();
  if (!bitmaps || !out) return fail(BGLS_ERR_ARG, "NULL argument");
  std::shared_ptr<KeySet> ks;
  int rc;
  if ((rc = subsets_keyset(handle, stride, n_sets, &ks))) return rc;
  if (!subset_rows_clean(bitmaps, stride, n_sets, ks->n)) return fail(BGLS_ERR_ARG, "a signer bitmap has a bit at a position beyond the key set");
  DISPATCH(ks->curve, aggregate_subsets_t<CV>(*ks, bitmaps, stride, n_sets, out));
} BGLS_ABI_GUARD

int bgls_verify_multi_subsets_h(bgls_keys_t handle, const uint8_t* sigs, const uint8_t* bitmaps, size_t stride, size_t n_sets, const uint8_t* msg_blob,
                                const uint64_t* msg_off, uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out) try {
  if (n_sets == 0) return 0;
  if (n_sets >= MAX_BATCH) return too_large();
  if (!sigs || !bitmaps || !msg_off || !verdicts) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("msg_off", msg_off, n_sets, 0))) return rc;
  if (msg_off[n_sets] && !msg_blob) return fail(BGLS_ERR_ARG, "NULL argument");
  std::shared_ptr<KeySet> ks;
  if ((rc = subsets_keyset(handle, stride, n_sets, &ks))) return rc;
  if (!subset_rows_clean(bitmaps, stride, n_sets, ks->n)) return fail(BGLS_ERR_ARG, "a signer bitmap has a bit at a position beyond the key set");
  DISPATCH(ks->curve, verify_multi_subsets_t<CV>(*ks, sigs, bitmaps, stride, n_sets, msg_blob, msg_off, verdicts, apk_out, gt_out));
} BGLS_ABI_GUARD

int bgls_verify_multi_subsets_keys_dev(bgls_keys_t handle, const void* d_sigs, const void* d_bitmaps, size_t stride, size_t n_sets, const void* d_msgs,
                                       size_t msg_len, size_t msg_stride, uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out, void* stream) try {
  if (n_sets == 0) return 0;
  if (n_sets >= MAX_BATCH) return too_large();
  if (!d_sigs || !d_bitmaps || !verdicts || (msg_len && !d_msgs)) return fail(BGLS_ERR_ARG, "NULL argument");
  if ((stride & 3) || ((uintptr_t)d_bitmaps & 3)) return fail(BGLS_ERR_ARG, "device bitmaps: the stride and the pointer must be multiples of 4 bytes");
  std::shared_ptr<KeySet> ks;
  int rc;
  if ((rc = subsets_keyset(handle, stride, n_sets, &ks))) return rc;
  DISPATCH(ks->curve, verify_multi_subsets_dev_t<CV>(*ks, d_sigs, d_bitmaps, stride, n_sets, d_msgs, msg_len, msg_stride, verdicts, apk_out, gt_out, stream));
} BGLS_ABI_GUARD

int bgls_set_subset_complement(int mode) try {
  if (mode < 0 || mode > 2) return fail(BGLS_ERR_ARG, "mode must be 0 (per set), 1 (never) or 2 (always)");
  g_subset_complement.store(mode);
  return 0;
} BGLS_ABI_GUARD

// Grouped aggregate verification over a one-device key set by signer bitmap.  The refusals come in the order of the subset calls: the
// arguments alone, the machine, the handle, then (host form) the row against the handle's n.
static int grouped_keys_keyset(bgls_keys_t handle, std::shared_ptr<KeySet>* ks) {
  int rc;
  if ((rc = subsets_no_device())) return rc;
  if (!(*ks = keyset(handle))) return fail(BGLS_ERR_ARG, "unknown key-set handle");
  return grouped_keys_args_ok(**ks);
}

int bgls_verify_aggregate_grouped_h(bgls_keys_t handle, const uint8_t* sig, const uint8_t* bitmap, size_t bitmap_len, const uint8_t* msg_blob,
                                    const uint64_t* msg_off, size_t n_msgs, size_t* n_groups, uint8_t* gt_out) try {
  if (n_msgs >= MAX_BATCH) return too_large();
  if (!sig || !msg_off) return fail(BGLS_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = offsets_ok("msg_off", msg_off, n_msgs, 0))) return rc;
  if (msg_off[n_msgs] > msg_off[0] && !msg_blob) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n_groups) *n_groups = 0;
  std::shared_ptr<KeySet> ks;
  if ((rc = grouped_keys_keyset(handle, &ks))) return rc;
  size_t selected = ks->n;
  if (bitmap) {
    if (bitmap_len < (ks->n + 7) / 8) return fail(BGLS_ERR_ARG, "the signer bitmap is shorter than ceil(n / 8) bytes");
    if (!subset_rows_clean(bitmap, bitmap_len, 1, ks->n)) return fail(BGLS_ERR_ARG, "a signer bitmap has a bit at a position beyond the key set");
    selected = subset_row_popcount(bitmap, ks->n);
  }
  if (selected != n_msgs) return fail(BGLS_ERR_ARG, "the signer bitmap does not select as many keys as there are messages");
  DISPATCH(ks->curve, verify_aggregate_grouped_keys_t<CV>(*ks, sig, bitmap, msg_blob, msg_off, n_msgs, n_groups, gt_out));
} BGLS_ABI_GUARD

int bgls_verify_aggregate_grouped_keys_dev(bgls_keys_t handle, const void* d_sig, const void* d_bitmap, size_t bitmap_len, const void* d_msgs,
                                           size_t msg_len, size_t msg_stride, size_t n_msgs, size_t* n_groups, uint8_t* gt_out, void* stream) try {
  if (n_msgs >= MAX_BATCH) return too_large();
  if (!d_sig || (n_msgs && !d_msgs)) return fail(BGLS_ERR_ARG, "NULL argument");
  if (msg_stride < msg_len) return fail(BGLS_ERR_ARG, "msg_stride below msg_len");
  if (d_bitmap && ((bitmap_len & 3) || ((uintptr_t)d_bitmap & 3)))
    return fail(BGLS_ERR_ARG, "device bitmap: the length and the pointer must be multiples of 4 bytes");
  if (n_groups) *n_groups = 0;
  std::shared_ptr<KeySet> ks;
  int rc;
  if ((rc = grouped_keys_keyset(handle, &ks))) return rc;
  if (d_bitmap && bitmap_len < 4 * ((ks->n + 31) / 32)) return fail(BGLS_ERR_ARG, "the device signer bitmap is shorter than 4 ceil(n / 32) bytes");
  DISPATCH(ks->curve, verify_aggregate_grouped_keys_dev_t<CV>(*ks, d_sig, d_bitmap, bitmap_len, d_msgs, msg_len, msg_stride, n_msgs, n_groups, gt_out, stream));
} BGLS_ABI_GUARD

int bgls_set_group_small(size_t keys) try {
  g_group_small.store(keys);
  return 0;
} BGLS_ABI_GUARD

int bgls_set_prepare_shape(size_t ng, size_t chunk) try {
  if (ng != 0 && (ng < (size_t)PREP_NG_MIN || ng > (size_t)PREP_NG_MAX))
    return fail(BGLS_ERR_ARG, "prepared shape: ng must be 0 (automatic) or lie in 6..96");
  std::lock_guard<std::mutex> lk(g_prep_shape_mu);
  g_prep_shape.ng = ng;
  g_prep_shape.chunk = chunk;
  return 0;
} BGLS_ABI_GUARD

int bgls_verify_aggregate_multi(int curve, const uint8_t* sig, const uint8_t* keys, const uint8_t* msg_blob, const uint64_t* msg_off,
                                size_t n, int allow_duplicates, const int* devices, int n_devices) try {
  if (n >= MAX_BATCH) return too_large();
  bgls_keys_t h;
  // host keys arrive unvalidated here (no Point construction in between): the upload checks the order-r subgroup as the
  // reference's constructors do, so a small-order twist point is an encoding error, not an unspecified verdict
  int rc = bgls_keys_upload(curve, keys, n, devices, n_devices, BGLS_KEYS_CHECK, &h);
  if (rc) return rc;
  rc = bgls_verify_aggregate_h(h, sig, msg_blob, msg_off, n, allow_duplicates);
  const int ex = g_last_exchange;
  (void)bgls_keys_free(h);
  g_last_exchange = ex;
  return rc;
} BGLS_ABI_GUARD

int bgls_verify_multi_multi(int curve, const uint8_t* sig, const uint8_t* keys, size_t n, const uint8_t* msg, size_t msg_len,
                            const int* devices, int n_devices) try {
  if (n >= MAX_BATCH) return too_large();
  bgls_keys_t h;
  int rc = bgls_keys_upload(curve, keys, n, devices, n_devices, BGLS_KEYS_CHECK, &h);
  if (rc) return rc;
  rc = bgls_verify_multi_h(h, sig, msg, msg_len);
  const int ex = g_last_exchange;
  (void)bgls_keys_free(h);
  g_last_exchange = ex;
  return rc;
} BGLS_ABI_GUARD

int bgls_last_exchange(void) { return g_last_exchange; }

int bgls_generator(int curve, int group, uint8_t* out) try {
  if (!group_ok(group) || !out) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  DISPATCH(curve, generator_t<CV>(group, out));
} BGLS_ABI_GUARD

int bgls_pair(int curve, const uint8_t* g1, const uint8_t* g2, uint8_t* gt_out) try {
  return bgls_pairing_product(curve, g1, g2, 1, gt_out);
} BGLS_ABI_GUARD

int bgls_gt_mul(int curve, const uint8_t* a, const uint8_t* b, uint8_t* out) try {
  if (!a || !b || !out) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, gt_mul_t<CV>(a, b, out));
} BGLS_ABI_GUARD

int bgls_gt_pow(int curve, const uint8_t* gt, const uint8_t* k_be32, int negative, uint8_t* out) try {
  if (!gt || !k_be32 || !out) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, gt_pow_t<CV>(gt, k_be32, negative ? 1 : 0, out));
} BGLS_ABI_GUARD

int bgls_gt_identity(int curve, uint8_t* out) try {
  size_t n = bgls_gt_size(curve);
  if (!n || !out) return fail(BGLS_ERR_ARG, "unknown curve id or NULL argument");
  memset(out, 0, n);
  out[n - 1] = 1;
  return 0;
} BGLS_ABI_GUARD

int bgls_profile_enable(int on) try {
  Ctx* all = ctx_pool();
  for (int k = 0; k < MAX_DEVICES * NCTX; ++k) {
    Ctx& c = all[k];
    std::lock_guard<std::mutex> lk(c.mu);
    c.prof = on != 0;
    for (int i = 0; i < ST_NUM; ++i) { c.stage_ms[i] = 0; c.stage_cnt[i] = 0; }
  }
  return 0;
} BGLS_ABI_GUARD

int bgls_profile_get(const char* stage, double* total_ms, unsigned long long* launches) try {
  if (!stage || !total_ms || !launches) return fail(BGLS_ERR_ARG, "NULL argument");
  for (int i = 0; i < ST_NUM; ++i)
    if (!strcmp(stage, STAGE_NAMES[i])) {
      *total_ms = 0;
      *launches = 0;
      Ctx* all = ctx_pool();
      for (int k = 0; k < MAX_DEVICES * NCTX; ++k) {        // summed over the contexts of every device
        std::lock_guard<std::mutex> lk(all[k].mu);
        *total_ms += all[k].stage_ms[i];
        *launches += all[k].stage_cnt[i];
      }
      return 0;
    }
  return fail(BGLS_ERR_ARG, "unknown stage name");
} BGLS_ABI_GUARD

// Self-test of the exception barrier (no device needed): raises the named C++ exception inside a guarded body -- kind 0
// std::bad_alloc, 1 std::length_error, 2 std::system_error, 3 std::runtime_error, 4 a non-standard object, 5 a vector whose
// size no allocator can serve, 6 an exception on a shard's host thread -- and returns what the guard made of it.
int bgls_selftest_exception_barrier(int kind) try {
  switch (kind) {
    case 0: throw std::bad_alloc();
    case 1: throw std::length_error("selftest");
    case 2: throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again), "selftest");
    case 3: throw std::runtime_error("selftest");
    case 4: throw 42;
    case 5: {
      std::vector<uint64_t> v((size_t)-1 / 16);
      return (int)v.size();
    }
    case 6: {
      KeySet ks;
      ks.shards.resize(2);
      ks.shards[0].device = ks.shards[1].device = 0;
      return for_each_shard(ks, [&](int s) -> int {
        if (s == 1) throw std::bad_alloc();
        return 0;
      });
    }
    case 7: {      // advice r5: the thread's device / context selection must survive an exception caught further up
      const int d0 = g_dev, s0 = g_sel;
      try {
        SelectionGuard keep_selection;
        g_dev = 5;
        g_sel = 3;
        throw std::bad_alloc();
      } catch (const std::bad_alloc&) {
      }
      if (g_dev != d0 || g_sel != s0) return fail(BGLS_ERR_ARG, "selftest: the selection was not restored");
      {          // and a shard thread that cannot be started leaves a message behind
        KeySet ks;
        ks.shards.resize(1);
        ks.shards[0].device = 0;
        g_sel = 2;
        const int r = for_each_shard(ks, [&](int) -> int { throw std::length_error("selftest"); });
        const bool kept = g_sel == 2 && g_dev == d0;
        g_sel = s0;
        if (!kept) return fail(BGLS_ERR_ARG, "selftest: for_each_shard changed the selection");
        return r;
      }
    }
    default: return 0;
  }
} BGLS_ABI_GUARD

// Self-test of the workspace contract (DESIGN.md section 5, "Workspace contract"; tests/test_gpu_stale_workspace.py): every cached
// workspace of every ready context of every device, over its whole CAPACITY (a slot keeps bytes + bytes / 4 and is never cleared on
// reuse), and the context's pinned result words are set to `byte`; with a key-set handle also the exchange records d_rec / d_all of each
// of its shards.  Nothing else is touched: not the device tables, not the resident key data, not a caller's buffer.
// All or nothing: every ready context is asked first, and while any has a verification in flight the call refuses (BGLS_ERR_ARG) before
// one byte is set -- the words are that verification's.  *bytes_filled (nullable) is the bytes set, in every outcome: a verification
// submitted by another thread between the question and a context's turn ends the call there, with what was set until then.
// The fills are enqueued on each context's OWN stream and waited for: work a caller has queued on a stream of its own (the *_dev entries)
// is not ordered against them -- the caller of this hook synchronises such a stream first.
int bgls_selftest_fill_workspaces(int byte, uint64_t keys, uint64_t* bytes_filled) try {
  if (bytes_filled) *bytes_filled = 0;
  int cnt = 0;
  const hipError_t e0 = hipGetDeviceCount(&cnt);
  if (e0 != hipSuccess || cnt <= 0) return fail(BGLS_ERR_NO_DEVICE, "no HIP device available", e0);
  std::shared_ptr<KeySet> ks;
  if (keys && !(ks = keyset(keys))) return fail(BGLS_ERR_ARG, "unknown key set handle");
  int dev0 = 0;
  HIPCHK(hipGetDevice(&dev0));
  struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{dev0};
  uint64_t total = 0;
  struct Report { uint64_t* out; const uint64_t& v; ~Report() { if (out) *out = v; } } report{bytes_filled, total};
  Ctx* all = ctx_pool();
  for (int k = 0; k < MAX_DEVICES * NCTX; ++k) {          // the question first: no context is touched while one refuses
    std::lock_guard<std::mutex> lk(all[k].mu);
    if (all[k].ready && all[k].res_pending) return in_flight();
  }
  for (int k = 0; k < MAX_DEVICES * NCTX; ++k) {
    Ctx& c = all[k];
    std::lock_guard<std::mutex> lk(c.mu);
    if (!c.ready) continue;
    if (c.res_pending) return in_flight();
    HIPCHK(hipSetDevice(c.device));
    for (auto& w : c.ws)
      if (w.first && w.second) {
        HIPCHK(hipMemsetAsync(w.first, byte, w.second, c.stream));
        total += w.second;
      }
    HIPCHK(hipStreamSynchronize(c.stream));
    memset(c.h_res, byte, 64);
    total += 64;
  }
  if (ks) {
    std::lock_guard<std::mutex> lk_set(ks->mu);
    const size_t REC = (ks->curve == 0 ? Engine<BN254>::GTB : Engine<BLS381>::GTB) + REC_PAD;
    for (auto& sh : ks->shards) {
      HIPCHK(hipSetDevice(sh.device));
      if (sh.d_rec) { HIPCHK(hipMemset(sh.d_rec, byte, REC)); total += REC; }
      if (sh.d_all) { HIPCHK(hipMemset(sh.d_all, byte, REC * ks->shards.size())); total += REC * ks->shards.size(); }
      HIPCHK(hipDeviceSynchronize());
    }
  }
  return 0;
} BGLS_ABI_GUARD

// The capacities of the calling thread's context's workspace slots (0: never allocated) to caps[0 .. min(n, slots)); returns the slot
// count.  Without a device: the no-device code, as every entry that would enter the context.
int bgls_selftest_workspace_caps(size_t* caps, int n) try {
  if (n < 0 || (n > 0 && !caps)) return fail(BGLS_ERR_ARG, "NULL argument");
  int cnt = 0;
  const hipError_t e0 = hipGetDeviceCount(&cnt);
  if (e0 != hipSuccess || cnt <= 0) return fail(BGLS_ERR_NO_DEVICE, "no HIP device available", e0);
  Ctx& c = ctx();
  std::lock_guard<std::mutex> lk(c.mu);
  for (int i = 0; i < n && i < WS_NUM; ++i) caps[i] = c.ready ? c.ws[i].second : 0;
  return WS_NUM;
} BGLS_ABI_GUARD

int bgls_probe_mad_peak(double* mac_per_s) try {
  if (!mac_per_s) return fail(BGLS_ERR_ARG, "NULL argument");
  Call k;
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  void* sink;
  if ((rc = c.get(WS_OUT, 16, &sink))) return rc;
  const int iters = 4096, blocks = 256 * 8, threads = 256;
  hipEvent_t a, b;
  HIPCHK(hipEventCreate(&a));
  HIPCHK(hipEventCreate(&b));
  double best = 0;
  for (int rep = 0; rep < 4; ++rep) {
    HIPCHK(hipEventRecord(a, st));
    kl::mad_probe(st, blocks, threads, 12345u + rep, iters, (uint64_t*)sink);
    HIPCHK(hipEventRecord(b, st));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    double macs = (double)blocks * threads * iters * 16.0;
    double rate = macs / (ms * 1e-3);
    if (rep > 0 && rate > best) best = rate;
  }
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  *mac_per_s = best;
  return 0;
} BGLS_ABI_GUARD

int bgls_miller_product_dev(int curve, const void* d_sig, const void* d_keys, const void* d_msgs, size_t msg_len,
                            size_t msg_stride, size_t n, int check_duplicates, void* d_partial_out, void* d_flags,
                            void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (!d_partial_out || !d_flags || (n && (!d_keys || (!d_msgs && msg_len)))) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, miller_product_dev_t<CV>(d_sig, d_keys, d_msgs, msg_len, msg_stride, n, check_duplicates, d_partial_out,
                                           d_flags, stream));
} BGLS_ABI_GUARD

int bgls_set_throughput_mode(int on) try {
  g_throughput.store(on == 2 ? 2 : (on ? 1 : 0));
  return 0;
} BGLS_ABI_GUARD

int bgls_set_miller_shape(int shape, int mode) try {
  // 0: automatic; 4: k_miller_x60 always, `mode` = its role / priority / block-form word (see bgls_hip.h); 5: the 32-bit fused kernel always.
  // (Shapes 1-3, the decoupled k_lines / k_fold forms of rounds 2-4, were removed in round 5.)  `mode` is ignored for shapes 0 and 5.
  if (shape != 0 && shape != 4 && shape != 5) return fail(BGLS_ERR_ARG, "bad Miller shape (0, 4 or 5)");
#ifndef BGLS_LEGACY_KERNELS
  if (shape == 5) return fail(BGLS_ERR_ARG, "Miller shape 5 (k_miller_ab64) is compiled by `make LEGACY=1` only");
#endif
  if (shape == 4 && (mode < 0 || mode > 31 || (mode & 3) == 3)) return fail(BGLS_ERR_ARG, "bad k_miller_x60 mode word");
  g_x60_rot.store(shape == 4 ? mode : -1);    // shapes 0 / 5: back to the automatic role / priority mode
  g_shape.store(shape);
  return 0;
} BGLS_ABI_GUARD

int bgls_set_msm_min(size_t n) try {
  g_msm_min.store(n);
  return 0;
} BGLS_ABI_GUARD

int bgls_set_msm_plan(int c, int S) try {
  if (c != 0 && (c < 4 || c > 13)) return fail(BGLS_ERR_ARG, "bad window width (0 or 4..13)");
  if (S != 0 && S != 1 && S != 2 && S != 4 && S != 8 && S != 16) return fail(BGLS_ERR_ARG, "bad threads per bucket (0, 1, 2, 4, 8 or 16)");
  g_msm_plan.store(c << 8 | S);
  return 0;
} BGLS_ABI_GUARD

// What the last weighted sum of the calling thread's context did (tests/test_gpu_msm_plans.py): out = {path, c, S, W, largest bucket,
// listed pairs}; path 0 = per-point below bgls_set_msm_min's threshold (or past the 32-bit list guard), 1 = bucket method, 2 = per-point
// after the histogram showed a bucket above max(8 (n >> c), 64).  All zero before the first sum; n == 0 leaves the report as it was.
int bgls_selftest_msm_last(uint32_t* out) try {
  if (!out) return fail(BGLS_ERR_ARG, "NULL argument");
  int cnt = 0;
  const hipError_t e0 = hipGetDeviceCount(&cnt);
  if (e0 != hipSuccess || cnt <= 0) return fail(BGLS_ERR_NO_DEVICE, "no HIP device available", e0);
  Ctx& c = ctx();
  std::lock_guard<std::mutex> lk(c.mu);
  for (int i = 0; i < 6; ++i) out[i] = c.msm_last[i];
  return 0;
} BGLS_ABI_GUARD

int bgls_weighted_sum_dev(int curve, int group, const void* d_pts, const void* d_w16, size_t n, void* d_out, void* stream) try {
  if (group != BGLS_G1 && group != BGLS_G2) return fail(BGLS_ERR_ARG, "bad group");
  if (!d_out || (n && (!d_pts || !d_w16))) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n >= MAX_BATCH) return too_large();
  DISPATCH(curve, weighted_sum_dev_t<CV>(group, d_pts, d_w16, n, d_out, stream));
} BGLS_ABI_GUARD

int bgls_select_context(int index) try {
  if (index < 0 || index >= NCTX) return fail(BGLS_ERR_ARG, "context index out of range");
  g_sel = index;
  return 0;
} BGLS_ABI_GUARD

int bgls_final_verify_submit_dev(int curve, const void* d_partials, size_t count, const void* d_flags, void* stream) try {
  if (!d_partials || !count) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, final_verify_submit_dev_t<CV>(d_partials, count, d_flags, stream));
} BGLS_ABI_GUARD

int bgls_final_verify_collect(int curve) try {
  Ctx& c = ctx();
  std::lock_guard<std::mutex> lk(c.mu);
  DISPATCH(curve, Engine<CV>::finalize_collect(c));
} BGLS_ABI_GUARD

int bgls_duplicate_scan_dev(const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n, void* d_flags, void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (!d_flags || (n && !d_msgs && msg_len)) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n >= (1ull << 30)) return fail(BGLS_ERR_ARG, "too many messages for one scan");
  return duplicate_scan_dev(d_msgs, msg_len, msg_stride, n, d_flags, stream);
} BGLS_ABI_GUARD

int bgls_duplicate_scan_bucket_dev(const void* d_recs, size_t rec_len, size_t rec_stride, size_t n, unsigned bucket, unsigned n_buckets, void* d_flags,
                                   void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (!d_flags || (n && !d_recs && rec_len)) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n_buckets < 1 || n_buckets > 256 || bucket >= n_buckets) return fail(BGLS_ERR_ARG, "bucket out of range (bucket < n_buckets <= 256)");
  return duplicate_scan_dev(d_recs, rec_len, rec_stride, n, d_flags, stream, bucket, n_buckets);
} BGLS_ABI_GUARD

int bgls_digest_pack_dev(const void* d_digests16, size_t n, unsigned n_buckets, size_t cap, void* d_out, void* d_flags, void* stream) try {
  if (n >= MAX_BATCH || cap >= MAX_BATCH) return fail(BGLS_ERR_ARG, "batch too large (n and cap must be below 2^30)");
  if (n_buckets < 2 || n_buckets > 256) return fail(BGLS_ERR_ARG, "n_buckets out of range (2 <= n_buckets <= 256)");
  if (!d_out || !d_flags || cap == 0 || (n && !d_digests16)) return fail(BGLS_ERR_ARG, "NULL argument");
  if ((((uintptr_t)d_out | (uintptr_t)d_digests16) & 15) != 0) return fail(BGLS_ERR_ARG, "digest buffers must be 16-byte aligned");
  return digest_pack_dev(d_digests16, n, n_buckets, cap, d_out, d_flags, stream);
} BGLS_ABI_GUARD

int bgls_duplicate_scan_packed_dev(const void* d_recs16, size_t n_slots, unsigned bucket, unsigned n_buckets, void* d_flags, void* stream) try {
  if (n_slots >= MAX_BATCH) return too_large();
  if (!d_flags || (n_slots && !d_recs16)) return fail(BGLS_ERR_ARG, "NULL argument");
  if (n_buckets < 2 || n_buckets > 256 || bucket >= n_buckets) return fail(BGLS_ERR_ARG, "bucket out of range (bucket < n_buckets, 2 <= n_buckets <= 256)");
  return duplicate_scan_dev(d_recs16, 16, 16, n_slots, d_flags, stream, bucket, n_buckets, true);
} BGLS_ABI_GUARD

int bgls_message_digests_dev(const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n, void* d_out16, void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (n && (!d_out16 || (!d_msgs && msg_len))) return fail(BGLS_ERR_ARG, "NULL argument");
  if (((uintptr_t)d_out16 & 15) != 0) return fail(BGLS_ERR_ARG, "digest buffer must be 16-byte aligned");
  if (n == 0) return 0;
  Call k(stream);
  if (k.rc) return k.rc;
  Ctx& c = k.c;
  const hipStream_t st = k.st;
  int rc;
  MsgView mv = {(const uint8_t*)d_msgs, nullptr, msg_len, msg_stride};
  kl::msg_digest(st, mv, n, (uint8_t*)d_out16);
  HIPCHK(hipGetLastError());
  return 0;
} BGLS_ABI_GUARD

int bgls_final_verify_dev(int curve, const void* d_partials, size_t count, const void* d_flags, void* stream) try {
  if (!d_partials || !count) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, final_verify_dev_t<CV>(d_partials, count, d_flags, stream));
} BGLS_ABI_GUARD

int bgls_aggregate_points_dev(int curve, int group, const void* d_pts, size_t n, void* d_out, void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (!group_ok(group) || !d_out || (n && !d_pts)) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  DISPATCH(curve, aggregate_points_dev_t<CV>(group, d_pts, n, d_out, stream));
} BGLS_ABI_GUARD

int bgls_verify_multi_dev(int curve, const void* d_sig, const void* d_keys, size_t n, const void* d_msg, size_t msg_len,
                          void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (!d_sig || (n && !d_keys) || (msg_len && !d_msg)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_dev_entry_t<CV>(d_sig, d_keys, n, d_msg, msg_len, stream));
} BGLS_ABI_GUARD

int bgls_verify_multi_submit_dev(int curve, const void* d_sig, const void* d_keys, size_t n, const void* d_msg, size_t msg_len,
                                 void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (!d_sig || (n && !d_keys) || (msg_len && !d_msg)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_dev_entry_t<CV>(d_sig, d_keys, n, d_msg, msg_len, stream, true));
} BGLS_ABI_GUARD

/* ---- hashed aggregation exponents (bgls/blsHAE.go) and multiplicities (bgls/blsKosk.go:137-150) ---- */
int bgls_hae_exponents(int curve, const uint8_t* keys, size_t n, uint8_t* t_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (n && (!keys || !t_out)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, hae_exponents_t<CV>(keys, n, t_out));
} BGLS_ABI_GUARD

int bgls_aggregate_signatures_hae(int curve, const uint8_t* sigs, const uint8_t* keys, size_t n, uint8_t* out) try {
  if (n >= MAX_BATCH) return too_large();
  if (!out || (n && (!sigs || !keys))) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, aggregate_signatures_hae_t<CV>(sigs, keys, n, out));
} BGLS_ABI_GUARD

int bgls_verify_multi_hae(int curve, const uint8_t* sig, const uint8_t* keys, size_t n, const uint8_t* msg, size_t msg_len) try {
  if (n >= MAX_BATCH) return too_large();
  if (!sig || (n && !keys) || (msg_len && !msg)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_multi_weighted_t<CV>(sig, keys, nullptr, n, msg, msg_len));
} BGLS_ABI_GUARD

int bgls_verify_aggregate_hae(int curve, const uint8_t* sig, const uint8_t* keys, const uint8_t* msg_blob, const uint64_t* msg_off,
                              size_t n) try {
  if (n >= MAX_BATCH) return too_large();
  if (!sig || !msg_off || (n && !keys)) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, verify_aggregate_hae_t<CV>(sig, keys, msg_blob, msg_off, n));
} BGLS_ABI_GUARD

int bgls_verify_multi_multiplicity(int curve, const uint8_t* sig, const uint8_t* keys, const int64_t* multiplicity, size_t n,
                                   const uint8_t* msg, size_t msg_len) try {
  if (n >= MAX_BATCH) return too_large();
  if (!sig || (n && !keys) || (msg_len && !msg)) return fail(BGLS_ERR_ARG, "NULL argument");
  if (!multiplicity) DISPATCH(curve, verify_multi_t<CV>(sig, keys, n, msg, msg_len));
  DISPATCH(curve, verify_multi_weighted_t<CV>(sig, keys, multiplicity, n, msg, msg_len));
} BGLS_ABI_GUARD

/* ---- compressed wire formats (alt-bn128; curves/altbn128.go:81-89,203-221,296-376) ---- */
int bgls_compress_points(int curve, int group, const uint8_t* pts, size_t n, uint8_t* out) try {
  if (n >= MAX_BATCH) return too_large();
  if (!group_ok(group) || (n && (!pts || !out))) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  return wire_points(curve, group, true, pts, n, out, nullptr);
} BGLS_ABI_GUARD

int bgls_decompress_points(int curve, int group, const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok) try {
  if (n >= MAX_BATCH) return too_large();
  if (!group_ok(group) || (n && (!in || !out || !ok))) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  return wire_points(curve, group, false, in, n, out, ok);
} BGLS_ABI_GUARD

int bgls_decompress_points_dev(int curve, int group, const void* d_in, size_t n, void* d_out, void* d_ok, void* stream) try {
  if (n >= MAX_BATCH) return too_large();
  if (n == 0) return 0;
  if (!group_ok(group) || !d_in || !d_out || !d_ok) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  DISPATCH(curve, decompress_points_dev_t<CV>(group, d_in, n, d_out, d_ok, stream));
} BGLS_ABI_GUARD

/* ---- batch key generation / signing (bgls/bgls.go:40-56) ---- */
int bgls_scale_generator(int curve, int group, const uint8_t* scalars, size_t n, uint8_t* out) try {
  if (n >= MAX_BATCH) return too_large();
  if (!group_ok(group) || (n && (!scalars || !out))) return fail(BGLS_ERR_ARG, "bad group or NULL argument");
  DISPATCH(curve, scale_generator_t<CV>(group, scalars, n, out));
} BGLS_ABI_GUARD

int bgls_sign_batch(int curve, const uint8_t* sks, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n, uint8_t* sigs_out) try {
  if (n >= MAX_BATCH) return too_large();
  if (!msg_off || (n && (!sks || !sigs_out))) return fail(BGLS_ERR_ARG, "NULL argument");
  DISPATCH(curve, sign_batch_t<CV>(sks, msg_blob, msg_off, n, sigs_out));
} BGLS_ABI_GUARD

}  // extern "C"



