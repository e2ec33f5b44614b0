/*
 * bgls_hip.h -- C ABI of the MI355X aggregate-signature verification engine.
 *
 * Drop-in boundary for the hot path of Project-Arda/bgls: everything the Go package `curves`
 * reaches through its CurveSystem / Point / PointT interfaces (curves/curve.go:12-70) and the
 * goroutine helpers built on them (curves/curve.go:73-223), restated as BATCH entry points so
 * one cgo call replaces n goroutines.  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   curve   : BGLS_CURVE_ALTBN128 (curves.Altbn128, curves/altbn128.go:32) or
 *             BGLS_CURVE_BLS12_381 (curves.Bls12, curves/bls12_381.go:31)
 *   return  : verify-style calls return 1 (valid) / 0 (invalid); every call returns < 0 on a
 *             usage or runtime error.  The Go shim maps anything != 1 to `false` / `nil,false`,
 *             which is the reference's only error convention (curves/curve.go:15-22,46-48;
 *             bgls/bgls.go:95-97,115-118).  No exceptions, no abort().
 *   formats : uncompressed big-endian wire formats of the reference --
 *             G1 = x||y (curves/altbn128.go:42-57; curves/testcases/bls12G1Hash.dat),
 *             G2 = x_im||x_re||y_im||y_re (curves/altbn128.go:157-179, altbn128_test.go:26-38;
 *                  curves/bls12_381.go:147-158,209-226),
 *             infinity = all-zero bytes (curves/altbn128.go:431-439),
 *             GT = 12 field elements (384 B / 576 B; curves/altbn128.go:378-387), layout in
 *                  DESIGN.md (byte-parity with the upstream Go libraries is unpinned).
 *             Sizes: bgls_g1_size / bgls_g2_size / bgls_gt_size.
 *   memory  : the caller owns every buffer; inputs are const and never modified (the reference's
 *             in-place mutation quirks, curves/altbn128.go:306-309,344-349 and
 *             curves/bls12_381.go:70,131, are NOT reproduced).
 *   threads : every entry point may be called concurrently; calls on one context serialise.
 *   device  : all arithmetic runs in HIP kernels on the selected GPU; there is no CPU fallback.
 *             If no gfx950 device is usable every compute call returns BGLS_ERR_NO_DEVICE.
 */
#ifndef BGLS_HIP_H
#define BGLS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGLS_CURVE_ALTBN128 0
#define BGLS_CURVE_BLS12_381 1

#define BGLS_G1 1
#define BGLS_G2 2

#define BGLS_ERR_ARG (-1)       /* bad curve/group id, NULL pointer, inconsistent offsets */
#define BGLS_ERR_ENCODING (-2)  /* a coordinate >= q, a point not on its curve, or (where checked) a point outside the order-r subgroup */
#define BGLS_ERR_HASH (-3)      /* try-and-increment exhausted 256 counters (probability 2^-256) */
#define BGLS_ERR_NO_DEVICE (-4) /* no usable HIP device */
#define BGLS_ERR_HIP (-5)       /* a HIP runtime call failed; see bgls_last_error() */
#define BGLS_ERR_NOMEM (-6)     /* a host allocation failed inside the library (std::bad_alloc); nothing was verified */

/* ---- runtime ---------------------------------------------------------------------------- */
/* Select the default HIP device of the calling process (default 0) and bring it up.  May be called again with another
 * device; contexts, workspaces and key sets of devices used earlier stay valid. */
int bgls_init(int device);
/* Device used by the calling thread's subsequent calls (-1 = the process default set by bgls_init). */
int bgls_select_device(int device);
/* Human-readable text for the last error on this thread ("" if none). */
const char* bgls_last_error(void);
/* ABI version; bumped on any signature change. */
int bgls_abi_version(void);

size_t bgls_fp_size(int curve); /* 32 / 48 */
size_t bgls_g1_size(int curve); /* 64 / 96 */
size_t bgls_g2_size(int curve); /* 128 / 192 */
size_t bgls_gt_size(int curve); /* 384 / 576 */

/* ---- the hot path, host buffers ------------------------------------------------------------ */
/* The Verify* entry points take keys as the reference's Verify* functions take Points: already constructed, i.e.
 * validated by MakeG2Point / UnmarshalG2 (here: bgls_point_check, bgls_check_points, bgls_decompress_points or
 * bgls_keys_upload with BGLS_KEYS_CHECK).  They re-check canonical encoding and curve membership of every key (an
 * encoding error is BGLS_ERR_ENCODING, never an accept) but not G2 subgroup membership, exactly as bgls.Verify*
 * does not re-validate its Point arguments. */

/* bgls.VerifyAggregateSignature (bgls/bgls.go:82-84) -> verifyAggSig (bgls/bgls.go:94-119).
 * keys: n G2 points; messages: msg_blob[msg_off[i] .. msg_off[i+1]), i < n (msg_off has n+1
 * entries).  allow_duplicates = 0 reproduces the duplicate-message rejection
 * (containsDuplicateMessage, bgls/bgls.go:139-150); 1 is the Kosk / distinct-message callers'
 * mode (bgls/blsKosk.go:100-106, bgls/blsDistinctMessage.go:45-57).
 * Computes e(-sig, g2) * prod_i e(HashToG1(m_i), pk_i) == 1. */
int bgls_verify_aggregate(int curve, const uint8_t* sig, const uint8_t* keys, const uint8_t* msg_blob,
                          const uint64_t* msg_off, size_t n, int allow_duplicates);

/* n_inst independent VerifyAggregateSignature calls (bgls/bgls.go:82-84,94-119) in one set of launches.  Instance b is the
 * signature sigs[b] (n_inst G1 points), the keys keys[inst_off[b] .. inst_off[b+1]) and the messages with the same indices
 * (msg_off: inst_off[n_inst] + 1 entries, as in bgls_verify_aggregate).  inst_off: n_inst + 1 offsets, monotone from 0, below
 * 2^30 pairs in all (BGLS_ERR_ARG otherwise); n_inst == 0 returns 0.
 * Verdicts: verdicts[b] = 1 / 0 is what bgls_verify_aggregate returns for instance b alone -- an instance without keys is accepted
 * iff its signature is the point at infinity.  With allow_duplicates = 0 duplicate messages are searched for WITHIN each instance
 * (such an instance gets 0); the same message in two instances is no duplicate.  gt_out: NULL or n_inst GT elements, gt_out[b] =
 * e(-sig_b, g2) * prod e(H(m_i), pk_i) after the final exponentiation, byte-equal to what the single path computes for instance b.
 * Errors: a non-canonical or off-curve key or signature, a degenerate point step or an exhausted hash ANYWHERE in the batch fails
 * the whole call with the single call's code (BGLS_ERR_ENCODING / BGLS_ERR_HASH) and leaves verdicts undefined -- the Verify*
 * convention that keys are constructed Points (see above); bgls_check_points is the per-item validation.
 * Returns the number of accepted instances (>= 0) or < 0. */
int bgls_verify_aggregate_batch(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* inst_off, size_t n_inst,
                                const uint8_t* msg_blob, const uint64_t* msg_off, int allow_duplicates, uint8_t* verdicts,
                                uint8_t* gt_out);

/* ---- aggregate verification that pairs once per DISTINCT message ---------------------------------------------------------------
 * KoskVerifyAggregateSignature (bgls/blsKosk.go:100-106) lets many signers sign the same message.  By bilinearity
 * prod_i e(H(m_i), pk_i) = prod over the distinct messages m of e(H(m), sum of the keys of the signers of m), so n signers over d distinct
 * messages need d hashes, d + 1 Miller loops and n G2 additions instead of n hashes and n + 1 Miller loops.  The caller passes the
 * reference's own argument shape, flat keys[] and msgs[]; the grouping is done on the device.
 *
 * bgls_group_messages: group_of[i] = number of the group of message i.  Two messages share a group iff they are byte-identical (same
 * length, same bytes).  Groups are numbered 0 .. *n_groups - 1 in the order of their FIRST occurrence, so the result is a function of
 * the input alone.  n_groups may be NULL.  n == 0 returns 0 with *n_groups = 0 and touches no other pointer.  The _dev form takes n
 * messages of msg_len bytes at msg_stride on the device and writes n uint32 to d_group_of; it returns after the result is complete.
 * Returns 0 or < 0.
 *
 * bgls_verify_aggregate_grouped returns 1 / 0 / < 0 exactly as bgls_verify_aggregate(curve, sig, keys, msg_blob, msg_off, n,
 * allow_duplicates = 1) does.  n_groups: NULL or the number of distinct messages.  gt_out: NULL or the GT element
 * e(-sig, g2) * prod e(H(m), sum of that message's keys) after the final exponentiation.
 *   Keys in G2, signature in G1: Points constructed through bgls_check_points and its kin.  For such inputs the verdict AND the GT bytes
 *     equal those of the ungrouped product over all n pairs.  Canonical encoding and curve membership of every key are checked as
 *     everywhere else; for on-curve points outside the subgroups the verdict is unspecified (the call still does not fault).
 *   Key sum at infinity: a group whose keys sum to the point at infinity contributes the factor 1.
 *   n == 0: returns what bgls_verify_aggregate returns for n = 0 (1 iff sig is the point at infinity), and *n_groups = 0.
 *   Whole-call errors are the sibling's: BGLS_ERR_ENCODING, BGLS_ERR_HASH, and BGLS_ERR_NO_DEVICE without a device (no CPU fallback).
 *   BGLS_ERR_ARG, returned before any device work: non-monotone offsets, NULL arrays with n > 0, n at or above 2^30, and in the
 *     _dev forms a msg_stride below msg_len.
 *   There is no duplicate rule: this is the Kosk / distinct-message callers' mode.
 * Grouping is by exact bytes: messages that differ in one byte or in length are different messages. */
int bgls_group_messages(const uint8_t* msg_blob, const uint64_t* msg_off, size_t n, uint32_t* group_of, size_t* n_groups);
int bgls_group_messages_dev(const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n, void* d_group_of, size_t* n_groups,
                            void* stream);
int bgls_verify_aggregate_grouped(int curve, const uint8_t* sig, const uint8_t* keys, const uint8_t* msg_blob,
                                  const uint64_t* msg_off, size_t n, size_t* n_groups, uint8_t* gt_out);
int bgls_verify_aggregate_grouped_dev(int curve, const void* d_sig, const void* d_keys, const void* d_msgs, size_t msg_len,
                                      size_t msg_stride, size_t n, size_t* n_groups, uint8_t* gt_out, void* stream);

/* ---- distinct messages (bgls/blsDistinctMessage.go) and key registration (bgls/blsKosk.go:44-69) ----------------------------------
 * The message that is hashed is derived from the signer's key: key i's uncompressed wire bytes followed by message i
 * (BGLS_KEYED_PREFIX: append(keys[i].MarshalUncompressed(), msgs[i]...), blsDistinctMessage.go:51; the key bytes go in verbatim, as the
 * caller or the key set holds them), or the compressed key alone (BGLS_KEYED_POP: pubkey.Marshal(), blsKosk.go:66).  The library builds
 * these hash inputs on the device from the keys it has there; callers pass plain messages and never prefix anything.  There is no
 * duplicate rule (blsDistinctMessage.go:53-56), everything else is the sibling call's contract.
 *
 * HashToG1 of the n built inputs (n G1 points to g1_out, as bgls_hash_to_g1 returns them for a host-built blob): the hash of
 * DistinctMsgSign (mode BGLS_KEYED_PREFIX) and of Authenticate (mode BGLS_KEYED_POP: msg_blob / msg_off are ignored and may be NULL; a
 * key that does not compress is BGLS_ERR_ENCODING, as in bgls_compress_points).  Any other mode is BGLS_ERR_ARG. */
#define BGLS_KEYED_PREFIX 0
#define BGLS_KEYED_POP 1
int bgls_hash_to_g1_keyed(int curve, int mode, const uint8_t* keys, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n,
                          uint8_t* g1_out);
/* DistinctMsgVerifyAggregateSignature (blsDistinctMessage.go:45-57): returns 1 / 0 / < 0 exactly as
 * bgls_verify_aggregate(..., allow_duplicates = 1) does on messages the caller prefixed itself. */
int bgls_verify_aggregate_distinct(int curve, const uint8_t* sig, const uint8_t* keys, const uint8_t* msg_blob,
                                   const uint64_t* msg_off, size_t n);
/* n_inst independent DistinctMsgVerifyAggregateSignature calls: bgls_verify_aggregate_batch's contract (limits, whole-call errors,
 * return value, gt_out) with allow_duplicates = 1 on the prefixed messages. */
int bgls_verify_aggregate_distinct_batch(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* inst_off, size_t n_inst,
                                         const uint8_t* msg_blob, const uint64_t* msg_off, uint8_t* verdicts, uint8_t* gt_out);
/* n independent DistinctMsgVerifySingleSignature calls (blsDistinctMessage.go:37-40): item b is sigs[b], keys[b] and message b.
 * bgls_verify_multi_sets' contract on one-key sets with the prefixed messages (verdicts, gt_out, whole-call errors, return value; n == 0
 * returns 0). */
int bgls_verify_single_distinct_batch(int curve, const uint8_t* sigs, const uint8_t* keys, const uint8_t* msg_blob,
                                      const uint64_t* msg_off, size_t n, uint8_t* verdicts, uint8_t* gt_out);
/* n independent CheckAuthentication calls (blsKosk.go:59-69): item b is the key keys[b] and its proof of possession auths[b] (G1), a
 * signature on the compressed key.  The single-signature batch above with BGLS_KEYED_POP inputs. */
int bgls_check_authentication_batch(int curve, const uint8_t* keys, const uint8_t* auths, size_t n, uint8_t* verdicts,
                                    uint8_t* gt_out);

/* verifyMultiSignature (bgls/bgls.go:89-92): apk = sum(keys) (AggregatePoints,
 * curves/curve.go:73-121) then VerifySingleSignature (bgls/bgls.go:59-70) on msg.
 * KoskVerifyMultiSignature (bgls/blsKosk.go:117-120) is this call with 0x01 prepended to msg. */
int bgls_verify_multi(int curve, const uint8_t* sig, const uint8_t* keys, size_t n, const uint8_t* msg,
                      size_t msg_len);

/* KoskVerifyBatchMultiSignature's body (bgls/blsKosk.go:126-133): aggsig = AggregateSignatures(sigs) (n_sets G1 points),
 * key_b = AggregateKeys(set b) with set b = keys[key_off[b] .. key_off[b+1]) (counts of points, n_sets + 1 offsets), then
 * verifyAggSig(aggsig, key_0 .. key_{n_sets-1}, msgs, allow_duplicates) -- ONE launch for all key sums, one Miller launch and
 * one final exponentiation for all the sets.  The Go function prepends 0x01 to every message and passes
 * allow_duplicates = true (KoskVerifyAggregateSignature, bgls/blsKosk.go:100-106); the host mirrors do the same.
 * Keys are checked for canonical encoding and curve membership, NOT for subgroup membership: like every Verify* entry point
 * this call takes Points the caller has constructed (validated) already -- bgls_check_points / bgls_keys_upload(BGLS_KEYS_CHECK)
 * are the constructors' checks; a degenerate point step of a small-order key is reported as BGLS_ERR_ENCODING.
 * One call handles what fits one launch: at most 2^30 blocks of the key-sum pass and 8 GiB of partial sums (a set of up to
 * 128 keys takes one block and one 192 / 288-byte partial: 2^25 such sets); larger jobs return BGLS_ERR_ARG and are cut by
 * the caller. */
int bgls_verify_multi_batch(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t n_sets,
                            const uint8_t* msg_blob, const uint64_t* msg_off, int allow_duplicates);
/* n_sets independent verifyMultiSignature calls (bgls/bgls.go:89-92) in one set of launches.  Set b is the signature sigs[b]
 * (n_sets G1 points), the keys keys[key_off[b] .. key_off[b+1]) and the message msg_blob[msg_off[b] .. msg_off[b+1]).  A set of
 * one key is VerifySingleSignature (bgls/bgls.go:59-70): this is also the batched single-signature check.
 * Verdicts: verdicts[b] = 1 / 0 is exactly what bgls_verify_multi returns for set b alone -- an empty set sums to the point at
 * infinity, as in the single call.  There is no duplicate rule (one message per set): the same message in several sets is fine.
 * gt_out: NULL or n_sets GT elements, gt_out[b] = e(-sig_b, g2) * e(H(m_b), apk_b) after the final exponentiation, byte-equal to
 * what the single path computes for set b.
 * Errors as bgls_verify_aggregate_batch: a non-canonical or off-curve key or signature, a degenerate point step or an exhausted hash
 * ANYWHERE fails the whole call with the single call's code and leaves verdicts undefined.  Size limits are bgls_verify_multi_batch's
 * (BGLS_ERR_ARG past them); non-monotone key_off / msg_off are BGLS_ERR_ARG; n_sets == 0 returns 0.
 * Returns the number of accepted sets (>= 0) or < 0. */
int bgls_verify_multi_sets(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t n_sets,
                           const uint8_t* msg_blob, const uint64_t* msg_off, uint8_t* verdicts, uint8_t* gt_out);
/* "Are these n_sets multi-signatures all valid?" under ONE combined check per group of consecutive sets: one final exponentiation per
 * group instead of one per set.  Sets are described exactly as for bgls_verify_multi_sets.  With the coefficients r_b of
 * bgls_rlc_coefficients(seed, n_sets) -- r_b belongs to the index b of the set in the call, whatever the grouping --
 *   verdicts[g] = 1  iff  e(-sum_b r_b sigs[b], g2) * prod_b e(r_b H(m_b), apk_b) = 1  over the sets b of group g,  apk_b = sum of set b's keys.
 * Groups: group_off holds n_groups + 1 HOST offsets into the sets, monotone, from 0, ending at n_sets; group_off == NULL with
 * n_groups == 1 means one group holding all sets.  An empty group is accepted (the empty product).  A caller localises a failure by
 * running the per-set call over the sets of the rejected groups only (the host mirrors' VerifyMultiSignaturesLocated does).
 * gt_out: NULL or n_groups GT elements, the product above after the final exponentiation.
 * THE CONTRACT.  A group whose sets bgls_verify_multi would all accept is always accepted.  A group holding a set that bgls_verify_multi
 * rejects is rejected, except with probability about 2^-127 over a seed the adversary cannot predict (128-bit coefficients, one bit
 * spent on keeping them non-zero).  The seed MUST be drawn from a CSPRNG AFTER the inputs are fixed and must never be reused where an
 * adversary can see it first: whoever knows the coefficients in advance can shift two signatures by +r_2 D and -r_1 D and pass.
 * (bgls_verify_multi_batch is this shape with every r_b = 1: it accepts such a shifted pair and cannot stand in for n_sets verdicts.)
 * The equivalence is promised for signatures in G1 and keys in G2, i.e. Points constructed through bgls_check_points and its kin; for
 * on-curve points outside the subgroups the verdict is unspecified (the call still does not fault).
 * Errors as bgls_verify_multi_sets: a non-canonical or off-curve key or signature, a degenerate point step or an exhausted hash
 * ANYWHERE fails the whole call (BGLS_ERR_ENCODING / BGLS_ERR_HASH) and leaves verdicts undefined; BGLS_ERR_NO_DEVICE without a device
 * (no CPU fallback).  BGLS_ERR_ARG, checked before any device work: non-monotone offsets, group_off not from 0 or not ending at
 * n_sets, group_off == NULL with n_groups != 1, a NULL seed, n_sets at or above 2^28 (the XOF length 16 n_sets is a uint32).
 * n_sets == 0 returns 0.  Returns the number of accepted groups (>= 0) or < 0. */
int bgls_verify_multi_sets_combined(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t n_sets,
                                    const uint8_t* msg_blob, const uint64_t* msg_off, const uint64_t* group_off, size_t n_groups,
                                    const uint8_t seed[32], uint8_t* verdicts, uint8_t* gt_out);
/* The coefficients of the combined check, defined here once: the XOF is BLAKE2Xb without a key (golang.org/x/crypto/blake2b NewXOF(16 n, nil))
 * over "bgls-rlc-v1" || seed (32 bytes) || u64le(n) with output length 16 n; r_b is bytes [16 b, 16 b + 16) of its output, read
 * big-endian, with the lowest bit set (never zero, at the cost of one bit of soundness).  r_out: n x 16 bytes, big-endian, the bit
 * already set.  n < 2^28.  Returns 0 or < 0. */
int bgls_rlc_coefficients(const uint8_t seed[32], size_t n, uint8_t* r_out);
/* n independent bbsigs.Verify calls (bbsigs/bbsigs.go:68-73) in one set of launches: Boneh-Boyen signatures, item b is the signature
 * (sigmas[b], rs[b]) on the message scalar ms[b] under the key (U_b, V_b).
 * sigmas: n G1 points; rs, ms: n x 32-byte big-endian magnitudes; keys: n x (U || V), 2 G2 points each.
 * verdicts[b] = 1 / 0; gt_out: NULL or n GT elements, gt_out[b] = e(sigma_b, Q_b), Q_b = m_b g2 + U_b + r_b V_b, byte-equal to
 * bgls_pair(sigma_b, Q_b); item b is accepted iff gt_out[b] equals bgls_pair(g1, g2) (GetGT()).
 * Scalars are used as the given 256-bit magnitudes, unreduced (as bgls_scale_points).  Q_b is the exact point for every on-curve
 * key, inside the order-r subgroup or not: keys are constructed Points, as for every Verify* call (see above bgls_verify_aggregate).
 * A sigma, U or V at infinity, a zero scalar or Q_b at infinity give a verdict (e(inf, Q) = e(sigma, inf) = 1: rejected).  A
 * non-canonical or off-curve sigma, U or V ANYWHERE, or a degenerate point step, fails the whole call with BGLS_ERR_ENCODING and
 * leaves verdicts undefined.  n == 0 returns 0; n at or above 2^30 is BGLS_ERR_ARG.  The hashed form (VerifyHashed) is host work:
 * m = blake2b-256(msg) mod r.
 * Returns the number of accepted items (>= 0) or < 0. */
int bgls_bb_verify_batch(int curve, const uint8_t* sigmas, const uint8_t* rs, const uint8_t* keys, const uint8_t* ms,
                         size_t n, uint8_t* verdicts, uint8_t* gt_out);
/* "Are these n Boneh-Boyen signatures all valid?" under ONE combined check per group of consecutive items: the Miller loops of a group
 * share their squarings and a group costs one final exponentiation instead of one per item.  Items are laid out exactly as for
 * bgls_bb_verify_batch.  With the coefficients rho_b of bgls_rlc_coefficients(seed, n) -- 16 bytes big-endian, the lowest bit set; rho_b
 * belongs to the index b of the item in the call, whatever the grouping -- and s_g = sum of rho_b over the items of group g as a plain
 * integer (below 2^156, used as an unreduced magnitude, as bgls_scale_generator takes them),
 *   verdicts[g] = 1  iff  prod_b e(rho_b sigmas[b], Q_b) * e(-s_g g1, g2) = 1  over the items b of group g,  Q_b = m_b g2 + U_b + r_b V_b.
 * Groups: group_off holds n_groups + 1 HOST offsets into the items, monotone, from 0, ending at n; group_off == NULL with
 * n_groups == 1 means one group holding all items.  An empty group is accepted, and its GT element is one.  A caller localises a failure
 * by running bgls_bb_verify_batch over the items of the rejected groups only (the host mirrors' VerifyBatchLocated /
 * bb_verify_batch_located do).
 * gt_out: NULL or n_groups GT elements, the product above after the final exponentiation, byte-equal to bgls_pairing_product over the
 * pairs (rho_b sigmas[b], Q_b) of the group and (-s_g g1, g2).
 * THE CONTRACT.  A group whose items bgls_bb_verify_batch would all accept is always accepted.  A group holding an item that
 * bgls_bb_verify_batch rejects is rejected, except with probability about 2^-127 over a seed the adversary cannot predict (128-bit
 * coefficients, one bit spent on keeping them non-zero).  A group with exactly ONE bad item is rejected with certainty: the product is
 * then e(g1, g2)^(-rho_b) * e(rho_b sigma_b, Q_b), and rho_b is odd and below the group order.  The seed MUST be drawn from a CSPRNG AFTER
 * the inputs are fixed and must never be reused where an adversary can see it first: whoever knows the coefficients in advance can shift
 * two signatures under one Q by +rho_2 D and -rho_1 D and pass.  The equivalence is promised for sigma in G1 and U, V in G2, i.e. Points
 * constructed through bgls_check_points and its kin; for on-curve points outside the subgroups the verdict is unspecified (the call still
 * does not fault).  An item with sigma or Q_b at infinity contributes e = 1: its group is rejected, as the per-item call rejects the item.
 * Errors: a non-canonical or off-curve sigma, U or V ANYWHERE, or a degenerate point step, fails the whole call with
 * BGLS_ERR_ENCODING and leaves verdicts undefined; BGLS_ERR_NO_DEVICE without a device (no CPU fallback).  BGLS_ERR_ARG, checked before
 * any device work: non-monotone offsets, group_off not from 0 or not ending at n, group_off == NULL with n_groups != 1, a NULL seed, NULL
 * arrays with n > 0, n at or above 2^28 (the XOF length 16 n is a uint32).  n == 0 returns 0 without touching a pointer.
 * Returns the number of accepted groups (>= 0) or < 0. */
int bgls_bb_verify_batch_combined(int curve, const uint8_t* sigmas, const uint8_t* rs, const uint8_t* keys, const uint8_t* ms, size_t n,
                                  const uint64_t* group_off, size_t n_groups, const uint8_t seed[32], uint8_t* verdicts, uint8_t* gt_out);
/* AggregatePoints (curves/curve.go:73-121) over n_sets sets in one pass: out[b] = sum of pts[set_off[b] .. set_off[b+1])
 * (an empty set gives the point at infinity).  What the n_sets AggregateKeys calls of blsKosk.go:128-131 cost. */
int bgls_aggregate_sets(int curve, int group, const uint8_t* pts, const uint64_t* set_off, size_t n_sets, uint8_t* out);

/* CurveSystem.PairingProduct (curves/altbn128.go:143-145, curves/bls12_381.go:238-240 ->
 * concurrentPairingProduct, curves/curve.go:125-170): gt_out = prod_i e(g1s[i], g2s[i]). */
int bgls_pairing_product(int curve, const uint8_t* g1s, const uint8_t* g2s, size_t n, uint8_t* gt_out);

/* CurveSystem.HashToG1 over a batch (curves/altbn128.go:509-513, curves/bls12_381.go:349-351;
 * the per-message goroutines of bgls/bgls.go:107-111,134-137). g1_out: n G1 points. */
int bgls_hash_to_g1(int curve, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n, uint8_t* g1_out);

/* curves.AggregatePoints (curves/curve.go:73-121): out = sum of n points of `group`.
 * n == 0 yields infinity (the reference spins forever there, curves/curve.go:94-108). */
int bgls_aggregate_points(int curve, int group, const uint8_t* pts, size_t n, uint8_t* out);

/* curves.ScalePoints (curves/curve.go:190-214) -> Point.Mul (curves/altbn128.go:107-121,235-249;
 * curves/bls12_381.go:65-76,126-137): out[i] = k_i * pts[i].  scalars: n x 32-byte big-endian
 * magnitudes; signs: NULL (all non-negative) or n bytes, 0 = +, 1 = negative (negate-then-mul),
 * 2 = nil factor (copy the point). */
int bgls_scale_points(int curve, int group, const uint8_t* pts, const uint8_t* scalars, const uint8_t* signs,
                      size_t n, uint8_t* out);

/* ---- hashed aggregation exponents (bgls/blsHAE.go) and multiplicities (bgls/blsKosk.go:137-150) ---- */
/* hashPubKeysToExponents (bgls/blsHAE.go:80-93): t_out = n 16-byte big-endian exponents read from BLAKE2Xb
 * (golang.org/x/crypto/blake2b NewXOF(16 n, nil)) over MarshalUncompressed(pk_0) || ... || pk_{n-1}, i.e. over the
 * n x bgls_g2_size bytes of `keys` (curves/altbn128.go:223-225; BLS12-381's upstream layout is unpinned).
 * The root digest is one sequential compression chain over all key bytes (host side of the boundary); the XOF
 * expansion runs on the device.  n < 2^28 (the XOF length is a uint32). */
int bgls_hae_exponents(int curve, const uint8_t* keys, size_t n, uint8_t* t_out);
/* AggregateSignaturesWithHAE (bgls/blsHAE.go:39-46): out = sum_i t_i * sigs[i] (G1); the caller checks the lengths. */
int bgls_aggregate_signatures_hae(int curve, const uint8_t* sigs, const uint8_t* keys, size_t n, uint8_t* out);
/* VerifyMultiSignatureWithHAE (bgls/blsHAE.go:56-58) -> getAggregatePubKey (:74-77): apk = sum_i t_i * keys[i], then
 * VerifySingleSignature (bgls/bgls.go:59-70). */
int bgls_verify_multi_hae(int curve, const uint8_t* sig, const uint8_t* keys, size_t n, const uint8_t* msg,
                          size_t msg_len);
/* VerifyAggregateSignatureWithHAE (bgls/blsHAE.go:49-53): keys scaled by their exponents (ScalePoints), then
 * verifyAggSig with duplicate messages allowed. */
int bgls_verify_aggregate_hae(int curve, const uint8_t* sig, const uint8_t* keys, const uint8_t* msg_blob,
                              const uint64_t* msg_off, size_t n);
/* n_sets independent VerifyMultiSignatureWithHAE calls (bgls/blsHAE.go:56-58,74-93) in one set of launches.  Set b is the signature
 * sigs[b], the keys keys[key_off[b] .. key_off[b+1]) (wire bytes) and the message msg_blob[msg_off[b] .. msg_off[b+1]).
 * verdicts[b] = 1 / 0 is what bgls_verify_multi_hae returns for set b alone (the exponents are hashed from set b's keys only).
 * apk_out: NULL or n_sets G2 points, apk_out[b] = getAggregatePubKey(set b) = sum_i t_i pk_i, byte-equal to the single path's sum.
 * gt_out: NULL or n_sets GT elements, e(-sig_b, g2) * e(H(m_b), apk_b) after the final exponentiation.
 * Errors as bgls_verify_multi_sets: a non-canonical or off-curve key or signature, a degenerate point step or an exhausted hash
 * ANYWHERE fails the whole call with the single call's code and leaves verdicts undefined; non-monotone offsets, NULL arguments, 2^30
 * keys or more in all or 2^28 or more in one set (the XOF length is a uint32) are BGLS_ERR_ARG; n_sets == 0 returns 0.
 * Returns the number of accepted sets (>= 0) or < 0. */
int bgls_verify_multi_hae_sets(int curve, const uint8_t* sigs, const uint8_t* keys, const uint64_t* key_off, size_t n_sets,
                               const uint8_t* msg_blob, const uint64_t* msg_off, uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out);
/* hashPubKeysToExponents (bgls/blsHAE.go:80-93) per set: t_out[16 key_off[b] ..] = the 16-byte exponents of set b, byte-equal to
 * bgls_hae_exponents on that set alone.  Offsets and limits as bgls_verify_multi_hae_sets. */
int bgls_hae_exponents_sets(int curve, const uint8_t* keys, const uint64_t* key_off, size_t n_sets, uint8_t* t_out);
/* Sets with more than n keys have their BLAKE2Xb root computed on the host by the host-pointer entries (bgls_verify_multi_hae_sets,
 * bgls_hae_exponents_sets); the others on the device, one lane per set.  Results do not depend on it.  Returns 0. */
int bgls_set_hae_root_host_min(size_t n);
/* n independent AmsVerifySignature calls (accountable-subgroup multisignatures, bgls/blsAsmSigs.go:48-59,73-86) in one set of launches.
 * Item b is the group key apks[b] and the signers' key sum agg_keys[b] (G2 wire bytes), the signature agg_sigs[b] (G1 wire bytes), the
 * signer indices signers[signer_off[b] .. signer_off[b+1]) and the message msg_blob[msg_off[b] .. msg_off[b+1]).  verdicts[b] = 1 iff
 *   e(H(0x00 || m_b), aggKey_b) * e(sum_k H(0x01 || apk_b wire bytes || strconv.Itoa(signers[k])), apk_b) * e(-sigma_b, g2) = 1;
 * a repeated index is added twice, as the reference does.  An item with an empty signer list gets verdict 0 (the reference panics); its
 * gt_out entry is unspecified.  gt_out: NULL or n GT elements, the product above after the final exponentiation.
 * A non-canonical or off-curve apk, aggKey or sigma, a degenerate point step or an exhausted hash ANYWHERE fails the whole call with the
 * single path's code and leaves verdicts undefined; non-monotone offsets, NULL arguments where a count is non-zero, n or n + the number
 * of signers at 2^30 or more are BGLS_ERR_ARG, checked before any device work; n == 0 returns 0 without touching a pointer.
 * There is no CPU fallback: BGLS_ERR_NO_DEVICE without a device.  Returns the number of accepted items (>= 0) or < 0. */
int bgls_ams_verify_batch(int curve, const uint8_t* apks, const uint8_t* agg_keys, const uint8_t* agg_sigs, const uint32_t* signers,
                          const uint64_t* signer_off, size_t n, const uint8_t* msg_blob, const uint64_t* msg_off, uint8_t* verdicts,
                          uint8_t* gt_out);
/* Items per pass of the segmented G1 sum inside bgls_ams_verify_batch (default 2^16: the sum keeps 64 partial sums per item).  Results do
 * not depend on it; tests lower it to reach a second pass.  n == 0 is BGLS_ERR_ARG.  Returns 0. */
int bgls_set_ams_sum_cut(size_t n);
/* getAggregatePubKey over device-resident inputs (bgls/blsHAE.go:74-77 = AggregatePoints(ScalePoints(points, w)),
 * curves/curve.go:73-121,190-214): d_out (affine bytes of the group) = sum_i w_i P_i, weights = n 16-byte big-endian
 * magnitudes.  Computed by the bucket method (k_msm.hip: a counting sort of the (point, window) pairs by digit, one
 * thread per bucket, running sums) when n >= the threshold below and the digits are balanced, else by one
 * double-and-add per point; both give the same bytes. */
int bgls_weighted_sum_dev(int curve, int group, const void* d_pts, const void* d_w16, size_t n, void* d_out, void* stream);
/* Smallest n for which weighted sums take the bucket method (default 32; tests pin both paths with 0 / SIZE_MAX). */
int bgls_set_msm_min(size_t n);
/* Test-only, process-wide: the bucket method's window width c (4..13 bits; 0 = by size, clamp(floor(log2 n) - 3, 4, 13)) and its
 * threads per bucket S (1, 2, 4, 8 or 16; 0 = by size) for every later weighted sum.  The windows ceil(128 / c), the bucket and chunk
 * counts and the workspace sizes follow c and S; results do not depend on the setting.  Any other value is BGLS_ERR_ARG and leaves the
 * setting as it was.  Needs no device.  Returns 0. */
int bgls_set_msm_plan(int c, int S);
/* verifyMultiSignature over ScalePoints(keys, multiplicity) -- the body of KoskVerifyMultiSignatureWithMultiplicity
 * (bgls/blsKosk.go:137-150; that function prepends 0x01 to msg like KoskVerifyMultiSignature, the host mirror does
 * the same).  multiplicity: n int64 factors, negative = negate-then-multiply (curves/curve.go:190-214); NULL = plain
 * bgls_verify_multi. */
int bgls_verify_multi_multiplicity(int curve, const uint8_t* sig, const uint8_t* keys, const int64_t* multiplicity,
                                   size_t n, const uint8_t* msg, size_t msg_len);

/* ---- batch key generation and signing ---------------------------------------------------- */
/* LoadPublicKey over a batch (bgls/bgls.go:40-43: curve.GetG2().Mul(sk)): out[i] = scalars[i] * generator of `group`
 * (BGLS_G2 for public keys).  scalars: n x 32-byte big-endian. */
int bgls_scale_generator(int curve, int group, const uint8_t* scalars, size_t n, uint8_t* out);
/* Sign over a batch (bgls/bgls.go:46-56: HashToG1(msg).Mul(sk)); KoskSign is this call with 0x01 prepended to every
 * message (bgls/blsKosk.go:73-77).  sigs_out: n G1 points. */
int bgls_sign_batch(int curve, const uint8_t* sks, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n,
                    uint8_t* sigs_out);

/* ---- compressed wire formats ------------------------------------------------------------- */
/* Point.Marshal over a batch: out = n compressed points.  Inputs are validated like every other point (BGLS_ERR_ENCODING).
 *   alt-bn128 (curves/altbn128.go:81-89 G1, :203-221 G2; the reference's OWN format): G1 = x (32-byte big-endian) with the top
 *     bit of byte 0 set iff 2y > q; G2 = x_im || x_re with the top bits set iff 2 y_im > q / 2 y_re > q; infinity = zeros.
 *   BLS12-381 (curves/bls12_381.go:54-62 G1, :115-123 G2): 48 / 96 bytes in the ebfull/pairing ("ZCash") layout, the layout the
 *     reference names as its target ("TODO Make this match ebfull/pairing marshalling"): G1 = x big-endian, G2 = x.c1 || x.c0;
 *     byte 0 bit 7 = compressed, bit 6 = infinity (every other bit zero), bit 5 = y is the lexicographically larger of
 *     {y, -y} (G2: compare c1, then c0).  PARITY UNPINNED against the un-vendored github.com/dis2/bls12 the reference links
 *     (no vector exists in the reference); pinned by the format's public known-answer values (the generators' encodings,
 *     tests/test_wire.py) and by round trips. */
int bgls_compress_points(int curve, int group, const uint8_t* pts, size_t n, uint8_t* out);
/* UnmarshalG1 / UnmarshalG2, compressed branches.  out = n uncompressed points (zeros where rejected), ok[i] = 1 / 0 = the
 * reference's (Point, bool).
 *   alt-bn128 (curves/altbn128.go:296-327, :329-376): square roots by calcQuadRes / calcComplexQuadRes (curves/hash.go:178-223),
 *     the component-wise sign rule, then the MakeG*Point validation (G2: subgroup membership included).
 *   BLS12-381 (curves/bls12_381.go:242-264, inputs of 48 / 96 bytes): the flag rules above (a clear compression flag, an
 *     infinity flag with any other bit set, x >= p are refused), y = sqrt(x^3 + b) selected by the sort flag, then Check():
 *     membership in the order-r subgroup, G1 and G2 alike. */
int bgls_decompress_points(int curve, int group, const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok);
/* The same decoding -- the same accepted set, the same bytes, G1 and G2, both curves -- over device-resident input, by the one-pass kernel
 * on the carry-free limbs (wire_x.hpp / k_wirex.hip).  d_in: n compressed points, d_out: n uncompressed points (zeros where refused),
 * d_ok: n bytes.  Asynchronous on `stream` (NULL: the calling thread's context stream), like the other _dev calls.  n == 0 returns 0
 * without touching a pointer; a NULL pointer with n > 0, a bad group or n >= 2^30 is BGLS_ERR_ARG before any device work. */
int bgls_decompress_points_dev(int curve, int group, const void* d_in, size_t n, void* d_out, void* d_ok, void* stream);

/* ---- per-point operations backing the Go Point / PointT methods --------------------------- */
/* Point.Add (curves/altbn128.go:59-66,181-188; curves/bls12_381.go:33-41,94-102) */
int bgls_point_add(int curve, int group, const uint8_t* a, const uint8_t* b, uint8_t* out);
/* MakeG1Point/MakeG2Point/Unmarshal* validation (curves/altbn128.go:42-57,157-179;
 * curves/bls12_381.go:196-264 pt.Check()): 1 if the coordinates are canonical, the point is on the curve AND in the
 * order-r subgroup (G2 on both curves; G1 on BLS12-381, whose E(Fp) has cofactor (x-1)^2/3 -- alt-bn128's G1 is the whole
 * curve), 0 otherwise. */
int bgls_point_check(int curve, int group, const uint8_t* a);
/* The same validation over a batch (what constructing n Points costs in the reference: MakeG1Point / MakeG2Point with
 * check, UnmarshalG1 / UnmarshalG2; curves/altbn128.go:149-179,296-376, curves/bls12_381.go:196-264): ok_out[i] = 1 iff
 * point i has canonical coordinates, lies on its curve and in the order-r subgroup: G2 on both curves (endomorphism
 * criterion, exact), G1 on BLS12-381 ([r]P = infinity; alt-bn128's G1 is the whole curve).  The pairing value itself does
 * not see a G1 point's cofactor-order component (e(P + T, Q) = e(P, Q)), which is exactly why such points must be refused
 * at construction: sigma + T would be a second valid encoding of a signature, and scalars reduced mod r act wrongly on it.
 * Returns 0 or < 0. */
int bgls_check_points(int curve, int group, const uint8_t* pts, size_t n, uint8_t* ok_out);
/* GetG1 / GetG2 (curves/altbn128.go:423-429, curves/bls12_381.go:275-281) */
int bgls_generator(int curve, int group, uint8_t* out);
/* CurveSystem.Pair (curves/altbn128.go:130-141, curves/bls12_381.go:228-236) */
int bgls_pair(int curve, const uint8_t* g1, const uint8_t* g2, uint8_t* gt_out);
/* n independent CurveSystem.Pair calls in one set of launches: gt_out[b] = e(g1s[b], g2s[b]), n GT elements, byte-equal to bgls_pair on
 * the same pair for every pair of on-curve points, inside the order-r subgroups or not.  A pair with a point at infinity yields GT one.
 * A non-canonical or off-curve point ANYWHERE fails the whole call with BGLS_ERR_ENCODING and leaves gt_out as the caller passed it.
 * n == 0 returns 0 without touching a pointer; NULL arrays with n > 0 and n at or above 2^30 are BGLS_ERR_ARG, checked before any device
 * work; BGLS_ERR_NO_DEVICE without a device (no CPU fallback).  Returns 0 or < 0. */
int bgls_pair_batch(int curve, const uint8_t* g1s, const uint8_t* g2s, size_t n, uint8_t* gt_out);
/* n independent final exponentiations in one launch: gt_out[b] = gt_in[b]^((p^12 - 1) / r), is_one[b] = (gt_out[b] == 1) as 1 / 0.
 * gt_in: n GT-size wire values as bgls_miller_product_dev writes partials; any canonical Fp12 value is a legal input (0 gives 0, an
 * element of Fp6* gives one).  gt_out and is_one are nullable, not both.  A non-canonical coefficient (>= p) ANYWHERE fails the whole
 * call with BGLS_ERR_ENCODING and leaves the outputs as the caller passed them.  n == 0 returns 0 without touching a pointer; a NULL
 * gt_in with n > 0, both outputs NULL and n at or above 2^30 are BGLS_ERR_ARG, checked before any device work; BGLS_ERR_NO_DEVICE
 * without a device.  The batched finish of a caller who shards several verifications: one partial per verification in, one verdict
 * each out.  Returns 0 or < 0. */
int bgls_final_exp_batch(int curve, const uint8_t* gt_in, size_t n, uint8_t* gt_out, uint8_t* is_one);
/* PointT.Add = Fp12 multiplication (curves/altbn128.go:264-271, curves/bls12_381.go:160-168) */
int bgls_gt_mul(int curve, const uint8_t* a, const uint8_t* b, uint8_t* out);
/* PointT.Mul (curves/altbn128.go:273-281, curves/bls12_381.go:170-173): gt^k, k a 32-byte big-endian magnitude,
 * negative != 0 for k < 0 (the inverse of a GT element is its conjugate: GT elements are unitary).  The reference only ever raises
 * pairing values (its PointT comes out of Pair and Add alone) and hands the signed scalar to its upstream library, so it sets no
 * contract for other input.  Here: any canonical Fp12 element is accepted; negative == 0 returns the plain power, negative != 0 the
 * CONJUGATE of the power, which is the inverse power on unitary elements (all of GT) and nowhere else
 * (tests/test_gpu_f12_arith.py pins both). */
int bgls_gt_pow(int curve, const uint8_t* gt, const uint8_t* k_be32, int negative, uint8_t* out);
/* GetGTIdentity (curves/altbn128.go:441-443,478; curves/bls12_381.go:295-297,341) */
int bgls_gt_identity(int curve, uint8_t* out);

/* ---- device-resident variants (inputs already in HBM; used by bench.py and multi-GPU) ------ */
/* All pointers prefixed d_ are device pointers on the current device; `stream` is a hipStream_t
 * (NULL = the context's own stream).  Calls are asynchronous unless they return a verdict. */

/* Partial Miller product of one shard: d_partial_out (bgls_gt_size bytes, GT wire format of the
 * UN-exponentiated Fp12 value) = [miller(-sig, g2) if d_sig != NULL] * prod_i miller(H(m_i), pk_i).
 * Messages are fixed-stride: message i is d_msgs[i*msg_stride .. i*msg_stride + msg_len).
 * check_duplicates != 0 runs the exact duplicate-message scan on the device; *d_flags (one
 * uint32 in HBM, bit 0 = duplicate found, bit 1 = bad encoding, bit 2 = hash failure) is OR-ed. */
int bgls_miller_product_dev(int curve, const void* d_sig, const void* d_keys, const void* d_msgs,
                            size_t msg_len, size_t msg_stride, size_t n, int check_duplicates,
                            void* d_partial_out, void* d_flags, void* stream);

/* containsDuplicateMessage (bgls/bgls.go:139-150) on its own: sets bit 0 of *d_flags when two of the n device-resident
 * fixed-stride messages are byte-identical.  The multi-GPU path runs it over the all-gathered messages of every shard
 * (a duplicate may straddle two shards); the per-shard scan inside bgls_miller_product_dev covers one GPU. */
int bgls_duplicate_scan_dev(const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n, void* d_flags,
                            void* stream);
/* The same scan restricted to ONE bucket of the records: only those whose first byte is `bucket` mod n_buckets (bucket < n_buckets
 * <= 256) enter the table.  Equal records share a bucket, so rank r of an N-rank verification scanning bucket r of the all-gathered
 * 16-byte digests finds, between the ranks, exactly what one scan of everything finds -- with 1/N of the inserts each, so the scan
 * scales with the number of GPUs (the OR of the ranks' words travels with their status words).  The table is sized for twice the
 * bucket's fair share; if it fills up (records that are not digests, or chosen by an adversary) bit 0 is set: callers treat a hit
 * as "undecided" and settle it with the exact scan over the messages, so this can cost time but never miss a duplicate. */
int bgls_duplicate_scan_bucket_dev(const void* d_recs, size_t rec_len, size_t rec_stride, size_t n, unsigned bucket,
                                   unsigned n_buckets, void* d_flags, void* stream);
/* The digest exchange as an all-to-all by bucket (round 6; bgls_amd/sharding.py enqueue_digest_probe(exchange="all_to_all")).  An
 * all-gather hands all N x n digests to every rank, which then discards (N - 1) / N of them; here rank r receives only the digests it
 * owns (first byte = r mod N).  bgls_digest_pack_dev sorts a rank's n digests (16 bytes each, as bgls_message_digests_dev writes
 * them) into n_buckets slots of `cap` records each in d_out (n_buckets x cap x 16 bytes): slot b is what goes to rank b.  Unused
 * records are padding that belongs to another bucket, so all chunks have one size and no counts are exchanged.  A slot that would
 * overflow sets bit 0 of *d_flags ("undecided": settled by the exact scan, like any digest hit; cap = 1.25 x n / n_buckets + 1024 never
 * overflows on real digests).  bgls_duplicate_scan_packed_dev is the receiving half: the exact scan of the n_slots = n_buckets x cap
 * records a rank holds after the exchange (its own bucket's digests; the padding is skipped), table sized for all of them.
 * Replaces nothing in the reference (one process there): containsDuplicateMessage, bgls/bgls.go:139-150, across GPUs. */
int bgls_digest_pack_dev(const void* d_digests16, size_t n, unsigned n_buckets, size_t cap, void* d_out, void* d_flags, void* stream);
int bgls_duplicate_scan_packed_dev(const void* d_recs16, size_t n_slots, unsigned bucket, unsigned n_buckets, void* d_flags, void* stream);
/* 16-byte digests (the first 16 bytes of BLAKE2b-512) of n device-resident fixed-stride messages, to d_out16 (n x 16 bytes,
 * 16-byte aligned).  What the ranks of a multi-GPU verification exchange for the global containsDuplicateMessage rule
 * (bgls/bgls.go:139-150) instead of the messages themselves: no two equal digests => no two equal messages; a pair of equal
 * digests is settled by the exact scan over the messages (bgls_amd/sharding.py global_duplicate_scan). */
int bgls_message_digests_dev(const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n, void* d_out16,
                             void* stream);

/* Multiply `count` partial products (count x bgls_gt_size bytes, e.g. the all-gathered shards),
 * apply the single shared final exponentiation and compare with 1.  Returns 1 / 0 / < 0.
 * d_flags (may be NULL) is read: any bit set forces 0 (duplicate) or the matching error. */
int bgls_final_verify_dev(int curve, const void* d_partials, size_t count, const void* d_flags,
                          void* stream);

/* The same, split in two so that a second verification can be enqueued while this one's serial tail (reduction, final
 * exponentiation) is still running: submit returns at once, collect waits and returns 1 / 0 / < 0.  One verification in
 * flight per context. */
int bgls_final_verify_submit_dev(int curve, const void* d_partials, size_t count, const void* d_flags, void* stream);
int bgls_final_verify_collect(int curve);
/* Throughput mode: tells the engine that several verifications are in flight, so that Miller launches keep the block form
 * that is fastest per pairing (60 pairings per block) even where a launch's last round of resident blocks is nearly empty --
 * the neighbours fill it -- and a multi-signature's key sum runs at one wave per SIMD so that the other checks' latency-bound tails find
 * wave slots.  Results are identical in every mode.  Off by default; BGLS_THROUGHPUT=1 turns it on from the environment.  on = 2: one stream
 * per verification (no fork onto the context's side stream) but the launch shapes of a verification that has the machine to itself -- for
 * timing ONE verification stage by stage. */
int bgls_set_throughput_mode(int on);
/* Environment switches, each read ONCE per process (four in all).  None changes a result: they select between kernels that
 * compute the same bytes and exist for A/B measurements and for the legacy-path tests (tests/test_gpu_legacy_paths.py,
 * tests/test_gpu_x60.py).
 *   BGLS_THROUGHPUT=1     = bgls_set_throughput_mode(1)
 *   BGLS_MILLER_SHAPE=4|5 = bgls_set_miller_shape(shape, 0) below
 *   BGLS_LEGACY=<mask>    the one 32-bit-limb fallback kept per stage: 1 final exponentiation (k_final36), 2 latency Miller loop
 *                         (k_miller_lat), 4 epilogue (k_cofactor_epilogue), 8 G2 key sums (k_sum_main), 16 key-sum tree as one launch
 *                         per level, 32 BLS12-381 G1 scalar multiplications on 32-bit limbs, 64 every reduce pass on k_reduce_coop
 *   BGLS_NO_RCCL=1        host exchange between the devices of a key set instead of RCCL */
/* Shape of the Miller stage.  0 (default): automatic -- up to 128 pairings the latency kernel; above, k_miller_x60 (carry-free
 * limbs: nine of 29 bits on alt-bn128, fourteen of 28 on BLS12-381; lane-pair point steps) with 60 pairings per block, or with 64
 * per block where that saves a nearly empty last round of the 1024 resident blocks outside throughput mode (61 441..65 536
 * pairings: exactly 2^16 is one round).  4: k_miller_x60 for every batch; `mode` is then a development mode word, validated: bits
 * 0-1 role placement (0 by SIMD id, 1 wave 2 consumes, 2 rotate by block), bit 2 consumer priority, bit 3 producer priority, bit 4
 * the 64-pairing block form (clear: the 60-pairing form); values above 31 are rejected.  5: the 32-bit fused kernel
 * (k_miller_ab64) for every batch.  `mode` is ignored for shapes 0 and 5; any other shape is BGLS_ERR_ARG (shapes 1-3, the Miller loop
 * as two kernels joined through a line table in HBM, were removed in round 5: never faster than the fused kernels).
 * Results (partial products, GT bytes, verdicts) are identical for every shape. */
int bgls_set_miller_shape(int shape, int mode);
/* Contexts 0..15: each owns a HIP stream, its device workspaces and stage timers; the calling thread works on the one it
 * selected (default 0).  Two contexts let one host thread keep two verifications in flight (bench.py). */
int bgls_select_context(int index);

/* Device-resident key sum for the multisig path: d_out = projective partial sum of n G2 keys,
 * serialised as affine G2 bytes (bgls_g2_size).  Shards combine with bgls_aggregate_points. */
int bgls_aggregate_points_dev(int curve, int group, const void* d_pts, size_t n, void* d_out, void* stream);

/* bgls_verify_multi_batch with everything on the device: d_key_off = n_sets + 1 uint64 offsets (from 0), max_set = the
 * largest set's size, messages at a fixed stride.  _submit_dev enqueues only (collect with bgls_final_verify_collect). */
int bgls_verify_multi_batch_dev(int curve, const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets, size_t max_set,
                                const void* d_msgs, size_t msg_len, size_t msg_stride, int allow_duplicates, void* stream);
int bgls_verify_multi_batch_submit_dev(int curve, const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets, size_t max_set,
                                       const void* d_msgs, size_t msg_len, size_t msg_stride, int allow_duplicates, void* stream);
/* bgls_verify_multi_sets with everything on the device: d_key_off and max_set as in bgls_verify_multi_batch_dev (n_sets + 1
 * uint64 offsets from 0, the largest set's size; the call reads them back and returns BGLS_ERR_ARG unless they are monotone and
 * within max_set), message b at d_msgs + b * msg_stride (msg_len bytes).  Same semantics and return value; synchronises `stream`
 * (NULL: the context's stream) before it returns.  The Miller stage is k_miller_sets whatever bgls_set_miller_shape says. */
int bgls_verify_multi_sets_dev(int curve, const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets,
                               size_t max_set, const void* d_msgs, size_t msg_len, size_t msg_stride,
                               uint8_t* verdicts, uint8_t* gt_out, void* stream);
/* bgls_verify_multi_sets_combined with everything on the device: the arguments of bgls_verify_multi_sets_dev, then the HOST words
 * group_off / n_groups / seed as in the host-pointer call. */
int bgls_verify_multi_sets_combined_dev(int curve, const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets,
                                        size_t max_set, const void* d_msgs, size_t msg_len, size_t msg_stride, const uint64_t* group_off,
                                        size_t n_groups, const uint8_t seed[32], uint8_t* verdicts, uint8_t* gt_out, void* stream);
/* bgls_verify_multi_hae_sets with everything on the device, shaped as bgls_verify_multi_sets_dev (d_key_off read back and checked,
 * every root on the device).  Same semantics and return value; synchronises `stream` (NULL: the context's stream) before it returns. */
int bgls_verify_multi_hae_sets_dev(int curve, const void* d_sigs, const void* d_keys, const void* d_key_off, size_t n_sets,
                                   size_t max_set, const void* d_msgs, size_t msg_len, size_t msg_stride,
                                   uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out, void* stream);
/* bgls_ams_verify_batch with everything on the device: d_signers (uint32 indices) and d_signer_off (n + 1 uint64 offsets from 0) are read
 * back and checked before any launch (monotone, no list above max_signers: BGLS_ERR_ARG; a process without a device has no device
 * memory, so there d_signer_off is read where it lies and a bad argument is still BGLS_ERR_ARG); message b is msg_len bytes at
 * d_msgs + b msg_stride.  Same semantics and return value; synchronises `stream` (NULL: the context's stream) before it returns. */
int bgls_ams_verify_batch_dev(int curve, const void* d_apks, const void* d_agg_keys, const void* d_agg_sigs, const void* d_signers,
                              const void* d_signer_off, size_t n, size_t max_signers, const void* d_msgs, size_t msg_len,
                              size_t msg_stride, uint8_t* verdicts, uint8_t* gt_out, void* stream);
/* bgls_bb_verify_batch with its inputs on the device (same layouts).  Same semantics and return value; synchronises `stream`
 * (NULL: the context's stream) before it returns. */
int bgls_bb_verify_batch_dev(int curve, const void* d_sigmas, const void* d_rs, const void* d_keys, const void* d_ms,
                             size_t n, uint8_t* verdicts, uint8_t* gt_out, void* stream);
/* bgls_pair_batch and bgls_final_exp_batch with inputs AND outputs on the device (same layouts; d_is_one: n bytes).  Same semantics and
 * return value, except that after a failed call the device outputs are undefined; both synchronise `stream` (NULL: the context's
 * stream) before they return. */
int bgls_pair_batch_dev(int curve, const void* d_g1s, const void* d_g2s, size_t n, void* d_gt_out, void* stream);
int bgls_final_exp_batch_dev(int curve, const void* d_gt_in, size_t n, void* d_gt_out, void* d_is_one, void* stream);
/* bgls_bb_verify_batch_combined with its items on the device (same layouts), then the HOST words group_off, n_groups and seed (they plan
 * the launches).  Same contract and return value; synchronises `stream` (NULL: the context's stream) before it returns. */
int bgls_bb_verify_batch_combined_dev(int curve, const void* d_sigmas, const void* d_rs, const void* d_keys, const void* d_ms, size_t n,
                                      const uint64_t* group_off, size_t n_groups, const uint8_t seed[32], uint8_t* verdicts,
                                      uint8_t* gt_out, void* stream);
/* bgls_verify_aggregate_batch with signatures, keys and messages on the device: d_sigs = n_inst G1 points, d_keys = inst_off[n_inst]
 * G2 points, message i at d_msgs + i * msg_stride (msg_len bytes).  inst_off stays a HOST array (it plans the launches).  Same
 * semantics and return value; synchronises `stream` (NULL: the context's stream) before it returns.  Every batch runs the Miller
 * stage as k_miller_x60 in its 60-pairing form, whatever bgls_set_miller_shape says. */
int bgls_verify_aggregate_batch_dev(int curve, const void* d_sigs, const void* d_keys, const uint64_t* inst_off, size_t n_inst,
                                    const void* d_msgs, size_t msg_len, size_t msg_stride, int allow_duplicates,
                                    uint8_t* verdicts, uint8_t* gt_out, void* stream);
/* bgls_verify_aggregate_distinct_batch / bgls_verify_single_distinct_batch with signatures, keys and fixed-stride messages on the device,
 * parameters as in bgls_verify_aggregate_batch_dev / bgls_verify_multi_sets_dev (item b of the single form: d_sigs[b], d_keys[b]). */
int bgls_verify_aggregate_distinct_batch_dev(int curve, const void* d_sigs, const void* d_keys, const uint64_t* inst_off, size_t n_inst,
                                             const void* d_msgs, size_t msg_len, size_t msg_stride, uint8_t* verdicts,
                                             uint8_t* gt_out, void* stream);
int bgls_verify_single_distinct_batch_dev(int curve, const void* d_sigs, const void* d_keys, size_t n, const void* d_msgs,
                                          size_t msg_len, size_t msg_stride, uint8_t* verdicts, uint8_t* gt_out, void* stream);
/* verify_multi with keys already on the device. */
int bgls_verify_multi_dev(int curve, const void* d_sig, const void* d_keys, size_t n, const void* d_msg,
                          size_t msg_len, void* stream);
/* The same without waiting: the verdict is collected with bgls_final_verify_collect on the same context. */
int bgls_verify_multi_submit_dev(int curve, const void* d_sig, const void* d_keys, size_t n, const void* d_msg,
                                 size_t msg_len, void* stream);

/* ---- measurement hooks (bench.py; not part of the reference's interface) ------------------ */
/* ---- device-resident key sets (opaque handles so keys uploaded once are verified many times) -------------
 * A key set is n G2 public keys, parsed and validated once, resident in HBM as Montgomery-form affine points next to
 * their wire bytes, cut into contiguous ranges over n_devices GPUs (devices[] lists them; NULL = 0 .. n_devices-1; an id
 * may repeat, which is how the multi-device code is exercised on a one-GPU box).  This is what the Go shim's
 * altbn128Point2 / bls12Point2 slices become (curves/altbn128.go:19-29, curves/bls12_381.go:18-28): the shim uploads a
 * []Point once, keeps the handle (runtime.SetFinalizer -> bgls_keys_free) and passes it to every Verify*.
 * flags: BGLS_KEYS_CHECK also requires every key to lie in the order-r subgroup (the reference's construction-time
 * check); any invalid key fails the upload with BGLS_ERR_ENCODING.
 * BGLS_KEYS_PREPARE additionally walks the G2 point steps of the Miller loop once per key and keeps every step's line
 * function in HBM (13-17 KB per key: a 2^20-key set is 14-18 GB of the 288), so that verifications against the set only
 * scale and fold those lines (prepared.hpp): the fixed-argument precomputation pairing libraries offer as "prepared G2".
 * Verdicts and the final GT element are identical to the unprepared path. */
typedef uint64_t bgls_keys_t;
#define BGLS_KEYS_CHECK 1u
#define BGLS_KEYS_PREPARE 2u
int bgls_keys_upload(int curve, const uint8_t* keys, size_t n, const int* devices, int n_devices, unsigned flags, bgls_keys_t* handle_out);
/* Lifetime: a key set must not be freed while a call that uses it is in progress or has device work outstanding (the *_dev
 * entry points return before their kernels finish: synchronise the stream first); calls on one key set from several threads
 * are otherwise safe, each running on the calling thread's context. */
int bgls_keys_free(bgls_keys_t handle);
int bgls_keys_info(bgls_keys_t handle, int* curve, size_t* n, int* n_devices);
/* A key set from n COMPRESSED G2 keys (Point.Marshal: 64 bytes on alt-bn128, 96 on BLS12-381).  Every shard uploads its range of the
 * compressed bytes and decodes it on its device in one pass (UnmarshalG2: square root, sign rule, curve check, subgroup membership), so
 * validation is always on: BGLS_KEYS_CHECK is implied and ignored, BGLS_KEYS_PREPARE acts as in bgls_keys_upload.  Any refused key fails
 * the upload with BGLS_ERR_ENCODING, frees everything and, where first_bad is not NULL, writes the smallest refused index over all
 * shards there; first_bad is left untouched on success and on every other error.  The set is the one bgls_keys_upload makes from the
 * decompressed keys on the same devices with the same flags (keys at infinity included).  Devices and argument errors as there. */
int bgls_keys_upload_compressed(int curve, const uint8_t* keys_c, size_t n, const int* devices, int n_devices, unsigned flags, bgls_keys_t* handle_out,
                                size_t* first_bad);
/* The uncompressed wire bytes of keys [first, first + count) of any key set, across its shards.  BGLS_ERR_ARG for an unknown handle, a
 * range beyond the set, or a NULL out with count > 0. */
int bgls_keys_read(bgls_keys_t handle, size_t first, size_t count, uint8_t* out);
/* verifyAggSig (bgls/bgls.go:94-119) against a resident key set: message i belongs to key i; n must equal the set's size.
 * Every device of the set hashes its message range and multiplies its Miller values (one host thread per device), the
 * 384 / 576-byte partial products and status words meet on the first device (ncclAllGather over the devices' streams
 * when RCCL is usable and the devices are distinct, peer copies otherwise), which runs the single final exponentiation.
 * Same GT element, hence the same verdict, for any number of devices. */
int bgls_verify_aggregate_h(bgls_keys_t handle, const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n,
                            int allow_duplicates);
/* The same verification, also returning the GT element e(-sig, g2) * prod_i e(H(m_i), pk_i) (the PairingProduct value of
 * bgls/bgls.go:113-114; the identity iff the verdict is 1): canonical bytes, identical for any number of devices. */
int bgls_verify_aggregate_h_gt(bgls_keys_t handle, const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off, size_t n,
                               int allow_duplicates, uint8_t* gt_out);
/* DistinctMsgVerifyAggregateSignature against a resident key set (any number of shards, prepared or not): every shard builds its
 * hash inputs from its own resident wire bytes and uploads only its own range of messages.  n must equal the set's size
 * (BGLS_ERR_ARG).  gt_out: NULL or one GT element, byte-equal to bgls_verify_aggregate_h_gt on messages the caller prefixed. */
int bgls_verify_aggregate_distinct_h(bgls_keys_t handle, const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off,
                                     size_t n, uint8_t* gt_out);
/* verifyMultiSignature (bgls/bgls.go:89-92) against a ONE-device key set, signature and message already on the device, on the
 * calling thread's context and the given stream: the key sum reads the set's resident sum-ready records -- the keys are the
 * reference's already-constructed Points (parsed and validated at upload), so nothing but the n - 1 additions of
 * AggregatePoints (curves/curve.go:73-121) is left per key.  _submit_ enqueues and returns; the verdict is collected with
 * bgls_final_verify_collect(curve) on the same context, as for bgls_verify_multi_submit_dev. */
int bgls_verify_multi_keys_dev(bgls_keys_t handle, const void* d_sig, const void* d_msg, size_t msg_len, void* stream);
int bgls_verify_multi_keys_submit_dev(bgls_keys_t handle, const void* d_sig, const void* d_msg, size_t msg_len, void* stream);
/* bgls_miller_product_dev against a ONE-device key set (prepared or not) with device-resident fixed-stride messages, on
 * the calling thread's context and the given stream; finish with bgls_final_verify_(submit_)dev. */
int bgls_miller_product_keys_dev(bgls_keys_t handle, const void* d_sig, const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n,
                                 int check_duplicates, void* d_partial_out, void* d_flags, void* stream);
/* verifyMultiSignature (bgls/bgls.go:89-92) against a resident key set: per-device partial key sums (projective G2
 * points) are gathered on the first device, added, and the two-pairing check runs there. */
int bgls_verify_multi_h(bgls_keys_t handle, const uint8_t* sig, const uint8_t* msg, size_t msg_len);
/* Multi-signatures by SIGNER BITMAP against a ONE-device key set: MultiSig{keys, sig, msg} (bgls/blsKosk.go:108-112) whose keys are a
 * sub-slice of the registered keys.  Set b of n_sets is a bitmap row over the set's n keys, `stride` bytes apart: key i is selected iff
 * (row[i >> 3] >> (i & 7)) & 1.  Nothing of a key is uploaded, parsed or checked again: the key sums read the resident sum-ready records,
 * and their work follows the selected keys -- or, where more than half of the set is selected, the absentees, subtracted from the sum of
 * the whole set (computed once per key set, by the first of these calls).
 *   bgls_aggregate_subsets_h            out[b] = sum of the keys selected by row b (AggregateKeys over the sub-slice): n_sets G2 points
 *   bgls_verify_multi_subsets_h         n_sets verifyMultiSignature calls (bgls/bgls.go:89-92): set b = sigs[b], the selected keys, message b
 *   bgls_verify_multi_subsets_keys_dev  the same with signatures, rows and fixed-stride messages on the device, on the calling thread's
 *                                       context and the given stream; rows are read as 32-bit words: stride and d_bitmaps multiples of 4
 * verdicts[b], gt_out[b] and apk_out[b] are byte-equal to what bgls_verify_multi_sets and bgls_aggregate_sets return for the gathered keys
 * of subset b; gt_out and apk_out may be NULL.  An empty subset sums to infinity, and its set is accepted iff its signature is the point at
 * infinity, as bgls_verify_multi with n = 0.  Returns the number of accepted sets (aggregate: 0) or, for the whole call, the codes of
 * bgls_verify_multi_sets: BGLS_ERR_ENCODING for a bad signature, BGLS_ERR_HASH for an exhausted hash.
 * BGLS_ERR_ARG, before any device work: NULL arrays with n_sets > 0; for the device form a stride or pointer that is not 4-byte aligned;
 * an unknown handle; a key set on more than one device; stride < ceil(n / 8); a batch beyond the launch bounds of bgls_aggregate_sets (2^30
 * blocks / 8 GiB of partial sums); the lane-pair key sum switched off (BGLS_LEGACY bit 8); a row with a bit at a position >= n, anywhere in
 * its stride -- found on the host by the host forms, by the planning pass of the device form, which then fails the whole call with the same
 * code.  n_sets == 0 returns 0 without touching a pointer.  Without a device: BGLS_ERR_NO_DEVICE (decided after the NULL and alignment
 * checks and before the handle is looked at: a handle can only come from an upload to a device). */
int bgls_aggregate_subsets_h(bgls_keys_t handle, const uint8_t* bitmaps, size_t stride, size_t n_sets, uint8_t* out);
int bgls_verify_multi_subsets_h(bgls_keys_t handle, const uint8_t* sigs, const uint8_t* bitmaps, size_t stride, size_t n_sets,
                                const uint8_t* msg_blob, const uint64_t* msg_off, uint8_t* verdicts, uint8_t* apk_out, uint8_t* gt_out);
int bgls_verify_multi_subsets_keys_dev(bgls_keys_t handle, const void* d_sigs, const void* d_bitmaps, size_t stride, size_t n_sets,
                                       const void* d_msgs, size_t msg_len, size_t msg_stride, uint8_t* verdicts, uint8_t* apk_out,
                                       uint8_t* gt_out, void* stream);
/* Which side of a row the subset key sums add: 0 = chosen per set (complement when 2 popcount > n; default), 1 = never the complement,
 * 2 = always.  Process-wide; results do not depend on it (A/B measurements and tests). */
int bgls_set_subset_complement(int mode);
/* GROUPED aggregate verification by SIGNER BITMAP against a ONE-device key set: verifyAggSig with allowDuplicates = true
 * (KoskVerifyAggregateSignature, bgls/blsKosk.go:100-106) whose keys are the sub-slice of the registered keys that ONE bitmap selects, with
 * one hash and one pairing per DISTINCT message (bgls_verify_aggregate_grouped's product).  Key i is selected iff
 * (bitmap[i >> 3] >> (i & 7)) & 1, the bit rule of the subset calls; bitmap == NULL selects every key (bitmap_len is then ignored).  Message j
 * belongs to the j-th selected key in ascending key index, and n_msgs must equal the number of selected keys.  Nothing of a key is
 * uploaded, parsed or checked again: the key sums read the resident sum-ready records (a set uploaded with BGLS_KEYS_PREPARE gives the
 * same bytes).
 *   bgls_verify_aggregate_grouped_h         signature, bitmap and messages (blob + n_msgs + 1 offsets) on the host
 *   bgls_verify_aggregate_grouped_keys_dev  all three on the device, messages of msg_len bytes at msg_stride, on the calling thread's context
 *                                           and the given stream; the bitmap is read as 32-bit words: bitmap_len and d_bitmap multiples of 4
 * Returns 1 / 0 / < 0 exactly as bgls_verify_aggregate_grouped does on the gathered keys and the same messages; *n_groups (nullable) is the
 * number of distinct messages and gt_out (nullable) the GT element, byte-equal to that call's.  No signer (no bit set and n_msgs == 0, or
 * an empty key set) returns 1 iff sig is the point at infinity, with *n_groups = 0.  There is no duplicate rule.
 * BGLS_ERR_ARG, before any device work: NULL sig; NULL msg_off (host form, also for n_msgs == 0); NULL msg_blob with bytes to read;
 * non-monotone offsets; n_msgs at or above 2^30; device form: NULL d_msgs with n_msgs > 0, msg_stride < msg_len, d_bitmap or bitmap_len not a
 * multiple of 4.  Then, without a device, BGLS_ERR_NO_DEVICE (before the handle is looked at).  Then BGLS_ERR_ARG again: an unknown
 * handle; a key set on more than one device; the lane-pair key sum switched off (BGLS_LEGACY bit 8); bitmap_len < ceil(n / 8) (device
 * form: < 4 ceil(n / 32)); a bit at a position >= n anywhere in bitmap_len; a popcount different from n_msgs -- the last two found on the
 * host by the host form, by the selection pass of the device form, which then fails the whole call.  Whole-call errors are the
 * sibling's: BGLS_ERR_ENCODING for a bad signature, BGLS_ERR_HASH. */
int bgls_verify_aggregate_grouped_h(bgls_keys_t handle, const uint8_t* sig, const uint8_t* bitmap, size_t bitmap_len,
                                    const uint8_t* msg_blob, const uint64_t* msg_off, size_t n_msgs, size_t* n_groups, uint8_t* gt_out);
int bgls_verify_aggregate_grouped_keys_dev(bgls_keys_t handle, const void* d_sig, const void* d_bitmap, size_t bitmap_len,
                                           const void* d_msgs, size_t msg_len, size_t msg_stride, size_t n_msgs, size_t* n_groups,
                                           uint8_t* gt_out, void* stream);
/* Groups of at most min(keys, 128) keys are summed by one lane pair each instead of a block (k_sumpairgrp_main); 0 switches that kernel
 * off.  Default 32.  Process-wide; results never depend on it (A/B measurements and tests).  Returns 0, with or without a device. */
int bgls_set_group_small(size_t keys);
/* Shape of the key sets uploaded with BGLS_KEYS_PREPARE from now on: ng = pairings per group and squaring of the fold (0: chosen by the set's
 * size; else 6..96), chunk = keys per preparation launch (0: 2^17).  A resident set keeps its shape.  Process-wide; results never depend on
 * it (tests and A/B measurements).  Returns 0, or BGLS_ERR_ARG with the setting unchanged; with or without a device. */
int bgls_set_prepare_shape(size_t ng, size_t chunk);
/* Contexts: a key-set verification runs shard s on context (selected + s) mod 16 of the shard's device, `selected` being the
 * calling thread's bgls_select_context (default 0); the final product / exponentiation runs on shard 0's context. */
/* The same two calls with host keys, for callers without a resident set: upload (with BGLS_KEYS_CHECK: the keys have not been
 * through a Point constructor, so subgroup membership is checked here; a key outside G2 gives BGLS_ERR_ENCODING), verify, free. */
int bgls_verify_aggregate_multi(int curve, const uint8_t* sig, const uint8_t* keys, const uint8_t* msg_blob, const uint64_t* msg_off,
                                size_t n, int allow_duplicates, const int* devices, int n_devices);
int bgls_verify_multi_multi(int curve, const uint8_t* sig, const uint8_t* keys, size_t n, const uint8_t* msg, size_t msg_len,
                            const int* devices, int n_devices);
/* Which exchange the last multi-device call on this thread used: 0 none (one device), 1 peer / device copies, 2 RCCL. */
int bgls_last_exchange(void);
/* 1 if librccl was found and its entry points resolved (dlopen at first use), else 0. */
int bgls_rccl_available(void);

/* Per-stage device time, measured with HIP events on the stream the kernels are launched on.
 * Stages: "dup_check", "h2c", "miller", "reduce", "final_exp", "sum_points" (one scope per key sum: main pass, tree and
 * conversion), "sum_main" (the main-pass kernel of a key sum alone, nested in "sum_points"). */
int bgls_profile_enable(int on); /* also resets the counters */
int bgls_profile_get(const char* stage, double* total_ms, unsigned long long* launches);
/* Measured peak of dependent-free v_mad_u64_u32 chains on this GPU, in 32x32->64 MAC/s:
 * the roofline denominator for the integer-multiply-bound kernels. */
int bgls_probe_mad_peak(double* mac_per_s);
/* Self-test of the ABI's exception barrier, usable without a device: raises a C++ exception of the given kind inside the
 * library (0 bad_alloc, 1 length_error, 2 system_error, 3 runtime_error, 4 a non-standard object, 5 an unservable std::vector,
 * 6 bad_alloc on a shard's host thread) and returns the error code the barrier maps it to (BGLS_ERR_NOMEM / _HIP / _ARG).
 * No entry point lets an exception unwind into the caller (the reference never panics: curves/curve.go:15-22). */
int bgls_selftest_exception_barrier(int kind);
/* Self-tests of the workspace contract: the library never frees or clears its device scratch between calls, so
 * every word a kernel reads must have been written earlier in the same call.  bgls_selftest_fill_workspaces sets the whole capacity of
 * every cached workspace of every ready context of every device, and the contexts' pinned result words, to `byte`; with keys != 0 also
 * the exchange records of that key set's shards.  Device tables, resident key data and caller buffers are left alone.  It waits for the
 * fills, refuses with BGLS_ERR_ARG before it sets one byte while a verification is in flight on any context, and reports the bytes set
 * in *bytes_filled (nullable).  The fills run on the contexts' own streams: synchronise a stream of your own first.  bgls_selftest_workspace_caps writes the capacity of each workspace slot of the calling thread's context (0: never
 * allocated) to caps[0 .. min(n, slots)) and returns the slot count.  Test-only: no binding mirrors them. */
int bgls_selftest_fill_workspaces(int byte, uint64_t keys, uint64_t* bytes_filled);
int bgls_selftest_workspace_caps(size_t* caps, int n);
/* What the last weighted sum (bgls_weighted_sum_dev, the hashed-exponent entries, bgls_verify_multi_multiplicity) on the calling thread's
 * context did: out[0] = path (0 per-point form because n was below bgls_set_msm_min's threshold or n * windows reached 2^32, 1 bucket
 * method, 2 per-point form after the histogram showed a bucket above max(8 (n >> c), 64)), out[1] = window bits c, out[2] = threads per
 * bucket S, out[3] = windows W, out[4] = largest bucket, out[5] = listed (point, window) pairs; the last two are 0 for path 0.  All zero
 * before the first sum; an empty sum reports nothing.  NULL is BGLS_ERR_ARG; without a device BGLS_ERR_NO_DEVICE.  Test-only: no
 * binding mirrors it. */
int bgls_selftest_msm_last(uint32_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* BGLS_HIP_H */
