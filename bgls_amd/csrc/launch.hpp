// Host-callable launchers of every kernel in the library.  Each k_*.hip translation unit defines the launchers of the
// kernels it holds (a <<<>>> launch must sit in the unit that defines the kernel; the units are compiled in parallel and
// linked without relocatable device code); engine.hip only sees these declarations.
#pragma once
#include "dev_common.hpp"

namespace bgls {
namespace kl {

// ---- k_hash.hip
void digest_pack(hipStream_t st, const uint8_t* dig, size_t n, uint8_t* out, size_t cap, uint32_t n_buckets, uint32_t* counts, uint32_t* flags);
constexpr uint32_t DUP_MAX_PROBE = 1023;      // bucketed duplicate scan: probes per record before it reports "undecided"
void dup_check(hipStream_t st, MsgView mv, size_t n, uint32_t* table, uint32_t mask, uint32_t* flags, uint32_t bucket = 0, uint32_t n_buckets = 1, uint64_t seed = 0,
               bool unbounded = false);
// segmented scan of a batch of instances (inst_off: n_inst + 1 device offsets): a duplicate within instance b sets inst_flags[b]
void dup_check_seg(hipStream_t st, MsgView mv, size_t n, const uint64_t* inst_off, uint32_t n_inst, uint32_t* table, uint32_t mask, uint32_t* inst_flags,
                   uint64_t seed);
void msg_digest(hipStream_t st, MsgView mv, size_t n, uint8_t* out);
void h2c_bn(hipStream_t st, MsgView mv, size_t n, uint32_t* lists, uint32_t* counters, Aff<F1<BN254>>* out, uint32_t* flags, bool lean);
void h2c_bls(hipStream_t st, MsgView mv, size_t n, Jac<F1<BLS381>>* pts, uint32_t* kinds, Aff<F1<BLS381>>* out, bool raw);   // pts: 2n Jacobian work items
void blake2x_expand(hipStream_t st, const uint64_t* root, uint32_t xof_len, uint8_t* out);

// ---- k_msggroup.hip   (grouping of messages by exact bytes; the stages in the order Engine::group_messages runs them, see the unit's head)
// scan_excl: out[0 .. n] = the exclusive prefix sums of in[0 .. n) and the total; bsum: scan_tiles(n) words of scratch
size_t scan_tiles(size_t n);
template <class TI, class TO> void scan_excl(hipStream_t st, const TI* in, size_t n, TO* bsum, TO* out);
void grp_resolve(hipStream_t st, MsgView mv, size_t n, uint32_t* table, uint32_t mask, uint32_t* first, uint32_t* slot_of, uint64_t seed);
void grp_mark(hipStream_t st, size_t n, const uint32_t* slot_of, const uint32_t* first, uint32_t* rep);
void grp_assign(hipStream_t st, size_t n, const uint32_t* rep, const uint32_t* rank, const uint32_t* slot_of, uint32_t* table, uint32_t* rep_idx);
void grp_groups(hipStream_t st, size_t n, const uint32_t* slot_of, const uint32_t* table, uint32_t* group_of, uint32_t* count);
void grp_scatter(hipStream_t st, size_t n, const uint32_t* group_of, const uint32_t* start, uint32_t* cursor, uint32_t* idx);
// small: groups of at most that many keys get no item (grpkeys.hpp; 0: every group has items)
void grp_nitems(hipStream_t st, size_t d, const uint32_t* start, uint32_t chunk, uint32_t small, uint32_t* nitems, uint32_t* meta);      // meta[0] <- max(meta[0], largest group)
// selection pass (grpkeys.hpp): cnt[w] for the grpkeys_words(n) words below n, FLAG_SUBSET_STRAY for a bit >= n anywhere in row_words words;
// then, behind the scan of cnt, sel[rank[w] ..] = the positions word w selects (nothing at or beyond cap)
void sel_count(hipStream_t st, const uint32_t* row, size_t row_words, size_t n, uint32_t* cnt, uint32_t* flags);
void sel_scatter(hipStream_t st, const uint32_t* row, size_t n, const uint32_t* rank, uint32_t cap, uint32_t* sel);
// items: {lo, hi} per item; joins / multi: the meta[1] groups of several items, {first, last + 1} of their partials and the group (meta[1] from 0)
void grp_items(hipStream_t st, size_t d, const uint32_t* start, const uint64_t* item_start, uint32_t chunk, void* items, void* joins, uint32_t* multi, uint32_t* meta);
// key sums to their places (rec_bytes each, a multiple of 16): a one-item group's partial from parts[item_start[g]]; joined sum k to group multi[k]
void grp_pick(hipStream_t st, size_t d, const uint64_t* item_start, const uint8_t* parts, size_t rec_bytes, uint8_t* sums);
void grp_place(hipStream_t st, size_t m, const uint32_t* multi, const uint8_t* joined, size_t rec_bytes, uint8_t* sums);
void grp_lens(hipStream_t st, MsgView mv, size_t d, const uint32_t* rep_idx, uint64_t* lens);
void grp_compact(hipStream_t st, MsgView mv, size_t d, const uint32_t* rep_idx, const uint64_t* out_off, size_t out_stride, uint8_t* out);

// ---- k_points.hip   (group = BGLS_G1 / BGLS_G2; Jacobian workspaces are passed as void*)
template <class C> void g1_to_bytes(hipStream_t st, const Aff<F1<C>>* in, size_t n, uint8_t* out);
template <class C> void g1_parse(hipStream_t st, const uint8_t* in, size_t n, int negate, Aff<F1<C>>* out, uint32_t* flags);
template <class C> void sum_main(hipStream_t st, int group, bool parsed, const uint8_t* pts, size_t n, unsigned waves, void* out, uint32_t* flags);
template <class C> void sumseg_main(hipStream_t st, int group, const uint8_t* pts, const uint64_t* off, size_t nsets, unsigned P, void* out, uint32_t* flags);
// ---- k_sumpair.hip   (G2 key sums on lane pairs, carry-free limbs: rx_jacpair.hpp)
template <class C> void sumpair_main(hipStream_t st, int src, const uint8_t* pts, size_t n, unsigned partials, void* out, uint32_t* flags);
template <class C> void sumpairseg_main(hipStream_t st, const uint8_t* pts, const uint64_t* off, size_t nsets, unsigned P, void* out, uint32_t* flags);
// items: n_items pairs {lo, hi} (uint2) of positions in the index list idx (nullptr: the positions themselves), one block and one Jacobian
// partial per item (msggroup.hpp)
template <class C> void sumpairidx_main(hipStream_t st, const uint8_t* pts, const uint32_t* idx, const void* items, size_t n_items, void* out, uint32_t* flags);
// the same over a key set's sum-ready records (no parsing, no curve check); sel != nullptr: idx holds ranks among the keys a signer bitmap
// selects, the key is sel[idx[k]] (grpkeys.hpp)
template <class C> void sumpairidx_recs(hipStream_t st, const uint8_t* recs, const uint32_t* idx, const uint32_t* sel, const void* items, size_t n_items, void* out, uint32_t* flags);
// d Jacobian sums, one per group and lane pair: the sum of a group of at most `small` keys (its run start[g] .. start[g + 1] of idx), the
// point at infinity for every other group
template <class C> void sumpairgrp_main(hipStream_t st, const uint8_t* recs, const uint32_t* idx, const uint32_t* sel, const uint32_t* start, size_t d, uint32_t small, void* out);
template <class C> void sum_wave(hipStream_t st, int group, const void* in, size_t n, void* out);
template <class C> void sum_pair(hipStream_t st, int group, const void* in, size_t n, void* out);
template <class C> void sum_coop(hipStream_t st, const void* in, size_t n, void* out);        // G2, one wave per addition (jac_coop.hpp)
template <class C> void sum_next(hipStream_t st, int group, const void* in, size_t n, int R, void* out);
template <class C> void jac_to_bytes(hipStream_t st, int group, const void* in, size_t n, uint8_t* out);
template <class C> void wsum_first(hipStream_t st, int group, const uint8_t* pts, const uint8_t* w16, const uint8_t* signs, size_t n, void* out, uint32_t* flags);
template <class C> void scale(hipStream_t st, int group, const uint8_t* pts, const uint8_t* scalars, const uint8_t* signs, size_t n, uint8_t* out, uint32_t* flags, int sbytes);
template <class C> void scale_aff(hipStream_t st, int group, const Aff<F1<C>>* g1_pts, const uint8_t* scalars, size_t n, uint8_t* out);
template <class C> void check(hipStream_t st, int group, const uint8_t* pts, size_t n, uint32_t* flags, uint8_t* ok);
template <class C> void g2_parse(hipStream_t st, const uint8_t* in, size_t n, int check_subgroup, void* out, uint32_t* flags);
template <class C> size_t g2_parsed_bytes();
template <class C> void g2_sumready(hipStream_t st, const void* mont, size_t n, void* out);      // k_sumpair.hip: a key set's sum-ready records
template <class C> size_t g2_sumready_bytes();
template <class C> void generator(hipStream_t st, int group, uint8_t* out);
void compress_bn(hipStream_t st, int group, const uint8_t* in, size_t n, uint8_t* out, uint32_t* flags);
void decompress_bn(hipStream_t st, int group, const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok);
// ---- k_wire.hip   (BLS12-381 compressed forms, ebfull/pairing layout)
void compress_bls(hipStream_t st, int group, const uint8_t* in, size_t n, uint8_t* out, uint32_t* flags);
void decompress_bls(hipStream_t st, int group, const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok);
// ---- k_wirex.hip   (both curves' compressed forms on the carry-free limbs, wire_x.hpp: decompress + membership + key-set record in one pass)
// out: n uncompressed points (zeros where refused), ok: n bytes or nullptr, mont: n records of g2_parse or nullptr (G2 only),
// first_bad: one word the caller set to 0xFFFFFFFF, lowered to the smallest refused index (atomicMin), or nullptr
template <class C> void wirex_decode(hipStream_t st, int group, const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok, void* mont, uint32_t* first_bad);
void mad_probe(hipStream_t st, unsigned blocks, unsigned threads, uint32_t seed, int iters, uint64_t* sink);
template <class C> size_t jac_bytes(int group) { return (size_t)3 * (group == 1 ? 1 : 2) * C::L * 4; }

// ---- k_msm.hip   (bucket-method weighted sums, fixed-base generator multiples, in-place G1 scaling)
struct MsmPlan { int c, W, K, S; uint32_t NB, NQ, NCH; };    // window bits, windows, digits per chunk, threads per bucket, buckets, chunks per window, chunks
MsmPlan msm_plan(size_t n, int force_c = 0, int force_s = 0);      // force_*: bgls_set_msm_plan's override, 0 = chosen by n
template <class C> size_t msm_aff_bytes(int group);
template <class C>
void msm_parse(hipStream_t st, int group, const uint8_t* pts, const uint8_t* w16, const uint8_t* signs, size_t n, const MsmPlan& p, void* aff,
               uint32_t* cnt, uint32_t* flags);
void msm_scan(hipStream_t st, uint32_t* cnt, uint32_t NB, uint32_t* start, uint32_t* meta);
template <class C>
void msm_scatter(hipStream_t st, int group, const void* aff, const uint8_t* w16, size_t n, const MsmPlan& p, uint32_t* cursor, uint32_t* list);
template <class C>
void msm_buckets(hipStream_t st, int group, const void* aff, const uint32_t* list, const uint32_t* start, const MsmPlan& p, void* parts);
// buckets (one Jacobian point each) -> the weighted sum; scratch: msm_tail_points(p) Jacobian points, the result is *result
size_t msm_tail_points(const MsmPlan& p);
template <class C> void msm_tail(hipStream_t st, int group, const void* buckets, const MsmPlan& p, void* scratch, void** result);
template <class C> size_t fb_table_bytes(int group);
template <class C> void fb_build(hipStream_t st, int group, void* table);
template <class C> void fb_scale(hipStream_t st, int group, const void* table, const uint8_t* scalars, size_t n, uint8_t* out);
template <class C> void scale_g1_inplace(hipStream_t st, Aff<F1<C>>* pts, const uint8_t* w16, size_t n);

// ---- k_miller_bn.hip / k_miller_bls.hip   (the legacy library only)
template <class C>
void miller_ab64(hipStream_t st, unsigned nblocks, const Aff<F1<C>>* g1s, const uint8_t* g2s, size_t n, long long sig_at,
                 const LineCoeffs<C>* gen_lines, Fp2<C>* out, uint32_t* flags, uint32_t* qp);
template <class C> constexpr size_t miller_qp_bytes(size_t nblocks) { return nblocks * 64 * 6 * C::L * 4; }    // parked Q, P of every producer lane

// ---- k_millerx_{bn,bls}.hip (NP = 60), k_millerx64_{bn,bls}.hip (NP = 64)
template <class C, int NP>
void miller_x(hipStream_t st, unsigned nblocks, const Aff<F1<C>>* g1s, const uint8_t* g2s, size_t n, Fp2<C>* out, uint32_t* flags, uint32_t* park, int rot_mode);
template <class C, int NP> size_t miller_x_park_bytes(size_t nblocks);

// ---- k_batchagg.hip: hash points and keys of a batch of instances to their padded positions (one instance per run of whole six-pairing groups)
template <class C>
void batch_scatter(hipStream_t st, const Aff<F1<C>>* g1s, const uint8_t* keys, const uint64_t* inst_off, const uint64_t* pad_off, size_t n_inst, size_t n_pad,
                   Aff<F1<C>>* g1_out, uint8_t* key_out);

// ---- k_millersets.hip: the Miller loop of n two-pairing sets (bgls_verify_multi_sets), one accumulator per set, sets_per_block sets per block.
// Set b: (g1s[b], key sum g2s[b]) and, on alt-bn128, (sigs[b], g2) on the generator lines -- GT bytes (no final exponentiation) to
// out_bytes + b GTB; on BLS12-381 the hash pair alone, six w-basis Fp2 to out_w + 6 b (the epilogue's rest).  park: miller_sets_park_bytes.
template <class C>
void miller_sets(hipStream_t st, unsigned nblocks, const Aff<F1<C>>* g1s, const uint8_t* g2s, const Aff<F1<C>>* sigs, const LineCoeffs<C>* gen_lines, size_t n,
                 Fp2<C>* out_w, uint8_t* out_bytes, uint32_t* flags, uint32_t* park);
template <class C> size_t miller_sets_park_bytes(size_t nblocks);
template <class C> size_t miller_sets_per_block();

// ---- k_bbsigs.hip: batched Boneh-Boyen verification (bgls_bb_verify_batch).  bb_keys: Q_b = m_b g2 + U_b + r_b V_b as wire bytes to
// q_out + b G2B for b < n (keys: n x (U || V) wire bytes, rs / ms: n x 32-byte big-endian scalars, fb_g2: the fixed-base table of g2), and
// the reference pair (g1, g2) at index n: g1s[n], q_out + n G2B; nosig (nullable): n + 1 G1 points at infinity.  ref_pair = false (the
// combined check): index n is not written, g1s is not read.  bb_w_bytes: n w-basis Miller values (six Fp2 each) to GT bytes.
// bb_verdicts: verdicts[b] = (gt[b] == gt[n]) for b < n.
template <class C>
void bb_keys(hipStream_t st, const uint8_t* keys, const uint8_t* rs, const uint8_t* ms, const void* fb_g2, size_t n, uint8_t* q_out, Aff<F1<C>>* g1s,
             Aff<F1<C>>* nosig, uint32_t* flags, bool ref_pair = true);
template <class C> void bb_w_bytes(hipStream_t st, const Fp2<C>* w, size_t n, uint8_t* out);
template <class C> void bb_verdicts(hipStream_t st, const uint8_t* gt, size_t n, uint32_t* verdicts);

// ---- k_pairbatch.hip: batched pairings and final exponentiations (bgls_pair_batch, bgls_final_exp_batch).  g1_inf_fill: n G1 points at
// infinity.  is_one_bytes: out[b] = (words[b] != 0) for b < n.
template <class C> void g1_inf_fill(hipStream_t st, Aff<F1<C>>* out, size_t n);
void is_one_bytes(hipStream_t st, const uint32_t* words, size_t n, uint8_t* out);

// ---- k_bbrlc.hip: the coefficients of the combined Boneh-Boyen check (bgls_bb_verify_batch_combined; body: bb_rlc.hpp).  bb_rlc_odd: the
// lowest bit of each of the n 16-byte coefficients set in place.  bb_rlc_sums: out + 32 g <- the sum of the coefficients group_off[g] ..
// group_off[g + 1] (device offsets) as a 32-byte big-endian magnitude, one wave per group; r16 is 16-byte aligned.
void bb_rlc_odd(hipStream_t st, uint8_t* r16, size_t n);
void bb_rlc_sums(hipStream_t st, const uint8_t* r16, const uint64_t* group_off, size_t n_groups, uint8_t* out);

// ---- k_haesets.hip: batched hashed aggregation exponents and weighted key sums (bgls_verify_multi_hae_sets).  hae_root_seg: the BLAKE2Xb
// root of every set with 1 .. host_min keys to roots + 8 b (keys: wire bytes of g2b each, key_off: n_sets + 1 device offsets), and the
// n_host host-made roots (records of nine words: set index, root) to their places.  hae_expand_seg: nodes = n_nodes pairs (set, node
// index), the exponents of set b to t + 16 key_off[b].  hae_wsum_main: P (a power of two) Jacobian partials of sum t_i pk_i per set to
// out + b P, bad keys set FLAG_ENC.
void hae_root_seg(hipStream_t st, const uint8_t* keys, const uint64_t* key_off, size_t n_sets, unsigned g2b, size_t host_min, const uint64_t* host,
                  size_t n_host, uint64_t* roots);
void hae_expand_seg(hipStream_t st, const uint64_t* roots, const uint32_t* nodes, size_t n_nodes, const uint64_t* key_off, uint8_t* t);
template <class C>
void hae_wsum_main(hipStream_t st, const uint8_t* keys, const uint64_t* key_off, const uint8_t* t, size_t n_sets, unsigned P, void* out, uint32_t* flags);

// ---- k_ams.hip: the hash inputs of a batch of accountable-subgroup multisignature checks (bgls_ams_verify_batch).  Input b < n is
// 0x00 || message b of mv, input n + s is 0x01 || apks[item of s] (g2b wire bytes) || decimal(signers[s]); signer_off: n + 1 device offsets
// from 0 (total = signer_off[n]), hoff: the n + total + 1 offsets of the inputs in blob (a prefix of their exact lengths).  An item without
// signers gets inst_flags[b] set.
void ams_msgs(hipStream_t st, const uint8_t* apks, const uint32_t* signers, const uint64_t* signer_off, size_t n, size_t total, MsgView mv, unsigned g2b,
              const uint64_t* hoff, uint8_t* blob, uint32_t* inst_flags);

// ---- k_keymsgs.hip: hash inputs made of the keys themselves, n of them (curve: BGLS_CURVE_*; keys: n G2 wire rows).  mode BGLS_KEYED_PREFIX:
// input i = key row i || message i of mv at out_off(i) = (start of message i - start of message 0) + i G2B of blob, nothing written past
// cap bytes; out_off (device, n + 1 words) is written when mv is in the offset form and may be NULL when it is the fixed-stride one (the
// blob then has the stride G2B + mv.len).  mode BGLS_KEYED_POP: input i = the compressed key i at stride G2B / 2, mv / cap / out_off
// unused, a key that does not compress sets FLAG_ENC in flags.
void key_msgs(hipStream_t st, int curve, int mode, const uint8_t* keys, size_t n, MsgView mv, uint8_t* blob, size_t cap, uint64_t* out_off, uint32_t* flags);

// ---- k_millerams.hip: the Miller loop of n accountable-subgroup multisignature checks, one accumulator per item, ams_per_block items per
// block.  Item b: (g1a[b], q2a[b]) and (g1b[b], q2b[b]) walked (keys as wire bytes) and, on alt-bn128, (sigs[b], g2) on the generator lines
// -- GT bytes (no final exponentiation) to out_bytes + b GTB; on BLS12-381 the two walked pairs alone, six w-basis Fp2 to out_w + 6 b (the
// epilogue's rest).  park: miller_ams_park_bytes.
template <class C>
void miller_ams(hipStream_t st, unsigned nblocks, const Aff<F1<C>>* g1a, const uint8_t* q2a, const Aff<F1<C>>* g1b, const uint8_t* q2b, const Aff<F1<C>>* sigs,
                const LineCoeffs<C>* gen_lines, size_t n, Fp2<C>* out_w, uint8_t* out_bytes, uint32_t* flags, uint32_t* park);
template <class C> size_t miller_ams_park_bytes(size_t nblocks);
template <class C> size_t miller_ams_per_block();

// prepared key sets (prepared.hpp): bytes per key of the line table, per pairing of the point table, per key of k_prepare's scratch
struct PrepSizes { size_t line_bytes_per_key, point_bytes, tmp_bytes_per_key; };
template <class C> PrepSizes prep_sizes();
template <class C>
void prepare_keys(hipStream_t st, const void* keys_mont, size_t n, size_t n_pad, size_t i0, size_t count, uint32_t* table, uint8_t* kinf,
                  uint32_t* tmp, uint32_t* flags);
template <class C> void prep_points(hipStream_t st, const Aff<F1<C>>* g1s, const uint8_t* kinf, size_t n, size_t n_pad, uint32_t* ptab);
template <class C> void fold_prep(hipStream_t st, const uint32_t* table, const uint32_t* ptab, size_t n_pad, int ng, Fp2<C>* out);

// ---- k_tail_bn.hip / k_tail_bls.hip
template <class C> void gen_lines(hipStream_t st, LineCoeffs<C>* table, int* nsteps);
template <class C> void reduce_coop(hipStream_t st, const Fp2<C>* in, size_t count, int R, Fp2<C>* out);
template <class C> void reduce_coop_seg(hipStream_t st, const Fp2<C>* in, const uint32_t* seg, size_t nout, int R, Fp2<C>* out);
template <class C> void w_to_bytes(hipStream_t st, const Fp2<C>* in, uint8_t* out);
template <class C> void final36(hipStream_t st, const uint8_t* partials, size_t count, int do_final_exp, uint8_t* gt_out, uint32_t* verdict, uint32_t* flags);
template <class C> void finalx(hipStream_t st, const uint8_t* partials, size_t count, int do_final_exp, uint8_t* gt_out, uint32_t* verdict, uint32_t* flags);
template <class C>
void miller_lat(hipStream_t st, const Aff<F1<C>>* g1s, const uint8_t* g2s, size_t n, long long sig_at, const LineCoeffs<C>* gen_lines, Fp2<C>* out,
                uint32_t* flags);
template <class C>
void miller_latx(hipStream_t st, const Aff<F1<C>>* g1s, const uint8_t* g2s, size_t n, long long sig_at, const LineCoeffs<C>* gen_lines, Fp2<C>* out,
                uint32_t* flags);
template <class C> void gt_pow(hipStream_t st, const uint8_t* gt_in, const uint8_t* k_be32, int negate, uint8_t* gt_out, uint32_t* flags);
template <class C> void cofactor_epilogue(hipStream_t st, const Fp2<C>* rest, const Aff<F1<C>>* sig, const LineCoeffs<C>* gen_lines, uint8_t* out);
// power = false: rest is not raised to the cofactor (its pairs held G1 points, not uncleared hash points); the signature pair is folded in all the same
template <class C> void cofactor_epiloguex(hipStream_t st, const Fp2<C>* rest, const Aff<F1<C>>* sig, const LineCoeffs<C>* gen_lines, Fp2<C>* tmp, uint8_t* out, uint32_t* flags,
                                           bool power = true);

}  // namespace kl
}  // namespace bgls
