// Launchers of k_sumtree.hip and k_g1x.hip (declared apart from launch.hpp, which every unit includes: only engine.hip needs these).
#pragma once
#include "dev_common.hpp"

namespace bgls {
namespace kl {

// The tree above a key sum's main pass in ONE launch (k_sumtree.hip): cnt Jacobian partial sums (G2) -> their sum, as affine
// wire bytes (d_bytes != nullptr) and / or as one Jacobian record (d_jac != nullptr).  store: sum_tree_store_bytes(cnt) of scratch,
// tickets: cnt words, zero on entry and zero again on exit.
template <class C> void sum_tree(hipStream_t st, const void* in, size_t cnt, void* store, uint32_t* tickets, uint8_t* d_bytes, void* d_jac);
template <class C> size_t sum_tree_store_bytes(size_t cnt);

// ---- k_finalx.hip: the final exponentiation with its three result words {verdict, this stage's flags, *flags_in} written side by side
// (res3: 12 bytes), so that ONE copy brings them to the host and no flag word has to be cleared beforehand
// one block per instance of a batch: partials + b GTB -> gt_out + b GTB (nullable), verdicts[b] = (result == 1 && inst_flags[b] == 0)
template <class C>
void finalx_batch(hipStream_t st, const uint8_t* partials, size_t n_inst, uint8_t* gt_out, uint32_t* verdicts, const uint32_t* inst_flags, uint32_t* flags);
// ---- k_finalxt.hip: the same n final exponentiations in the throughput form (finalxt.hpp: ten items per wave, no block barrier); same
// arguments and results as finalx_batch, byte for byte
template <class C>
void finalxt_batch(hipStream_t st, const uint8_t* partials, size_t n_inst, uint8_t* gt_out, uint32_t* verdicts, const uint32_t* inst_flags, uint32_t* flags);
template <class C> void finalx_res(hipStream_t st, const uint8_t* partials, size_t count, int do_final_exp, uint8_t* gt_out, uint32_t* res3, const uint32_t* flags_in);

// ---- k_g1x.hip: scalar multiplications on G1, one point per lane on the carry-free limbs (rx_jac1.hpp)
template <class C> void scale_aff_g1x(hipStream_t st, const Aff<F1<C>>* g1_pts, const uint8_t* scalars, size_t n, uint8_t* out);
template <class C> void scale_g1x(hipStream_t st, const uint8_t* pts, const uint8_t* scalars, const uint8_t* signs, size_t n, uint8_t* out, uint32_t* flags, int sbytes);

// ---- k_rlc.hip: the combined check's per-set pair, hs[b] <- r_b hs[b] in place and out[b] <- r_b sigs[b] as wire bytes (r16: n x 16 bytes)
template <class C> void rlc_pair(hipStream_t st, Aff<F1<C>>* hs, const uint8_t* sigs, const uint8_t* r16, size_t n, uint8_t* out, uint32_t* flags);

// ---- k_millerlatx.hip: the narrow passes of the reduce stage on the two-wave 36-lane product (finalx.hpp)
template <class C> void reduce_fx(hipStream_t st, const Fp2<C>* in, size_t count, int R, Fp2<C>* out);
// segmented form: out[G] = prod in[seg[2G] .. seg[2G] + seg[2G + 1]) for G < nout (an empty segment gives one)
template <class C> void reduce_fx_seg(hipStream_t st, const Fp2<C>* in, const uint32_t* seg, size_t nout, Fp2<C>* out);
// the epilogue of n_inst instances: rest[6 b ..] ^ h times the signature pair (sigs[b], g2), GT bytes to out + b GTB; tmp: 12 n_inst Fp2.
// power = false: rest[6 b ..] itself times the signature pair (the walked pairs held G1 points, not uncleared hash points)
template <class C>
void epiloguex_seg(hipStream_t st, size_t n_inst, const Fp2<C>* rest, const Aff<F1<C>>* sigs, const LineCoeffs<C>* gen_lines, Fp2<C>* tmp, uint8_t* out,
                   uint32_t* flags, bool power = true);
// the verification epilogue's two chains as separate launches (1: the signature pair, 2: rest^h and the product of the two)
template <class C> void cofactor_epiloguex_part(hipStream_t st, int part, const Fp2<C>* rest, const Aff<F1<C>>* sig, const LineCoeffs<C>* gen_lines, Fp2<C>* tmp, uint8_t* out);

}  // namespace kl
}  // namespace bgls
