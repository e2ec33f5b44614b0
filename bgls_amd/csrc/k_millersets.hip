// k_miller_sets: the Miller loop of a batch of independent two-pairing sets (bgls_verify_multi_sets: n_sets verifyMultiSignature
// calls, bgls/bgls.go:89-92), ONE Fp12 accumulator per set.  It is miller_group.hpp's block (one accumulator per six-lane group, walks
// on lane pairs; the layout, the barrier pattern and the stand-ins are described there) with ONE producer wave.
//
// Block = 4 waves, 30 sets, 168 registers per lane (three waves per SIMD, three blocks per CU):
//   one PRODUCER wave   30 sets, one per LANE PAIR: walks (H(m_b), apk_b) from the key sum; on alt-bn128 it also scales the
//                       generator's pre-computed line of the step (Engine::gen_lines) by -sigma_b
//   three CONSUMER waves 10 groups x 6 lanes each; group = set:  f <- f^2 l_hash [l_gen]
//
// Why this shape ("Batched multi-signature verification").  In units of NL^2 multiplier instructions per line step
// (miller_x.hpp's header): a walked pairing costs its lane pair 2 x 27 (doubling), the fold of one line 66 over the six lanes of a
// group, the squaring 84.  k_miller_x60 shares one squaring among six walked pairings (per pairing 54 + 66 + 14 = 134) and one
// consumer wave serves two producer waves.  Here every set has exactly one walk and one squaring: 54 + 66 + 84 = 204 per
// BLS12-381 set, 54 + 2 x 66 + 84 + ~4 (the generator line's two scalings) = 274 per alt-bn128 set -- per LANE: producer 27,
// consumer 25 / 36.  Six consumer lanes per producer lane pair balance that; one producer wave and three consumer waves are the
// block that keeps all four SIMDs of a CU busy with one block.  The padded path (one set per six-pairing group of k_miller_x60)
// pays 6 x 134 = 804 per set.
//
// Keys / hash points at infinity are an empty set: the constant line 1 for the pair.
#include "miller_group.hpp"
#include "launch.hpp"

namespace bgls {

template <class X, int NLN>
using MSets = MG<X, 1, NLN == 2>;                          // one walk; alt-bn128 (NLN = 2) folds the generator's line as well

// C: the curve (32-bit Montgomery types of the inputs and outputs), X: the kernel's number form (MxForm).  NLN = 2: the generator
// line scaled by sigs[b] is folded as well and the kernel writes GT bytes (no final exponentiation) to out_bytes + b GTB;
// NLN = 1: the hash pair alone, six w-basis Fp2 per set to out_w (the epilogue's rest).
template <class C, class X, int NLN>
__global__ void __launch_bounds__(256, 3) k_miller_sets(const Aff<F1<X>>* g1s, const uint8_t* g2s, const Aff<F1<X>>* sigs, const LineCoeffs<X>* gen_lines,
                                                        size_t n, Fp2<X>* out_w, uint8_t* out_bytes, uint32_t* flags, u32* park) {
  typedef MSets<X, NLN> K;
  const int w = threadIdx.x >> 6;
  if (w == 0) mg_producer<C, X, K>(0, g1s, g2s, sigs, gen_lines, n, flags, park);
  else mg_consumer<C, X, K>(w - 1, n, out_w, out_bytes);
}

namespace kl {
template <class C>
constexpr int sets_lines() { return C::CURVE_ID == 0 ? 2 : 1; }
template <class C>
size_t miller_sets_park_bytes(size_t nblocks) { return MSets<typename MxForm<C>::type, sets_lines<C>()>::park_bytes(nblocks); }
template <class C>
size_t miller_sets_per_block() { return MSets<typename MxForm<C>::type, sets_lines<C>()>::ITEMS; }
template <class C>
void miller_sets(hipStream_t st, unsigned nblocks, const Aff<F1<C>>* g1s, const uint8_t* g2s, const Aff<F1<C>>* sigs, const LineCoeffs<C>* gen_lines, size_t n,
                 Fp2<C>* out_w, uint8_t* out_bytes, uint32_t* flags, uint32_t* park) {
  typedef typename MxForm<C>::type X;
  typedef MSets<X, sets_lines<C>()> K;
  k_miller_sets<C, X, sets_lines<C>()><<<nblocks, K::THREADS, K::BLOCK_BYTES, st>>>(
      reinterpret_cast<const Aff<F1<X>>*>(g1s), g2s, reinterpret_cast<const Aff<F1<X>>*>(sigs), reinterpret_cast<const LineCoeffs<X>*>(gen_lines), n,
      reinterpret_cast<Fp2<X>*>(out_w), out_bytes, flags, park);
}
#define BGLS_SETS_INST(C)                                                                                                                     \
  template size_t miller_sets_park_bytes<C>(size_t);                                                                                          \
  template size_t miller_sets_per_block<C>();                                                                                                 \
  template void miller_sets<C>(hipStream_t, unsigned, const Aff<F1<C>>*, const uint8_t*, const Aff<F1<C>>*, const LineCoeffs<C>*, size_t, Fp2<C>*, \
                               uint8_t*, uint32_t*, uint32_t*);
BGLS_SETS_INST(BN254)
BGLS_SETS_INST(BLS381)
}  // namespace kl
}  // namespace bgls
