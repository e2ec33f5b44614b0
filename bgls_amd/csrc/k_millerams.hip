// k_miller_ams: the Miller loop of a batch of accountable-subgroup multisignature checks (bgls_ams_verify_batch: n AmsVerifySignature
// calls, bgls/blsAsmSigs.go:48-59), ONE Fp12 accumulator per item over BOTH walked pairs (H0(m_b), aggKey_b) and (aggMsg_b, apk_b) and,
// on alt-bn128, the generator's line scaled by -sigma_b.  It is miller_group.hpp's block (one accumulator per six-lane group, walks on
// lane pairs; the layout, the barrier pattern and the stand-ins are described there) with TWO producer waves.
//
// Block = 5 waves, 30 items, 168 registers per lane (three waves per SIMD, two blocks per CU):
//   PRODUCER wave 0      30 items, one per LANE PAIR: walks (H0(m_b), aggKey_b); on alt-bn128 it also scales the generator's
//                        pre-computed line of the step (Engine::gen_lines) by -sigma_b
//   PRODUCER wave 1      the same 30 items: walks (aggMsg_b, apk_b)
//   three CONSUMER waves 10 groups x 6 lanes each; group = item:  f <- f^2 l_key l_apk [l_gen]
//
// Why this shape ("Batched AMS verification").  In units of NL^2 multiplier instructions per line step (miller_x.hpp's
// header): a walked pairing costs its lane pair 2 x 27, the fold of one line 66 over a group's six lanes, the squaring 84.  One
// accumulator for both walks pays the squaring once: 2 x 54 + 2 x 66 + 84 = 324 per BLS12-381 item (two k_miller_sets sets and a
// product: 2 x 204 = 408), + 66 + ~4 = 394 on alt-bn128 (478).  Per LANE: producer 27, consumer 36 / 47.
//
// A key, a hash point or a hash sum at infinity gives the constant line 1 for ITS pair only.
#include "miller_group.hpp"
#include "launch.hpp"

namespace bgls {

template <class X, int NLN>
using MAms = MG<X, 2, NLN == 3>;                           // two walks; alt-bn128 (NLN = 3) folds the generator's line as well

// C: the curve (32-bit Montgomery types of the inputs and outputs), X: the kernel's number form (MxForm).  Item b: g1a[b] = H0(m_b)
// against the key q2a[b] = aggKey_b, g1b[b] = aggMsg_b against q2b[b] = apk_b (keys as wire bytes, checked in the producer).  NLN = 3:
// the generator line scaled by sigs[b] = -sigma_b is folded as well and the kernel writes GT bytes (no final exponentiation) to
// out_bytes + b GTB; NLN = 2: the two walked pairs alone, six w-basis Fp2 per item to out_w (the epilogue's rest).
template <class C, class X, int NLN>
// three waves per SIMD (168 registers, k_miller_sets' budget): two blocks fit a CU, at the price of 57 / 84 spilled registers and 364 / 244
// bytes of scratch per lane inside the loop (k_miller_sets: 58 / 82 and 368 / 240).  Left to itself the compiler takes 230 / 243 registers
// without spilling any, and then one 5-wave block is all a CU holds.  Neither form has been timed.
__global__ void __launch_bounds__(320) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_miller_ams(const Aff<F1<X>>* g1a, const uint8_t* q2a, const Aff<F1<X>>* g1b, const uint8_t* q2b,
                                                       const Aff<F1<X>>* sigs, const LineCoeffs<X>* gen_lines, size_t n, Fp2<X>* out_w, uint8_t* out_bytes,
                                                       uint32_t* flags, u32* park) {
  typedef MAms<X, NLN> K;
  const int w = threadIdx.x >> 6;
  if (w < 2) {
    const bool second = w == 1;                              // wave-uniform: the (aggMsg, apk) walk
    mg_producer<C, X, K>(w, second ? g1b : g1a, second ? q2b : q2a, sigs, gen_lines, n, flags, park);
  } else {
    mg_consumer<C, X, K>(w - 2, n, out_w, out_bytes);
  }
}

namespace kl {
template <class C>
constexpr int ams_lines() { return C::CURVE_ID == 0 ? 3 : 2; }
template <class C>
size_t miller_ams_park_bytes(size_t nblocks) { return MAms<typename MxForm<C>::type, ams_lines<C>()>::park_bytes(nblocks); }
template <class C>
size_t miller_ams_per_block() { return MAms<typename MxForm<C>::type, ams_lines<C>()>::ITEMS; }
template <class C>
void miller_ams(hipStream_t st, unsigned nblocks, const Aff<F1<C>>* g1a, const uint8_t* q2a, const Aff<F1<C>>* g1b, const uint8_t* q2b, const Aff<F1<C>>* sigs,
                const LineCoeffs<C>* gen_lines, size_t n, Fp2<C>* out_w, uint8_t* out_bytes, uint32_t* flags, uint32_t* park) {
  typedef typename MxForm<C>::type X;
  typedef MAms<X, ams_lines<C>()> K;
  k_miller_ams<C, X, ams_lines<C>()><<<nblocks, K::THREADS, K::BLOCK_BYTES, st>>>(
      reinterpret_cast<const Aff<F1<X>>*>(g1a), q2a, reinterpret_cast<const Aff<F1<X>>*>(g1b), q2b, reinterpret_cast<const Aff<F1<X>>*>(sigs),
      reinterpret_cast<const LineCoeffs<X>*>(gen_lines), n, reinterpret_cast<Fp2<X>*>(out_w), out_bytes, flags, park);
}
#define BGLS_AMS_INST(C)                                                                                                                        \
  template size_t miller_ams_park_bytes<C>(size_t);                                                                                             \
  template size_t miller_ams_per_block<C>();                                                                                                    \
  template void miller_ams<C>(hipStream_t, unsigned, const Aff<F1<C>>*, const uint8_t*, const Aff<F1<C>>*, const uint8_t*, const Aff<F1<C>>*,   \
                              const LineCoeffs<C>*, size_t, Fp2<C>*, uint8_t*, uint32_t*, uint32_t*);
BGLS_AMS_INST(BN254)
BGLS_AMS_INST(BLS381)
}  // namespace kl
}  // namespace bgls
