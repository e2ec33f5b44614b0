// The per-set work of the combined multi-signature check (bgls_verify_multi_sets_combined), one set per lane:
//   k_rlc_pair   hs[b] <- r_b H_b in place (resident affine Montgomery points, as hash_to_g1 leaves them: uncleared on BLS12-381),
//                out[b] <- r_b sigma_b as wire bytes, where the segmented G1 sum reads them.  sigma_b arrives as wire bytes and is parsed
//                and checked on the curve here (FLAG_ENC, as k_scale_g1x does); r_b is bytes [16 b, 16 b + 16) of the XOF output, read
//                big-endian with the lowest bit set (rlc_scalar).
// The body is rlc_pair.hpp: one walk over the digits of r_b for both points, one inversion for both results.
#include "dev_common.hpp"
#include "rlc_pair.hpp"
#include "launch_tail.hpp"

using namespace bgls;

template <class C>
__global__ void __launch_bounds__(64) k_rlc_pair(Aff<F1<C>>* hs, const uint8_t* sigs, const uint8_t* r16, size_t n, uint8_t* out, uint32_t* flags) {
  typedef F1<C> F;
  constexpr int PT = 2 * C::FP_BYTES;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  Aff<F> p[2], q[2];
  p[0] = hs[i];
  bool ok = g1_from_bytes<C>(p[1], sigs + i * PT);
  ok = ok && aff_on_curve<F>(p[1]);
  if (!ok) atomicOr(flags, FLAG_ENC);
  u32 k[4];
  rlc_scalar(r16 + i * 16, k);
  rlc_pair<C>(p, k, q);
  hs[i] = q[0];
  g1_to_bytes<C>(out + i * PT, q[1]);
}

namespace bgls {
namespace kl {

template <class C>
void rlc_pair(hipStream_t st, Aff<F1<C>>* hs, const uint8_t* sigs, const uint8_t* r16, size_t n, uint8_t* out, uint32_t* flags) {
  if (n) k_rlc_pair<C><<<nblk(n, 64), 64, 0, st>>>(hs, sigs, r16, n, out, flags);
}
template void rlc_pair<BN254>(hipStream_t, Aff<F1<BN254>>*, const uint8_t*, const uint8_t*, size_t, uint8_t*, uint32_t*);
template void rlc_pair<BLS381>(hipStream_t, Aff<F1<BLS381>>*, const uint8_t*, const uint8_t*, size_t, uint8_t*, uint32_t*);

}  // namespace kl
}  // namespace bgls
