// Batched Boneh-Boyen verification (bgls_bb_verify_batch: n bbsigs.Verify calls, bbsigs/bbsigs.go:68-73), the stages that are not
// shared with the other verifications:
//   k_bb_keys      Q_b = m_b g2 + U_b + r_b V_b, one item per lane on the carry-free limbs (rx_g2mul.hpp): r_b V_b by the windowed
//                  chain, U_b and m_b g2 by mixed additions -- the latter from the resident table of window multiples of g2
//                  (k_fb_build: one addition per non-zero byte of m_b) -- then one inversion to affine wire bytes, the form
//                  k_miller_sets reads.  Item n is the reference pair (g1, g2), whose GT element is GetGT().
//   k_bb_w_bytes   BLS12-381: the Miller value of (sigma_b, Q_b) that k_miller_sets leaves in w-basis (its epilogue's rest, NOT raised
//                  to the cofactor: sigma is a G1 point already) to GT bytes for the batched final exponentiation
//   k_bb_verdicts  verdicts[b] = (gt[b] == gt[n]), byte for byte
// Scalars are the given 256-bit magnitudes, unreduced.  An off-curve or non-canonical U or V sets FLAG_ENC (the whole call fails).
#include "dev_common.hpp"
#include "rx_g2mul.hpp"
#include "points_inl.hpp"
#include "launch.hpp"

namespace bgls {

// layout of k_fb_build's table (k_msm.inc): entry j * 255 + d - 1 = d 2^(8 j) g, 32 byte positions
constexpr int BB_FB_ROW = 255, BB_FB_WINDOWS = 32;

// 32-byte big-endian magnitude -> eight little-endian words and its bit length
__device__ __forceinline__ int bb_scalar_words(const uint8_t* s, u32 (&k)[8]) {
  int top = -1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint8_t* q = s + 4 * (7 - j);
    k[j] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
  }
  for (int j = 7; j >= 0 && top < 0; --j)
    if (k[j]) top = j * 32 + (31 - __clz(k[j]));
  return top + 1;
}

template <class C>
__global__ void __launch_bounds__(64) k_bb_keys(const uint8_t* keys, const uint8_t* rs, const uint8_t* ms, const Aff<F2<C>>* fb, size_t n, uint8_t* q_out,
                                                Aff<F1<C>>* g1s, Aff<F1<C>>* nosig, uint32_t* flags, bool ref_pair) {
  typedef F2<C> F;
  constexpr size_t G2B = 4 * C::FP_BYTES;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i > n || (i == n && !ref_pair)) return;
  if (nosig) nosig[i] = Aff<F1<C>>{fp_zero<C>(), fp_zero<C>(), true};       // alt-bn128: no generator pair in k_miller_sets
  if (i == n) {
    g1s[n] = Aff<F1<C>>{fp_load<C>(C::G1X), fp_load<C>(C::G1Y), false};
    aff_to_bytes<F>(q_out + n * G2B, Aff<F>{f2_load<C>(C::G2), f2_load<C>(C::G2 + 2 * C::L), false});
    return;
  }
  AffX<C> U, V;
  bool ok = affx_from_bytes<C>(U, keys + i * 2 * G2B);
  ok = affx_from_bytes<C>(V, keys + i * 2 * G2B + G2B) && ok;
  ok = ok && affx_on_curve<C>(U) && affx_on_curve<C>(V);
  if (!ok) {                                                                 // the call fails; the Miller stage sees infinity
    atomicOr(flags, FLAG_ENC);
    aff_to_bytes<F>(q_out + i * G2B, Aff<F>{f2_zero<C>(), f2_zero<C>(), true});
    return;
  }
  u32 k[8];
  const int nbits = bb_scalar_words(rs + i * 32, k);
  JacX<C> acc = jacx_mul_w4<C>(V, k, nbits);
  acc = jacx_madd<C>(acc, U);
#pragma unroll 1
  for (int j = 0; j < BB_FB_WINDOWS; ++j) {
    const u32 d = ms[i * 32 + 31 - j];
    if (d) acc = jacx_madd<C>(acc, affx_from_mont<C>(fb[j * BB_FB_ROW + d - 1]));
  }
  aff_to_bytes<F>(q_out + i * G2B, jac_to_aff<F>(jacx_to_mont<C>(acc)));
}

// six threads per item: coefficient j of the w-basis value to its GT byte position (k_w_to_bytes' layout, imaginary part first)
template <class C>
__global__ void __launch_bounds__(192) k_bb_w_bytes(const Fp2<C>* w, size_t n, uint8_t* out) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= n * 6) return;
  const size_t b = t / 6;
  const int j = (int)(t % 6);
  const int order_pos[6] = {5, 2, 4, 1, 3, 0};
  const Fp2<C> e = w[b * 6 + j];
  uint8_t* o = out + b * 12 * C::FP_BYTES + (size_t)(2 * order_pos[j]) * C::FP_BYTES;
  fp_to_be<C>(o, fp_from_mont<C>(e.c1));
  fp_to_be<C>(o + C::FP_BYTES, fp_from_mont<C>(e.c0));
}

template <class C>
__global__ void __launch_bounds__(64) k_bb_verdicts(const uint8_t* gt, size_t n, uint32_t* verdicts) {
  constexpr int GW = 12 * C::FP_BYTES / 4;
  const size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (b >= n) return;
  const uint32_t* x = reinterpret_cast<const uint32_t*>(gt + b * GW * 4);
  const uint32_t* ref = reinterpret_cast<const uint32_t*>(gt + n * GW * 4);
  uint32_t diff = 0;
#pragma unroll 4
  for (int k = 0; k < GW; ++k) diff |= x[k] ^ ref[k];
  verdicts[b] = diff == 0 ? 1u : 0u;
}

namespace kl {
template <class C>
void bb_keys(hipStream_t st, const uint8_t* keys, const uint8_t* rs, const uint8_t* ms, const void* fb_g2, size_t n, uint8_t* q_out, Aff<F1<C>>* g1s,
             Aff<F1<C>>* nosig, uint32_t* flags, bool ref_pair) {
  k_bb_keys<C><<<nblk(n + 1, 64), 64, 0, st>>>(keys, rs, ms, (const Aff<F2<C>>*)fb_g2, n, q_out, g1s, nosig, flags, ref_pair);
}
template <class C>
void bb_w_bytes(hipStream_t st, const Fp2<C>* w, size_t n, uint8_t* out) {
  k_bb_w_bytes<C><<<nblk(n * 6, 192), 192, 0, st>>>(w, n, out);
}
template <class C>
void bb_verdicts(hipStream_t st, const uint8_t* gt, size_t n, uint32_t* verdicts) {
  if (n) k_bb_verdicts<C><<<nblk(n, 64), 64, 0, st>>>(gt, n, verdicts);
}
#define BGLS_BB_INST(C)                                                                                                                     \
  template void bb_keys<C>(hipStream_t, const uint8_t*, const uint8_t*, const uint8_t*, const void*, size_t, uint8_t*, Aff<F1<C>>*, Aff<F1<C>>*, \
                           uint32_t*, bool);                                                                                                \
  template void bb_w_bytes<C>(hipStream_t, const Fp2<C>*, size_t, uint8_t*);                                                                \
  template void bb_verdicts<C>(hipStream_t, const uint8_t*, size_t, uint32_t*);
BGLS_BB_INST(BN254)
BGLS_BB_INST(BLS381)
}  // namespace kl
}  // namespace bgls
