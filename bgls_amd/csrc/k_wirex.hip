// Compressed points over a batch on the carry-free limbs (wire_x.hpp): UnmarshalG1 / UnmarshalG2 of both curves -- parse, square root,
// sign rule, curve check, subgroup membership -- and, for a key set built from compressed keys (bgls_keys_upload_compressed), the resident
// Montgomery record of k_g2_parse from the same pass, so that a key is parsed and checked once.  One lane owns one point.
//
// Shape: one wave per block, no barrier (a lane only ever reads its own column of the LDS table).  The square-root powers keep their
// WX_TE = 4 window entries in dynamic LDS, column layout ((e * NL + i) * 64 + lane) words: conflict-free 4-byte accesses, 10 240 B per
// wave on alt-bn128 and 14 336 B on BLS12-381.  Registers, not LDS, set the occupancy: the G2 instantiations take the whole register file
// of a SIMD or most of it (390 / 512 registers as compiled, AGPRs included: ONE wave per SIMD, four per CU, 56 KB of the 160 KB of LDS at
// the most), the G1 ones 79 and 250 (six and two waves per SIMD).  No static LDS.  Every output byte of every lane below n is written on every path.
#include "dev_common.hpp"
#include "wire_x.hpp"
#include "launch.hpp"
#include "../../include/bgls_hip.h"

using namespace bgls;

// a lane's column of the wave's window table
template <class C>
struct WxTabLds {
  i32* col;
  __device__ __forceinline__ i32 ld(int e, int i) const { return col[(e * C::RX_NL + i) * 64]; }
  __device__ __forceinline__ void st(int e, int i, i32 v) { col[(e * C::RX_NL + i) * 64] = v; }
};

template <class C, int GROUP>
__global__ void __launch_bounds__(64) k_wirex(const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok, Aff<F2<C>>* mont, uint32_t* first_bad) {
  extern __shared__ i32 wx_lds[];
  const size_t i = blockIdx.x * (size_t)64 + threadIdx.x;
  if (i >= n) return;
  constexpr int FB = C::FP_BYTES, NC = GROUP == BGLS_G1 ? 2 : 4;
  WxTabLds<C> tab{wx_lds + threadIdx.x};
  Fp<C> pl[NC];
  bool good;
  if constexpr (GROUP == BGLS_G1) good = wx_g1_decode<C>(in + i * FB, tab, pl);
  else good = wx_g2_decode<C>(in + i * 2 * FB, tab, pl);
#pragma unroll
  for (int k = 0; k < NC; ++k)
    if (!good) pl[k] = fp_zero<C>();
  uint8_t* o = out + i * NC * FB;
  if constexpr (GROUP == BGLS_G1) {
    fp_to_be<C>(o, pl[0]);
    fp_to_be<C>(o + FB, pl[1]);
  } else {
    fp_to_be<C>(o, pl[1]);                                   // x_im || x_re || y_im || y_re
    fp_to_be<C>(o + FB, pl[0]);
    fp_to_be<C>(o + 2 * FB, pl[3]);
    fp_to_be<C>(o + 3 * FB, pl[2]);
    if (mont) {                                              // what g2_from_bytes makes of those bytes; the padding behind `inf`, which
      Aff<F2<C>> p;                                          // k_g2_parse leaves as it finds it, is zero here
      memset(&p, 0, sizeof(p));
      p.x = Fp2<C>{fp_to_mont<C>(pl[0]), fp_to_mont<C>(pl[1])};
      p.y = Fp2<C>{fp_to_mont<C>(pl[2]), fp_to_mont<C>(pl[3])};
      p.inf = fp_is_zero<C>(pl[0]) && fp_is_zero<C>(pl[1]) && fp_is_zero<C>(pl[2]) && fp_is_zero<C>(pl[3]);
      mont[i] = p;
    }
  }
  if (ok) ok[i] = good ? 1 : 0;
  if (!good && first_bad) atomicMin(first_bad, (uint32_t)i);
}

namespace bgls {
namespace kl {

template <class C>
void wirex_decode(hipStream_t st, int group, const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok, void* mont, uint32_t* first_bad) {
  if (n == 0) return;
  const size_t lds = (size_t)WX_TE * C::RX_NL * 64 * sizeof(i32);
  if (group == BGLS_G1) k_wirex<C, BGLS_G1><<<nblk(n, 64), 64, lds, st>>>(in, n, out, ok, nullptr, first_bad);
  else k_wirex<C, BGLS_G2><<<nblk(n, 64), 64, lds, st>>>(in, n, out, ok, (Aff<F2<C>>*)mont, first_bad);
}
template void wirex_decode<BN254>(hipStream_t, int, const uint8_t*, size_t, uint8_t*, uint8_t*, void*, uint32_t*);
template void wirex_decode<BLS381>(hipStream_t, int, const uint8_t*, size_t, uint8_t*, uint8_t*, void*, uint32_t*);

}  // namespace kl
}  // namespace bgls
