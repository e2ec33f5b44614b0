// Miller-loop kernels instantiated for one curve (BGLS_MILLER_CURVE); templates in miller_kernels.hpp.
#include "miller_kernels.hpp"
#include "prepared.hpp"
#include "launch.hpp"

namespace bgls {
namespace kl {

#ifdef BGLS_LEGACY_KERNELS           // k_miller_ab64, the 32-bit fused Miller kernel behind BGLS_MILLER_SHAPE=5: `make LEGACY=1` only
template <class C>
void miller_ab64(hipStream_t st, unsigned nblocks, const Aff<F1<C>>* g1s, const uint8_t* g2s, size_t n, long long sig_at,
                 const LineCoeffs<C>* gen_lines, Fp2<C>* out, uint32_t* flags, uint32_t* qp) {
  const size_t lds = Coop64<C>::BLOCK_BYTES;
  k_miller_ab64<C><<<nblocks, 128, lds, st>>>(g1s, g2s, n, sig_at, gen_lines, out, flags, 0u, qp);
}
template void miller_ab64<BGLS_MILLER_CURVE>(hipStream_t, unsigned, const Aff<F1<BGLS_MILLER_CURVE>>*, const uint8_t*, size_t, long long,
                                             const LineCoeffs<BGLS_MILLER_CURVE>*, Fp2<BGLS_MILLER_CURVE>*, uint32_t*, uint32_t*);
#endif

// ---- prepared key sets (prepared.hpp): the fold on the carry-free limbs of the Miller kernel (nine of 29 bits / fourteen of 28)
template <class C>
PrepSizes prep_sizes() {
  typedef Prep<C> T;
  return {(size_t)T::NSTEPS * T::LINE_DW * 4, (size_t)T::P_DW * 4, (size_t)T::NSTEPS * T::TMP_DW * 4};
}
template <class C>
void prepare_keys(hipStream_t st, const void* keys_mont, size_t n, size_t n_pad, size_t i0, size_t count, uint32_t* table, uint8_t* kinf,
                  uint32_t* tmp, uint32_t* flags) {
  k_prepare<C><<<nblk(count, 64), 64, 0, st>>>((const Aff<F2<C>>*)keys_mont, n, n_pad, i0, count, table, kinf, tmp, flags);
}
template <class C>
void prep_points(hipStream_t st, const Aff<F1<C>>* g1s, const uint8_t* kinf, size_t n, size_t n_pad, uint32_t* ptab) {
  k_prep_points<C><<<nblk(n_pad, 256), 256, 0, st>>>(g1s, kinf, n, n_pad, ptab);
}
template <class C>
void fold_prep(hipStream_t st, const uint32_t* table, const uint32_t* ptab, size_t n_pad, int ng, Fp2<C>* out) {
  const unsigned waves = (unsigned)(n_pad / ((size_t)ng * 10));
  k_fold_prep<C><<<waves, 64, PrepX<typename MxForm<C>::type>::WAVE_BYTES, st>>>(table, ptab, n_pad, ng, out);
}
template PrepSizes prep_sizes<BGLS_MILLER_CURVE>();
template void prepare_keys<BGLS_MILLER_CURVE>(hipStream_t, const void*, size_t, size_t, size_t, size_t, uint32_t*, uint8_t*, uint32_t*, uint32_t*);
template void prep_points<BGLS_MILLER_CURVE>(hipStream_t, const Aff<F1<BGLS_MILLER_CURVE>>*, const uint8_t*, size_t, size_t, uint32_t*);
template void fold_prep<BGLS_MILLER_CURVE>(hipStream_t, const uint32_t*, const uint32_t*, size_t, int, Fp2<BGLS_MILLER_CURVE>*);

}  // namespace kl
}  // namespace bgls
