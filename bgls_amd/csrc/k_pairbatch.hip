// Batched pairings and final exponentiations with one GT element per item (bgls_pair_batch, bgls_final_exp_batch), the two steps that are
// not shared with the other batches:
//   k_g1_inf_fill   n G1 points at infinity: the signature slots of k_miller_sets on alt-bn128, where a pair has no generator pair beside it
//   k_is_one_bytes  the per-item words of k_finalx_batch (1: the GT element is one) as the n bytes the caller reads
#include "dev_common.hpp"
#include "launch.hpp"

namespace bgls {

template <class C>
__global__ void __launch_bounds__(64) k_g1_inf_fill(Aff<F1<C>>* out, size_t n) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = Aff<F1<C>>{fp_zero<C>(), fp_zero<C>(), true};
}

__global__ void __launch_bounds__(64) k_is_one_bytes(const uint32_t* words, size_t n, uint8_t* out) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = words[i] ? 1 : 0;
}

namespace kl {
template <class C>
void g1_inf_fill(hipStream_t st, Aff<F1<C>>* out, size_t n) {
  if (n) k_g1_inf_fill<C><<<nblk(n, 64), 64, 0, st>>>(out, n);
}
void is_one_bytes(hipStream_t st, const uint32_t* words, size_t n, uint8_t* out) {
  if (n) k_is_one_bytes<<<nblk(n, 64), 64, 0, st>>>(words, n, out);
}
template void g1_inf_fill<BN254>(hipStream_t, Aff<F1<BN254>>*, size_t);
template void g1_inf_fill<BLS381>(hipStream_t, Aff<F1<BLS381>>*, size_t);
}  // namespace kl
}  // namespace bgls
