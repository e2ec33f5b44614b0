// k_finalxt_batch: n independent final exponentiations in the throughput form of finalxt.hpp -- one value per six-lane group, ten values
// per wave, one wave per block, the chain's temporaries in registers and no block barrier.  Same interface and results as
// k_finalx_batch (k_finalx.hip), byte for byte: item b reads partials + b GTB and writes gt_out + b GTB (gt_out may be nullptr) and
// verdicts[b] = (result == 1 and inst_flags[b] clear); a non-canonical coefficient is OR-ed into *flags as FLAG_ENC.  Own translation
// unit (both curves).
#include "dev_common.hpp"
#include "finalx.hpp"
#include "finalxt.hpp"
#include "launch.hpp"
#include "launch_tail.hpp"

namespace bgls {

// a group's region in dynamic LDS, as finalxt.hpp's routines see it
template <class C>
struct FxtLds {
  int base;                                                   // dwords
  __device__ __forceinline__ Sx<C, SX_T> ld(int off) const { return fx_ld<C>(base + off); }
  __device__ __forceinline__ void st(int off, const Sx<C, SX_T>& v) const { fx_st<C>(base + off, v); }
  __device__ __forceinline__ void sync() const { wave_sync(); }
};

template <class C>
__global__ void __launch_bounds__(64) k_finalxt_batch(const uint8_t* partials, size_t n, uint8_t* gt_out, uint32_t* verdicts, const uint32_t* inst_flags,
                                                     uint32_t* flags) {
  typedef FXT<C> E;
  const int lane = threadIdx.x;
  const int g = lane / 6, j = lane % 6;
  const size_t b = (size_t)blockIdx.x * E::GROUPS + g;
  const bool act = lane < 6 * E::GROUPS && b < n;            // global memory is touched by the lanes of real items only
  FxtLds<C> m{(lane < 6 * E::GROUPS ? g : 0) * E::GROUP_DW};
  const int order_pos[6] = {5, 2, 4, 1, 3, 0};
  bool bad = false;
  X2<C, SX_T> x = {sx_const<C>(C::RX_ONE), ux_to_sx<C>(ux_zero<C>())};
  if (act) {
    const uint8_t* p = partials + b * 12 * C::FP_BYTES + (size_t)(2 * order_pos[j]) * C::FP_BYTES;
    const Fp<C> im = fp_from_be<C>(p), re = fp_from_be<C>(p + C::FP_BYTES);
    bad = fp_geq_p<C>(im) || fp_geq_p<C>(re);
    x = X2<C, SX_T>{sx_from_plain<C>(re), sx_from_plain<C>(im)};
  }
  // every group publishes into its own region (an idle one exponentiates one); lanes 60..63 read along in group 0's and store nothing
  x = fxt_final_exp<C>(m, j, lane < 6 * E::GROUPS, x);
  const Fp2<C> v = {sx_to_mont<C>(x.c0), sx_to_mont<C>(x.c1)};
  const bool mine = j == 0 ? f2_eq<C>(v, f2_one<C>()) : f2_is_zero<C>(v);
  if (act && gt_out) {
    uint8_t* o = gt_out + b * 12 * C::FP_BYTES + (size_t)(2 * order_pos[j]) * C::FP_BYTES;
    fp_to_be<C>(o, fp_from_mont<C>(v.c1));
    fp_to_be<C>(o + C::FP_BYTES, fp_from_mont<C>(v.c0));
  }
  const unsigned long long ones = __ballot(mine);
  const unsigned long long bball = __ballot(bad);
  if (act && j == 0) verdicts[b] = (((ones >> (6 * g)) & 63ull) == 63ull && inst_flags[b] == 0u) ? 1u : 0u;
  if (lane == 0 && bball) atomicOr(flags, FLAG_ENC);
}

namespace kl {
template <class C>
void finalxt_batch(hipStream_t st, const uint8_t* partials, size_t n, uint8_t* gt_out, uint32_t* verdicts, const uint32_t* inst_flags, uint32_t* flags) {
  if (n) k_finalxt_batch<C><<<nblk(n, FXT<C>::GROUPS), 64, FXT<C>::WAVE_BYTES, st>>>(partials, n, gt_out, verdicts, inst_flags, flags);
}
template void finalxt_batch<BN254>(hipStream_t, const uint8_t*, size_t, uint8_t*, uint32_t*, const uint32_t*, uint32_t*);
template void finalxt_batch<BLS381>(hipStream_t, const uint8_t*, size_t, uint8_t*, uint32_t*, const uint32_t*, uint32_t*);
}  // namespace kl
}  // namespace bgls
