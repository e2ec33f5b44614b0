// The coefficient work of the combined Boneh-Boyen check (bgls_bb_verify_batch_combined) that is not a point operation:
//   k_bb_rlc_odd    the lowest bit of every coefficient of the XOF output set in place (bgls_rlc_coefficients: never zero), so that the
//                   launches that read the 16 bytes as they are (k_scale_g1_inplace) multiply by the defined rho_b
//   k_bb_rlc_sums   s_g = sum of rho_b over group g as a 32-byte big-endian magnitude, one wave per group: the lanes stride over the
//                   group's items with six-word carry chains of their own, a shuffle tree folds the 64 lane sums, lane 0 writes.  A group
//                   of 2^20 items is 2^14 additions per lane and six shuffle rounds, not 2^20 additions on one lane.  An empty group
//                   writes zero.
// The body is bb_rlc.hpp, which the host tests compile with the lane loop emulated.
#include "dev_common.hpp"
#include "bb_rlc.hpp"
#include "launch.hpp"

using namespace bgls;

__global__ void __launch_bounds__(64) k_bb_rlc_odd(uint8_t* r16, size_t n) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) r16[i * 16 + 15] |= 1;
}

static_assert(BB_RLC_LANES == 64, "one wave per group");
__global__ void __launch_bounds__(BB_RLC_LANES) k_bb_rlc_sums(const uint8_t* r16, const uint64_t* group_off, uint8_t* out) {
  const size_t g = blockIdx.x;
  BbRlcSum acc = bb_rlc_lane_sum(r16, group_off[g], group_off[g + 1], threadIdx.x);
  for (int off = BB_RLC_LANES / 2; off; off >>= 1) {
    BbRlcSum other;                                 // lanes at and above 64 - off read their own words: they feed no lane below them
#pragma unroll
    for (int j = 0; j < BB_RLC_WORDS; ++j) other.w[j] = __shfl_down(acc.w[j], off);
    bb_rlc_add(acc, other);
  }
  if (threadIdx.x == 0) bb_rlc_store(out + g * 32, acc);
}

namespace bgls {
namespace kl {

void bb_rlc_odd(hipStream_t st, uint8_t* r16, size_t n) {
  if (n) k_bb_rlc_odd<<<nblk(n, 64), 64, 0, st>>>(r16, n);
}
void bb_rlc_sums(hipStream_t st, const uint8_t* r16, const uint64_t* group_off, size_t n_groups, uint8_t* out) {
  if (n_groups) k_bb_rlc_sums<<<(unsigned)n_groups, BB_RLC_LANES, 0, st>>>(r16, group_off, out);
}

}  // namespace kl
}  // namespace bgls
