// The coefficient sums of the combined Boneh-Boyen check (bgls_bb_verify_batch_combined): s_g = sum of the 128-bit coefficients rho_b over
// the items of group g, as a plain integer.  Fewer than 2^28 coefficients below 2^128 each: a sum is below 2^156 and lives in six 32-bit
// words, little-endian, added with explicit carries.  One wave serves a group: lane l adds the items lo + l, lo + l + 64, ... of the group
// (bb_rlc_lane_sum), the 64 lane sums are folded by a tree of bb_rlc_add over the offsets 32, 16, .. 1 (k_bb_rlc_sums does it with lane
// shuffles, the host harness of the tests with a loop over the lanes), and lane 0 holds the sum, written as a 32-byte big-endian
// magnitude -- the form the fixed-base multiplication of the generator reads.
#pragma once
#include "fp.hpp"

namespace bgls {

constexpr int BB_RLC_WORDS = 6;
constexpr int BB_RLC_LANES = 64;
struct BbRlcSum { u32 w[BB_RLC_WORDS]; };

// rho as four little-endian words from its 16 big-endian bytes (16-byte aligned), the lowest bit set (bgls_rlc_coefficients)
BGLS_HD void bb_rlc_coefficient(const uint8_t* r16, u32 (&k)[4]) {
  u32 be[4];
  __builtin_memcpy(be, __builtin_assume_aligned(r16, 16), 16);
#pragma unroll
  for (int j = 0; j < 4; ++j) k[j] = __builtin_bswap32(be[3 - j]);
  k[0] |= 1u;
}

// a += b
BGLS_HD void bb_rlc_add(BbRlcSum& a, const BbRlcSum& b) {
  u64 c = 0;
#pragma unroll
  for (int j = 0; j < BB_RLC_WORDS; ++j) {
    c += (u64)a.w[j] + b.w[j];
    a.w[j] = (u32)c;
    c >>= 32;
  }
}

// the share of lane `lane` in the sum over the coefficients lo .. hi: items lo + lane, lo + lane + 64, ...
BGLS_HD BbRlcSum bb_rlc_lane_sum(const uint8_t* r16, u64 lo, u64 hi, unsigned lane) {
  BbRlcSum acc = {{0, 0, 0, 0, 0, 0}};
#pragma unroll 4
  for (u64 i = lo + lane; i < hi; i += BB_RLC_LANES) {
    u32 k[4];
    bb_rlc_coefficient(r16 + i * 16, k);
    u64 c = 0;
#pragma unroll
    for (int j = 0; j < BB_RLC_WORDS; ++j) {
      c += (u64)acc.w[j] + (j < 4 ? k[j] : 0u);
      acc.w[j] = (u32)c;
      c >>= 32;
    }
  }
  return acc;
}

// the sum as a 32-byte big-endian magnitude
BGLS_HD void bb_rlc_store(uint8_t* out32, const BbRlcSum& s) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const u32 v = j < BB_RLC_WORDS ? s.w[j] : 0u;
    uint8_t* o = out32 + 4 * (7 - j);
    o[0] = (uint8_t)(v >> 24);
    o[1] = (uint8_t)(v >> 16);
    o[2] = (uint8_t)(v >> 8);
    o[3] = (uint8_t)v;
  }
}

}  // namespace bgls
