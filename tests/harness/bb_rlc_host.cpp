// TEST-ONLY: bgls_amd/csrc/bb_rlc.hpp compiled for the host as a stand-alone program, the wave of k_bb_rlc_sums emulated: the 64 lane sums
// of a group one after the other (bb_rlc_lane_sum), then the kernel's tree over the offsets 32, 16, .. 1, in which lane l adds the words
// of lane l + off (a lane at or above 64 - off adds its own words, as the shuffle hands them to it), and lane 0 stores.  Built by
// tests/test_bb_rlc_host.py into its temporary directory (once more under -fsanitize=address,undefined).  Standard input:
//     <n> <n_groups>
//     <n_groups + 1 offsets>
//     <n coefficients: 16 bytes big-endian, hex>
// Answer: one line per group, the sum as 32 bytes big-endian, hex.  Exit status 0 when the input was well-formed.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../bgls_amd/csrc/bb_rlc.hpp"

using namespace bgls;

int main() {
  unsigned long long n, n_groups;
  if (scanf("%llu %llu", &n, &n_groups) != 2) return 2;
  std::vector<u64> off(n_groups + 1);
  for (u64& o : off) {
    unsigned long long v;
    if (scanf("%llu", &v) != 1) return 2;
    o = v;
  }
  uint8_t* r16 = (uint8_t*)aligned_alloc(16, (size_t)(n + 1) * 16);      // the kernel's coefficients are 16-byte aligned
  if (!r16) return 2;
  for (u64 i = 0; i < n; ++i) {
    char h[64];
    if (scanf("%63s", h) != 1) return 2;
    for (int j = 0; j < 16; ++j) {
      unsigned v;
      if (sscanf(h + 2 * j, "%2x", &v) != 1) return 2;
      r16[i * 16 + j] = (uint8_t)v;
    }
  }
  for (u64 g = 0; g < n_groups; ++g) {
    BbRlcSum lanes[BB_RLC_LANES];
    for (unsigned l = 0; l < (unsigned)BB_RLC_LANES; ++l) lanes[l] = bb_rlc_lane_sum(r16, off[g], off[g + 1], l);
    for (int o = BB_RLC_LANES / 2; o; o >>= 1) {
      BbRlcSum other[BB_RLC_LANES];
      for (int l = 0; l < BB_RLC_LANES; ++l) other[l] = lanes[l + o < BB_RLC_LANES ? l + o : l];
      for (int l = 0; l < BB_RLC_LANES; ++l) bb_rlc_add(lanes[l], other[l]);
    }
    uint8_t out[32];
    bb_rlc_store(out, lanes[0]);
    for (int j = 0; j < 32; ++j) printf("%02x", out[j]);
    printf("\n");
  }
  free(r16);
  return 0;
}
