// TEST-ONLY: bgls_amd/csrc/rlc_pair.hpp compiled for the host as a stand-alone program, with every column accumulation of the
// carry-free limbs checked (BGLS_RX_CHECK).  Built by tests/test_rlc_host.py into its temporary directory (once more under
// -fsanitize=address,undefined) and fed cases on standard input, one per line:
//     <curve id 0 / 1> <mode> <H: G1 wire bytes, hex> <sigma: G1 wire bytes, hex> <r: 16 bytes big-endian, hex>
// mode 0 multiplies by r as given, mode 1 by r with its lowest bit set (rlc_scalar, what k_rlc_pair does).  Answer per line:
//     <r H, hex> <r sigma, hex> <1 if a column overflowed, else 0>
// or "bad" for a non-canonical or off-curve point.  Exit status 0 when every line was read.
#include <stdio.h>
#include <string.h>
#define BGLS_RX_CHECK 1
#include "../../bgls_amd/csrc/rlc_pair.hpp"

namespace bgls { int g_rx_overflow = 0; }
using namespace bgls;

static bool unhex(const char* s, uint8_t* out, size_t n) {
  if (strlen(s) != 2 * n) return false;
  for (size_t i = 0; i < n; ++i) {
    unsigned v;
    if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}
static void hex(const uint8_t* b, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", b[i]);
}

template <class C>
static bool one(int mode, const char* hs, const char* ss, const char* rs) {
  constexpr size_t PT = 2 * C::FP_BYTES;
  uint8_t hb[PT], sb[PT], rb[16], out[2][PT];
  if (!unhex(hs, hb, PT) || !unhex(ss, sb, PT) || !unhex(rs, rb, 16)) return false;
  Aff<F1<C>> p[2], q[2];
  bool ok = g1_from_bytes<C>(p[0], hb) && aff_on_curve<F1<C>>(p[0]);
  ok = g1_from_bytes<C>(p[1], sb) && aff_on_curve<F1<C>>(p[1]) && ok;
  if (!ok) return false;
  u32 k[4];
  rlc_scalar(rb, k);
  if (mode == 0 && !(rb[15] & 1)) k[0] &= ~1u;
  g_rx_overflow = 0;
  rlc_pair<C>(p, k, q);
  g1_to_bytes<C>(out[0], q[0]);
  g1_to_bytes<C>(out[1], q[1]);
  hex(out[0], PT);
  printf(" ");
  hex(out[1], PT);
  printf(" %d\n", g_rx_overflow ? 1 : 0);
  return true;
}

int main() {
  static char h[256], s[256], r[64];
  int cid, mode;
  while (scanf("%d %d %255s %255s %63s", &cid, &mode, h, s, r) == 5) {
    const bool ok = cid == 0 ? one<BN254>(mode, h, s, r) : cid == 1 ? one<BLS381>(mode, h, s, r) : false;
    if (!ok) printf("bad\n");
  }
  return 0;
}
