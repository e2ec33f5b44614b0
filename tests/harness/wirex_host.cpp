// TEST-ONLY: bgls_amd/csrc/wire_x.hpp (the compressed wire formats on the carry-free limbs) compiled for the host, with every column
// accumulation checked (BGLS_RX_CHECK).  As a shared library (build_harness_wirex.py) it serves tests/test_wirex_host.py; compiled with
// -DWIREX_MAIN it is a stand-alone program (the sanitizer run) fed one encoding per line on standard input,
//     <curve id 0 / 1> <group 1 / 2> <compressed bytes, hex>
// which answers "<ok 0 / 1> <uncompressed bytes, hex> <1 if a column overflowed, else 0>" per line.
// Every entry returns -3 when a column accumulation overflowed.
#include <stdio.h>
#include <string.h>
#define BGLS_RX_CHECK 1
#include "../../bgls_amd/csrc/wire_x.hpp"

namespace bgls { int g_rx_overflow = 0; }
using namespace bgls;

namespace {

#ifndef WIREX_MAIN      // the stand-alone program decodes whole points only: the function-level entries stay out of its (slow, sanitized) build
template <class C>
Sx<C, SX_T> load_be(const uint8_t* b) { return sx_from_plain<C>(fp_from_be<C>(b)); }

template <class C>
int f2_root(const uint8_t* a_re, const uint8_t* a_im, uint8_t* r_re, uint8_t* r_im) {
  WxTabLocal<C> tab;
  const X2<C, SX_T> a = {load_be<C>(a_re), load_be<C>(a_im)};
  X2<C, SX_T> r;
  g_rx_overflow = 0;
  bool ok = wx_f2_root<C>(r, a, tab);
  ok = ok && el_is_zero<C>(el_sub<C>(x2_sqr<C>(r), a));
  fp_to_be<C>(r_re, ok ? wx_plain<C>(r.c0) : fp_zero<C>());
  fp_to_be<C>(r_im, ok ? wx_plain<C>(r.c1) : fp_zero<C>());
  if (g_rx_overflow) return -3;
  return ok ? 1 : 0;
}

// pt: uncompressed wire bytes of a finite point with canonical coordinates
template <class C>
int psi(const uint8_t* pt, uint8_t* out) {
  AffX<C> q;
  if (!affx_from_bytes<C>(q, pt) || q.inf) return -1;
  const X2<C, SX_T> px = {sx_from_mont<C>(fp_load<C>(C::PSI_X)), sx_from_mont<C>(fp_load<C>(C::PSI_X + C::L))};
  const X2<C, SX_T> py = {sx_from_mont<C>(fp_load<C>(C::PSI_Y)), sx_from_mont<C>(fp_load<C>(C::PSI_Y + C::L))};
  g_rx_overflow = 0;
  const JacX<C> r = wx_psi<C>(jacx_from_aff<C>(q), px, py);
  g2_to_bytes<C>(out, jac_to_aff<F2<C>>(jacx_to_mont<C>(r)));
  return g_rx_overflow ? -3 : 0;
}

template <class C>
int in_subgroup(int group, const uint8_t* pt) {
  g_rx_overflow = 0;
  bool in;
  if (group == 2) {
    AffX<C> q;
    if (!affx_from_bytes<C>(q, pt)) return -1;
    in = q.inf || wx_g2_in_subgroup<C>(q);
  } else {
    Aff<F1<C>> a;
    if (!g1_from_bytes<C>(a, pt)) return -1;
    in = a.inf || wx_g1_in_subgroup<C>(aff1_from_mont<C>(a));
  }
  if (g_rx_overflow) return -3;
  return in ? 1 : 0;
}

#endif

#ifdef WIREX_MAIN
#define WIREX_SUB(sub, CALL_T, CALL_F) (CALL_T)
#else
#define WIREX_SUB(sub, CALL_T, CALL_F) ((sub) ? (CALL_T) : (CALL_F))
#endif

template <class C>
int decode(int group, const uint8_t* in, size_t n, int subgroup, uint8_t* out, uint8_t* ok) {
  constexpr size_t FB = C::FP_BYTES;
  WxTabLocal<C> tab;
  g_rx_overflow = 0;
  for (size_t i = 0; i < n; ++i) {
    bool good;
    if (group == 1) {
      Fp<C> pl[2];
      good = WIREX_SUB(subgroup, (wx_g1_decode<C, true>(in + i * FB, tab, pl)), (wx_g1_decode<C, false>(in + i * FB, tab, pl)));
      for (int k = 0; k < 2; ++k) fp_to_be<C>(out + (2 * i + k) * FB, good ? pl[k] : fp_zero<C>());
    } else {
      Fp<C> pl[4];
      good = WIREX_SUB(subgroup, (wx_g2_decode<C, true>(in + i * 2 * FB, tab, pl)), (wx_g2_decode<C, false>(in + i * 2 * FB, tab, pl)));
      const int order[4] = {1, 0, 3, 2};                     // x_im || x_re || y_im || y_re
      for (int k = 0; k < 4; ++k) fp_to_be<C>(out + (4 * i + k) * FB, good ? pl[order[k]] : fp_zero<C>());
    }
    ok[i] = good ? 1 : 0;
  }
  return g_rx_overflow ? -3 : 0;
}

}  // namespace

extern "C" {

#ifndef WIREX_MAIN
int wirex_f2_root(int curve, const uint8_t* a_re, const uint8_t* a_im, uint8_t* r_re, uint8_t* r_im) {
  return curve == 0 ? f2_root<BN254>(a_re, a_im, r_re, r_im) : f2_root<BLS381>(a_re, a_im, r_re, r_im);
}
int wirex_psi(int curve, const uint8_t* pt, uint8_t* out) { return curve == 0 ? psi<BN254>(pt, out) : psi<BLS381>(pt, out); }
int wirex_in_subgroup(int curve, int group, const uint8_t* pt) { return curve == 0 ? in_subgroup<BN254>(group, pt) : in_subgroup<BLS381>(group, pt); }
#endif
int wirex_decode(int curve, int group, const uint8_t* in, size_t n, int subgroup, uint8_t* out, uint8_t* ok) {
  return curve == 0 ? decode<BN254>(group, in, n, subgroup, out, ok) : decode<BLS381>(group, in, n, subgroup, out, ok);
}

}  // extern "C"

#ifdef WIREX_MAIN
int main() {
  static char hexin[512];
  int cid, group;
  while (scanf("%d %d %511s", &cid, &group, hexin) == 3) {
    if ((cid != 0 && cid != 1) || (group != 1 && group != 2)) { printf("bad\n"); continue; }
    const size_t cb = (size_t)(cid ? 48 : 32) * group;
    uint8_t in[96], out[192], ok = 0;
    if (strlen(hexin) != 2 * cb) { printf("bad\n"); continue; }
    for (size_t i = 0; i < cb; ++i) {
      unsigned v;
      if (sscanf(hexin + 2 * i, "%2x", &v) != 1) v = 0;
      in[i] = (uint8_t)v;
    }
    const int rc = wirex_decode(cid, group, in, 1, 1, out, &ok);
    printf("%d ", ok);
    for (size_t i = 0; i < 2 * cb; ++i) printf("%02x", out[i]);
    printf(" %d\n", rc == -3 ? 1 : 0);
  }
  return 0;
}
#endif
