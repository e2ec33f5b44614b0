// TEST-ONLY: one element of the point-layer exports, shared by host_harness.cpp (ht_rx_padd / ht_rx_pmul) and device_harness_points.hip
// (dh_padd / dh_pmul) so that both builds run the SAME statements around rx_jac1.hpp (G1, over Fp) and rx_jac.hpp / rx_g2mul.hpp (the
// twists, over Fp2): what differs between them is what the tests compare -- the multiply rows under sx_montr, the storage of the
// chain's table, and the lanes' divergence.
//
// An operand of pt_add is wire bytes plus a field element lambda (FP_BYTES big-endian, canonical, non-zero): the Jacobian input is
// (lambda^2 x, lambda^3 y, lambda), so equal and opposite points arrive with different Z.  has_lambda == 0: the form the chain's table
// starts from (Z = one exactly, jac1_from_aff / jacx_from_aff).
// raw: PT_RAW words per element -- word 0 the infinity flag, then X, Y, Z as RX_NL signed limbs each (G2: X.c0 X.c1 Y.c0 ...), zero-padded.
#pragma once
#include "../../bgls_amd/csrc/rx_jac1.hpp"
#include "../../bgls_amd/csrc/rx_g2mul.hpp"

namespace bgls {

constexpr int PT_RAW = 88;                 // 1 + 6 * 14 (BLS12-381 on the twist), rounded up

template <class C>
BGLS_HD Sx<C, SX_T> pt_lambda(const uint8_t* z, bool& ok) {
  const Fp<C> l = fp_from_be<C>(z);
  ok = ok && !fp_geq_p<C>(l) && !fp_is_zero<C>(l);
  return sx_from_plain<C>(l);
}

// ---- G1
template <class C>
BGLS_HD bool pt1_affine(Aff1<C>& q, const uint8_t* b) {
  Aff<F1<C>> a;
  const bool ok = g1_from_bytes<C>(a, b) && aff_on_curve<F1<C>>(a);
  q = aff1_from_mont<C>(a);                                   // the kernels' way in (k_g1x.hip)
  return ok;
}
template <class C>
BGLS_HD bool pt1_jacobian(Jac1<C>& p, const uint8_t* b, const uint8_t* z, int has_lambda) {
  Aff1<C> q;
  bool ok = pt1_affine<C>(q, b);
  if (q.inf) { p = jac1_inf<C>(); return ok; }
  if (!has_lambda) { p = jac1_from_aff<C>(q); return ok; }
  const Sx<C, SX_T> l = pt_lambda<C>(z, ok), l2 = s1_sqr<C>(l);
  p.X = sx_as<SX_F, C>(s1_mul<C>(q.x, l2));
  p.Y = sx_as<SX_F, C>(s1_mul<C>(s1_mul<C>(q.y, l2), l));
  p.Z = sx_as<SX_F, C>(l);
  p.inf = false;
  return ok;
}
template <class C>
BGLS_HD void pt1_store(const Jac1<C>& r, uint8_t* out, i32* raw) {
  constexpr int N = C::RX_NL;
  for (int i = 0; i < PT_RAW; ++i) raw[i] = 0;
  raw[0] = r.inf ? 1 : 0;
  for (int i = 0; i < N; ++i) { raw[1 + i] = r.X.v[i]; raw[1 + N + i] = r.Y.v[i]; raw[1 + 2 * N + i] = r.Z.v[i]; }
  g1_to_bytes<C>(out, jac_to_aff<F1<C>>(jac1_to_mont<C>(r)));
}
// form 0: a + b, both Jacobian (jac1_add); 1: a + b, b affine (jac1_madd); 2: 2 a (jac1_dbl); 3: 2 a + b, b affine, and 4: 2 a + b, both Jacobian --
// the running point straight from a doubling, whose coordinates are not reductions' outputs.  false on a bad point or lambda.
template <class C>
BGLS_HD bool pt1_add(const uint8_t* a, const uint8_t* za, int la, const uint8_t* b, const uint8_t* zb, int lb, int form, uint8_t* out, i32* raw) {
  Jac1<C> p, r;
  bool ok = pt1_jacobian<C>(p, a, za, la);
  if (form == 3 || form == 4) p = jac1_dbl<C>(p);
  if (form == 0 || form == 4) {
    Jac1<C> q;
    ok = pt1_jacobian<C>(q, b, zb, lb) && ok;
    r = jac1_add<C>(p, q);
  } else if (form == 1 || form == 3) {
    Aff1<C> q;
    ok = pt1_affine<C>(q, b) && ok;
    r = jac1_madd<C>(p, q);
  } else {
    r = jac1_dbl<C>(p);
  }
  pt1_store<C>(r, out, raw);
  return ok;
}
template <class C>
BGLS_HD bool pt1_mul(const uint8_t* pt, const u32* k, int nbits, uint8_t* out, i32* raw) {
  Aff1<C> q;
  const bool ok = pt1_affine<C>(q, pt);
  pt1_store<C>(jac1_mul_w4<C>(q, k, nbits), out, raw);
  return ok;
}

// ---- the twists
template <class C>
BGLS_HD bool pt2_affine(AffX<C>& q, const uint8_t* b) {
  const bool ok = affx_from_bytes<C>(q, b);                   // the kernels' way in (k_bbsigs.hip, k_haesets.hip)
  return affx_on_curve<C>(q) && ok;
}
template <class C>
BGLS_HD bool pt2_jacobian(JacX<C>& p, const uint8_t* b, const uint8_t* z, int has_lambda) {
  AffX<C> q;
  bool ok = pt2_affine<C>(q, b);
  if (q.inf) { p = jacx_inf<C>(); return ok; }
  if (!has_lambda) { p = jacx_from_aff<C>(q); return ok; }
  const X2<C, SX_T> l = {pt_lambda<C>(z, ok), ux_to_sx<C>(ux_zero<C>())};
  const X2<C, SX_T> l2 = x2_sqr<C>(l);
  p.X = x2_as<SX_F, C>(x2_mul<C>(q.x, l2));
  p.Y = x2_as<SX_F, C>(x2_mul<C>(x2_mul<C>(q.y, l2), l));
  p.Z = x2_as<SX_F, C>(l);
  p.inf = false;
  return ok;
}
template <class C>
BGLS_HD void pt2_store(const JacX<C>& r, uint8_t* out, i32* raw) {
  constexpr int N = C::RX_NL;
  for (int i = 0; i < PT_RAW; ++i) raw[i] = 0;
  raw[0] = r.inf ? 1 : 0;
  for (int i = 0; i < N; ++i) {
    raw[1 + i] = r.X.c0.v[i]; raw[1 + N + i] = r.X.c1.v[i];
    raw[1 + 2 * N + i] = r.Y.c0.v[i]; raw[1 + 3 * N + i] = r.Y.c1.v[i];
    raw[1 + 4 * N + i] = r.Z.c0.v[i]; raw[1 + 5 * N + i] = r.Z.c1.v[i];
  }
  g2_to_bytes<C>(out, jac_to_aff<F2<C>>(jacx_to_mont<C>(r)));
}
template <class C>
BGLS_HD bool pt2_add(const uint8_t* a, const uint8_t* za, int la, const uint8_t* b, const uint8_t* zb, int lb, int form, uint8_t* out, i32* raw) {
  JacX<C> p, r;
  bool ok = pt2_jacobian<C>(p, a, za, la);
  if (form == 3 || form == 4) p = jacx_dbl<C>(p);
  if (form == 0 || form == 4) {
    JacX<C> q;
    ok = pt2_jacobian<C>(q, b, zb, lb) && ok;
    r = jacx_add<C>(p, q);
  } else if (form == 1 || form == 3) {
    AffX<C> q;
    ok = pt2_affine<C>(q, b) && ok;
    r = jacx_madd<C>(p, q);
  } else {
    r = jacx_dbl<C>(p);
  }
  pt2_store<C>(r, out, raw);
  return ok;
}
template <class C>
BGLS_HD bool pt2_mul(const uint8_t* pt, const u32* k, int nbits, uint8_t* out, i32* raw) {
  AffX<C> q;
  const bool ok = pt2_affine<C>(q, pt);
  pt2_store<C>(jacx_mul_w4<C>(q, k, nbits), out, raw);
  return ok;
}

}  // namespace bgls
