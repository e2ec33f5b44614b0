// Compressed wire formats decoded on ONE lane in the carry-free 28-bit-limb form (rx.hpp): parse, square root, sign rule, curve check and
// subgroup membership of one point, the same accepted set and the same bytes as wire.hpp's g1_decompress / g2_decompress (alt-bn128,
// curves/altbn128.go:296-376) and g1_decompress_zc / g2_decompress_zc (BLS12-381, curves/bls12_381.go:242-264) followed by curve.hpp's
// g1_in_subgroup / g2_in_subgroup.  What a key set built from compressed keys runs (k_wirex.hip).
//
// Square roots.  p = 3 mod 4 on both curves.  One windowed power t = a^((p - 3) / 4) (rx_pow.hpp) gives the candidate root c = t a =
// a^((p + 1) / 4) of calcQuadRes, the residue symbol (c^2 == a iff a is zero or a residue) and, for a residue, the inverse 1 / c = t.
// Fp2 = Fp[i] / (i^2 + 1), a = a0 + a1 i with a1 != 0: lam = cand(a0^2 + a1^2), delta = (a0 + lam) / 2, t = delta^((p - 3) / 4), c = t delta.
//   delta a residue (or zero):  root = (c, a1 t / 2)                          -- f2_complex_quad_res / f2_sqrt with 1 / c = t
//   delta a non-residue:        root = (a1 t / 2, -c)                          -- t^2 delta = -1, so ((a0 - lam) / 2) = (a1 t / 2)^2 and 1 / t = -c
// Two powers whatever the residue symbols say, no Euler power, no inversion, no second candidate: the second line is +- the root that
// wire.hpp finds through the fallback delta, and the sign of the root does not reach the output -- alt-bn128 sends each component
// through its own sign bit (fp_apply_sign maps y and -y to the same representative, and refuses a set bit on a zero component either
// way), BLS12-381 selects by the sort flag.  Where a is NOT a square (lam is then no root of the norm on alt-bn128, where the reference
// does not test it) whatever comes out fails the final y^2 == x^3 + b, which both formats apply and which decides here as there.
// a1 == 0: alt-bn128 takes (cand(a0), 0) untested (a non-residue a0 then fails the final check although i sqrt(-a0) is a root: the
// reference's quirk); BLS12-381 takes (cand(a0), 0) or (0, cand(-a0)).
//
// Membership: the endomorphism criterion of curve.hpp's g2_in_subgroup on rx_jac.hpp's formulas (P = +-Q and infinity exact), the public
// scalar |u| walked bit by bit with wave-uniform branches; BLS12-381's G1 by [r]P = infinity on rx_jac1.hpp's chain.  Both are blind to
// the sign of y.
#pragma once
#include "wire.hpp"
#include "rx_pow.hpp"
#include "rx_jac1.hpp"
#include "rx_g2mul.hpp"

namespace bgls {

// window width of the powers and the entries of a lane's table (entry e holds a^(2 e + 1)); tab.ld(e, i) / tab.st(e, i, v): limb i of entry e
constexpr int WX_W = 3;
constexpr int WX_TE = 1 << (WX_W - 1);

// a lane's table in its own memory (the host build; the kernel keeps it in LDS columns)
template <class C>
struct WxTabLocal {
  i32 t[WX_TE * C::RX_NL];
  BGLS_HD i32 ld(int e, int i) const { return t[e * C::RX_NL + i]; }
  BGLS_HD void st(int e, int i, i32 v) { t[e * C::RX_NL + i] = v; }
};

// a^((p - 3) / 4); a: tight limbs, value in (-p, 3 p)
template <class C, class Tab>
BGLS_FN Sx<C, SX_T> wx_pow_m1(const Sx<C, SX_T>& a, Tab& tab) {
  return sx_pow_sqrt<C, WX_W, true>(a, [&](int e, int i) { return tab.ld(e, i); }, [&](int e, int i, i32 v) { tab.st(e, i, v); });
}
// (a + b) / 2 and (a - b) / 2 ... with the limbs tight again
template <class C, int LA>
BGLS_HD Sx<C, SX_T> wx_half(const Sx<C, LA>& a) { return sx_norm<C>(sx_half<C>(a)); }
template <class C>
BGLS_HD bool wx_eq(const Sx<C, SX_T>& a, const Sx<C, SX_T>& b) { return sx_is_zero_mod_p<C>(sx_sub<C>(a, b)); }
template <class C>
BGLS_HD Sx<C, SX_T> wx_zero() { return ux_to_sx<C>(ux_zero<C>()); }
template <class C>
BGLS_HD Sx<C, SX_T> wx_neg(const Sx<C, SX_T>& a) { return sx_norm<C>(sx_neg<C>(a)); }

// the candidate root a^((p + 1) / 4); *t_out = a^((p - 3) / 4)
template <class C, class Tab>
BGLS_HD Sx<C, SX_T> wx_cand(const Sx<C, SX_T>& a, Tab& tab, Sx<C, SX_T>* t_out = nullptr) {
  const Sx<C, SX_T> t = wx_pow_m1<C>(a, tab);
  if (t_out) *t_out = t;
  return s1_mul<C>(t, a);
}

// A square-root candidate of a in Fp2 by the rules of the curve's format (header); the caller's y^2 == a decides.  false: refused outright.
template <class C, class Tab>
BGLS_HD bool wx_f2_root(X2<C, SX_T>& r, const X2<C, SX_T>& a, Tab& tab) {
  typedef Sx<C, SX_T> T;
  if (sx_is_zero_mod_p<C>(a.c1)) {
    const T c = wx_cand<C>(a.c0, tab);
    r = {c, wx_zero<C>()};
    if constexpr (C::CURVE_ID != 0) {
      if (!wx_eq<C>(s1_sqr<C>(c), a.c0)) r = {wx_zero<C>(), wx_cand<C>(wx_neg<C>(a.c0), tab)};    // a0 a non-residue: i times a root of -a0
    }
    return true;
  }
  T norm;
  {
    const i32* const cols[2] = {a.c0.v, a.c1.v};
    norm = sx_montr<C, 2, 2 * SX_T * SX_T>(cols, [&](int k, int i) { return k == 0 ? a.c0.v[i] : a.c1.v[i]; });
  }
  const T lam = wx_cand<C>(norm, tab);
  const T delta = wx_half<C>(sx_add<C>(a.c0, lam));
  T t;
  const T c = wx_cand<C>(delta, tab, &t);
  const T o = s1_mul<C>(t, wx_half<C>(a.c1));              // a1 t / 2
  if (wx_eq<C>(s1_sqr<C>(c), delta)) {
    if (sx_is_zero_mod_p<C>(c)) return false;                // delta = 0: the reference's ModInverse(0) / f2_sqrt's refusal
    r = {c, o};
  } else {
    r = {o, wx_neg<C>(c)};
  }
  return true;
}

// the canonical plain integer of an element (tight limbs, value in (-p, 4 p))
template <class C>
BGLS_HD Fp<C> wx_plain(const Sx<C, SX_T>& a) { return sx_over_r_words<C>(a); }

// alt-bn128's sign rule on one component (fp_apply_sign): y and its canonical plain value follow the bit; false for a set bit on zero
template <class C>
BGLS_HD bool wx_apply_sign(Sx<C, SX_T>& y, Fp<C>& plain, bool sgn) {
  if (sgn != fp_plain_gt_half<C>(plain)) {
    if (fp_is_zero<C>(plain)) return false;
    plain = fp_neg<C>(plain);
    y = wx_neg<C>(y);
  }
  return true;
}
template <class C>
BGLS_HD void wx_negate(Sx<C, SX_T>& y, Fp<C>& plain) {
  if (fp_is_zero<C>(plain)) return;
  plain = fp_neg<C>(plain);
  y = wx_neg<C>(y);
}

// ---- parse: the flag bits and x, exactly as wire.hpp.  kind: 0 refused, 1 infinity, 2 a finite x below p
template <class C, int NX>
BGLS_HD int wx_parse(const uint8_t* b, Fp<C> (&x)[NX], bool (&sgn)[NX]) {
  bool zero = true, big = false;
  if constexpr (C::CURVE_ID == 0) {
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      x[k] = fp_from_be_clear_top<C>(b + k * C::FP_BYTES, sgn[k]);
      zero = zero && fp_is_zero<C>(x[k]);
      big = big || fp_geq_p<C>(x[k]);
    }
    if (zero) return 1;                                      // altbn128.go:311-313,349-351: infinity whatever the flags say
    return big ? 0 : 2;
  } else {
    uint8_t fl;
    x[0] = fp_from_be_zc<C>(b, fl);
    if constexpr (NX == 2) x[1] = fp_from_be<C>(b + C::FP_BYTES);
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      sgn[k] = (fl & ZC_LARGER) != 0;
      zero = zero && fp_is_zero<C>(x[k]);
      big = big || fp_geq_p<C>(x[k]);
    }
    if (!(fl & ZC_COMPRESSED)) return 0;
    if (fl & ZC_INFINITY) return (!(fl & ZC_LARGER) && zero) ? 1 : 0;
    return big ? 0 : 2;
  }
}

// ---- membership
template <class C>
BGLS_HD JacX<C> wx_psi(const JacX<C>& p, const X2<C, SX_T>& px, const X2<C, SX_T>& py) {
  JacX<C> r;
  const X2<C, SX_F> cx = {p.X.c0, el_negf<C>(p.X.c1)}, cy = {p.Y.c0, el_negf<C>(p.Y.c1)};
  r.X = el_as<SX_F, C>(x2_mul<C>(cx, px));
  r.Y = el_as<SX_F, C>(x2_mul<C>(cy, py));
  r.Z = {p.Z.c0, el_negf<C>(p.Z.c1)};
  r.inf = p.inf;
  return r;
}
template <class C>
BGLS_HD bool wx_jacx_eq(const JacX<C>& a, const JacX<C>& b) {
  if (a.inf || b.inf) return a.inf && b.inf;
  const X2<C, SX_T> za = x2_sqr<C>(a.Z), zb = x2_sqr<C>(b.Z);
  if (!el_is_zero<C>(x2_mulsub<C>(a.X, zb, b.X, za))) return false;
  return el_is_zero<C>(x2_mulsub<C>(a.Y, x2_mul<C>(zb, b.Z), b.Y, x2_mul<C>(za, a.Z)));
}
// q on the twist (the caller checked) and finite.  curve.hpp's g2_in_subgroup:
//     alt-bn128   [u + 1] Q + psi([u] Q) + psi^2([u] Q) = psi^3([2 u] Q)          BLS12-381   psi(Q) = [x] Q, x = -|u|
template <class C>
BGLS_HD bool wx_g2_in_subgroup(const AffX<C>& q) {
  const X2<C, SX_T> px = {sx_from_mont<C>(fp_load<C>(C::PSI_X)), sx_from_mont<C>(fp_load<C>(C::PSI_X + C::L))};
  const X2<C, SX_T> py = {sx_from_mont<C>(fp_load<C>(C::PSI_Y)), sx_from_mont<C>(fp_load<C>(C::PSI_Y + C::L))};
  int i = C::U_BITS - 1;
  while (i > 0 && !((C::U_ABS[i >> 5] >> (i & 31)) & 1u)) --i;
  JacX<C> xq = jacx_from_aff<C>(q);
#pragma unroll 1
  for (--i; i >= 0; --i) {                                    // the scalar is public: every branch here is the whole wave's
    xq = jacx_dbl<C>(xq);
    if ((C::U_ABS[i >> 5] >> (i & 31)) & 1u) xq = jacx_madd<C>(xq, q);
  }
  if constexpr (C::CURVE_ID == 0) {
    const JacX<C> p1 = wx_psi<C>(xq, px, py), p2 = wx_psi<C>(p1, px, py);
    const JacX<C> lhs = jacx_add<C>(jacx_add<C>(jacx_madd<C>(xq, q), p1), p2);
    const JacX<C> rhs = wx_psi<C>(wx_psi<C>(wx_psi<C>(jacx_dbl<C>(xq), px, py), px, py), px, py);
    return wx_jacx_eq<C>(lhs, rhs);
  } else {
    if (!xq.inf) xq.Y = el_negf<C>(xq.Y);
    return wx_jacx_eq<C>(wx_psi<C>(jacx_from_aff<C>(q), px, py), xq);
  }
}
template <class C>
BGLS_HD bool wx_g1_in_subgroup(const Aff1<C>& p) {
  if constexpr (C::CURVE_ID == 0) return true;               // cofactor 1
  else return jac1_mul_w4<C>(p, C::ORDER, 255).inf;
}

// ---- whole decodes.  plain: the canonical coordinates as plain integers, G1 (x, y), G2 (x_re, x_im, y_re, y_im); all zero at infinity.
// Returns the reference's (Point, bool): false = refused (plain is then unspecified).  SUBGROUP = false stops before the membership test.
template <class C, bool SUBGROUP = true, class Tab>
BGLS_HD bool wx_g1_decode(const uint8_t* b, Tab& tab, Fp<C> (&plain)[2]) {
  Fp<C> x[1];
  bool sgn[1];
  const int kind = wx_parse<C, 1>(b, x, sgn);
  plain[0] = plain[1] = fp_zero<C>();
  if (kind < 2) return kind == 1;
  Aff1<C> p;
  p.inf = false;
  p.x = sx_from_plain<C>(x[0]);
  const Sx<C, SX_T> y2 = sx_norm<C>(sx_add<C>(s1_mul<C>(s1_sqr<C>(p.x), p.x), sx_from_mont<C>(fp_load<C>(C::B))));
  p.y = wx_cand<C>(y2, tab);
  if (!wx_eq<C>(s1_sqr<C>(p.y), y2)) return false;
  plain[0] = x[0];
  plain[1] = wx_plain<C>(p.y);
  if constexpr (C::CURVE_ID == 0) {
    if (!wx_apply_sign<C>(p.y, plain[1], sgn[0])) return false;
  } else {
    if (fp_plain_gt_half<C>(plain[1]) != sgn[0]) wx_negate<C>(p.y, plain[1]);
  }
  if constexpr (SUBGROUP) return wx_g1_in_subgroup<C>(p);
  return true;
}

template <class C, bool SUBGROUP = true, class Tab>
BGLS_HD bool wx_g2_decode(const uint8_t* b, Tab& tab, Fp<C> (&plain)[4]) {
  Fp<C> x[2];                                                // x_im, x_re: the order of the wire
  bool sgn[2];
  const int kind = wx_parse<C, 2>(b, x, sgn);
  plain[0] = plain[1] = plain[2] = plain[3] = fp_zero<C>();
  if (kind < 2) return kind == 1;
  AffX<C> q;
  q.inf = false;
  q.x = {sx_from_plain<C>(x[1]), sx_from_plain<C>(x[0])};
  const X2<C, SX_T> b2 = {sx_const<C>(C::RX_B2_RE), sx_const<C>(C::RX_B2_IM)};
  const X2<C, 2 * SX_T> y2w = el_add<C>(x2_mul<C>(x2_sqr<C>(q.x), q.x), b2);
  const X2<C, SX_T> y2 = {sx_norm<C>(y2w.c0), sx_norm<C>(y2w.c1)};
  if (!wx_f2_root<C>(q.y, y2, tab)) return false;
  if (!el_is_zero<C>(el_sub<C>(x2_sqr<C>(q.y), y2))) return false;       // the final curve check of both formats: sign-blind
  plain[0] = x[1];
  plain[1] = x[0];
  plain[2] = wx_plain<C>(q.y.c0);
  plain[3] = wx_plain<C>(q.y.c1);
  if constexpr (C::CURVE_ID == 0) {
    // the two components follow their own bits (altbn128.go:360-371): inconsistent bits yield a non-point, which MakeG2Point refuses
    Sx<C, SX_T> y0 = q.y.c0, y1 = q.y.c1;
    if (!wx_apply_sign<C>(q.y.c1, plain[3], sgn[0])) return false;
    if (!wx_apply_sign<C>(q.y.c0, plain[2], sgn[1])) return false;
    // y^2 = a has the roots y and -y only: both components kept or both flipped (a zero component counts for either)
    const bool f0 = !wx_eq<C>(y0, q.y.c0), f1 = !wx_eq<C>(y1, q.y.c1);
    if (f0 != f1 && !fp_is_zero<C>(plain[2]) && !fp_is_zero<C>(plain[3])) return false;
  } else {
    const bool larger = !fp_is_zero<C>(plain[3]) ? fp_plain_gt_half<C>(plain[3]) : fp_plain_gt_half<C>(plain[2]);
    if (larger != sgn[0]) {
      wx_negate<C>(q.y.c0, plain[2]);
      wx_negate<C>(q.y.c1, plain[3]);
    }
  }
  if constexpr (SUBGROUP) return wx_g2_in_subgroup<C>(q);
  return true;
}

}  // namespace bgls
