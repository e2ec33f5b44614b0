// Points on ONE lane in the carry-free 28-bit-limb form of rx.hpp (signed limbs, compile-time bounds), over either coordinate field:
// G1 over Fp (Sx, named jac1_* in rx_jac1.hpp) and the twists over Fp2 (X2, named jacx_* here; their chain in rx_g2mul.hpp).  One
// Jacobian formula set (dbl-2009-l, madd-2007-bl, add-2007-bl) and one windowed chain, written in field operations that both element
// types spell the same way.  Born as the G2 key sum (AggregatePoints, curves/curve.go:73-121: n - 1 additions of unit-weight keys).
//
// Why: the 32-bit form of this loop (points_inl.hpp jac_madd_inl) runs at 0.24 of the multiplier's peak -- three VALU
// instructions per multiplier instruction, 256 registers with 70 spilled.  Here an Fp2 product is four interleaved
// limb products and two reductions (sx_montr: bare v_mad_i64_i32 into NL + 1 live columns), differences are limb-wise, and
// the sum of two products shares one reduction.  Same group law, same exceptional cases (P = Q doubles, P = -Q and the
// point at infinity are exact), so the sum is the same point; the result leaves in the library's 32-bit Montgomery form.
#pragma once
#include "curve.hpp"
#include "rx.hpp"

namespace bgls {

template <class C, int LB>
struct X2 {
  Sx<C, LB> c0, c1;
};

// ---- products: Fp
template <class C, int LA, int LB>
BGLS_HD Sx<C, SX_T> s1_mul(const Sx<C, LA>& a, const Sx<C, LB>& b) {
  const i32* const cols[1] = {b.v};
  return sx_montr<C, 1, LA * LB>(cols, [&](int, int i) { return a.v[i]; });
}
template <class C, int LA>
BGLS_HD Sx<C, SX_T> s1_sqr(const Sx<C, LA>& a) {
  const i32* const cols[1] = {a.v};
  return sx_montr<C, 1, LA * LA>(cols, [&](int, int i) { return a.v[i]; });
}
// a b - c d, one reduction
template <class C, int LA, int LB, int LC, int LD>
BGLS_HD Sx<C, SX_T> s1_mulsub(const Sx<C, LA>& a, const Sx<C, LB>& b, const Sx<C, LC>& c, const Sx<C, LD>& d) {
  const i32* const cols[2] = {b.v, d.v};
  return sx_montr<C, 2, LA * LB + LC * LD>(cols, [&](int k, int i) { return k == 0 ? a.v[i] : -c.v[i]; });
}

// ---- products: Fp2
// a * b: (a0 b0 - a1 b1) + (a0 b1 + a1 b0) i, two products and one reduction per component
template <class C, int LA, int LB>
BGLS_HD X2<C, SX_T> x2_mul(const X2<C, LA>& a, const X2<C, LB>& b) {
  X2<C, SX_T> r;
  {
    const i32* const cols[2] = {b.c0.v, b.c1.v};
    r.c0 = sx_montr<C, 2, 2 * LA * LB>(cols, [&](int k, int i) { return k == 0 ? a.c0.v[i] : -a.c1.v[i]; });
  }
  {
    const i32* const cols[2] = {b.c1.v, b.c0.v};
    r.c1 = sx_montr<C, 2, 2 * LA * LB>(cols, [&](int k, int i) { return k == 0 ? a.c0.v[i] : a.c1.v[i]; });
  }
  return r;
}
// a^2: (a0 + a1)(a0 - a1) + 2 a0 a1 i
template <class C, int LA>
BGLS_HD X2<C, SX_T> x2_sqr(const X2<C, LA>& a) {
  X2<C, SX_T> r;
  {
    const Sx<C, 2 * LA> u = sx_add<C>(a.c0, a.c1);
    const i32* const cols[1] = {u.v};
    r.c0 = sx_montr<C, 1, 4 * LA * LA>(cols, [&](int, int i) { return a.c0.v[i] - a.c1.v[i]; });
  }
  {
    const i32* const cols[1] = {a.c1.v};
    r.c1 = sx_montr<C, 1, 2 * LA * LA>(cols, [&](int, int i) { return 2 * a.c0.v[i]; });
  }
  return r;
}
// a b - c d, one reduction per component
template <class C, int LA, int LB, int LC, int LD>
BGLS_HD X2<C, SX_T> x2_mulsub(const X2<C, LA>& a, const X2<C, LB>& b, const X2<C, LC>& c, const X2<C, LD>& d) {
  X2<C, SX_T> r;
  {
    const i32* const cols[4] = {b.c0.v, b.c1.v, d.c0.v, d.c1.v};
    r.c0 = sx_montr<C, 4, 2 * LA * LB + 2 * LC * LD>(cols, [&](int k, int i) { return k == 0 ? a.c0.v[i] : (k == 1 ? -a.c1.v[i] : (k == 2 ? -c.c0.v[i] : c.c1.v[i])); });
  }
  {
    const i32* const cols[4] = {b.c1.v, b.c0.v, d.c1.v, d.c0.v};
    r.c1 = sx_montr<C, 4, 2 * LA * LB + 2 * LC * LD>(cols, [&](int k, int i) { return k == 0 ? a.c0.v[i] : (k == 1 ? a.c1.v[i] : (k == 2 ? -c.c0.v[i] : -c.c1.v[i])); });
  }
  return r;
}

// widen the static bound (no code), as rx.hpp's sx_as
template <int LB, class C, int LA>
BGLS_HD X2<C, LB> x2_as(const X2<C, LA>& a) { return {sx_as<LB, C>(a.c0), sx_as<LB, C>(a.c1)}; }

// ---- one spelling for both fields: what the point formulas below are written in.  Fp forwards to rx.hpp's sx_* and the s1_* above,
// Fp2 works component-wise around the x2_* above; no arithmetic of its own.
template <class C, int LA, int LB>
BGLS_HD Sx<C, SX_T> el_mul(const Sx<C, LA>& a, const Sx<C, LB>& b) { return s1_mul<C>(a, b); }
template <class C, int LA, int LB>
BGLS_HD X2<C, SX_T> el_mul(const X2<C, LA>& a, const X2<C, LB>& b) { return x2_mul<C>(a, b); }
template <class C, int LA>
BGLS_HD Sx<C, SX_T> el_sqr(const Sx<C, LA>& a) { return s1_sqr<C>(a); }
template <class C, int LA>
BGLS_HD X2<C, SX_T> el_sqr(const X2<C, LA>& a) { return x2_sqr<C>(a); }
template <class C, int LA, int LB, int LC, int LD>
BGLS_HD Sx<C, SX_T> el_mulsub(const Sx<C, LA>& a, const Sx<C, LB>& b, const Sx<C, LC>& c, const Sx<C, LD>& d) { return s1_mulsub<C>(a, b, c, d); }
template <class C, int LA, int LB, int LC, int LD>
BGLS_HD X2<C, SX_T> el_mulsub(const X2<C, LA>& a, const X2<C, LB>& b, const X2<C, LC>& c, const X2<C, LD>& d) { return x2_mulsub<C>(a, b, c, d); }
template <class C, int LA, int LB>
BGLS_HD Sx<C, LA + LB> el_add(const Sx<C, LA>& a, const Sx<C, LB>& b) { return sx_add<C>(a, b); }
template <class C, int LA, int LB>
BGLS_HD X2<C, LA + LB> el_add(const X2<C, LA>& a, const X2<C, LB>& b) { return {sx_add<C>(a.c0, b.c0), sx_add<C>(a.c1, b.c1)}; }
template <class C, int LA, int LB>
BGLS_HD Sx<C, LA + LB> el_sub(const Sx<C, LA>& a, const Sx<C, LB>& b) { return sx_sub<C>(a, b); }
template <class C, int LA, int LB>
BGLS_HD X2<C, LA + LB> el_sub(const X2<C, LA>& a, const X2<C, LB>& b) { return {sx_sub<C>(a.c0, b.c0), sx_sub<C>(a.c1, b.c1)}; }
template <int K, class C, int LA>
BGLS_HD Sx<C, K * LA> el_mulc(const Sx<C, LA>& a) { return sx_mulc<K, C>(a); }
template <int K, class C, int LA>
BGLS_HD X2<C, K * LA> el_mulc(const X2<C, LA>& a) { return {sx_mulc<K, C>(a.c0), sx_mulc<K, C>(a.c1)}; }
template <class C, int LA>
BGLS_HD Sx<C, SX_F> el_normf(const Sx<C, LA>& a) { return sx_normf<C>(a); }
template <class C, int LA>
BGLS_HD X2<C, SX_F> el_normf(const X2<C, LA>& a) { return {sx_normf<C>(a.c0), sx_normf<C>(a.c1)}; }
// widen the static bound (no code)
template <int LB, class C, int LA>
BGLS_HD Sx<C, LB> el_as(const Sx<C, LA>& a) { return sx_as<LB, C>(a); }
template <int LB, class C, int LA>
BGLS_HD X2<C, LB> el_as(const X2<C, LA>& a) { return x2_as<LB, C>(a); }
template <class C, int LA>
BGLS_HD bool el_is_zero(const Sx<C, LA>& a) { return sx_is_zero_mod_p<C>(a); }
template <class C, int LA>
BGLS_HD bool el_is_zero(const X2<C, LA>& a) { return sx_is_zero_mod_p<C>(a.c0) && sx_is_zero_mod_p<C>(a.c1); }
// for components in (-11 p, 13 p): differences against a doubling's X and Y (rx.hpp sx_is_zero_mod_p_wide)
template <class C, int LA>
BGLS_HD bool el_is_zero_wide(const Sx<C, LA>& a) { return sx_is_zero_mod_p_wide<C>(a); }
template <class C, int LA>
BGLS_HD bool el_is_zero_wide(const X2<C, LA>& a) { return sx_is_zero_mod_p_wide<C>(a.c0) && sx_is_zero_mod_p_wide<C>(a.c1); }
// -a with the limbs tight again (the sign sits in the top limb)
template <class C, int LA>
BGLS_HD Sx<C, SX_F> el_negf(const Sx<C, LA>& a) { return sx_as<SX_F, C>(sx_norm<C>(sx_neg<C>(a))); }
template <class C, int LA>
BGLS_HD X2<C, SX_F> el_negf(const X2<C, LA>& a) { return {el_negf<C>(a.c0), el_negf<C>(a.c1)}; }
// a base-field value as an element
template <class C>
BGLS_HD void el_set(Sx<C, SX_F>& r, const Sx<C, SX_T>& a) { r = sx_as<SX_F, C>(a); }
template <class C>
BGLS_HD void el_set(X2<C, SX_F>& r, const Sx<C, SX_T>& a) { r = {sx_as<SX_F, C>(a), sx_as<SX_F, C>(ux_to_sx<C>(ux_zero<C>()))}; }

// x R (the library's Montgomery form) -> R' form
template <class C>
BGLS_HD Sx<C, SX_T> sx_from_mont(const Fp<C>& y) { return ux_to_sx<C>(to_ux<C>(y)); }
// R' form (limbs below 2^29, |value| < 8 p) -> the library's form: a product by one brings the value into (-eps p, (1 + eps) p),
// adding p makes it positive, from_ux does the rest
template <class C, int LA>
BGLS_HD Fp<C> sx_to_mont(const Sx<C, LA>& a) {
  constexpr int N = C::RX_NL;
  const Sx<C, SX_T> one = sx_const<C>(C::RX_ONE);
  const i32* const cols[1] = {one.v};
  const Sx<C, SX_T> r = sx_montr<C, 1, LA * SX_T>(cols, [&](int, int i) { return a.v[i]; });
  Sx<C, 2 * SX_T> t;
#pragma unroll
  for (int i = 0; i < N; ++i) t.v[i] = r.v[i] + (i32)C::RX_PK[N + i];      // + p
  const Sx<C, SX_T> n = sx_norm<C>(t);
  Ux<C> u;
#pragma unroll
  for (int i = 0; i < N; ++i) u.v[i] = (u32)n.v[i];
  return from_ux<C>(u);
}

// ===================================================================================================== points over either field
// Jacobian (X, Y, Z), limbs almost tight, plus the infinity flag (the running sum of a key-sum thread, the entries of a chain's table)
template <template <class, int> class E, class C>
struct JacE {
  E<C, SX_F> X, Y, Z;
  bool inf;
};
template <template <class, int> class E, class C>
struct AffE {
  E<C, SX_T> x, y;
  bool inf;
};
template <class C> using JacX = JacE<X2, C>;       // the twist, over Fp2 (G1 over Fp: Jac1 / Aff1, rx_jac1.hpp)
template <class C> using AffX = AffE<X2, C>;

// A field's own from_aff / dbl / madd / add: the jacx_* at the end of this header and the jac1_* of rx_jac1.hpp, each behind the attribute measured for
// it.  The formulas reach their rare branches, and the chain every step, through here, so that they land on exactly those functions.
template <template <class, int> class E, class C>
struct JacLaw;

template <template <class, int> class E, class C>
BGLS_HD JacE<E, C> jace_inf() {
  JacE<E, C> r;
  el_set<C>(r.X, ux_to_sx<C>(ux_zero<C>()));
  r.Y = r.X; r.Z = r.X;
  r.inf = true;
  return r;
}
template <template <class, int> class E, class C>
BGLS_HD JacE<E, C> jace_from_aff(const AffE<E, C>& q) {
  JacE<E, C> r;
  r.X = el_as<SX_F, C>(q.x);
  r.Y = el_as<SX_F, C>(q.y);
  el_set<C>(r.Z, sx_const<C>(C::RX_ONE));
  r.inf = q.inf;
  return r;
}

// 2 p (dbl-2009-l, a = 0): 2 products + 5 squarings
template <template <class, int> class E, class C>
BGLS_HD JacE<E, C> jace_dbl(const JacE<E, C>& p) {
  typedef E<C, SX_T> T;
  typedef E<C, SX_F> F;
  if (p.inf) return p;
  const T A = el_sqr<C>(p.X), B = el_sqr<C>(p.Y), Cc = el_sqr<C>(B);
  const F D = el_normf<C>(el_mulc<2, C>(el_sub<C>(el_sub<C>(el_sqr<C>(el_normf<C>(el_add<C>(p.X, B))), A), Cc)));
  const F Ee = el_normf<C>(el_mulc<3, C>(A));
  const T Ff = el_sqr<C>(Ee);
  JacE<E, C> r;
  r.X = el_normf<C>(el_sub<C>(Ff, el_mulc<2, C>(D)));
  r.Y = el_normf<C>(el_sub<C>(el_mul<C>(Ee, el_normf<C>(el_sub<C>(D, r.X))), el_mulc<2, C>(el_normf<C>(el_mulc<4, C>(Cc)))));
  r.Z = el_normf<C>(el_mulc<2, C>(el_mul<C>(p.Y, p.Z)));
  r.inf = false;
  return r;
}

// p + q, q affine (madd-2007-bl): 7 products + 4 squarings (over Fp2: 56 units of NL^2 multiplier instructions)
template <template <class, int> class E, class C>
BGLS_HD JacE<E, C> jace_madd(const JacE<E, C>& p, const AffE<E, C>& q) {
  typedef E<C, SX_T> T;
  typedef E<C, SX_F> F;
  if (q.inf) return p;
  if (p.inf) return jace_from_aff<E, C>(q);
  const T Z1Z1 = el_sqr<C>(p.Z);
  const T U2 = el_mul<C>(q.x, Z1Z1);
  const T S2 = el_mul<C>(el_mul<C>(q.y, p.Z), Z1Z1);
  const auto Hd = el_sub<C>(U2, p.X);
  const auto Rd = el_sub<C>(S2, p.Y);
  if (el_is_zero_wide<C>(Hd)) {                                // same x: P = Q (double) or P = -Q (infinity); p may be a doubling's
    if (el_is_zero_wide<C>(Rd)) return JacLaw<E, C>::dbl(p);   // output: X up to 9 p, Y down to -8 p
    return jace_inf<E, C>();
  }
  const F H = el_normf<C>(Hd);
  const F rr = el_normf<C>(el_mulc<2, C>(Rd));
  const T HH = el_sqr<C>(H);
  const F I = el_normf<C>(el_mulc<4, C>(HH));
  const T J = el_mul<C>(H, I);
  const T V = el_mul<C>(p.X, I);
  JacE<E, C> r;
  r.X = el_normf<C>(el_sub<C>(el_sub<C>(el_sqr<C>(rr), J), el_mulc<2, C>(V)));
  r.Y = el_as<SX_F, C>(el_mulsub<C>(rr, el_normf<C>(el_sub<C>(V, r.X)), el_mulc<2, C>(p.Y), J));
  r.Z = el_normf<C>(el_sub<C>(el_sub<C>(el_sqr<C>(el_normf<C>(el_add<C>(p.Z, H))), Z1Z1), HH));
  r.inf = false;
  return r;
}

// p + q, both Jacobian (add-2007-bl): 11 products + 5 squarings
template <template <class, int> class E, class C>
BGLS_HD JacE<E, C> jace_add(const JacE<E, C>& p, const JacE<E, C>& q) {
  typedef E<C, SX_T> T;
  typedef E<C, SX_F> F;
  if (q.inf) return p;
  if (p.inf) return q;
  const T Z1Z1 = el_sqr<C>(p.Z), Z2Z2 = el_sqr<C>(q.Z);
  const T U1 = el_mul<C>(p.X, Z2Z2), U2 = el_mul<C>(q.X, Z1Z1);
  const T S1 = el_mul<C>(el_mul<C>(p.Y, q.Z), Z2Z2), S2 = el_mul<C>(el_mul<C>(q.Y, p.Z), Z1Z1);
  const auto Hd = el_sub<C>(U2, U1);
  const auto Rd = el_sub<C>(S2, S1);
  if (el_is_zero<C>(Hd)) {                                     // same x: P = Q (double) or P = -Q (infinity)
    if (el_is_zero<C>(Rd)) return JacLaw<E, C>::dbl(p);
    return jace_inf<E, C>();
  }
  const F H = el_normf<C>(Hd);
  const F rr = el_normf<C>(el_mulc<2, C>(Rd));
  const F I = el_normf<C>(el_mulc<4, C>(el_sqr<C>(H)));
  const T J = el_mul<C>(H, I);
  const T V = el_mul<C>(U1, I);
  JacE<E, C> r;
  r.X = el_normf<C>(el_sub<C>(el_sub<C>(el_sqr<C>(rr), J), el_mulc<2, C>(V)));
  r.Y = el_as<SX_F, C>(el_mulsub<C>(rr, el_normf<C>(el_sub<C>(V, r.X)), el_mulc<2, C>(S1), J));
  r.Z = el_as<SX_F, C>(el_mul<C>(el_normf<C>(el_sub<C>(el_sub<C>(el_sqr<C>(el_normf<C>(el_add<C>(p.Z, q.Z))), Z1Z1), Z2Z2)), H));
  r.inf = false;
  return r;
}

// k * P for a per-lane scalar of up to 256 bits (k: eight little-endian words, nbits: the position of the top set bit + 1):
// curve.hpp's jac_mul_w4 (signed radix-16 digits against P .. 8P, four doublings and ONE general addition per window whatever
// the digit) on this arithmetic.  Same point as curve.hpp's jac_mul / jac_mul_w4.
template <template <class, int> class E, class C>
BGLS_HD JacE<E, C> jace_mul_w4(const AffE<E, C>& p, const u32* k, int nbits) {
  typedef JacLaw<E, C> L;
  if (p.inf || nbits <= 0) return jace_inf<E, C>();
  u32 w[9];
  const int nl = (nbits + 31) >> 5;
#pragma unroll
  for (int j = 0; j < 9; ++j) w[j] = j < nl && j < 8 ? k[j] : 0u;
  if (nbits & 31) w[nl - 1] &= (1u << (nbits & 31)) - 1u;
  JacE<E, C> tab[8];                               // tab[a - 1] = a P
  tab[0] = L::from_aff(p);
  tab[1] = L::dbl(tab[0]);
  tab[2] = L::madd(tab[1], p);
  tab[3] = L::dbl(tab[1]);
  tab[4] = L::madd(tab[3], p);
  tab[5] = L::dbl(tab[2]);
  tab[6] = L::madd(tab[5], p);
  tab[7] = L::dbl(tab[3]);
  const int nw = (nbits + 4) >> 2;                 // one bit above the scalar: the top window's sign bit is clear
  JacE<E, C> r = jace_inf<E, C>();
#pragma unroll 1
  for (int i = nw - 1; i >= 0; --i) {
    if (i != nw - 1) {
#pragma unroll 1
      for (int d = 0; d < 4; ++d) r = L::dbl(r);
    }
    const int val = w4_digit<true>(w, i);
    const int a = val < 0 ? -val : val;
    if (a) {
      JacE<E, C> q = tab[a - 1];
      if (val < 0) q.Y = el_negf<C>(q.Y);
      r = L::add(r, q);
    }
  }
  return r;
}

// ===================================================================================================== the twists, over Fp2
template <class C>
BGLS_HD JacX<C> jacx_inf() { return jace_inf<X2, C>(); }
template <class C>
BGLS_HD JacX<C> jacx_from_aff(const AffX<C>& q) {
  if (q.inf) return jacx_inf<C>();
  return jace_from_aff<X2, C>(q);
}
// the rare branch of the mixed addition (a key met twice in one thread's slice), every step of the chain
template <class C>
BGLS_FN JacX<C> jacx_dbl(const JacX<C>& p) { return jace_dbl<X2, C>(p); }
template <class C>
BGLS_HD JacX<C> jacx_madd(const JacX<C>& p, const AffX<C>& q) { return jace_madd<X2, C>(p, q); }
template <class C>
BGLS_FN JacX<C> jacx_add(const JacX<C>& p, const JacX<C>& q) { return jace_add<X2, C>(p, q); }
template <class C>
struct JacLaw<X2, C> {
  static BGLS_HD JacX<C> from_aff(const AffX<C>& q) { return jacx_from_aff<C>(q); }
  static BGLS_HD JacX<C> dbl(const JacX<C>& p) { return jacx_dbl<C>(p); }
  static BGLS_HD JacX<C> madd(const JacX<C>& p, const AffX<C>& q) { return jacx_madd<C>(p, q); }
  static BGLS_HD JacX<C> add(const JacX<C>& p, const JacX<C>& q) { return jacx_add<C>(p, q); }
};

// y^2 = x^3 + b' on the twist
template <class C>
BGLS_HD bool affx_on_curve(const AffX<C>& q) {
  if (q.inf) return true;
  const X2<C, SX_T> b2 = {sx_const<C>(C::RX_B2_RE), sx_const<C>(C::RX_B2_IM)};
  const X2<C, SX_T> x3 = x2_mul<C>(x2_sqr<C>(q.x), q.x);
  return el_is_zero<C>(el_sub<C>(x2_sqr<C>(q.y), el_add<C>(x3, b2)));
}
// wire bytes (x_im || x_re || y_im || y_re, big-endian; all zero = infinity) -> R' form; false when a coordinate is not canonical
template <class C>
BGLS_HD bool affx_from_bytes(AffX<C>& out, const uint8_t* b) {
  constexpr int N = C::FP_BYTES;
  const Fp<C> xi = fp_from_be<C>(b), xr = fp_from_be<C>(b + N), yi = fp_from_be<C>(b + 2 * N), yr = fp_from_be<C>(b + 3 * N);
  const bool ok = !fp_geq_p<C>(xi) && !fp_geq_p<C>(xr) && !fp_geq_p<C>(yi) && !fp_geq_p<C>(yr);
  out.inf = fp_is_zero<C>(xi) && fp_is_zero<C>(xr) && fp_is_zero<C>(yi) && fp_is_zero<C>(yr);
  out.x = {sx_from_plain<C>(xr), sx_from_plain<C>(xi)};
  out.y = {sx_from_plain<C>(yr), sx_from_plain<C>(yi)};
  return ok;
}
template <class C>
BGLS_HD AffX<C> affx_from_mont(const Aff<F2<C>>& a) {
  AffX<C> r;
  r.inf = a.inf;
  r.x = {sx_from_mont<C>(a.x.c0), sx_from_mont<C>(a.x.c1)};
  r.y = {sx_from_mont<C>(a.y.c0), sx_from_mont<C>(a.y.c1)};
  return r;
}
template <class C>
BGLS_HD Jac<F2<C>> jacx_to_mont(const JacX<C>& p) {
  Jac<F2<C>> r;
  if (p.inf) return jac_inf<F2<C>>();
  r.X = {sx_to_mont<C>(p.X.c0), sx_to_mont<C>(p.X.c1)};
  r.Y = {sx_to_mont<C>(p.Y.c0), sx_to_mont<C>(p.Y.c1)};
  r.Z = {sx_to_mont<C>(p.Z.c0), sx_to_mont<C>(p.Z.c1)};
  return r;
}

}  // namespace bgls
