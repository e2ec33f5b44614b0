// One set of a combined multi-signature check (bgls_verify_multi_sets_combined), on one lane: the pair (r H, r sigma) for the set's
// hash point H, its signature sigma and its 128-bit coefficient r, both as affine Montgomery points.
//
// The two multiplications are ONE walk: the signed radix-16 digits of r (curve.hpp's jac_mul_w4 recoding: four doublings and one
// general addition per window whatever the digit) are taken once per window and applied to both running points against their own
// tables P .. 8P.  The walk has a fixed length (33 windows: the coefficients are 128-bit values, and the lanes of a wave run the union
// of their paths anyway); windows above the scalar's top digit leave the running points at infinity.  The two Jacobian results go to
// affine through ONE field inversion: (Z1 Z2)^-1, then Z1^-1 = (Z1 Z2)^-1 Z2 and Z2^-1 = (Z1 Z2)^-1 Z1 -- three products more than one
// conversion instead of a second Fermat inversion.  A result at infinity (an input at infinity, or r P = infinity on a point of small
// order) enters the shared product as one, so it cannot poison the other point.
// Field arithmetic as the finding in k_g1x.hip's header has it: BLS12-381 on the carry-free limbs (rx_jac1.hpp), alt-bn128's G1 on the
// 32-bit Montgomery limbs (curve.hpp).  The group law is exact in both (P = Q, P = -Q, infinity), so the points are those of k (x) P.
#pragma once
#include "curve.hpp"
#include "rx_jac1.hpp"

namespace bgls {

// the point layer under the walk
template <class C, bool CARRY_FREE = (C::CURVE_ID == 1)>
struct RlcPt;
template <class C>
struct RlcPt<C, false> {
  typedef F1<C> F;
  typedef Jac<F> J;
  static BGLS_HD J inf() { return jac_inf<F>(); }
  static BGLS_HD J from_aff(const Aff<F>& p) { return jac_from_aff<F>(p); }
  static BGLS_HD J dbl(const J& p) { return jac_dbl<F>(p); }
  static BGLS_HD J madd(const J& p, const Aff<F>& q) { return jac_add_aff<F>(p, q); }
  static BGLS_HD J add(const J& p, const J& q) { return jac_add<F>(p, q); }
  static BGLS_HD void negate(J& q) { q.Y = F::neg(q.Y); }
  static BGLS_HD Jac<F> to_mont(const J& p) { return p; }
};
template <class C>
struct RlcPt<C, true> {
  typedef F1<C> F;
  typedef Jac1<C> J;
  static BGLS_HD J inf() { return jac1_inf<C>(); }
  static BGLS_HD J from_aff(const Aff<F>& p) { return jac1_from_aff<C>(aff1_from_mont<C>(p)); }
  static BGLS_HD J dbl(const J& p) { return jac1_dbl<C>(p); }
  static BGLS_HD J madd(const J& p, const Aff<F>& q) { return jac1_madd<C>(p, aff1_from_mont<C>(q)); }
  static BGLS_HD J add(const J& p, const J& q) { return jac1_add<C>(p, q); }
  static BGLS_HD void negate(J& q) { q.Y = el_negf<C>(q.Y); }
  static BGLS_HD Jac<F> to_mont(const J& p) { return jac1_to_mont<C>(p); }
};

// r as four little-endian words from its 16 big-endian bytes, the lowest bit set (bgls_rlc_coefficients: never zero)
BGLS_HD void rlc_scalar(const uint8_t* r16, u32 (&k)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint8_t* q = r16 + 4 * (3 - j);
    k[j] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
  }
  k[0] |= 1u;
}

// out[t] = k * p[t] for t = 0, 1 (Jacobian, Montgomery form; Z = 0 at infinity)
template <class C>
BGLS_FN void rlc_mul2(const Aff<F1<C>> (&p)[2], const u32 (&k)[4], Jac<F1<C>> (&out)[2]) {
  typedef RlcPt<C> P;
  typedef typename P::J J;
  J tab[2][8];                                     // tab[t][a - 1] = a p[t]
  J acc[2];
#pragma unroll 1
  for (int t = 0; t < 2; ++t) {
    J* T = tab[t];
    T[0] = P::from_aff(p[t]);
    T[1] = P::dbl(T[0]);
    T[2] = P::madd(T[1], p[t]);
    T[3] = P::dbl(T[1]);
    T[4] = P::madd(T[3], p[t]);
    T[5] = P::dbl(T[2]);
    T[6] = P::madd(T[5], p[t]);
    T[7] = P::dbl(T[3]);
    acc[t] = P::inf();
  }
#pragma unroll 1
  for (int i = 32; i >= 0; --i) {
    const int val = w4_digit<false>(k, i);         // one decomposition for both points; bits above word 3 read as zero
    const int a = val < 0 ? -val : val;
#pragma unroll 1
    for (int t = 0; t < 2; ++t) {
      J r = acc[t];
      if (i != 32) {
#pragma unroll 1
        for (int d = 0; d < 4; ++d) r = P::dbl(r);
      }
      if (a) {
        J q = tab[t][a - 1];
        if (val < 0) P::negate(q);
        r = P::add(r, q);
      }
      acc[t] = r;
    }
  }
  out[0] = P::to_mont(acc[0]);
  out[1] = P::to_mont(acc[1]);
}

// both Jacobian points to affine through one inversion
template <class C>
BGLS_FN void rlc_to_aff2(const Jac<F1<C>> (&j)[2], Aff<F1<C>> (&out)[2]) {
  typedef F1<C> F;
  typedef typename F::T T;
  const bool i0 = F::is_zero(j[0].Z), i1 = F::is_zero(j[1].Z);
  const T z0 = F::select(i0, F::one(), j[0].Z), z1 = F::select(i1, F::one(), j[1].Z);
  const T ti = F::inv(F::mul(z0, z1));
  const T zi[2] = {F::mul(ti, z1), F::mul(ti, z0)};
  const bool inf[2] = {i0, i1};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const T zi2 = F::sqr(zi[t]);
    out[t].x = F::select(inf[t], F::zero(), F::mul(j[t].X, zi2));
    out[t].y = F::select(inf[t], F::zero(), F::mul(F::mul(j[t].Y, zi2), zi[t]));
    out[t].inf = inf[t];
  }
}

// (r H, r sigma): p = {H, sigma} in, out = {r H, r sigma}
template <class C>
BGLS_HD void rlc_pair(const Aff<F1<C>> (&p)[2], const u32 (&k)[4], Aff<F1<C>> (&out)[2]) {
  Jac<F1<C>> j[2];
  rlc_mul2<C>(p, k, j);
  rlc_to_aff2<C>(j, out);
}

}  // namespace bgls
