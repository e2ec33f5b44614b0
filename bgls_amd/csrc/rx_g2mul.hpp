// Variable-base G2 scalar multiplication on ONE lane in the carry-free 28-bit-limb form (rx.hpp, rx_jac.hpp): the r V of a
// Boneh-Boyen verification (bbsigs/bbsigs.go:68-73, k_bbsigs.hip).  rx_jac.hpp has the doubling (dbl-2009-l) and the mixed
// addition (madd-2007-bl) of the G2 key sums; this header adds the general addition (add-2007-bl) and the windowed chain.
//
// Why: the only G2 scalar multiplication the library had is k_scale's jac_mul_w4 on curve.hpp's 32-bit Montgomery form, whose
// G2 additions run at about 0.24 of the multiplier peak (rx_jac.hpp's header).  Here it is rx_jac1.hpp's jac1_mul_w4 over Fp2:
// signed radix-16 digits against a table P .. 8P, four doublings and ONE general addition per window whatever the digit (the
// lanes of a wave hold different scalars: a fixed schedule is what a wave wants, curve.hpp's note on jac_mul_w4).
//
// Exactness: no endomorphism, no reduction of the scalar -- the 256-bit magnitude is walked bit for bit, so k P is the exact point
// for EVERY point on the twist, inside the order-r subgroup or not.  P = Q doubles, P = -Q and infinity are exact in both additions.
#pragma once
#include "rx_jac.hpp"

namespace bgls {

template <class C>
BGLS_HD JacX<C> jacx_from_aff(const AffX<C>& q) {
  if (q.inf) return jacx_inf<C>();
  JacX<C> r;
  r.X = x2_as<SX_F, C>(q.x);
  r.Y = x2_as<SX_F, C>(q.y);
  const Sx<C, SX_F> z = sx_as<SX_F, C>(ux_to_sx<C>(ux_zero<C>()));
  r.Z = {sx_as<SX_F, C>(sx_const<C>(C::RX_ONE)), z};
  r.inf = false;
  return r;
}

// p + q, both Jacobian (add-2007-bl): 11 products + 5 squarings over Fp2
template <class C>
BGLS_FN JacX<C> jacx_add(const JacX<C>& p, const JacX<C>& q) {
  if (q.inf) return p;
  if (p.inf) return q;
  const X2<C, SX_T> Z1Z1 = x2_sqr<C>(p.Z), Z2Z2 = x2_sqr<C>(q.Z);
  const X2<C, SX_T> U1 = x2_mul<C>(p.X, Z2Z2), U2 = x2_mul<C>(q.X, Z1Z1);
  const X2<C, SX_T> S1 = x2_mul<C>(x2_mul<C>(p.Y, q.Z), Z2Z2), S2 = x2_mul<C>(x2_mul<C>(q.Y, p.Z), Z1Z1);
  const auto Hd = x2_sub<C>(U2, U1);
  const auto Rd = x2_sub<C>(S2, S1);
  if (x2_is_zero<C>(Hd)) {                                     // same x: P = Q (double) or P = -Q (infinity)
    if (x2_is_zero<C>(Rd)) return jacx_dbl<C>(p);
    return jacx_inf<C>();
  }
  const X2<C, SX_F> H = x2_normf<C>(Hd);
  const X2<C, SX_F> rr = x2_normf<C>(x2_mulc<2, C>(Rd));
  const X2<C, SX_F> I = x2_normf<C>(x2_mulc<4, C>(x2_sqr<C>(H)));
  const X2<C, SX_T> J = x2_mul<C>(H, I);
  const X2<C, SX_T> V = x2_mul<C>(U1, I);
  JacX<C> r;
  r.X = x2_normf<C>(x2_sub<C>(x2_sub<C>(x2_sqr<C>(rr), J), x2_mulc<2, C>(V)));
  r.Y = x2_as<SX_F, C>(x2_mulsub<C>(rr, x2_normf<C>(x2_sub<C>(V, r.X)), x2_mulc<2, C>(S1), J));
  r.Z = x2_as<SX_F, C>(x2_mul<C>(x2_normf<C>(x2_sub<C>(x2_sub<C>(x2_sqr<C>(x2_normf<C>(x2_add<C>(p.Z, q.Z))), Z1Z1), Z2Z2)), H));
  r.inf = false;
  return r;
}

// k * P for a per-lane scalar of up to 256 bits (k: eight little-endian words, nbits: the position of the top set bit + 1):
// rx_jac1.hpp's jac1_mul_w4 over Fp2.  Same point as curve.hpp's jac_mul / jac_mul_w4.
template <class C>
BGLS_FN JacX<C> jacx_mul_w4(const AffX<C>& p, const u32* k, int nbits) {
  if (p.inf || nbits <= 0) return jacx_inf<C>();
  u32 w[9];
  const int nl = (nbits + 31) >> 5;
#pragma unroll
  for (int j = 0; j < 9; ++j) w[j] = j < nl && j < 8 ? k[j] : 0u;
  if (nbits & 31) w[nl - 1] &= (1u << (nbits & 31)) - 1u;
  JacX<C> tab[8];                                  // tab[a - 1] = a P
  tab[0] = jacx_from_aff<C>(p);
  tab[1] = jacx_dbl<C>(tab[0]);
  tab[2] = jacx_madd<C>(tab[1], p);
  tab[3] = jacx_dbl<C>(tab[1]);
  tab[4] = jacx_madd<C>(tab[3], p);
  tab[5] = jacx_dbl<C>(tab[2]);
  tab[6] = jacx_madd<C>(tab[5], p);
  tab[7] = jacx_dbl<C>(tab[3]);
  const int nw = (nbits + 4) >> 2;                 // one bit above the scalar: the top window's sign bit is clear
  JacX<C> r = jacx_inf<C>();
#pragma unroll 1
  for (int i = nw - 1; i >= 0; --i) {
    if (i != nw - 1) {
#pragma unroll 1
      for (int d = 0; d < 4; ++d) r = jacx_dbl<C>(r);
    }
    const int pos = 4 * i - 1;                     // bits pos .. pos + 4
    u32 b5;
    if (pos < 0) {
      b5 = (w[0] << 1) & 31u;
    } else {
      const int q = pos >> 5, sh = pos & 31;
      u32 lo = w[q] >> sh;
      if (sh > 27) lo |= w[q + 1 < 9 ? q + 1 : 8] << (32 - sh);
      b5 = lo & 31u;
    }
    const int mag = (int)(((b5 & 15u) + 1u) >> 1), neg8 = (int)(b5 >> 4) * 8;
    const int val = mag - neg8;
    const int a = val < 0 ? -val : val;
    if (a) {
      JacX<C> q = tab[a - 1];
      if (val < 0) q.Y = {sx_as<SX_F, C>(sx_norm<C>(sx_neg<C>(q.Y.c0))), sx_as<SX_F, C>(sx_norm<C>(sx_neg<C>(q.Y.c1)))};
      r = jacx_add<C>(r, q);
    }
  }
  return r;
}

}  // namespace bgls
