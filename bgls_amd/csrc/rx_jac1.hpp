// G1 arithmetic on ONE lane in the carry-free 28-bit-limb form of rx.hpp (signed limbs, compile-time bounds): the scalar
// multiplications at the seam that work on G1 -- Sign = HashToG1(m).Mul(sk) (bgls/bgls.go:46-56), ScalePoints / Point.Mul
// on G1 (curves/curve.go:190-214), and the cofactor clearing inside BLS12-381's HashToG1 (curves/bls12_381.go:361-376).
//
// Why: these ran on curve.hpp's 32-bit Montgomery form -- three VALU instructions per multiplier instruction and dependent
// carry chains (k_scale_aff<BLS381, G1> 139 ms and k_bls_combine<false> 51 ms per 2^20 points in round 3).  Here a field
// product is NL^2 bare multiplier instructions into NL + 1 live columns plus NL^2 for its reduction (sx_montr), sums and
// differences are limb-wise, and a difference of two products shares one reduction.  The formulas and the chain are rx_jac.hpp's,
// the ones that serve the twists over Fp2, instantiated over Fp; exceptional cases (P = Q, P = -Q, infinity) are exact, so every
// chain gives the same POINT as curve.hpp's and, after normalisation, the same bytes.
#pragma once
#include "rx_jac.hpp"

namespace bgls {

template <class C> using Jac1 = JacE<Sx, C>;
template <class C> using Aff1 = AffE<Sx, C>;
template <class C>
BGLS_HD Jac1<C> jac1_inf() { return jace_inf<Sx, C>(); }
template <class C>
BGLS_HD Jac1<C> jac1_from_aff(const Aff1<C>& q) { return jace_from_aff<Sx, C>(q); }
template <class C>
BGLS_HD Jac1<C> jac1_dbl(const Jac1<C>& p) { return jace_dbl<Sx, C>(p); }
template <class C>
BGLS_HD Jac1<C> jac1_madd(const Jac1<C>& p, const Aff1<C>& q) { return jace_madd<Sx, C>(p, q); }
template <class C>
BGLS_HD Jac1<C> jac1_add(const Jac1<C>& p, const Jac1<C>& q) { return jace_add<Sx, C>(p, q); }
template <class C>
BGLS_FN Jac1<C> jac1_mul_w4(const Aff1<C>& p, const u32* k, int nbits) { return jace_mul_w4<Sx, C>(p, k, nbits); }
template <class C>
struct JacLaw<Sx, C> {
  static BGLS_HD Jac1<C> from_aff(const Aff1<C>& q) { return jac1_from_aff<C>(q); }
  static BGLS_HD Jac1<C> dbl(const Jac1<C>& p) { return jac1_dbl<C>(p); }
  static BGLS_HD Jac1<C> madd(const Jac1<C>& p, const Aff1<C>& q) { return jac1_madd<C>(p, q); }
  static BGLS_HD Jac1<C> add(const Jac1<C>& p, const Jac1<C>& q) { return jac1_add<C>(p, q); }
};

template <class C>
BGLS_HD Aff1<C> aff1_from_mont(const Aff<F1<C>>& a) {
  Aff1<C> r;
  r.inf = a.inf;
  r.x = sx_from_mont<C>(a.x);
  r.y = sx_from_mont<C>(a.y);
  return r;
}
template <class C>
BGLS_HD Aff1<C> aff1_neg(const Aff1<C>& a) {
  Aff1<C> r = a;
  r.y = sx_norm<C>(sx_neg<C>(a.y));          // limbs tight again, the sign sits in the top limb
  return r;
}
template <class C>
BGLS_HD Jac<F1<C>> jac1_to_mont(const Jac1<C>& p) {
  if (p.inf) return jac_inf<F1<C>>();
  return {sx_to_mont<C>(p.X), sx_to_mont<C>(p.Y), sx_to_mont<C>(p.Z)};
}

}  // namespace bgls
