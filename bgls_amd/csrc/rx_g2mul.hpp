// Variable-base G2 scalar multiplication on ONE lane in the carry-free 28-bit-limb form (rx.hpp, rx_jac.hpp): the r V of a
// Boneh-Boyen verification (bbsigs/bbsigs.go:68-73, k_bbsigs.hip), on rx_jac.hpp's doubling, additions and windowed chain over Fp2.
//
// Why: the only G2 scalar multiplication the library had is k_scale's jac_mul_w4 on curve.hpp's 32-bit Montgomery form, whose
// G2 additions run at about 0.24 of the multiplier peak (rx_jac.hpp's header).  Here it is the chain that G1 runs (rx_jac1.hpp):
// signed radix-16 digits against a table P .. 8P, four doublings and ONE general addition per window whatever the digit (the
// lanes of a wave hold different scalars: a fixed schedule is what a wave wants, curve.hpp's note on jac_mul_w4).
//
// Exactness: no endomorphism, no reduction of the scalar -- the 256-bit magnitude is walked bit for bit, so k P is the exact point
// for EVERY point on the twist, inside the order-r subgroup or not.  P = Q doubles, P = -Q and infinity are exact in both additions.
#pragma once
#include "rx_jac.hpp"

namespace bgls {

// k * P for a per-lane scalar of up to 256 bits (k: eight little-endian words, nbits: the position of the top set bit + 1).
// Same point as curve.hpp's jac_mul / jac_mul_w4.
template <class C>
BGLS_FN JacX<C> jacx_mul_w4(const AffX<C>& p, const u32* k, int nbits) { return jace_mul_w4<X2, C>(p, k, nbits); }

}  // namespace bgls
