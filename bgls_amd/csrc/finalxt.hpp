// Throughput-oriented final exponentiation on the carry-free 28-bit limbs (rx.hpp, the forms and bounds of finalx.hpp): MANY
// independent Fp12 values per wave, no block barrier anywhere.
//
// finalx.hpp serves ONE value with 72 lanes of a four-wave block and a block barrier behind every stage of a product: right for the
// lone final exponentiation of a verification, ten times a Miller loop per item where a batch has one value per item.  Here a value
// belongs to a GROUP of six lanes, ten groups per wave (lanes 60..63 idle), the layout of the Miller consumer (coop.hpp, miller_x.hpp):
// lane j of a group owns coefficient e_j of f = sum e_j w^j, and it keeps its coefficient of EVERY temporary of the chain in registers
// (FxtK<C>::NT temporaries of 2 NL registers).  Only the operands of the product in flight go through LDS: the group's region holds
// the six coefficients of a (plain) and the six of b with their xi multiples, 18 Fp2 entries = 1728 B (alt-bn128) / 2304 B (BLS12-381)
// per group, 17 280 / 23 040 B per wave.  A lane computes its output coefficient as the six-term dot product
//     c_j = sum_t a_t b_(j-t)        (the xi multiple of b where the index wraps, w^6 = xi)
// two terms -- four limb products -- per interleaved reduction (sx_montr takes at most four), three reductions per half, added
// limb-wise and carry-normalised.  wave_sync() is the only ordering point: the DS unit runs a wave's accesses in order.
//
// The exponentiation itself is data: FxtK<C>::PROG (tools/gen_constants.py, where every value of the program is checked to be the input
// to a known exponent and the last one to be (p^12 - 1) / r) is a straight-line program over the temporaries, run by ONE loop, so the
// code holds one site of the product.  The operands of a step are picked out of the register file by wave-uniform compares.  Same
// chains as fx_final_exp with left-to-right powers; squarings are plain products (finalx.hpp's header says why Granger-Scott does not
// fit a redundant representation).  Conjugation and the Frobenius maps are lane-local; the one inversion per value is the norm chain
// of fx_inv, its Fp2 norm handed to all six lanes through the region's first entry and inverted on each of them (the lanes of a wave run
// the same instructions anyway).
//
// Magnitudes (units of p; finalx.hpp states the bounds its products accept: a coefficient below 6.1, its xi multiple below 61 on
// alt-bn128 / 12.2 on BLS12-381, limbs below the top one under 2^28 in magnitude).  A reduction of four products of such values leaves
// (T / R', T / R' + p) with T / R' below 2^-3 p, so a coefficient -- three of them -- lies in (-0.4, 3.4) and a published one, which
// may be a conjugate's, is below 3.4 in magnitude: inside 6.1, its xi multiple ((XI_RE + 1) times as much) inside 34 / 6.8.  The column budget of a four-product reduction, 4 x 256 units of 2^48 per row, is the
// one sx_montr asserts at compile time (MontAcc).  Conjugates are negated limb by limb (bound kept), Frobenius images and scaled
// values are single products (tight, below 1.01).
//
// The header compiles for the host (tests/harness/host_harness_fxt.cpp): the group's region is a policy M with ld / st / sync, LDS and
// wave_sync() in the kernel (k_finalxt.hip), an array and a barrier of six threads there, where BGLS_RX_CHECK checks every column
// accumulation and st checks the bounds above on every published entry.
#pragma once
#include "rx_jac.hpp"
#include "constants_latx_gen.hpp"
#include "constants_fxt_gen.hpp"

namespace bgls {

template <class C>
struct FXT {
  static constexpr int N = C::RX_NL;
  static constexpr int HS = (N + 3) & ~3;            // one half (Fp), 16-byte granules (as FX<C>)
  static constexpr int ES = 2 * HS;                  // one Fp2
  static constexpr int GROUPS = 10;
  static constexpr int GROUP_DW = 18 * ES;           // a: 6 plain entries; b: 6 x {plain, xi multiple}
  static constexpr int WAVE_DW = GROUPS * GROUP_DW;
  static constexpr int WAVE_BYTES = WAVE_DW * 4;
  // dword offsets of an entry's real half inside the group's region (the imaginary half HS behind it)
  BGLS_HD static int a_off(int t) { return t * ES; }
  BGLS_HD static int b_off(int k, int xi) { return (6 + 2 * k + xi) * ES; }
};

// this half of xi * (re + i im), carry-normalised (finalx.hpp fx_mulxi_half): the real half is XI_RE re - im, the imaginary half XI_RE im + re
template <class C, int LA>
BGLS_HD Sx<C, SX_T> fxt_mulxi_half(const Sx<C, LA>& mine, const Sx<C, LA>& other, bool is_im) {
  constexpr int N = C::RX_NL;
  const i32 sgn = is_im ? 1 : -1;
  Sx<C, SX_T> r;
  i64 c = 0;
#pragma unroll
  for (int i = 0; i < N - 1; ++i) {
    c += (i64)C::XI_RE * mine.v[i] + (i64)(sgn * other.v[i]);
    r.v[i] = (i32)((u32)c & RX_MASK);
    c >>= 28;
  }
  r.v[N - 1] = (i32)(c + (i64)C::XI_RE * mine.v[N - 1] + (i64)(sgn * other.v[N - 1]));
  return r;
}

template <class C, class M>
BGLS_HD X2<C, SX_T> fxt_ld2(M& m, int off) {
  return {m.ld(off), m.ld(off + FXT<C>::HS)};
}

// own coefficient j of the operands a and b into the group's region (pub == false: the lane stores nothing)
template <class C, class M>
BGLS_HD void fxt_publish(M& m, int j, bool pub, const X2<C, SX_T>& a, const X2<C, SX_T>& b) {
  typedef FXT<C> E;
  if (!pub) return;
  m.st(E::a_off(j), a.c0);
  m.st(E::a_off(j) + E::HS, a.c1);
  m.st(E::b_off(j, 0), b.c0);
  m.st(E::b_off(j, 0) + E::HS, b.c1);
  m.st(E::b_off(j, 1), fxt_mulxi_half<C>(b.c0, b.c1, false));
  m.st(E::b_off(j, 1) + E::HS, fxt_mulxi_half<C>(b.c1, b.c0, true));
}

// coefficient j of a * b from the published operands
template <class C, class M>
BGLS_HD X2<C, SX_T> fxt_dot(M& m, int j) {
  typedef FXT<C> E;
  constexpr int N = C::RX_NL;
  Sx<C, 3 * SX_T> re, im;
#pragma unroll
  for (int i = 0; i < N; ++i) re.v[i] = im.v[i] = 0;
#pragma unroll 1
  for (int u = 0; u < 3; ++u) {
    int k0 = j - 2 * u, k1 = j - 2 * u - 1;
    const int w0 = k0 < 0 ? 1 : 0, w1 = k1 < 0 ? 1 : 0;
    k0 += 6 * w0;
    k1 += 6 * w1;
    const X2<C, SX_T> x0 = fxt_ld2<C>(m, E::a_off(2 * u)), x1 = fxt_ld2<C>(m, E::a_off(2 * u + 1));
    const X2<C, SX_T> y0 = fxt_ld2<C>(m, E::b_off(k0, w0)), y1 = fxt_ld2<C>(m, E::b_off(k1, w1));
    {
      const i32* const cols[4] = {y0.c0.v, y0.c1.v, y1.c0.v, y1.c1.v};
      const Sx<C, SX_T> t = sx_montr<C, 4, 4 * SX_T * SX_T>(cols, [&](int q, int i) { return q == 0 ? x0.c0.v[i] : q == 1 ? -x0.c1.v[i] : q == 2 ? x1.c0.v[i] : -x1.c1.v[i]; });
#pragma unroll
      for (int i = 0; i < N; ++i) re.v[i] += t.v[i];
    }
    {
      const i32* const cols[4] = {y0.c1.v, y0.c0.v, y1.c1.v, y1.c0.v};
      const Sx<C, SX_T> t = sx_montr<C, 4, 4 * SX_T * SX_T>(cols, [&](int q, int i) { return q == 0 ? x0.c0.v[i] : q == 1 ? x0.c1.v[i] : q == 2 ? x1.c0.v[i] : x1.c1.v[i]; });
#pragma unroll
      for (int i = 0; i < N; ++i) im.v[i] += t.v[i];
    }
  }
  return {sx_norm<C>(re), sx_norm<C>(im)};
}

// 1 / d in Fp2 for the coefficient 0 of the group's value x (lane j == 0 holds it), on every lane of the group: conj(d) / (d0^2 + d1^2),
// the ONE Fp inversion in the library's 32-bit form, as fx_inv takes it.  0 gives 0.
template <class C, class M>
BGLS_HD X2<C, SX_T> fxt_invd(M& m, int j, bool pub, const X2<C, SX_T>& x) {
  typedef FXT<C> E;
  if (pub && j == 0) {
    m.st(E::a_off(0), x.c0);
    m.st(E::a_off(0) + E::HS, x.c1);
  }
  m.sync();
  const X2<C, SX_T> d = fxt_ld2<C>(m, E::a_off(0));
  m.sync();
  const X2<C, SX_T> dc = {d.c0, sx_norm<C>(sx_neg<C>(d.c1))};
  const X2<C, SX_T> nn = x2_mul<C>(d, dc);
  const Sx<C, SX_T> ni = sx_from_mont<C>(fp_inv<C>(sx_to_mont<C>(nn.c0)));
  return x2_mul<C>(dc, X2<C, SX_T>{ni, ux_to_sx<C>(ux_zero<C>())});
}

// T[reg] for a wave-uniform reg: NT compares, no indexed register access
template <class C>
BGLS_HD X2<C, SX_T> fxt_pick(const X2<C, SX_T> (&T)[FxtK<C>::NT], int reg) {
  X2<C, SX_T> r = T[0];
#pragma unroll
  for (int k = 1; k < FxtK<C>::NT; ++k)
    if (reg == k) r = T[k];
  return r;
}

// Runs a program (words as FxtK<C>::PROG) on the lane's coefficient j of its group's values: T[1] = y, every other temporary = x on entry,
// T[out_reg] on exit.  m: the group's region; pub: the lane stores into it.
template <class C, class M>
BGLS_HD X2<C, SX_T> fxt_run(M& m, int j, bool pub, const X2<C, SX_T>& x, const X2<C, SX_T>& y, const u32* prog, int len, int out_reg) {
  typedef FxtK<C> K;
  typedef X2<C, SX_T> V;
  constexpr int N = C::RX_NL;
  V T[K::NT];
#pragma unroll
  for (int k = 0; k < K::NT; ++k) T[k] = k == 1 ? y : x;
#pragma unroll 1
  for (int s = 0; s < len; ++s) {
    const u32 w = prog[s];
    const int op = w & 15, dst = (w >> 4) & 15, ra = (w >> 8) & 15, rb = (w >> 12) & 15;
    const V a = fxt_pick<C>(T, ra);
    V r;
    if (op == FXT_MUL) {
      const V b = fxt_pick<C>(T, rb);
      fxt_publish<C>(m, j, pub, a, b);
      m.sync();
      r = fxt_dot<C>(m, j);
      m.sync();
    } else if (op == FXT_CONJ) {
      r = a;
      if (j & 1) {
        r.c0 = sx_neg<C>(a.c0);
        r.c1 = sx_neg<C>(a.c1);
      }
    } else if (op == FXT_FROB) {
      r = a;
      if (rb & 1) r.c1 = sx_neg<C>(a.c1);
      const u32* g = LatxK<C>::FROB_GAMMA + ((rb - 1) * 6 + j) * 2 * N;      // gamma_kk[j] in this form; gamma[0] = 1
      const V gx = {sx_const<C>(g), sx_const<C>(g + N)};
      const V mm = x2_mul<C>(r, gx);
      if (j != 0) r = mm;
    } else if (op == FXT_INVD) {
      r = fxt_invd<C>(m, j, pub, a);
    } else {
      r = x2_mul<C>(a, fxt_pick<C>(T, rb));
    }
#pragma unroll
    for (int k = 0; k < K::NT; ++k)
      if (dst == k) T[k] = r;
  }
  return fxt_pick<C>(T, out_reg);
}

// x <- x^((p^12 - 1) / r)
template <class C, class M>
BGLS_HD X2<C, SX_T> fxt_final_exp(M& m, int j, bool pub, const X2<C, SX_T>& x) {
  return fxt_run<C>(m, j, pub, x, x, FxtK<C>::PROG, FxtK<C>::PROG_LEN, FxtK<C>::OUT_REG);
}

}  // namespace bgls
