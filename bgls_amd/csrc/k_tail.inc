// Serial tails of a verification: generator line table, reduction of the per-group partial products, the 36-lane
// final exponentiation and the cofactor / signature-pair epilogue.
#include "dev_common.hpp"
#include "coop.hpp"
#include "finalexp.hpp"
#include "miller_kernels.hpp"
#include "launch.hpp"

using namespace bgls;

// ---- fixed-argument lines of the generator --------------------------------------------------------------
// The (-sigma, g2) pair of every verification has Q = GetG2(), a curve constant (curves/altbn128.go:427-429,
// curves/bls12_381.go:279-281): its point steps do not depend on the input, only the scaling of the line
// by P = -sigma does.  k_gen_lines walks the Miller loop of g2 once per context and stores the unscaled
// coefficients of every step.
template <class C>
__global__ void k_gen_lines(LineCoeffs<C>* table, int* nsteps) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Fp2<C> qx = f2_load<C>(C::G2), qy = f2_load<C>(C::G2 + 2 * C::L);
  G2Proj<C> T = {qx, qy, f2_one<C>()};
  const Fp2<C> nyq = f2_neg<C>(qy);
  int s = 0;
  for (int i = 1; i < C::LOOP_LEN; ++i) {
    table[s++] = dbl_step<C>(T);
    const int d = C::LOOP_NAF[i];
    if (d != 0) table[s++] = add_step<C>(T, qx, d > 0 ? qy : nyq);
  }
  if constexpr (C::CURVE_ID == 0) {
    Fp2<C> x1 = f2_mul<C>(f2_conj<C>(qx), gamma_const<C>(1, 2));
    Fp2<C> y1 = f2_mul<C>(f2_conj<C>(qy), gamma_const<C>(1, 3));
    Fp2<C> x2 = f2_mul<C>(qx, gamma_const<C>(2, 2));
    Fp2<C> y2 = f2_neg<C>(f2_mul<C>(qy, gamma_const<C>(2, 3)));
    table[s++] = add_step<C>(T, x1, y1);
    table[s++] = add_step<C>(T, x2, y2);
  }
  *nsteps = s;
}

// out[G] = prod in[G*R .. min(count, (G+1)*R))   (w-basis Fp12 arrays)
template <class C>
__global__ void __launch_bounds__(64) k_reduce_coop(const Fp2<C>* in, size_t count, int R, Fp2<C>* out) {
  typedef Coop<C> K;
  CoopLane<C> ln;
  const int j = ln.j, gb = ln.gb;
  const bool live = ln.live;
  const size_t G = (size_t)blockIdx.x * K::GROUPS + ln.g;
  const size_t lo = G * (size_t)R;
  const bool has = lo < count;
  const size_t hi = lo + R < count ? lo + R : count;
  Fp2<C> acc = has ? in[lo * 6 + j] : (j == 0 ? f2_one<C>() : f2_zero<C>());
#pragma unroll 1
  for (int t = 1; t < R; ++t) {                           // uniform trip count; missing operands are 1
    coop_publish<C>(gb + K::RB, j, acc, live);
    const size_t k = lo + t;
    Fp2<C> x = (has && k < hi) ? in[k * 6 + j] : (j == 0 ? f2_one<C>() : f2_zero<C>());
    acc = coop_mul<C>(gb, j, x, live);
  }
  if (live && has) out[G * 6 + j] = acc;
}
// segmented form (bgls_verify_aggregate_batch): out[G] = prod in[seg[2G] .. seg[2G] + seg[2G + 1]) for G < nout, 0 .. R operands; an empty
// segment gives one.  seg: the host's per-pass table (engine_core.inc Engine::reduce_seg).
template <class C>
__global__ void __launch_bounds__(64) k_reduce_coop_seg(const Fp2<C>* in, const uint32_t* seg, size_t nout, int R, Fp2<C>* out) {
  typedef Coop<C> K;
  CoopLane<C> ln;
  const int j = ln.j, gb = ln.gb;
  const bool live = ln.live;
  const size_t G = (size_t)blockIdx.x * K::GROUPS + ln.g;
  const bool has = G < nout;
  const size_t lo = has ? seg[2 * G] : 0;
  const int cnt = has ? (int)seg[2 * G + 1] : 0;
  Fp2<C> acc = cnt > 0 ? in[lo * 6 + j] : (j == 0 ? f2_one<C>() : f2_zero<C>());
#pragma unroll 1
  for (int t = 1; t < R; ++t) {                           // uniform trip count; missing operands are 1
    coop_publish<C>(gb + K::RB, j, acc, live);
    Fp2<C> x = t < cnt ? in[(lo + t) * 6 + j] : (j == 0 ? f2_one<C>() : f2_zero<C>());
    acc = coop_mul<C>(gb, j, x, live);
  }
  if (live && has) out[G * 6 + j] = acc;
}

template <class C>
__global__ void k_w_to_bytes(const Fp2<C>* in, uint8_t* out) {
  const int t = threadIdx.x;
  if (blockIdx.x != 0 || t >= 6) return;
  const int order[6] = {5, 3, 1, 4, 2, 0};                 // h.a2 h.a1 h.a0 g.a2 g.a1 g.a0
  Fp2<C> e = in[order[t]];
  fp_to_be<C>(out + (2 * t) * C::FP_BYTES, fp_from_mont<C>(e.c1));
  fp_to_be<C>(out + (2 * t + 1) * C::FP_BYTES, fp_from_mont<C>(e.c0));
}

// product of `count` serialised partials -> final exponentiation on 36 lanes (finalexp.hpp)
template <class C>
__global__ void __launch_bounds__(64) k_final36(const uint8_t* partials, size_t count, int do_final_exp, uint8_t* gt_out,
                                                uint32_t* verdict, uint32_t* flags) {
  typedef FE<C> E;
  const int lane = threadIdx.x;
  const int order_pos[6] = {5, 2, 4, 1, 3, 0};
  for (size_t k = 0; k < count; ++k) {
    if (lane < 6) {
      const uint8_t* b = partials + k * 12 * C::FP_BYTES + (size_t)(2 * order_pos[lane]) * C::FP_BYTES;
      Fp<C> im = fp_from_be<C>(b), re = fp_from_be<C>(b + C::FP_BYTES);
      if (fp_geq_p<C>(im) || fp_geq_p<C>(re)) atomicOr(flags, FLAG_ENC);
      fe_put<C>(k == 0 ? FE_F : FE_X, lane, Fp2<C>{fp_to_mont<C>(re), fp_to_mont<C>(im)});
    }
    wave_sync();
    if (k > 0) fe_mul<C>(FE_F, FE_F, FE_X);
  }
  if (do_final_exp) fe_final_exp<C>();
  bool is_one = true;
  if (lane < 6) {
    Fp2<C> v = lds_load_f2<C>(E::coef(FE_F, lane, 0));
    is_one = lane == 0 ? f2_eq<C>(v, f2_one<C>()) : f2_is_zero<C>(v);
    if (gt_out) {
      uint8_t* o = gt_out + (size_t)(2 * order_pos[lane]) * C::FP_BYTES;
      fp_to_be<C>(o, fp_from_mont<C>(v.c1));
      fp_to_be<C>(o + C::FP_BYTES, fp_from_mont<C>(v.c0));
    }
  }
  const unsigned long long ball = __ballot(is_one);
  if (lane == 0) verdict[0] = (ball == ~0ull) ? 1u : 0u;
}

// PointT.Mul (curves/altbn128.go:273-281, curves/bls12_381.go:170-173): gt^k for a 256-bit big-endian magnitude k on the
// 36-lane arithmetic; negate = 1 returns the inverse power, taken as the conjugate (GT elements are unitary: they come out
// of the final exponentiation).
template <class C>
__global__ void __launch_bounds__(64) k_gt_pow(const uint8_t* gt_in, const uint8_t* k_be32, int negate, uint8_t* gt_out, uint32_t* flags) {
  typedef FE<C> E;
  const int lane = threadIdx.x;
  const int order_pos[6] = {5, 2, 4, 1, 3, 0};
  if (lane < 6) {
    const uint8_t* b = gt_in + (size_t)(2 * order_pos[lane]) * C::FP_BYTES;
    Fp<C> im = fp_from_be<C>(b), re = fp_from_be<C>(b + C::FP_BYTES);
    if (fp_geq_p<C>(im) || fp_geq_p<C>(re)) atomicOr(flags, FLAG_ENC);
    fe_put<C>(FE_X, lane, Fp2<C>{fp_to_mont<C>(re), fp_to_mont<C>(im)});
    fe_put<C>(FE_F, lane, lane == 0 ? f2_one<C>() : f2_zero<C>());
  }
  wave_sync();
  bool started = false;                                  // uniform
  for (int i = 255; i >= 0; --i) {
    const int bit = (k_be32[31 - (i >> 3)] >> (i & 7)) & 1;
    if (started) fe_mul<C>(FE_F, FE_F, FE_F);
    if (bit) {
      fe_mul<C>(FE_F, FE_F, FE_X);
      started = true;
    }
  }
  if (negate) fe_conj<C>(FE_F, FE_F);
  if (lane < 6) {
    Fp2<C> v = lds_load_f2<C>(E::coef(FE_F, lane, 0));
    uint8_t* o = gt_out + (size_t)(2 * order_pos[lane]) * C::FP_BYTES;
    fp_to_be<C>(o, fp_from_mont<C>(v.c1));
    fp_to_be<C>(o + C::FP_BYTES, fp_from_mont<C>(v.c0));
  }
}


// ---- latency form of the Miller loop: ONE pairing per block ---------------------------------------------------------------
// The batch kernels (k_miller_ab64 / s60) run 64 point steps per wave, one per lane: a step takes a lane ~14 dependent Fp2
// products (45-50 us on a lone wave) whatever the batch size, so a handful of pairings -- the two-pairing tail of
// verifyMultiSignature (bgls/bgls.go:59-70,89-92), the reference's own n = 64 benchmark shape -- costs 88 x 52 us = 4.6 ms.
// Here a block is one pairing: wave 1 spreads the point step over five lanes (the step's products are three to four rounds
// of independent multiplications: one product per lane and round, operands exchanged through LDS), wave 0 keeps the Fp12
// accumulator on the 36-lane arithmetic of finalexp.hpp (one product deep + a reduction tree per multiplication) and folds
// the line of step s while wave 1 computes step s + 1.  Block `n` (when sig_at >= 0) is the (-sigma, g2) pair on the
// pre-computed generator lines.  out: one w-basis Fp12 (6 Fp2) per block.
template <class C>
__global__ void __launch_bounds__(128) k_miller_lat(const Aff<F1<C>>* g1s, const uint8_t* g2s, size_t n, long long sig_at,
                                                    const LineCoeffs<C>* gen_lines, Fp2<C>* out, uint32_t* flags) {
  typedef FE<C> E;
  extern __shared__ u32 lds[];
  constexpr int S2 = E::S2;
  enum { S_F = 0, S_L0 = 2, S_L1 = 3, S_PA = 4, S_PB = 5 };           // accumulator, two line buffers, producer scratch (2 x 12 Fp2)
  enum { PX = 0, PY, PZ, PQX, PQY, PB, PC, PS, PJ, PM, PE, PZN, PXN, PG, PE2, PT0, PT1, PU0, PU1, PD, PGG, PV0, PV1, PN };   // Fp2 entries of the scratch
  static_assert(PN <= 24, "producer scratch fits two slots");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t blk = blockIdx.x;
  const bool is_sig = sig_at >= 0 && blk == n;
  const int pbase = E::coef(S_PA, 0, 0);
  auto LD = [&](int e) { return lds_load_f2<C>(pbase + e * S2); };
  auto ST = [&](int e, const Fp2<C>& v) { lds_store_f2<C>(pbase + e * S2, v); };
  // line coefficients of a step into line buffer `buf`: D-type  k = 0: c0 yP, 1: c1 xP, 3: c2;  M-type  0: c2, 2: c1 xP, 3: c0 yP
  auto put_line = [&](int buf, int which, const Fp2<C>& v) {
    const int k = which == 0 ? (C::TWIST_D ? 0 : 3) : which == 1 ? (C::TWIST_D ? 1 : 2) : (C::TWIST_D ? 3 : 0);
    fe_put<C>(buf ? S_L1 : S_L0, k, v);
  };
  __shared__ int s_valid;
  if (wave == 0) {
    if (lane < 6) {
      fe_put<C>(S_F, lane, lane == 0 ? f2_one<C>() : f2_zero<C>());
      fe_put<C>(S_L0, lane, f2_zero<C>());
      fe_put<C>(S_L1, lane, f2_zero<C>());
    }
  } else if (lane == 0) {
    // parse this block's pair (block n: -sigma against the generator)
    bool valid = true;
    Aff<F1<C>> P = g1s[is_sig ? (size_t)sig_at : blk];
    Aff<F2<C>> Q;
    if (is_sig) {
      Q.x = f2_load<C>(C::G2);
      Q.y = f2_load<C>(C::G2 + 2 * C::L);
      Q.inf = false;
    } else {
      bool ok = g2_from_bytes<C>(Q, g2s + blk * 4 * C::FP_BYTES);
      ok = ok && aff_on_curve<F2<C>>(Q);
      if (!ok) atomicOr(flags, FLAG_ENC);
    }
    valid = !P.inf && !Q.inf;
    if (!valid) {
      Q.x = f2_load<C>(C::G2);
      Q.y = f2_load<C>(C::G2 + 2 * C::L);
      P.x = fp_load<C>(C::G1X);
      P.y = fp_load<C>(C::G1Y);
    }
    ST(PX, Q.x); ST(PY, Q.y); ST(PZ, f2_one<C>());
    ST(PQX, Q.x); ST(PQY, Q.y);
    ST(PT0, Fp2<C>{P.x, fp_zero<C>()});                      // xP, yP as Fp2 operands of the scaling products
    ST(PT1, Fp2<C>{P.y, fp_zero<C>()});
    s_valid = valid ? 1 : 0;
  }
  __syncthreads();
  const bool valid = s_valid != 0;
  if (wave == 1) {
    // ------------------------------------------------ producer: cooperative point steps, or generator lines
    // Product q of a round sits on lanes 4q .. 4q+2: lane 4q+k multiplies piece k of the Karatsuba triple (a0 b0, a1 b1,
    // (a0+a1)(b0+b1)) in double width, the triple is exchanged with lane shuffles, lane 4q reduces the real part and lane
    // 4q+1 the imaginary part (the SAME instruction stream on every lane: operand selects, no divergent branches) and each
    // stores its half.  One wide product and one reduction deep per round instead of three and two.
    constexpr int W = E::W, L = C::L;
    const Fp2<C> xP = LD(PT0), yP = LD(PT1);
    const int q = lane >> 2, piece = lane & 3;
    int buf = 0, step = 0;
    auto mulp = [&](const Fp2<C>& a, const Fp2<C>& b) -> Fp<C> {
      const Fp<C> x = piece == 0 ? a.c0 : piece == 1 ? a.c1 : fp_add_nr<C>(a.c0, a.c1);
      const Fp<C> y = piece == 0 ? b.c0 : piece == 1 ? b.c1 : fp_add_nr<C>(b.c0, b.c1);
      u32 w[W], v0[W], v1[W], sw[W], tmp[W];
      mul_wide<C>(w, x.v, y.v);
      const int base = lane & ~3;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        v0[k] = __shfl(w[k], base);
        v1[k] = __shfl(w[k], base + 1);
        sw[k] = __shfl(w[k], base + 2);
      }
      // uniform form R = X + K - V:  real: v0 + 6 p^2 - v1      imaginary: s + 0 - (v0 + v1)
      const u32 m0 = piece == 0 ? 0xFFFFFFFFu : 0u;
      u32 X[W], V[W];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        X[k] = (v0[k] & m0) | (sw[k] & ~m0);
        tmp[k] = v0[k] & ~m0;
      }
      w_add<W>(V, v1, tmp);
#pragma unroll
      for (int k = 0; k < W; ++k) tmp[k] = C::P2W6[k] & m0;
      w_add<W>(X, X, tmp);
      w_sub<W>(X, X, V);
      return redc_k<C, E::LAZY_K>(X);
    };
    auto st_half = [&](int off, const Fp<C>& r, bool active) {           // this lane's half of the Fp2 at dword offset off
      if (active && piece < 2) {
        u32* o = lds + off + piece * L;
#pragma unroll
        for (int k = 0; k < L; ++k) o[k] = r.v[k];
      }
    };
    auto put_line_h = [&](int bf, int which, const Fp<C>& r, bool active) {
      const int k = which == 0 ? (C::TWIST_D ? 0 : 3) : which == 1 ? (C::TWIST_D ? 1 : 2) : (C::TWIST_D ? 3 : 0);
      const Fp<C> z = mulxi_half<C>(r, piece == 1);
      st_half(E::coef(bf ? S_L1 : S_L0, k, 0), r, active);
      st_half(E::coef(bf ? S_L1 : S_L0, k, 1), z, active);
    };
    auto publish = [&]() {                                    // line of this step is in the buffer: hand it over
      ++step;
      __syncthreads();
      buf ^= 1;
    };
    auto gen_step = [&]() {                                   // (-sigma, g2): scale the pre-computed coefficients
      const LineCoeffs<C> l = gen_lines[step];
      const Fp<C> r = mulp(q == 0 ? l.c0 : l.c1, q == 0 ? yP : xP);
      put_line_h(buf, q == 0 ? 0 : 1, r, q < 2);
      if (lane == 8) put_line(buf, 2, l.c2);
      publish();
    };
    auto dbl_step = [&]() {
      const Fp2<C> X = LD(PX), Y = LD(PY), Z = LD(PZ);
      {   // round 1: B = Y^2, C = Z^2, S = (Y+Z)^2, J = X^2, M = X Y
        Fp2<C> a = q == 0 ? Y : q == 1 ? Z : q == 2 ? f2_add<C>(Y, Z) : X;
        Fp2<C> b = q == 3 ? X : q == 4 ? Y : a;
        const int dst = q == 0 ? PB : q == 1 ? PC : q == 2 ? PS : q == 3 ? PJ : PM;
        const Fp<C> r = mulp(a, b);
        st_half(pbase + dst * S2, r, q < 5);
        wave_sync();
      }
      const Fp2<C> B = LD(PB), Cc = LD(PC);
      const Fp2<C> H = f2_sub<C>(LD(PS), f2_add<C>(B, Cc));
      {   // round 2: E = 3b' C (alt-bn128: a product; BLS12-381: additions), ZN = B H, line c1 xP = 3J xP, line c0 yP = -H yP
        Fp2<C> a, b;
        if (q == 0) { a = {fp_load<C>(C::B2X3_RE), fp_load<C>(C::B2X3_IM)}; b = Cc; }
        else if (q == 1) { a = B; b = H; }
        else if (q == 2) { a = f2_mul3<C>(LD(PJ)); b = xP; }
        else { a = f2_neg<C>(H); b = yP; }
        const Fp<C> r = mulp(a, b);
        if constexpr (!C::TWIST_D && C::XI_RE == 1) {
          if (lane == 0) ST(PE, f2_mul_3b<C, true>(Cc));
        } else {
          st_half(pbase + PE * S2, r, q == 0);
        }
        st_half(pbase + PZN * S2, r, q == 1);
        put_line_h(buf, q == 2 ? 1 : 0, r, q == 2 || q == 3);
        wave_sync();
      }
      const Fp2<C> Ev = LD(PE);
      const Fp2<C> Fv = f2_mul3<C>(Ev);
      {   // round 3: XN = (M/2)(B - Fv), G^2 with G = (B + Fv)/2, E^2
        Fp2<C> a = q == 0 ? f2_half<C>(LD(PM)) : q == 1 ? f2_half<C>(f2_add<C>(B, Fv)) : Ev;
        Fp2<C> b = q == 0 ? f2_sub<C>(B, Fv) : a;
        const int dst = q == 0 ? PXN : q == 1 ? PG : PE2;
        const Fp<C> r = mulp(a, b);
        st_half(pbase + dst * S2, r, q < 3);
        wave_sync();
      }
      if (lane == 0) {
        ST(PX, LD(PXN));
        ST(PZ, LD(PZN));
        ST(PY, f2_sub<C>(LD(PG), f2_mul3<C>(LD(PE2))));
        put_line(buf, 2, f2_sub<C>(Ev, B));
      }
      wave_sync();
      publish();
    };
    auto add_step = [&](const Fp2<C>& xq, const Fp2<C>& yq) {
      const Fp2<C> X = LD(PX), Y = LD(PY), Z = LD(PZ);
      {   // round 1: yq Z, xq Z
        const Fp<C> r = mulp(q == 0 ? yq : xq, Z);
        st_half(pbase + (q == 0 ? PU0 : PU1) * S2, r, q < 2);
        wave_sync();
      }
      const Fp2<C> th = f2_sub<C>(Y, LD(PU0)), la = f2_sub<C>(X, LD(PU1));
      {   // round 2: C = th^2, D = la^2, th xq, la yq, line c0 yP = la yP
        Fp2<C> a = (q == 0 || q == 2) ? th : la;
        Fp2<C> b = q == 0 ? th : q == 1 ? la : q == 2 ? xq : q == 3 ? yq : yP;
        const Fp<C> r = mulp(a, b);
        const int dst = q == 0 ? PC : q == 1 ? PD : q == 2 ? PV0 : PV1;
        st_half(pbase + dst * S2, r, q < 4);
        put_line_h(buf, 0, r, q == 4);
        wave_sync();
      }
      const Fp2<C> D = LD(PD);
      {   // round 3: E = la D, Fv = Z C, G = X D, line c1 xP = -th xP
        Fp2<C> a = q == 0 ? la : q == 1 ? Z : q == 2 ? X : f2_neg<C>(th);
        Fp2<C> b = q == 1 ? LD(PC) : q == 3 ? xP : D;
        const Fp<C> r = mulp(a, b);
        const int dst = q == 0 ? PE : q == 1 ? PS : PGG;
        st_half(pbase + dst * S2, r, q < 3);
        put_line_h(buf, 1, r, q == 3);
        if (lane == 16) put_line(buf, 2, f2_sub<C>(LD(PV0), LD(PV1)));
        wave_sync();
      }
      const Fp2<C> Ev = LD(PE), G = LD(PGG);
      const Fp2<C> Hh = f2_sub<C>(f2_add<C>(Ev, LD(PS)), f2_dbl<C>(G));
      {   // round 4: XN = la Hh, ZN = Z E, th (G - Hh), E Y
        Fp2<C> a = q == 0 ? la : q == 1 ? Z : q == 2 ? th : Ev;
        Fp2<C> b = q == 0 ? Hh : q == 1 ? Ev : q == 2 ? f2_sub<C>(G, Hh) : Y;
        const int dst = q == 0 ? PXN : q == 1 ? PZN : q == 2 ? PU0 : PU1;
        const Fp<C> r = mulp(a, b);
        st_half(pbase + dst * S2, r, q < 4);
        wave_sync();
      }
      if (lane == 0) {
        ST(PX, LD(PXN));
        ST(PZ, LD(PZN));
        ST(PY, f2_sub<C>(LD(PU0), LD(PU1)));
      }
      wave_sync();
      publish();
    };
    const Fp2<C> qx = LD(PQX), qy = LD(PQY);
#pragma unroll 1
    for (int i = 1; i < C::LOOP_LEN; ++i) {
      if (is_sig) gen_step(); else dbl_step();
      const int d = C::LOOP_NAF[i];
      if (d != 0) {
        if (is_sig) gen_step(); else add_step(qx, d > 0 ? qy : f2_neg<C>(qy));
      }
    }
    if constexpr (C::CURVE_ID == 0) {
      if (is_sig) {
        gen_step();
        gen_step();
      } else {
        const Fp2<C> x1 = f2_mul<C>(f2_conj<C>(qx), gamma_const<C>(1, 2));
        const Fp2<C> y1 = f2_mul<C>(f2_conj<C>(qy), gamma_const<C>(1, 3));
        add_step(x1, y1);
        const Fp2<C> x2 = f2_mul<C>(qx, gamma_const<C>(2, 2));
        const Fp2<C> y2 = f2_neg<C>(f2_mul<C>(qy, gamma_const<C>(2, 3)));
        add_step(x2, y2);
      }
    }
  } else {
    // ------------------------------------------------ consumer: f <- f^2 * line, one Fp12 on 36 lanes
    int buf = 0;
    auto fold = [&]() {
      __syncthreads();                                        // the line of this step is complete
      if (valid) fe_mul<C>(S_F, S_F, buf ? S_L1 : S_L0);
      buf ^= 1;
    };
#pragma unroll 1
    for (int i = 1; i < C::LOOP_LEN; ++i) {
      if (i > 1 && valid) fe_mul<C>(S_F, S_F, S_F);
      fold();
      if (C::LOOP_NAF[i] != 0) fold();
    }
    if constexpr (C::CURVE_ID == 0) {
      fold();
      fold();
    } else {
      fe_conj<C>(S_F, S_F);                                   // x < 0
    }
    if (lane < 6) out[blk * 6 + lane] = lds_load_f2<C>(E::coef(S_F, lane, 0));
  }
}

// BLS12-381 epilogue of the cofactor-in-GT verification path: out = miller(-sigma, g2) * rest^h, h = the G1
// cofactor, where rest = prod_i miller(S_i, pk_i) over the UNCLEARED hash points (k_bls_combine<true>).  Both
// factors are serial chains with no batch dimension, so they run side by side on the two waves of one block
// with the 36-lane arithmetic of finalexp.hpp: wave 0 raises rest to h (general squarings -- rest is not
// unitary before the final exponentiation), wave 1 walks the fixed-argument lines of g2 (k_gen_lines table)
// for the signature pair.  The result is an ordinary partial product: the final exponentiation maps it to the
// same GT element as the reference's prod e(H(m_i), pk_i) * e(-sigma, g2).
template <class C>
__global__ void __launch_bounds__(128) k_cofactor_epilogue(const Fp2<C>* rest, const Aff<F1<C>>* sig, const LineCoeffs<C>* gen_lines,
                                                           uint8_t* out) {
  typedef FE<C> E;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  enum { S_BASE = 0, S_ACC = 1, S_SIG = 8, S_LINE = 9 };
  if (wave == 0) {
    if (lane < 6) {
      const Fp2<C> v = rest[lane];
      fe_put<C>(S_BASE, lane, v);
      fe_put<C>(S_ACC, lane, v);
    }
    wave_sync();
    if constexpr (C::CURVE_ID == 1) {                       // alt-bn128 has cofactor 1: the epilogue only folds the signature pair in
      for (int i = C::COFACTOR_BITS - 2; i >= 0; --i) {
        fe_mul<C>(S_ACC, S_ACC, S_ACC);
        if ((C::COFACTOR[i >> 5] >> (i & 31)) & 1u) fe_mul<C>(S_ACC, S_ACC, S_BASE);
      }
    }
  } else {
    if (lane < 6) {
      fe_put<C>(S_SIG, lane, lane == 0 ? f2_one<C>() : f2_zero<C>());
      fe_put<C>(S_LINE, lane, f2_zero<C>());
    }
    wave_sync();
    const bool have = sig != nullptr && !sig->inf;          // uniform
    if (have) {
      const Fp<C> xP = sig->x, yP = sig->y;
      int step = 0;
      auto apply = [&]() {
        if (lane < 3) {
          const LineCoeffs<C> l = gen_lines[step];
          // D-type: c0 yP + c1 xP w + c2 w^3     M-type: c2 + c1 xP w^2 + c0 yP w^3   (coop.hpp COOP_SH_D / COOP_SH_M)
          const Fp2<C> e = lane == 0 ? (C::TWIST_D ? f2_muls<C>(l.c0, yP) : l.c2)
                         : lane == 1 ? f2_muls<C>(l.c1, xP)
                                     : (C::TWIST_D ? l.c2 : f2_muls<C>(l.c0, yP));
          const int k = lane == 0 ? 0 : lane == 1 ? (C::TWIST_D ? 1 : 2) : 3;
          fe_put<C>(S_LINE, k, e);
        }
        ++step;
        wave_sync();
        fe_mul<C>(S_SIG, S_SIG, S_LINE);
      };
      for (int i = 1; i < C::LOOP_LEN; ++i) {
        if (i > 1) fe_mul<C>(S_SIG, S_SIG, S_SIG);
        apply();
        if (C::LOOP_NAF[i] != 0) apply();
      }
      if constexpr (C::CURVE_ID == 0) {
        apply();
        apply();
      } else {
        fe_conj<C>(S_SIG, S_SIG);                            // x < 0
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    fe_mul<C>(S_ACC, S_ACC, S_SIG);
    if (lane < 6) {
      const int order_pos[6] = {5, 2, 4, 1, 3, 0};
      const Fp2<C> v = lds_load_f2<C>(E::coef(S_ACC, lane, 0));
      uint8_t* o = out + (size_t)(2 * order_pos[lane]) * C::FP_BYTES;
      fp_to_be<C>(o, fp_from_mont<C>(v.c1));
      fp_to_be<C>(o + C::FP_BYTES, fp_from_mont<C>(v.c0));
    }
  }
}

// ======================================================================= launchers
namespace bgls {
namespace kl {

template <class C>
void gen_lines(hipStream_t st, LineCoeffs<C>* table, int* nsteps) {
  k_gen_lines<C><<<1, 64, 0, st>>>(table, nsteps);
}
template <class C>
void reduce_coop(hipStream_t st, const Fp2<C>* in, size_t count, int R, Fp2<C>* out) {
  const size_t nout = (count + R - 1) / R;
  k_reduce_coop<C><<<nblk(nout, Coop<C>::GROUPS), 64, Coop<C>::WAVE_BYTES, st>>>(in, count, R, out);
}
template <class C>
void reduce_coop_seg(hipStream_t st, const Fp2<C>* in, const uint32_t* seg, size_t nout, int R, Fp2<C>* out) {
  k_reduce_coop_seg<C><<<nblk(nout, Coop<C>::GROUPS), 64, Coop<C>::WAVE_BYTES, st>>>(in, seg, nout, R, out);
}
template <class C>
void w_to_bytes(hipStream_t st, const Fp2<C>* in, uint8_t* out) {
  k_w_to_bytes<C><<<1, 64, 0, st>>>(in, out);
}
#ifdef BGLS_LEGACY_KERNELS           // the 32-bit fallbacks of the final exponentiation, the latency Miller loop and the epilogue: `make LEGACY=1` only
template <class C>
void final36(hipStream_t st, const uint8_t* partials, size_t count, int do_final_exp, uint8_t* gt_out, uint32_t* verdict, uint32_t* flags) {
  k_final36<C><<<1, 64, FE<C>::LDS_BYTES, st>>>(partials, count, do_final_exp, gt_out, verdict, flags);
}
template <class C>
void miller_lat(hipStream_t st, const Aff<F1<C>>* g1s, const uint8_t* g2s, size_t n, long long sig_at, const LineCoeffs<C>* gen_lines, Fp2<C>* out,
                uint32_t* flags) {
  const unsigned blocks = (unsigned)(n + (sig_at >= 0 ? 1 : 0));
  k_miller_lat<C><<<blocks, 128, FE<C>::LDS_BYTES, st>>>(g1s, g2s, n, sig_at, gen_lines, out, flags);
}
template <class C>
void cofactor_epilogue(hipStream_t st, const Fp2<C>* rest, const Aff<F1<C>>* sig, const LineCoeffs<C>* gen_lines, uint8_t* out) {
  k_cofactor_epilogue<C><<<1, 128, FE<C>::LDS_BYTES2, st>>>(rest, sig, gen_lines, out);
}
#endif
template <class C>
void gt_pow(hipStream_t st, const uint8_t* gt_in, const uint8_t* k_be32, int negate, uint8_t* gt_out, uint32_t* flags) {
  k_gt_pow<C><<<1, 64, FE<C>::LDS_BYTES, st>>>(gt_in, k_be32, negate, gt_out, flags);
}

#define BGLS_INST(C)                                                                                               \
  template void gen_lines<C>(hipStream_t, LineCoeffs<C>*, int*);                                                   \
  template void reduce_coop<C>(hipStream_t, const Fp2<C>*, size_t, int, Fp2<C>*);                                  \
  template void reduce_coop_seg<C>(hipStream_t, const Fp2<C>*, const uint32_t*, size_t, int, Fp2<C>*);            \
  template void w_to_bytes<C>(hipStream_t, const Fp2<C>*, uint8_t*);                                               \
  template void gt_pow<C>(hipStream_t, const uint8_t*, const uint8_t*, int, uint8_t*, uint32_t*);
BGLS_INST(BGLS_TAIL_CURVE)
#undef BGLS_INST
#ifdef BGLS_LEGACY_KERNELS
#define BGLS_INST(C)                                                                                               \
  template void final36<C>(hipStream_t, const uint8_t*, size_t, int, uint8_t*, uint32_t*, uint32_t*);              \
  template void miller_lat<C>(hipStream_t, const Aff<F1<C>>*, const uint8_t*, size_t, long long, const LineCoeffs<C>*, Fp2<C>*, uint32_t*); \
  template void cofactor_epilogue<C>(hipStream_t, const Fp2<C>*, const Aff<F1<C>>*, const LineCoeffs<C>*, uint8_t*);
BGLS_INST(BGLS_TAIL_CURVE)
#undef BGLS_INST
#endif

}  // namespace kl
}  // namespace bgls
