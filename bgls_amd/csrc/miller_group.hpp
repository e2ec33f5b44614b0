// The "one Fp12 accumulator per six-lane group, walks on lane pairs" block of k_miller_sets (k_millersets.hip) and k_miller_ams
// (k_millerams.hip): the layout MG, the line fold, the producer wave's body and the consumer wave's body.  Built from k_miller_x60's
// pieces (miller_x.hpp): its producer's point steps on lane pairs (rx_pair.hpp dbl_step_x / add_step_x) and its consumer's fold and
// squaring (mxk_publish, mxk_sqr / mxk_sqr3 and the line fold of ux_dot_k2p) on a layout of its own.
//
// Block = NWALK + 3 waves, 30 items:
//   NWALK PRODUCER waves 30 items each, one per LANE PAIR, the same 30 in every wave: wave `walk` walks its (P, Q) pair from the key Q;
//                        with GEN, walk 0 also scales the generator's pre-computed line of the step (Engine::gen_lines) by its
//                        sigs[b], as k_miller_latx's signature block
//   three CONSUMER waves 10 groups x 6 lanes each (lane = 10 j + g, as k_miller_x60's consumer); group = item, lane j owns
//                        coefficient j of f_b = sum e_j w^j:  f <- f^2 l_walk0 [l_walk1] [l_gen]
// Per line step as k_miller_x60: producers: point step | barrier A | store lines | barrier B;  consumers: squaring | A | B | folds.
// Every walk runs over the same loop, so all producer waves meet every barrier together.
//
// LDS per group: the accumulator's six entries, the xi copies of e_3..e_5 only (mxk_publish XI3: every wrapped factor of a fold or
// a squaring is one of them), the line entries (three per line: walk m at 3 m, the generator's behind the walks).  The P coordinates
// stay in the producer lanes' park (global).  Out-of-range items (a ragged last block), a key or a G1 point at infinity and a signature
// at infinity give the constant line 1 for THEIR pair only, as in k_miller_x60 / k_miller_latx; a final Z = 0 of any walk sets
// FLAG_DEGENERATE.
#pragma once
#include <type_traits>
#include "miller_x.hpp"
#include "pairing.hpp"

namespace bgls {

template <class X, int NWALK_, bool GEN_>
struct MG {
  static constexpr int NL = X::RX_NL;
  static constexpr bool PACKED = MX<X>::PACKED;
  static constexpr int HS = MX<X>::HS, ES = MX<X>::ES;
  static constexpr int NWALK = NWALK_;                                      // producer waves = walked pairs per accumulator
  static constexpr bool GEN = GEN_;                                         // the generator's line is folded as well (alt-bn128)
  static constexpr int NLINES = NWALK + GEN;                                // lines folded per step
  static constexpr int ITEMS = 30;                                          // accumulators per block
  static constexpr int THREADS = 64 * (NWALK + 3);
  // entries of ES dwords: e_0..e_5, xi e_3..e_5, then the line entries; the group stride rounded up to an odd number of 16-byte slots
  // (the ten groups of a consumer 16-lane group then start in ten different slots mod 16)
  static constexpr int RAW_DW = (9 + 3 * NLINES) * ES;
  static constexpr int GROUP_DW = ((RAW_DW / 4) | 1) * 4;
  static constexpr int BLOCK_BYTES = ITEMS * GROUP_DW * 4;
  static __device__ __forceinline__ int acc_off(int k, int wrap) { return (wrap ? k + 3 : k) * ES; }
  static __device__ __forceinline__ int line_off(int e) { return (9 + e) * ES; }
  // producer park per lane (every producer wave): xq yq [x1 y1 x2 y2] nyP xP [xS yS]
  static constexpr int NPARK_Q = X::CURVE_ID == 0 ? 6 : 2;
  static constexpr int P_NYP = NPARK_Q, P_XP = NPARK_Q + 1, P_XS = NPARK_Q + 2, P_YS = NPARK_Q + 3;
  static constexpr int NPARK = NPARK_Q + 2 + (GEN ? 2 : 0);
  static constexpr int PS = MX<X>::PS;
  static constexpr size_t park_bytes(size_t nblocks) { return nblocks * 64 * NWALK * NPARK * PS * 4; }
  static_assert(GROUP_DW >= RAW_DW && GROUP_DW % 4 == 0, "group layout");
};

// f <- f * line_m on layout K (mx_fold's body for a layout other than MX)
template <class X, class K>
__device__ __forceinline__ Ux2<X> mg_fold(int gb, int m, int j) {
  auto sh = [](int t) { return X::TWIST_D ? t + (t == 2 ? 1 : 0) : t + (t >= 1 ? 1 : 0); };
  return ux_dot_k2p<X, 3, (X::RX_NL <= 10)>(
      [&](int t, int h) { return mx_ld_half<X, K::PACKED>(gb + K::line_off(3 * m + t) + h * K::HS, h != 0); },
      [&](int t, int h) {
        int k = j - sh(t);
        const int wrap = k < 0 ? 1 : 0;
        k += 6 * wrap;
        return mx_ld_half<X, K::PACKED>(gb + K::acc_off(k, wrap) + h * K::HS, h != 0);
      });
}

// One producer wave: walk `walk` (wave-uniform) of the block's K::ITEMS items, one per lane pair: item b pairs g1s[b] with the key
// g2s[b] (wire bytes, checked here).  With K::GEN, walk 0 also stores the generator's line scaled by sigs[b].
template <class C, class X, class K>
__device__ __forceinline__ void mg_producer(int walk, const Aff<F1<X>>* g1s, const uint8_t* g2s, const Aff<F1<X>>* sigs, const LineCoeffs<X>* gen_lines,
                                            size_t n, uint32_t* flags, u32* park) {
  const int lane = threadIdx.x & 63;
  const int q = lane >> 1;
  const bool odd = lane & 1;
  const bool owner = q < K::ITEMS;
  const size_t idx = (size_t)blockIdx.x * K::ITEMS + (owner ? q : 0);
  u32* const mypark = park + ((size_t)blockIdx.x * 64 * K::NWALK + walk * 64 + lane) * (K::NPARK * K::PS);
  bool valid = owner && idx < n;
  bool svalid = valid;
  PointX<X> T;
  {
    // setup as k_miller_x60's: the even lane parses the real parts of the key, the odd lane the imaginary parts
    constexpr int NB = X::FP_BYTES;
    const uint8_t* kb = g2s + (valid ? idx : 0) * 4 * NB;
    const Fp<X> xw = fp_from_be<X>(kb + (odd ? 0 : NB)), yw = fp_from_be<X>(kb + (odd ? 2 * NB : 3 * NB));     // wire order: x_im x_re y_im y_re
    const bool canon_own = !fp_geq_p<X>(xw) && !fp_geq_p<X>(yw);
    const bool zero_own = fp_is_zero<X>(xw) && fp_is_zero<X>(yw);
    const bool canon = canon_own && pair_swap1(canon_own ? 1 : 0) != 0;
    const bool qinf = zero_own && pair_swap1(zero_own ? 1 : 0) != 0;
    Sx<X, SX_T> xq = sx_from_plain<X>(xw), yq = sx_from_plain<X>(yw);
    {
      const Sx<X, SX_T> b2 = sx_const<X>(odd ? X::RX_B2_IM : X::RX_B2_RE);
      const auto d = sx_sub<X>(pair_sqr<X>(yq, odd), sx_add<X>(pair_mul<X>(pair_sqr<X>(xq, odd), xq, odd), b2));
      const bool on_own = sx_is_zero_mod_p<X>(d);
      const bool on_curve = on_own && pair_swap1(on_own ? 1 : 0) != 0;
      if (valid && !(canon && (qinf || on_curve))) atomicOr(flags, FLAG_ENC);
    }
    Aff<F1<X>> P = g1s[valid ? idx : 0];
    if constexpr (K::GEN) {
      if (walk == 0) {
        Aff<F1<X>> S = sigs[valid ? idx : 0];
        svalid = valid && !S.inf;
        if (!svalid) {
          S.x = fp_load<X>(X::G1X);
          S.y = fp_load<X>(X::G1Y);
        }
        MxPark<X>::st(mypark, K::P_XS, ux_to_sx<X>(to_ux<X>(S.x)));
        MxPark<X>::st(mypark, K::P_YS, ux_to_sx<X>(to_ux<X>(S.y)));
      }
    }
    valid = valid && !P.inf && !qinf;
    if (!valid) {                         // harmless stand-ins: the generators (the lane's line is replaced by the constant 1)
      xq = ux_to_sx<X>(to_ux<X>(fp_load<X>(X::G2 + (odd ? X::L : 0))));
      yq = ux_to_sx<X>(to_ux<X>(fp_load<X>(X::G2 + 2 * X::L + (odd ? X::L : 0))));
      P.x = fp_load<X>(X::G1X);
      P.y = fp_load<X>(X::G1Y);
    }
    MxPark<X>::st(mypark, 0, xq);
    MxPark<X>::st(mypark, 1, yq);
    if constexpr (X::CURVE_ID == 0) {
      // Q1 = pi(Q) = (conj(x) g12, conj(y) g13), -Q2 = -pi^2(Q) = (x g22, -y g23) on the twist
      const Sx<X, SX_T> cx = sx_select<X>(odd, sx_neg<X>(xq), xq), cy = sx_select<X>(odd, sx_neg<X>(yq), yq);
      constexpr int N2 = 2 * X::RX_NL;
      MxPark<X>::st(mypark, 2, pair_mul_const<X>(cx, X::RX_GAMMA + 0 * N2, X::RX_GAMMA + 0 * N2 + X::RX_NL, odd));
      MxPark<X>::st(mypark, 3, pair_mul_const<X>(cy, X::RX_GAMMA + 1 * N2, X::RX_GAMMA + 1 * N2 + X::RX_NL, odd));
      MxPark<X>::st(mypark, 4, pair_mul_const<X>(xq, X::RX_GAMMA + 2 * N2, X::RX_GAMMA + 2 * N2 + X::RX_NL, odd));
      MxPark<X>::st(mypark, 5, sx_norm<X>(sx_neg<X>(pair_mul_const<X>(yq, X::RX_GAMMA + 3 * N2, X::RX_GAMMA + 3 * N2 + X::RX_NL, odd))));
    }
    MxPark<X>::st(mypark, K::P_NYP, ux_to_sx<X>(to_ux<X>(fp_neg<X>(P.y))));
    MxPark<X>::st(mypark, K::P_XP, ux_to_sx<X>(to_ux<X>(P.x)));
    T.X = xq;
    T.Y = yq;
    T.Z = sx_select<X>(odd, ux_to_sx<X>(ux_zero<X>()), sx_const<X>(X::RX_ONE));
  }
  const int rl_base = q * K::GROUP_DW + (odd ? K::HS : 0);
  const int my_line = 3 * walk;                            // first line entry of this wave's walk
  Ux<X> e[3];
  auto conv = [](const auto& v) __attribute__((always_inline)) {
    if constexpr (rx_lazy<X>) return sx_to_ux<X>(v);
    else if constexpr (std::is_same<std::decay_t<decltype(v)>, Sx<X, SX_T>>::value) return sx_to_ux_p<X>(v);
    else return sx_to_ux_k<1, X>(v);
  };
  // entry of line coefficient `which`: D-type c0 yP, c1 xP, c2;  M-type c2, c1 xP, c0 yP (k_miller_x60's order)
  auto entry_of = [](int which) { return which == 1 ? 1 : ((which == 0) == X::TWIST_D ? 0 : 2); };
  auto emit = [&](int which, const auto& v) __attribute__((always_inline)) { e[entry_of(which)] = conv(v); };
  int step = 0;
  auto hand_over = [&]() __attribute__((always_inline)) {
    if (__builtin_amdgcn_ballot_w64(owner && !valid) != 0) {
      if (!valid) {
        e[0] = odd ? ux_zero<X>() : ux_load<X>(X::RX_ONE);
        e[1] = ux_zero<X>();
        e[2] = ux_zero<X>();
      }
    }
    Ux<X> gl[3];
    if constexpr (K::GEN) {
      if (walk == 0) {
        // the generator's line of this step scaled by sigs[b] (k_miller_latx's signature block): c0 yS, c1 xS, c2
        const LineCoeffs<X> l = gen_lines[step];
        const u32* pk = MxPark<X>::launder(mypark);
        const Sx<X, SX_T> c0 = ux_to_sx<X>(to_ux<X>(odd ? l.c0.c1 : l.c0.c0));
        const Sx<X, SX_T> c1 = ux_to_sx<X>(to_ux<X>(odd ? l.c1.c1 : l.c1.c0));
        const Sx<X, SX_T> c2 = ux_to_sx<X>(to_ux<X>(odd ? l.c2.c1 : l.c2.c0));
        gl[entry_of(0)] = conv(pair_muls<X>(c0, MxPark<X>::ld(pk, K::P_YS)));
        gl[entry_of(1)] = conv(pair_muls<X>(c1, MxPark<X>::ld(pk, K::P_XS)));
        gl[entry_of(2)] = conv(c2);
        if (__builtin_amdgcn_ballot_w64(owner && !svalid) != 0) {
          if (!svalid) {
            gl[0] = odd ? ux_zero<X>() : ux_load<X>(X::RX_ONE);
            gl[1] = ux_zero<X>();
            gl[2] = ux_zero<X>();
          }
        }
      }
    }
    ++step;
    __syncthreads();                    // A: the consumers have finished with the previous lines
    if (owner) {
      mx_st_half<X, K::PACKED>(rl_base + K::line_off(my_line + 0), odd, e[0]);
      mx_st_half<X, K::PACKED>(rl_base + K::line_off(my_line + 1), odd, e[1]);
      mx_st_half<X, K::PACKED>(rl_base + K::line_off(my_line + 2), odd, e[2]);
      if constexpr (K::GEN) {
        if (walk == 0) {
          mx_st_half<X, K::PACKED>(rl_base + K::line_off(3 * K::NWALK + 0), odd, gl[0]);
          mx_st_half<X, K::PACKED>(rl_base + K::line_off(3 * K::NWALK + 1), odd, gl[1]);
          mx_st_half<X, K::PACKED>(rl_base + K::line_off(3 * K::NWALK + 2), odd, gl[2]);
        }
      }
    }
    __syncthreads();                    // B: lines visible
  };
  struct Env {
    const u32* pk;
    int xs, ys;
    bool neg_y;
    __device__ __forceinline__ Sx<X, SX_T> nyP() const { return MxPark<X>::ld(MxPark<X>::launder(pk), K::P_NYP); }
    __device__ __forceinline__ Sx<X, SX_T> xP() const { return MxPark<X>::ld(MxPark<X>::launder(pk), K::P_XP); }
    __device__ __forceinline__ Sx<X, SX_T> xq() const { return MxPark<X>::ld(MxPark<X>::launder(pk), xs); }
    __device__ __forceinline__ Sx<X, SX_T> yq() const {
      const Sx<X, SX_T> y = MxPark<X>::ld(MxPark<X>::launder(pk), ys);
      return sx_select<X>(neg_y, sx_neg<X>(y), y);
    }
  };
#pragma unroll 1
  for (int i = 1; i < X::LOOP_LEN; ++i) {
    dbl_step_x<X>(T, Env{mypark, 0, 1, false}, odd, emit);
    hand_over();
    const int d = X::LOOP_NAF[i];
    if (d != 0) {
      add_step_x<X>(T, Env{mypark, 0, 1, d < 0}, odd, emit);
      hand_over();
    }
  }
  if constexpr (X::CURVE_ID == 0) {
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
      add_step_x<X>(T, Env{mypark, 2 + 2 * s, 3 + 2 * s, false}, odd, emit);
      hand_over();
    }
  }
  // degenerate point steps leave Z = 0 (k_miller_x60): an encoding error, not an unspecified verdict
  const bool z_own = sx_is_zero_mod_p<X>(T.Z);
  const bool z_zero = z_own && pair_swap1(z_own ? 1 : 0) != 0;
  if (valid && z_zero && !odd) atomicOr(flags, FLAG_DEGENERATE);
}

// Consumer wave cw (0..2): 10 groups x 6 lanes, lane = 10 j + g, item = 10 cw + g.  With K::GEN the result goes out as GT bytes (no
// final exponentiation) to out_bytes + b GTB, otherwise as six w-basis Fp2 per item to out_w (the epilogue's rest).
template <class C, class X, class K>
__device__ __forceinline__ void mg_consumer(int cw, size_t n, Fp2<X>* out_w, uint8_t* out_bytes) {
  constexpr int NL = X::RX_NL;
  const int lane = threadIdx.x & 63;
  const bool live = lane < 60;
  const int cl = live ? lane : lane - 12;                // lanes 60..63 shadow lanes 48..51
  const int g = cl % 10;
  const int j = cl / 10;
  const int item = cw * 10 + g;
  const int gb = item * K::GROUP_DW;
  Ux2<X> fj;
  {
    const Ux<X> one = ux_load<X>(X::RX_ONE);
#pragma unroll
    for (int k = 0; k < NL; ++k) { fj.c0.v[k] = j == 0 ? one.v[k] : 0u; fj.c1.v[k] = 0u; }
  }
  mxk_publish<X, K, true>(gb, j, fj, live);
  unsigned sq_d = 0, sq_p = 0;
  if constexpr (!rx_lazy<X>) mx_sq_split(COOP_SQ_TAB[j], sq_d, sq_p);
  auto fold_all = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int m = 0; m < K::NLINES; ++m) {
      fj = mg_fold<X, K>(gb, m, j);
      mxk_publish<X, K, true>(gb, j, fj, live);
    }
  };
#pragma unroll 1
  for (int i = 1; i < X::LOOP_LEN; ++i) {
    if (i > 1) {                        // f = 1 before the first step; the squaring goes ahead of A as in k_miller_x60
      if constexpr (rx_lazy<X>) fj = mxk_sqr<X, K>(gb, j);
      else fj = mxk_sqr3<X, K>(gb, sq_d, sq_p);
      mxk_publish<X, K, true>(gb, j, fj, live);
    }
    __syncthreads();                    // A
    __syncthreads();                    // B
    fold_all();
    if (X::LOOP_NAF[i] != 0) {
      __syncthreads();
      __syncthreads();
      fold_all();
    }
  }
  if constexpr (X::CURVE_ID == 0) {
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
      __syncthreads();
      __syncthreads();
      fold_all();
    }
  }
  const size_t b = (size_t)blockIdx.x * K::ITEMS + item;
  if (live && b < n) {
    if constexpr (!rx_lazy<X>) fj = ux_quasi<X, 2, 1>(fj);        // the folds' fixed point is 3.7 p; from_ux_inl takes values below 4 p
    Fp2<X> r = {from_ux_inl<X>(fj.c0), from_ux_inl<X>(fj.c1)};
    if constexpr (X::CURVE_ID != 0) {
      if (j & 1) r = f2_neg<X>(r);                      // x < 0: f^(p^6), w -> -w
    }
    if constexpr (K::GEN) {
      // GT bytes as k_w_to_bytes writes them: coefficient j at position order_pos[j], imaginary part first
      const int order_pos[6] = {5, 2, 4, 1, 3, 0};
      const Fp2<C> rc = *reinterpret_cast<const Fp2<C>*>(&r);
      uint8_t* o = out_bytes + b * 12 * C::FP_BYTES + (size_t)(2 * order_pos[j]) * C::FP_BYTES;
      fp_to_be<C>(o, fp_from_mont<C>(rc.c1));
      fp_to_be<C>(o + C::FP_BYTES, fp_from_mont<C>(rc.c0));
    } else {
      out_w[b * 6 + j] = r;
    }
  }
}

}  // namespace bgls
