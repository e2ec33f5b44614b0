// TEST-ONLY: k_miller_x60's XL form ("xi on the line", bgls_amd/csrc/miller_x.hpp) walked on the host, against the form it replaces.
// Never linked into the product.  A library of its own (tests/harness/build_harness_xl.py), next to host_harness.cpp.
//
// One group of six pairings over the whole alt-bn128 loop (65 doublings, 21 + 2 additions) on the 29-bit number form, every column
// accumulation checked (BGLS_RX_CHECK):
//   producers  the lane pair of every pairing on two lock-stepped threads: dbl_step_x / add_step_x, the three line entries as the kernel's emit
//              forms them, and the two xi copies of the XL hand-over (pair_mulxi_half);
//   consumer   the six coefficient lanes of the group, in the kernel's order (squaring, publish, six folds with a publish each), twice:
//              OLD  every publish forms xi e_j (ux_mulxi), a fold's wrapped term is  L_t * (xi B_k);
//              NEW  a fold's wrapped term is  (xi L_t) * B_k  with B_k read from the second slot, which holds a plain copy -- the xi multiple
//                   only after the publish whose next reader is the squaring.
// Every published coefficient of NEW must be the field element OLD publishes, the group's output after from_ux_inl the same bytes, and (real
// lines only) the product of pairing.hpp's Miller values.
#include <type_traits>
#include <string.h>
#include <atomic>
#include <thread>
#define BGLS_RX_CHECK 1
#include "../../bgls_amd/csrc/pairing.hpp"
#include "../../bgls_amd/csrc/wire.hpp"
#include "../../bgls_amd/csrc/rx_pair.hpp"

namespace bgls { int g_rx_overflow = 0; }

// ---- host emulation of a lane pair (rx_pair.hpp): two threads in lock-step, values exchanged through a rendezvous (as host_harness.cpp)
static std::atomic<int> g_pair_slot[2];
static std::atomic<int> g_pair_cnt{0};
static std::atomic<int> g_pair_gen{0};
static thread_local int tl_pair_lane = 0;
static void pair_barrier() {
  const int gen = g_pair_gen.load();
  if (g_pair_cnt.fetch_add(1) == 1) {
    g_pair_cnt.store(0);
    g_pair_gen.fetch_add(1);
  } else {
    while (g_pair_gen.load(std::memory_order_acquire) == gen) { }
  }
}
int rx_host_pair_swap(int v) {
  g_pair_slot[tl_pair_lane].store(v);
  pair_barrier();
  const int r = g_pair_slot[1 - tl_pair_lane].load();
  pair_barrier();
  return r;
}
using namespace bgls;

typedef BN254W X;
static constexpr int N = X::RX_NL;
static constexpr int MAXS = 96;
static constexpr int TOP = N - 1;

// the squaring's table (coop.hpp COOP_SQ_TAB: a device constant there) and its split into two piles (miller_x.hpp mx_sq_split)
static const unsigned SQ_TAB[6] = {0x5be2e900u, 0xffe3ea88u, 0x64eb0990u, 0xffec9198u, 0x6d1299a0u, 0xff9aa1a8u};
static void sq_split(unsigned row, unsigned& pa, unsigned& pb) {
  unsigned d[3] = {0xffu, 0xffu, 0xffu}, p[2] = {0xffu, 0xffu};
  int nd = 0, np = 0;
  for (int t = 0; t < 4; ++t) {
    const unsigned e = (row >> (8 * t)) & 0xFFu;
    if ((e & 7u) == 7u) continue;
    if (e & 0x80u) d[nd++] = e; else p[np++] = e;
  }
  if (nd == 3) { pa = d[0] | (d[1] << 8) | (1u << 16); pb = d[2] | (0xffu << 8); }
  else { pa = d[0] | (p[0] << 8); pb = d[1] | (p[1] << 8); }
}

// ---- producers: one pairing's lines, five entries per step: [0..2] as today, [3] = xi [1], [4] = xi [2]
// mode 0: the walk's own lines; 1: every entry replaced by worst-case limbs (low limbs all ones, top limb at the entry's bound: 2.1 p / 2.1 p /
// 3.1 p) in two steps of three, top limb at the bound over random low limbs in the third -- the walk still runs, so that the step count and the
// lock-step are the kernel's.
struct Lines {
  Ux<X> e[MAXS][5][2];       // [step][entry][half]
  int nsteps[2];
};
struct Walk {
  Aff<F1<X>> P;
  Aff<F2<X>> Q;
  int mode;
  unsigned seed;
  Lines* out;
  struct Env {
    Sx<X, SX_T> nyp, xp, xq_, yq_;
    Sx<X, SX_T> nyP() const { return nyp; }
    Sx<X, SX_T> xP() const { return xp; }
    Sx<X, SX_T> xq() const { return xq_; }
    Sx<X, SX_T> yq() const { return yq_; }
  };
  void lane(int l) {
    tl_pair_lane = l;
    const bool odd = l == 1;
    auto half = [&](const Fp2<X>& v) { return ux_to_sx<X>(to_ux<X>(odd ? v.c1 : v.c0)); };
    Env env;
    env.nyp = ux_to_sx<X>(to_ux<X>(fp_neg<X>(P.y)));
    env.xp = ux_to_sx<X>(to_ux<X>(P.x));
    const Sx<X, SX_T> xq = half(Q.x), yq = half(Q.y);
    PointX<X> T;
    T.X = xq;
    T.Y = yq;
    T.Z = sx_select<X>(odd, ux_to_sx<X>(ux_zero<X>()), sx_const<X>(X::RX_ONE));
    int s = 0;
    unsigned lcg = seed * 2654435761u + (unsigned)l * 40503u + 12345u;
    auto emit = [&](int which, const auto& v) {              // miller_x.hpp's emit, XL
      const int entry = which == 1 ? 1 : (which == 0 ? 0 : 2);
      Ux<X> u;
      if constexpr (std::is_same<std::decay_t<decltype(v)>, Sx<X, SX_T>>::value) u = sx_to_ux_p<X>(v);
      else u = sx_to_ux_k<1, X>(v);
      if (mode == 1) {
        const u32 top = (entry == 2 ? 31u : 21u) * X::RX_P[TOP] / 10u;
        for (int i = 0; i < TOP; ++i) {
          lcg = lcg * 1664525u + 1013904223u;
          u.v[i] = (s % 3 == 2) ? (lcg >> 3) & X::RX_MASK : X::RX_MASK;
        }
        u.v[TOP] = top;
      }
      out->e[s][entry][l] = u;
      if (entry != 0) out->e[s][entry + 2][l] = pair_mulxi_half<X>(u, odd);
    };
    for (int i = 1; i < X::LOOP_LEN; ++i) {
      dbl_step_x<X>(T, env, odd, emit);
      ++s;
      const int d = X::LOOP_NAF[i];
      if (d != 0) {
        env.xq_ = xq;
        env.yq_ = d > 0 ? yq : sx_neg<X>(yq);
        add_step_x<X>(T, env, odd, emit);
        ++s;
      }
    }
    const Fp2<X> x1 = f2_mul<X>(f2_conj<X>(Q.x), gamma_const<X>(1, 2)), y1 = f2_mul<X>(f2_conj<X>(Q.y), gamma_const<X>(1, 3));
    const Fp2<X> x2 = f2_mul<X>(Q.x, gamma_const<X>(2, 2)), y2 = f2_neg<X>(f2_mul<X>(Q.y, gamma_const<X>(2, 3)));
    env.xq_ = half(x1); env.yq_ = half(y1);
    add_step_x<X>(T, env, odd, emit);
    ++s;
    env.xq_ = half(x2); env.yq_ = half(y2);
    add_step_x<X>(T, env, odd, emit);
    ++s;
    out->nsteps[l] = s;
  }
};

// ---- consumer: the group's LDS entries as arrays
struct Group {
  Ux2<X> acc[6];             // acc_off(k, 0)
  Ux2<X> sec[6];             // acc_off(k, 1): OLD xi e_k; NEW (k >= 3 only) a copy of e_k, or xi e_k ahead of the squaring
  bool xl;
  void publish(const Ux2<X> (&v)[6], bool sq_next) {         // mxk_publish
    for (int j = 0; j < 6; ++j) {
      acc[j] = v[j];
      if (!xl) sec[j] = ux_mulxi<X>(v[j]);
      else if (j >= 3) sec[j] = sq_next ? ux_mulxi<X>(v[j]) : v[j];
    }
  }
  // mx_fold: line = the five entries of one pairing's step
  void fold(const Ux<X> (&ln)[5][2], Ux2<X> (&r)[6]) const {
    for (int j = 0; j < 6; ++j) {
      r[j] = ux_dot_k2p<X, 3, (N <= 10)>(
          [&](int t, int h) { return ln[xl && mxl_wraps<X>(j, t) ? t + 2 : t][h]; },
          [&](int t, int h) {
            const Ux2<X>& b = mxl_wraps<X>(j, t) ? sec[mxl_acc_k<X>(j, t)] : acc[mxl_acc_k<X>(j, t)];
            return h ? b.c1 : b.c0;
          });
    }
  }
  void sqr(Ux2<X> (&r)[6]) const {                           // mxk_sqr3
    for (int j = 0; j < 6; ++j) {
      unsigned pa, pb;
      sq_split(SQ_TAB[j], pa, pb);
      const bool twice = (pa >> 16) & 1u;
      auto fetch = [&](unsigned sl, int t, int side, int h) {
        const unsigned e = (sl >> (8 * t)) & 0xFFu;
        const bool unused = (e & 7u) == 7u;
        const int i = unused ? 0 : (int)(e & 7u), k = unused ? 0 : (int)((e >> 3) & 7u), wrap = unused ? 0 : (int)((e >> 6) & 1u);
        const Ux2<X>& src = side == 0 ? acc[i] : (wrap ? sec[k] : acc[k]);
        Ux<X> a = h ? src.c1 : src.c0;
        if (side == 0 && unused) a = ux_zero<X>();
        return a;
      };
      r[j] = ux_sqr_dot3<X>([&](int t, int side, int h) { return fetch(pa, t, side, h); }, [&](int t, int side, int h) { return fetch(pb, t, side, h); },
                            [&](int t) { return t == 0 && !twice; }, [&](int t) { return t == 0; }, twice);
    }
  }
};

static Fp2<X> canon(const Ux2<X>& v) {
  const Ux2<X> q = ux_quasi<X, 2, 1>(v);
  return {from_ux_inl<X>(q.c0), from_ux_inl<X>(q.c1)};
}

// present[m] = 0: pairing m is absent (the constant line 1: entry 0 = 1, every other entry and both xi copies zero).
// out_old / out_new: the group's six Fp2 after from_ux_inl, raw (6 * 2 * sizeof(Fp)); out_ref: the product of pairing.hpp's Miller values in the
// same layout (mode 0).  Returns 0, -2 bad point, -3 column overflow or a violated bound, 1 + the index of the first publish at which a
// coefficient of NEW differs from OLD mod p.
extern "C" int ht_xl_group(const uint8_t* g1s, const uint8_t* g2s, const uint8_t* present, int mode, uint8_t* out_old, uint8_t* out_new, uint8_t* out_ref) {
  static Lines lines[6];
  g_rx_overflow = 0;
  Fp12<X> ref = f12_one<X>();
  for (int m = 0; m < 6; ++m) {
    Walk w;
    if (!g1_from_bytes<X>(w.P, g1s + 64 * m) || !g2_from_bytes<X>(w.Q, g2s + 128 * m)) return -2;
    w.mode = mode;
    w.seed = 977u * (unsigned)m + 5u;
    w.out = &lines[m];
    g_pair_cnt.store(0);
    std::thread t1([&] { w.lane(1); });
    w.lane(0);
    t1.join();
    if (lines[m].nsteps[0] != lines[m].nsteps[1]) return -4;
    if (!present[m]) {
      for (int s = 0; s < lines[m].nsteps[0]; ++s)
        for (int e = 0; e < 5; ++e) {
          lines[m].e[s][e][0] = e == 0 ? ux_load<X>(X::RX_ONE) : ux_zero<X>();
          lines[m].e[s][e][1] = ux_zero<X>();
        }
    } else {
      ref = f12_mul<X>(ref, miller_loop<X>(w.P, w.Q));
    }
  }
  if (g_rx_overflow) return -3;
  Group go, gn;
  go.xl = false;
  gn.xl = true;
  Ux2<X> fo[6], fn[6];
  for (int j = 0; j < 6; ++j) {
    fo[j].c0 = j == 0 ? ux_load<X>(X::RX_ONE) : ux_zero<X>();
    fo[j].c1 = ux_zero<X>();
    fn[j] = fo[j];
  }
  int npub = 0, bad = 0;
  auto publish = [&](bool sq_next) {
    go.publish(fo, sq_next);
    gn.publish(fn, sq_next);
    for (int j = 0; j < 6 && !bad; ++j) {
      const Fp2<X> a = canon(fo[j]), b = canon(fn[j]);
      if (!f2_eq<X>(a, b)) bad = 1 + npub;
    }
    ++npub;
  };
  int s = 0;
  auto fold_all = [&](bool sq_next) {                          // the kernel's fold_all
    for (int m = 0; m < 6; ++m) {
      go.fold(lines[m].e[s], fo);
      gn.fold(lines[m].e[s], fn);
      publish(sq_next && m == 5);
    }
    ++s;
  };
  publish(false);
  for (int i = 1; i < X::LOOP_LEN; ++i) {
    if (i > 1) {
      go.sqr(fo);
      gn.sqr(fn);
      publish(false);
    }
    fold_all(X::LOOP_NAF[i] == 0 && i + 1 < X::LOOP_LEN);
    if (X::LOOP_NAF[i] != 0) fold_all(i + 1 < X::LOOP_LEN);
  }
  for (int k = 0; k < 2; ++k) fold_all(false);
  if (s != lines[0].nsteps[0]) return -4;
  if (g_rx_overflow) return -3;
  if (bad) return bad;
  const Fp2<X> rw[6] = {ref.g.a0, ref.h.a0, ref.g.a1, ref.h.a1, ref.g.a2, ref.h.a2};       // w-basis: coefficient j of w^j
  for (int j = 0; j < 6; ++j) {
    const Fp2<X> a = canon(fo[j]), b = canon(fn[j]);
    memcpy(out_old + j * sizeof(Fp2<X>), &a, sizeof(Fp2<X>));
    memcpy(out_new + j * sizeof(Fp2<X>), &b, sizeof(Fp2<X>));
    memcpy(out_ref + j * sizeof(Fp2<X>), &rw[j], sizeof(Fp2<X>));
  }
  return 0;
}

// the number of line steps and publishes of one walk (the test states what it expects)
extern "C" int ht_xl_steps() {
  int s = 0;
  for (int i = 1; i < X::LOOP_LEN; ++i) s += X::LOOP_NAF[i] != 0 ? 2 : 1;
  return s + 2;
}
