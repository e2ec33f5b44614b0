// TEST-ONLY: the throughput final exponentiation (bgls_amd/csrc/finalxt.hpp) walked on the host.  Never linked into the product.  A library
// of its own (tests/harness/build_harness_fxt.py), next to host_harness_xl.cpp; with FXT_MAIN a stand-alone program over the same source
// (for a sanitizer build: its own main, nothing loaded into Python).
//
// One group: the six coefficient lanes on six lock-stepped threads run the very routine the kernel runs (fxt_run: the program loop, the
// publishes, the six-term dots, the norm chain's inversion), the group's LDS region an array here and wave_sync() a barrier of the six.
// Every column accumulation is checked for overflow (BGLS_RX_CHECK), and every entry a lane publishes is checked against the bounds
// finalxt.hpp states: limbs below the top one under 2^28 in magnitude; a plain entry below 3.4 p in magnitude (a product's output lies in
// (-0.4 p, 3.4 p), a conjugate is its negative), an xi multiple below 34 p (alt-bn128) / 6.8 p (BLS12-381).
#include <type_traits>
#include <string.h>
#include <stdio.h>
#include <atomic>
#include <thread>
#define BGLS_RX_CHECK 1
#include "../../bgls_amd/csrc/pairing.hpp"
#include "../../bgls_amd/csrc/wire.hpp"
#include "../../bgls_amd/csrc/finalxt.hpp"

namespace bgls { int g_rx_overflow = 0; }
using namespace bgls;

static std::atomic<int> g_bound_broken{0};

template <class C>
struct HostGroup {
  typedef FXT<C> E;
  i32 lds[E::GROUP_DW];
  std::atomic<int> cnt{0}, gen{0};
  void barrier() {
    const int g = gen.load();
    if (cnt.fetch_add(1) == 5) {
      cnt.store(0);
      gen.fetch_add(1);
    } else {
      while (gen.load(std::memory_order_acquire) == g) std::this_thread::yield();
    }
  }
};

template <class C>
struct HostMem {
  typedef FXT<C> E;
  HostGroup<C>* g;
  Sx<C, SX_T> ld(int off) const {
    Sx<C, SX_T> r;
    for (int i = 0; i < E::N; ++i) r.v[i] = g->lds[off + i];
    return r;
  }
  void st(int off, const Sx<C, SX_T>& v) const {
    constexpr int N = E::N;
    const int entry = off / E::ES;
    const bool xi = entry >= 6 && ((entry - 6) & 1);
    for (int i = 0; i < N - 1; ++i)
      if (v.v[i] <= -(1 << 28) || v.v[i] >= (1 << 28)) g_bound_broken = 1;
    // the value against its bound by the two top limbs (the rest is below one unit of the lower of them)
    const double val = (double)v.v[N - 1] * 268435456.0 + (double)v.v[N - 2];
    const double p2 = (double)C::RX_P[N - 1] * 268435456.0 + (double)C::RX_P[N - 2];
    const double hi = xi ? (C::CURVE_ID == 0 ? 34.0 : 6.8) : 3.4, lo = -hi;
    if (val + 1.0 > hi * p2 || val - 1.0 < lo * p2) g_bound_broken = 1;
    for (int i = 0; i < N; ++i) g->lds[off + i] = v.v[i];
  }
  void sync() const { g->barrier(); }
};

static const int ORDER_POS[6] = {5, 2, 4, 1, 3, 0};

template <class C>
static void parse(const uint8_t* gt, X2<C, SX_T> (&x)[6]) {
  for (int j = 0; j < 6; ++j) {
    const uint8_t* p = gt + (size_t)(2 * ORDER_POS[j]) * C::FP_BYTES;
    x[j] = X2<C, SX_T>{sx_from_plain<C>(fp_from_be<C>(p + C::FP_BYTES)), sx_from_plain<C>(fp_from_be<C>(p))};
  }
}

// out_gt <- the program's result on the values a_gt (every temporary but 1) and b_gt (temporary 1), as k_finalxt_batch parses and writes them
template <class C>
static int run(const uint8_t* a_gt, const uint8_t* b_gt, const u32* prog, int len, int out_reg, uint8_t* out_gt) {
  if (out_reg < 0 || out_reg >= FxtK<C>::NT) return -1;
  for (int s = 0; s < len; ++s) {
    const u32 w = prog[s];
    if ((w & 15) > 4 || (int)((w >> 4) & 15) >= FxtK<C>::NT || (int)((w >> 8) & 15) >= FxtK<C>::NT) return -1;
    if (((w & 15) == FXT_MUL || (w & 15) == FXT_SCALE) && (int)((w >> 12) & 15) >= FxtK<C>::NT) return -1;
    if ((w & 15) == FXT_FROB && (((w >> 12) & 15) < 1 || ((w >> 12) & 15) > 3)) return -1;
  }
  g_rx_overflow = 0;
  g_bound_broken = 0;
  static HostGroup<C> group;
  memset(group.lds, 0, sizeof group.lds);
  X2<C, SX_T> x[6], y[6], r[6];
  parse<C>(a_gt, x);
  parse<C>(b_gt, y);
  std::thread th[6];
  for (int j = 0; j < 6; ++j)
    th[j] = std::thread([&, j] {
      HostMem<C> m{&group};
      r[j] = fxt_run<C>(m, j, true, x[j], y[j], prog, len, out_reg);
    });
  for (int j = 0; j < 6; ++j) th[j].join();
  for (int j = 0; j < 6; ++j) {
    const Fp2<C> v = {sx_to_mont<C>(r[j].c0), sx_to_mont<C>(r[j].c1)};
    uint8_t* o = out_gt + (size_t)(2 * ORDER_POS[j]) * C::FP_BYTES;
    fp_to_be<C>(o, fp_from_mont<C>(v.c1));
    fp_to_be<C>(o + C::FP_BYTES, fp_from_mont<C>(v.c0));
  }
  return (g_rx_overflow || g_bound_broken.load()) ? -3 : 0;
}

extern "C" {
// 0, -1 (a malformed program), -3 (a column overflow or a published entry outside its stated bound)
int ht_fxt_run(int cid, const uint8_t* a_gt, const uint8_t* b_gt, const uint32_t* prog, int len, int out_reg, uint8_t* out_gt) {
  return cid == 0 ? run<BN254>(a_gt, b_gt, prog, len, out_reg, out_gt) : run<BLS381>(a_gt, b_gt, prog, len, out_reg, out_gt);
}
int ht_fxt_final_exp(int cid, const uint8_t* gt, uint8_t* out_gt) {
  return cid == 0 ? run<BN254>(gt, gt, FxtK<BN254>::PROG, FxtK<BN254>::PROG_LEN, FxtK<BN254>::OUT_REG, out_gt)
                  : run<BLS381>(gt, gt, FxtK<BLS381>::PROG, FxtK<BLS381>::PROG_LEN, FxtK<BLS381>::OUT_REG, out_gt);
}
int ht_fxt_nt(int cid) { return cid == 0 ? FxtK<BN254>::NT : FxtK<BLS381>::NT; }
int ht_fxt_prog_len(int cid) { return cid == 0 ? FxtK<BN254>::PROG_LEN : FxtK<BLS381>::PROG_LEN; }
}

#ifdef FXT_MAIN
// the stand-alone form: the final exponentiation of 0, of 1 and of a fixed dense element on both curves; 0 must give 0 and 1 must give 1
int main() {
  int bad = 0;
  for (int cid = 0; cid < 2; ++cid) {
    const size_t fb = cid == 0 ? 32 : 48, g = 12 * fb;
    uint8_t in[576], out[576];
    memset(in, 0, sizeof in);
    if (ht_fxt_final_exp(cid, in, out) != 0) bad = 1;
    for (size_t i = 0; i < g; ++i) bad |= out[i] != 0;
    in[g - 1] = 1;
    if (ht_fxt_final_exp(cid, in, out) != 0) bad = 1;
    for (size_t i = 0; i < g; ++i) bad |= out[i] != (i == g - 1 ? 1 : 0);
    for (size_t i = 0; i < g; ++i) in[i] = (uint8_t)(i % fb == 0 ? 1 : 37 * i + 11);
    if (ht_fxt_final_exp(cid, in, out) != 0) bad = 1;
    printf("curve %d: %s\n", cid, bad ? "FAILED" : "ok");
  }
  return bad;
}
#endif
