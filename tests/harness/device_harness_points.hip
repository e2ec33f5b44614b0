// TEST-ONLY: the point layer of the device harness -- a translation unit of its own, compiled in parallel with device_harness.hip
// (build_device_harness.py) and linked into the same libdevice_harness.so.  dh_padd / dh_pmul are the batched twins of the host
// harness's ht_rx_padd / ht_rx_pmul: the same statements (point_ops.hpp) around rx_jac1.hpp and rx_jac.hpp / rx_g2mul.hpp, compiled for
// gfx950, so that what only the device build has -- sx_montr on the inline-asm multiply rows, the chain's per-lane table indexed
// dynamically (scratch), its loops with a per-lane trip count and its per-lane branches into the doubling or infinity -- runs in waves
// whose lanes do different things (tests/test_gpu_point_arith.py).
//
// Element i runs on lane i mod 64 of block i / 64 (64-thread blocks).  ok[i] = 1, or 0 on a non-canonical / off-curve point or a bad
// lambda.  Returns 0, or a HIP error as a negative int (-1: bad argument).
#include "../../bgls_amd/csrc/dev_common.hpp"
#include "point_ops.hpp"
#include "dev_bufs.hpp"

using namespace bgls;

namespace {

constexpr int BS = 64;

// a, b: n points of PB wire bytes; za, zb: n lambdas of FP_BYTES; la, lb: n bytes, 0 = Z is one exactly (the lambda is not read)
template <class C, int G>
__global__ void __launch_bounds__(64) k_dh_padd(size_t n, const uint8_t* a, const uint8_t* za, const uint8_t* la, const uint8_t* b, const uint8_t* zb,
                                                const uint8_t* lb, const uint8_t* form, uint8_t* out, i32* raw, uint8_t* ok) {
  constexpr size_t FB = C::FP_BYTES, PB = 2 * G * FB;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool good;
  if constexpr (G == 1) good = pt1_add<C>(a + i * PB, za + i * FB, la[i], b + i * PB, zb + i * FB, lb[i], form[i], out + i * PB, raw + i * PT_RAW);
  else good = pt2_add<C>(a + i * PB, za + i * FB, la[i], b + i * PB, zb + i * FB, lb[i], form[i], out + i * PB, raw + i * PT_RAW);
  ok[i] = good ? 1 : 0;
}

// pts: n points; ks: n x 8 little-endian words; nbits: n ints in 0 .. 256
template <class C, int G>
__global__ void __launch_bounds__(64) k_dh_pmul(size_t n, const uint8_t* pts, const u32* ks, const int* nbits, uint8_t* out, i32* raw, uint8_t* ok) {
  constexpr size_t PB = 2 * G * C::FP_BYTES;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 k[8];
  for (int j = 0; j < 8; ++j) k[j] = ks[i * 8 + j];
  bool good;
  if constexpr (G == 1) good = pt1_mul<C>(pts + i * PB, k, nbits[i], out + i * PB, raw + i * PT_RAW);
  else good = pt2_mul<C>(pts + i * PB, k, nbits[i], out + i * PB, raw + i * PT_RAW);
  ok[i] = good ? 1 : 0;
}

template <class C, int G>
int padd_batch(size_t n, const uint8_t* a, const uint8_t* za, const uint8_t* la, const uint8_t* b, const uint8_t* zb, const uint8_t* lb, const uint8_t* form,
               uint8_t* out, i32* raw, uint8_t* ok) {
  constexpr size_t FB = C::FP_BYTES, PB = 2 * G * FB;
  for (size_t i = 0; i < n; ++i)
    if (form[i] > 4) return -1;
  if (n == 0) return 0;
  DevBufs d;
  uint8_t* din = (uint8_t*)d.get(n * (2 * PB + 2 * FB + 3));      // a | b | za | zb | la | lb | form
  uint8_t* dout = (uint8_t*)d.get(n * (PB + 1));                  // out | ok
  i32* draw = (i32*)d.get(n * PT_RAW * sizeof(i32));
  uint8_t *da = din, *db = da + n * PB, *dza = db + n * PB, *dzb = dza + n * FB, *dla = dzb + n * FB, *dlb = dla + n, *df = dlb + n;
  d.up(da, a, n * PB);
  d.up(db, b, n * PB);
  d.up(dza, za, n * FB);
  d.up(dzb, zb, n * FB);
  d.up(dla, la, n);
  d.up(dlb, lb, n);
  d.up(df, form, n);
  if (d.err == hipSuccess) d.err = hipMemset(dout, 0, n * (PB + 1));
  if (d.err == hipSuccess) d.err = hipMemset(draw, 0, n * PT_RAW * sizeof(i32));
  if (d.err == hipSuccess) k_dh_padd<C, G><<<nblk(n, BS), BS>>>(n, da, dza, dla, db, dzb, dlb, df, dout, draw, dout + n * PB);
  d.sync();
  d.down(out, dout, n * PB);
  d.down(ok, dout + n * PB, n);
  d.down(raw, draw, n * PT_RAW * sizeof(i32));
  return d.done();
}

template <class C, int G>
int pmul_batch(size_t n, const uint8_t* pts, const u32* ks, const int* nbits, uint8_t* out, i32* raw, uint8_t* ok) {
  constexpr size_t PB = 2 * G * C::FP_BYTES;
  for (size_t i = 0; i < n; ++i)
    if (nbits[i] < 0 || nbits[i] > 256) return -1;
  if (n == 0) return 0;
  DevBufs d;
  uint8_t* dp = (uint8_t*)d.get(n * PB);
  u32* dk = (u32*)d.get(n * 8 * sizeof(u32));
  int* dn = (int*)d.get(n * sizeof(int));
  uint8_t* dout = (uint8_t*)d.get(n * (PB + 1));
  i32* draw = (i32*)d.get(n * PT_RAW * sizeof(i32));
  d.up(dp, pts, n * PB);
  d.up(dk, ks, n * 8 * sizeof(u32));
  d.up(dn, nbits, n * sizeof(int));
  if (d.err == hipSuccess) d.err = hipMemset(dout, 0, n * (PB + 1));
  if (d.err == hipSuccess) d.err = hipMemset(draw, 0, n * PT_RAW * sizeof(i32));
  if (d.err == hipSuccess) k_dh_pmul<C, G><<<nblk(n, BS), BS>>>(n, dp, dk, dn, dout, draw, dout + n * PB);
  d.sync();
  d.down(out, dout, n * PB);
  d.down(ok, dout + n * PB, n);
  d.down(raw, draw, n * PT_RAW * sizeof(i32));
  return d.done();
}

}  // namespace

extern "C" {
// curve 0 / 1, group 1 / 2.  a, b: n points (2 or 4 FP_BYTES each); za, zb: n lambdas (FP_BYTES each); la, lb, form: n bytes each;
// out: n points; raw: n x PT_RAW int32; ok: n bytes
int dh_padd(int curve, int group, size_t n, const uint8_t* a, const uint8_t* za, const uint8_t* la, const uint8_t* b, const uint8_t* zb, const uint8_t* lb,
            const uint8_t* form, uint8_t* out, int32_t* raw, uint8_t* ok) {
  if (curve == 0 && group == 1) return padd_batch<BN254, 1>(n, a, za, la, b, zb, lb, form, out, raw, ok);
  if (curve == 0 && group == 2) return padd_batch<BN254, 2>(n, a, za, la, b, zb, lb, form, out, raw, ok);
  if (curve == 1 && group == 1) return padd_batch<BLS381, 1>(n, a, za, la, b, zb, lb, form, out, raw, ok);
  if (curve == 1 && group == 2) return padd_batch<BLS381, 2>(n, a, za, la, b, zb, lb, form, out, raw, ok);
  return -1;
}
int dh_pmul(int curve, int group, size_t n, const uint8_t* pts, const uint32_t* ks, const int* nbits, uint8_t* out, int32_t* raw, uint8_t* ok) {
  if (curve == 0 && group == 1) return pmul_batch<BN254, 1>(n, pts, ks, nbits, out, raw, ok);
  if (curve == 0 && group == 2) return pmul_batch<BN254, 2>(n, pts, ks, nbits, out, raw, ok);
  if (curve == 1 && group == 1) return pmul_batch<BLS381, 1>(n, pts, ks, nbits, out, raw, ok);
  if (curve == 1 && group == 2) return pmul_batch<BLS381, 2>(n, pts, ks, nbits, out, raw, ok);
  return -1;
}
}
