// TEST-ONLY: the device twin of host_harness.cpp.  The same arithmetic headers, compiled for gfx950 and run in 64-lane waves, so that
// the code that exists only under __HIP_DEVICE_COMPILE__ -- the wave-uniform exits of fp_inv_ds and fp_jacobi_phase (__ballot), the
// inline-asm multiply rows of rx.hpp / rx_rows_gen.hpp, the lane-strided LDS tables of the square-root powers, and the combine kernels'
// special kinds -- is diffed against Python integers in tests/test_gpu_device_arith.py.  Includes k_hash.hip for its device functions
// and kernels; never linked into the product and exports nothing of the library's ABI.
//
// Every export takes a batch: element i runs on lane i mod 64 of block i / 64 (64-thread blocks, as the product launches them: the LDS
// layouts assume lane = threadIdx.x & 63).  A host wrapper allocates, copies, launches, synchronises and frees; it returns 0, or a HIP
// error as a negative int (-1: bad argument).
#include "../../bgls_amd/csrc/k_hash.hip"
#include "../../bgls_amd/csrc/wire.hpp"
#include "dev_bufs.hpp"

namespace {

constexpr int BS = 64;

// ---- Fp: the ht_fp_op op codes (0 mul, 1 sqr, 2 add, 3 sub, 4 neg, 5 fp_inv, 6 fp_sqrt_candidate, 7 fp_jacobi of the Montgomery
// value, 8 fp_jacobi of the plain value); canonical big-endian bytes in, converted to Montgomery form here.  Ops 7 / 8 write the
// symbol as an int32, the others FP_BYTES of big-endian result.
template <class C>
__global__ void __launch_bounds__(64) k_dh_fp(int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  constexpr int FB = C::FP_BYTES;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fp<C> x = fp_to_mont<C>(fp_from_be<C>(a + i * FB));
  const Fp<C> y = fp_to_mont<C>(fp_from_be<C>(b + i * FB));
  Fp<C> r;
  switch (op) {
    case 0: r = fp_mul<C>(x, y); break;
    case 1: r = fp_sqr<C>(x); break;
    case 2: r = fp_add<C>(x, y); break;
    case 3: r = fp_sub<C>(x, y); break;
    case 4: r = fp_neg<C>(x); break;
    case 5: r = fp_inv<C>(x); break;
    case 6: r = fp_sqrt_candidate<C>(x); break;
    case 7: reinterpret_cast<int32_t*>(out)[i] = fp_jacobi<C>(x); return;
    case 8: reinterpret_cast<int32_t*>(out)[i] = fp_jacobi<C>(fp_from_mont<C>(x)); return;
    default: return;
  }
  fp_to_be<C>(out + i * FB, fp_from_mont<C>(r));
}

// ---- Fp2 (re || im): 0 f2_mul, 1 f2_sqr, 2 f2_inv, 3 wire.hpp f2_sqrt, 4 wire.hpp f2_complex_quad_res.  Record: 2 FP_BYTES of
// result, then one byte of success bit (1 for ops 0..2).
template <class C>
__global__ void __launch_bounds__(64) k_dh_f2(int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  constexpr int FB = C::FP_BYTES;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fp2<C> x = {fp_to_mont<C>(fp_from_be<C>(a + i * 2 * FB)), fp_to_mont<C>(fp_from_be<C>(a + i * 2 * FB + FB))};
  const Fp2<C> y = {fp_to_mont<C>(fp_from_be<C>(b + i * 2 * FB)), fp_to_mont<C>(fp_from_be<C>(b + i * 2 * FB + FB))};
  Fp2<C> r = f2_zero<C>();
  bool ok = true;
  switch (op) {
    case 0: r = f2_mul<C>(x, y); break;
    case 1: r = f2_sqr<C>(x); break;
    case 2: r = f2_inv<C>(x); break;
    case 3: ok = f2_sqrt<C>(r, x); break;
    case 4: ok = f2_complex_quad_res<C>(r, x); break;
    default: return;
  }
  uint8_t* o = out + i * (2 * FB + 1);
  fp_to_be<C>(o, fp_from_mont<C>(r.c0));
  fp_to_be<C>(o + FB, fp_from_mont<C>(r.c1));
  o[2 * FB] = ok ? 1 : 0;
}

// ---- k_hash.hip rx_sqrt_pow<C, M1>: a^((p + 1) / 4), or a^((p - 3) / 4) with M1, with the LDS table declared as k_bls_sw_jacobi declares it
template <class C, bool M1>
__global__ void __launch_bounds__(64, 3) k_dh_rx_sqrt(size_t n, const uint8_t* in, uint8_t* out) {
  constexpr int FB = C::FP_BYTES;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  __shared__ i32 tab[rxp_lds_words<C>()];
  const Fp<C> a = fp_to_mont<C>(fp_from_be<C>(in + i * FB));
  fp_to_be<C>(out + i * FB, fp_from_mont<C>(rx_sqrt_pow<C, M1>(a, tab)));
}

// ---- rx.hpp on raw limbs, the ht_rx_raw op codes: A and B hold up to four Fp2 operands per element as [t][half][NL] u32 (stride
// 8 NL words), out = [half][NL] (stride 2 NL).  0 ux_dot_k2p<3>, 1 ux_sqr_dot (kinds in `arg`), 2 ux_mulxi(A[0]), 3 ux_sqr_dot3 (arg bit 0:
// odd row), 4 ux_quasi (arg 0x42 / 0x21).  The ht_rx_conv directions as two more ops: 16 = to_ux(a R) of the plain value whose L
// little-endian words are A[0 .. L), out NL limbs; 17 = from_ux of the NL limbs A[0 .. NL), out the L words of the plain value.
template <class C>
__global__ void __launch_bounds__(64) k_dh_rx_raw(int op, int arg, size_t n, const u32* A0, const u32* B0, u32* out0) {
  constexpr int N = C::RX_NL;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32* A = A0 + i * 8 * N;
  const u32* Bv = B0 + i * 8 * N;
  u32* out = out0 + i * 2 * N;
  auto ld = [&](const u32* base, int t, int h) { Ux<C> r; for (int k = 0; k < N; ++k) r.v[k] = base[(t * 2 + h) * N + k]; return r; };
  if (op == 16) {
    Fp<C> a;
    for (int k = 0; k < C::L; ++k) a.v[k] = A[k];
    const Ux<C> u = to_ux<C>(fp_to_mont<C>(a));
    for (int k = 0; k < N; ++k) out[k] = u.v[k];
    return;
  }
  if (op == 17) {
    Ux<C> u;
    for (int k = 0; k < N; ++k) u.v[k] = A[k];
    const Fp<C> a = fp_from_mont<C>(from_ux<C>(u));
    for (int k = 0; k < C::L; ++k) out[k] = a.v[k];
    return;
  }
  Ux2<C> r;
  if (op == 0) {
    r = ux_dot_k2p<C, 3>([&](int t, int h) { return ld(A, t, h); }, [&](int t, int h) { return ld(Bv, t, h); });
  } else if (op == 1) {
    if constexpr (rx_lazy<C>) r = ux_sqr_dot<C>([&](int t) { return (arg >> (2 * t)) & 3; }, [&](int t, int h) { return ld(A, t, h); }, [&](int t, int h) { return ld(Bv, t, h); });
    else return;
  } else if (op == 2) {
    const Ux2<C> a = {ld(A, 0, 0), ld(A, 0, 1)};
    r = ux_mulxi<C>(a);
  } else if (op == 3) {
    const bool twice = arg & 1;
    auto lm = [&](const u32* base, int t, int h, bool used) { Ux<C> v = ld(base, t, h); if (!used) for (int k = 0; k < N; ++k) v.v[k] = 0; return v; };
    if constexpr (!rx_lazy<C>)
      r = ux_sqr_dot3<C>([&](int t, int side, int h) { return side ? ld(Bv, t, h) : lm(A, t, h, true); },
                         [&](int t, int side, int h) { return side ? ld(Bv, 2 + t, h) : lm(A, 2 + t, h, !(twice && t == 1)); },
                         [&](int t) { return t == 0 && !twice; }, [&](int t) { return t == 0; }, twice);
    else return;
  } else if (op == 4) {
    const Ux2<C> a = {ld(A, 0, 0), ld(A, 0, 1)};
    if constexpr (!rx_lazy<C>) {
      if (arg == 0x42) r = ux_quasi<C, 4, 2>(a);
      else r = ux_quasi<C, 2, 1>(a);
    } else return;
  } else {
    return;
  }
  for (int k = 0; k < N; ++k) {
    out[k] = r.c0.v[k];
    out[N + k] = r.c1.v[k];
  }
}

// ---- k_bls_sw_jacobi with the 16 digest words read from a buffer (big-endian 64-byte digests, one per work item) instead of hashed
// from a message: the launch bounds, the work item and the LDS table are k_bls_sw_jacobi's
__global__ void __launch_bounds__(64, 3) k_dh_bls_sw_digest(const uint8_t* digests, size_t n_items, Jac<F1<BLS381>>* pts, uint32_t* kinds) {
  typedef BLS381 C;
  constexpr int N = C::RX_NL;
  size_t item = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (item >= n_items) return;
  u32 d[16];
  const uint8_t* g = digests + 64 * item;
  for (int k = 0; k < 16; ++k) d[k] = ((u32)g[4 * k] << 24) | ((u32)g[4 * k + 1] << 16) | ((u32)g[4 * k + 2] << 8) | g[4 * k + 3];
  __shared__ i32 tab[rxp_lds_words<C>()];
  const int lane = threadIdx.x & 63;
  auto ld = [&](int e, int i) { return tab[(e * N + i) * 64 + lane]; };
  auto st = [&](int e, int i, i32 w) { tab[(e * N + i) * 64 + lane] = w; };
  Jac<F1<C>> pt;
  const uint32_t kind = bls_sw_jac_x<RXP_W, rxp_e0reg<C>()>(d, pt, ld, st);
  kinds[item] = kind;
  if (kind == H2C_SW) pts[item] = pt;
}

// affine bytes of the SW work items (zeros for the other kinds), read before a combine kernel overwrites the work items
__global__ void __launch_bounds__(64) k_dh_items_to_bytes(size_t n_items, const Jac<F1<BLS381>>* pts, const uint32_t* kinds, uint8_t* out) {
  typedef BLS381 C;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  Aff<F1<C>> a = {fp_zero<C>(), fp_zero<C>(), true};
  if (kinds[i] == H2C_SW) a = jac_to_aff<F1<C>>(pts[i]);
  g1_to_bytes<C>(out + i * 2 * C::FP_BYTES, a);
}

__global__ void __launch_bounds__(64) k_dh_aff_to_bytes(size_t n, const Aff<F1<BLS381>>* in, uint8_t* out) {
  typedef BLS381 C;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  g1_to_bytes<C>(out + i * 2 * C::FP_BYTES, in[i]);
}

// ---- host side (DevBufs: dev_bufs.hpp)
template <class C>
int fp_batch(int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  if (op < 0 || op > 8) return -1;
  if (n == 0) return 0;
  const size_t in = n * C::FP_BYTES, on = op >= 7 ? n * 4 : in;
  DevBufs d;
  uint8_t* da = (uint8_t*)d.get(in);
  uint8_t* db = (uint8_t*)d.get(in);
  uint8_t* dout = (uint8_t*)d.get(on);
  d.up(da, a, in);
  d.up(db, b, in);
  if (d.err == hipSuccess) k_dh_fp<C><<<nblk(n, BS), BS>>>(op, n, da, db, dout);
  d.sync();
  d.down(out, dout, on);
  return d.done();
}

template <class C>
int f2_batch(int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  if (op < 0 || op > 4) return -1;
  if (n == 0) return 0;
  const size_t in = n * 2 * C::FP_BYTES, on = n * (2 * C::FP_BYTES + 1);
  DevBufs d;
  uint8_t* da = (uint8_t*)d.get(in);
  uint8_t* db = (uint8_t*)d.get(in);
  uint8_t* dout = (uint8_t*)d.get(on);
  d.up(da, a, in);
  d.up(db, b, in);
  if (d.err == hipSuccess) k_dh_f2<C><<<nblk(n, BS), BS>>>(op, n, da, db, dout);
  d.sync();
  d.down(out, dout, on);
  return d.done();
}

template <class C>
int rx_sqrt_batch(int m1, size_t n, const uint8_t* in, uint8_t* out) {
  if (n == 0) return 0;
  const size_t nb = n * C::FP_BYTES;
  DevBufs d;
  uint8_t* din = (uint8_t*)d.get(nb);
  uint8_t* dout = (uint8_t*)d.get(nb);
  d.up(din, in, nb);
  if (d.err == hipSuccess) {
    if (m1) k_dh_rx_sqrt<C, true><<<nblk(n, BS), BS>>>(n, din, dout);
    else k_dh_rx_sqrt<C, false><<<nblk(n, BS), BS>>>(n, din, dout);
  }
  d.sync();
  d.down(out, dout, nb);
  return d.done();
}

template <class C>
int rx_raw_batch(int op, int arg, size_t n, const u32* A, const u32* Bv, u32* out) {
  constexpr int N = C::RX_NL;
  const bool ok = op == 0 || op == 2 || op == 16 || op == 17 || (op == 1 && rx_lazy<C>) || (op == 3 && !rx_lazy<C>) ||
                  (op == 4 && !rx_lazy<C> && (arg == 0x42 || arg == 0x21));
  if (!ok) return -1;
  if (n == 0) return 0;
  const size_t in = n * 8 * N * sizeof(u32), on = n * 2 * N * sizeof(u32);
  DevBufs d;
  u32* da = (u32*)d.get(in);
  u32* db = (u32*)d.get(in);
  u32* dout = (u32*)d.get(on);
  d.up(da, A, in);
  d.up(db, Bv, in);
  if (d.err == hipSuccess) d.err = hipMemset(dout, 0, on);
  if (d.err == hipSuccess) k_dh_rx_raw<C><<<nblk(n, BS), BS>>>(op, arg, n, da, db, dout);
  d.sync();
  d.down(out, dout, on);
  return d.done();
}

}  // namespace

extern "C" {
// n elements of FP_BYTES (curve 0: 32, 1: 48) in a and b; out: n x FP_BYTES, or n int32 symbols for ops 7 / 8
int dh_fp_op(int curve, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  return curve == 0 ? fp_batch<BN254>(op, n, a, b, out) : curve == 1 ? fp_batch<BLS381>(op, n, a, b, out) : -1;
}
// n elements of 2 FP_BYTES (re || im); out: n records of 2 FP_BYTES + 1 (the success byte)
int dh_f2_op(int curve, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  return curve == 0 ? f2_batch<BN254>(op, n, a, b, out) : curve == 1 ? f2_batch<BLS381>(op, n, a, b, out) : -1;
}
// k_hash.hip rx_sqrt_pow<C, m1 != 0> on n canonical big-endian elements
int dh_rx_sqrt(int curve, int m1, size_t n, const uint8_t* in, uint8_t* out) {
  return curve == 0 ? rx_sqrt_batch<BN254>(m1, n, in, out) : curve == 1 ? rx_sqrt_batch<BLS381>(m1, n, in, out) : -1;
}
// curve 0 / 1 / 2 (alt-bn128 on ten 28-bit limbs / BLS12-381 / alt-bn128 on nine 29-bit limbs), as ht_rx_raw; A, B: n x 8 NL words,
// out: n x 2 NL words
int dh_rx_raw(int curve, int op, int arg, size_t n, const u32* A, const u32* Bv, u32* out) {
  if (curve == 0) return rx_raw_batch<BN254>(op, arg, n, A, Bv, out);
  if (curve == 1) return rx_raw_batch<BLS381>(op, arg, n, A, Bv, out);
  if (curve == 2) return rx_raw_batch<BN254W>(op, arg, n, A, Bv, out);
  return -1;
}
// BLS12-381 Shallue-van de Woestijne items from 2 n_msgs 64-byte digests (items 2 i, 2 i + 1 belong to message i), then the combine kernel
// that `form` selects: 0 k_bls_combine_raw_x, 1 k_bls_combine_raw_batched<4>, 2 k_bls_combine_x.  Out: the 2 n_msgs kinds, the 2 n_msgs
// items' affine bytes (96 each, zeros unless kind 3), the n_msgs combined points' affine bytes (96 each, zeros at infinity).
int dh_bls_sw(size_t n_msgs, const uint8_t* digests, int form, uint32_t* kinds_out, uint8_t* items_out, uint8_t* pts_out) {
  typedef BLS381 C;
  if (form < 0 || form > 2) return -1;
  if (n_msgs == 0) return 0;
  const size_t items = 2 * n_msgs, PB = 2 * C::FP_BYTES;
  DevBufs d;
  uint8_t* dig = (uint8_t*)d.get(items * 64);
  Jac<F1<C>>* pts = (Jac<F1<C>>*)d.get(items * sizeof(Jac<F1<C>>));
  uint32_t* kinds = (uint32_t*)d.get(items * 4);
  Aff<F1<C>>* aff = (Aff<F1<C>>*)d.get(n_msgs * sizeof(Aff<F1<C>>));
  uint8_t* ib = (uint8_t*)d.get(items * PB);
  uint8_t* ob = (uint8_t*)d.get(n_msgs * PB);
  d.up(dig, digests, items * 64);
  if (d.err == hipSuccess) d.err = hipMemset(pts, 0, items * sizeof(Jac<F1<C>>));
  if (d.err == hipSuccess) {
    k_dh_bls_sw_digest<<<nblk(items, 64), 64>>>(dig, items, pts, kinds);
    k_dh_items_to_bytes<<<nblk(items, 64), 64>>>(items, pts, kinds, ib);
    // the launch shapes of kl::h2c_bls
    if (form == 0) k_bls_combine_raw_x<<<nblk(n_msgs, 64), 64>>>(n_msgs, pts, kinds, aff);
    else if (form == 1) k_bls_combine_raw_batched<4><<<nblk((n_msgs + 3) / 4, 64), 64>>>(n_msgs, pts, kinds, aff);
    else k_bls_combine_x<<<nblk(n_msgs, 64), 64>>>(n_msgs, pts, kinds, aff);
    k_dh_aff_to_bytes<<<nblk(n_msgs, 64), 64>>>(n_msgs, aff, ob);
  }
  d.sync();
  d.down(kinds_out, kinds, items * 4);
  d.down(items_out, ib, items * PB);
  d.down(pts_out, ob, n_msgs * PB);
  return d.done();
}
}
