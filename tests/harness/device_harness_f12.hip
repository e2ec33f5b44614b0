// TEST-ONLY: the Fp12 layer of the device harness -- a third translation unit of libdevice_harness.so (build_device_harness.py).  The
// cooperative Fp12 routines of finalx.hpp (carry-free 28-bit limbs) and finalexp.hpp (32-bit limbs) behind batched C exports, each in the
// block shape the product launches it in, so that tests/test_gpu_f12_arith.py can feed them the operand catalogue of tests/f12_cases.py
// and compare every result with Python integers.  Includes k_finalx.hip for kl::finalx / kl::finalx_batch (the product's own launchers,
// launched directly here); never linked into the product and exports nothing of the library's ABI.
//
// ONE ELEMENT PER BLOCK: block i reads element i as canonical big-endian GT bytes and writes GT bytes; the carry-free forms also write the
// raw limbs of every result slot (FX::SLOT words: six coefficients x {plain, xi multiple} x two halves of HS words, N limbs and HS - N
// padding words reported as 0).
//
//   form 0  fx/256  256 threads, FX::LDS_BYTES_PAIR (as k_finalx):       every fx op below
//   form 1  fx/128  128 threads, FX::LDS_BYTES (as k_reduce_fx):         fx_mul (ops 0, 9)
//   form 2  fx/1w   one wave, fx_mul1 (as k_miller_latx<1>):             ops 0, 9
//   form 3  fx/2w   192 threads, fx_mul2w on waves 0 and 1 after fx_mul2w_init, wave 2 does bounded LDS-free work (as k_miller_latx<2>):  ops 0, 9
//   form 4  fe/64   one wave, FE::LDS_BYTES (as k_final36 / k_gt_pow):   every fe op below
//
//   op 0   a b                                     (fe: want_xi = true)
//   op 1   fx_mul_pair, arg: 0 (a b | b b) in fresh slots, 1 d1 < 0 (a b | slot B untouched), 2 destinations = own first factors
//          (A <- a b | B <- b b), 3 one slot as both factors and destination (A <- a a | B <- b b), 4 destinations = the OTHER product's
//          factors (B <- a b | A <- b a).  Two results per element.
//   op 2   conj      op 3, 4, 5  frob 1, 2, 3      op 6  inverse      op 7  a^e (e: four words, top bit at nbits - 1; dst != a)
//   op 8   final exponentiation
//   op 9   chain of `steps` products in slot form, nothing canonicalised in between: acc <- a, then acc <- acc acc (arg 0) or acc <- acc b
//          (arg 1); `steps` results per element, one after every product
//   op 10  fe only: a b with want_xi = false, then fe_fix_xi       op 11  fe only: fe_cyclo_sqr (unitary input)
// fe ops other than 8 and 9 write a SECOND result, a x (the first result): the product reads its second factor's xi multiples, which the
// GT bytes of the first result do not show.
#include "../../bgls_amd/csrc/k_finalx.hip"
#include "dev_bufs.hpp"

using namespace bgls;

namespace {

enum { F_256 = 0, F_128, F_1W, F_2W, F_FE };
enum { S_A = FE_A, S_B = FE_B, S_D = FE_C, S_E = FE_Y0 };

__host__ __device__ constexpr int form_threads(int form) { return form == F_256 ? 256 : form == F_128 ? 128 : form == F_2W ? 192 : 64; }

// the wire order of k_finalx: lane k < 6 holds the w^k coefficient
__device__ __forceinline__ int wire_pos(int k) {
  const int order_pos[6] = {5, 2, 4, 1, 3, 0};
  return 2 * order_pos[k];
}

template <class C>
__device__ __forceinline__ void fx_from_bytes(int slot, const uint8_t* gt, int lane) {
  if (lane < 6) {
    const uint8_t* b = gt + (size_t)wire_pos(lane) * C::FP_BYTES;
    const Fp<C> im = fp_from_be<C>(b), re = fp_from_be<C>(b + C::FP_BYTES);
    fx_put<C>(slot, lane, X2<C, SX_T>{sx_from_plain<C>(re), sx_from_plain<C>(im)});
  }
}
// the first wave: canonical bytes and the slot's raw words (reads only)
template <class C>
__device__ __forceinline__ void fx_emit(int slot, uint8_t* out, i32* raw, int lane) {
  typedef FX<C> E;
  extern __shared__ u32 lds[];
  if (lane < 6) {
    const X2<C, SX_T> x = fx_ld2<C>(E::coef(slot, lane, 0));
    uint8_t* o = out + (size_t)wire_pos(lane) * C::FP_BYTES;
    fp_to_be<C>(o, fp_from_mont<C>(sx_to_mont<C>(x.c1)));
    fp_to_be<C>(o + C::FP_BYTES, fp_from_mont<C>(sx_to_mont<C>(x.c0)));
  }
  // a half is N limbs in HS words: no routine writes the HS - N words behind them (whatever the LDS held before), they are reported as 0
  for (int k = lane; k < E::SLOT; k += 64) raw[k] = k % E::HS < E::N ? (i32)lds[slot * E::SLOT + k] : 0;
}

template <class C, int FORM>
__device__ __forceinline__ void fx_prod(int d, int a, int b, u32& epoch) {
  if constexpr (FORM == F_256 || FORM == F_128) fx_mul<C>(d, a, b);
  else if constexpr (FORM == F_1W) fx_mul1<C>(d, a, b);
  else fx_mul2w<C>(d, a, b, ++epoch);
}

template <class C, int FORM>
__global__ void __launch_bounds__(form_threads(FORM)) k_dh_fx(int op, int arg, const uint8_t* a, const uint8_t* b, const u32* e, int nbits, int steps, int nout,
                                                              uint8_t* out, i32* raw, u32* sink) {
  typedef FX<C> E;
  constexpr size_t GTB = 12 * C::FP_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t blk = blockIdx.x;
  uint8_t* o = out + blk * nout * GTB;
  i32* rw = raw + blk * nout * E::SLOT;
  if (wave == 0) {
    fx_from_bytes<C>(op == 8 ? FE_F : S_A, a + blk * GTB, lane);
    fx_from_bytes<C>(S_B, b + blk * GTB, lane);
    if (op == 9) fx_from_bytes<C>(S_D, a + blk * GTB, lane);
    if constexpr (FORM == F_2W) {
      if (lane == 0) fx_mul2w_init<C>();
    }
  }
  __syncthreads();
  u32 epoch = 0;
  if constexpr (FORM == F_2W) {
    if (wave == 2) {                                     // takes no part in the product: bounded arithmetic in registers, one word out
      u32 x = (u32)blk + 1u;
      for (int k = 0; k < 4096; ++k) x = x * 1664525u + 1013904223u;
      if (lane == 0) sink[blk] = x;
      return;
    }
  }
  if (op == 0) {
    fx_prod<C, FORM>(S_D, S_A, S_B, epoch);
    if (wave == 0) fx_emit<C>(S_D, o, rw, lane);
    return;
  }
  if (op == 9) {
    for (int s = 0; s < steps; ++s) {
      fx_prod<C, FORM>(S_D, S_D, arg ? S_B : S_D, epoch);
      if (wave == 0) fx_emit<C>(S_D, o + s * GTB, rw + s * E::SLOT, lane);
    }
    return;
  }
  if constexpr (FORM == F_256) {
    int r0 = S_D, r1 = -1;
    switch (op) {
      case 1:
        if (arg == 0) { fx_mul_pair<C>(S_D, S_A, S_B, S_E, S_B, S_B); r1 = S_E; }
        else if (arg == 1) { fx_mul_pair<C>(S_D, S_A, S_B, -1, 0, 0); r1 = S_B; }
        else if (arg == 2) { fx_mul_pair<C>(S_A, S_A, S_B, S_B, S_B, S_B); r0 = S_A; r1 = S_B; }
        else if (arg == 3) { fx_mul_pair<C>(S_A, S_A, S_A, S_B, S_B, S_B); r0 = S_A; r1 = S_B; }
        else { fx_mul_pair<C>(S_B, S_A, S_B, S_A, S_B, S_A); r0 = S_B; r1 = S_A; }
        break;
      case 2: fx_conj<C>(S_D, S_A); break;
      case 3: case 4: case 5: fx_frob<C>(S_D, S_A, op - 2); break;
      case 6: fx_inv<C>(S_D, S_A, FE_X, FE_Y5, FE_Y6); break;
      case 7: fx_pow<C>(S_D, S_A, e, nbits, FE_T0); break;
      case 8: fx_final_exp<C>(); r0 = FE_F; break;
      default: return;
    }
    if (wave == 0) {
      fx_emit<C>(r0, o, rw, lane);
      if (r1 >= 0) fx_emit<C>(r1, o + GTB, rw + E::SLOT, lane);
    }
  }
}

template <class C>
__device__ __forceinline__ void fe_from_bytes(int slot, const uint8_t* gt, int lane) {
  if (lane < 6) {
    const uint8_t* b = gt + (size_t)wire_pos(lane) * C::FP_BYTES;
    const Fp<C> im = fp_from_be<C>(b), re = fp_from_be<C>(b + C::FP_BYTES);
    fe_put<C>(slot, lane, Fp2<C>{fp_to_mont<C>(re), fp_to_mont<C>(im)});
  }
}
template <class C>
__device__ __forceinline__ void fe_emit(int slot, uint8_t* out, int lane) {
  if (lane < 6) {
    const Fp2<C> v = lds_load_f2<C>(FE<C>::coef(slot, lane, 0));
    uint8_t* o = out + (size_t)wire_pos(lane) * C::FP_BYTES;
    fp_to_be<C>(o, fp_from_mont<C>(v.c1));
    fp_to_be<C>(o + C::FP_BYTES, fp_from_mont<C>(v.c0));
  }
}

template <class C>
__global__ void __launch_bounds__(64) k_dh_fe(int op, int arg, const uint8_t* a, const uint8_t* b, const u32* e, int nbits, int steps, int nout, uint8_t* out) {
  constexpr size_t GTB = 12 * C::FP_BYTES;
  const int lane = threadIdx.x;
  const size_t blk = blockIdx.x;
  uint8_t* o = out + blk * nout * GTB;
  fe_from_bytes<C>(op == 8 ? FE_F : S_A, a + blk * GTB, lane);
  fe_from_bytes<C>(S_B, b + blk * GTB, lane);
  if (op == 9) fe_from_bytes<C>(S_D, a + blk * GTB, lane);
  wave_sync();
  if (op == 9) {
    for (int s = 0; s < steps; ++s) {
      fe_mul<C>(S_D, S_D, arg ? S_B : S_D);
      fe_emit<C>(S_D, o + s * GTB, lane);
    }
    return;
  }
  switch (op) {
    case 0: fe_mul<C>(S_D, S_A, S_B); break;
    case 2: fe_conj<C>(S_D, S_A); break;
    case 3: case 4: case 5: fe_frob<C>(S_D, S_A, op - 2); break;
    case 6: fe_inv<C>(S_D, S_A); break;
    case 7: fe_pow<C>(S_D, S_A, e, nbits); break;
    case 8: fe_final_exp<C>(); fe_emit<C>(FE_F, o, lane); return;
    case 10: fe_mul<C>(S_D, S_A, S_B, false); fe_fix_xi<C>(S_D); break;
    case 11: fe_cyclo_sqr<C>(S_D, S_A); break;
    default: return;
  }
  fe_emit<C>(S_D, o, lane);
  fe_mul<C>(S_E, S_A, S_D);                              // reads the xi multiples of the result
  fe_emit<C>(S_E, o + GTB, lane);
}

int results_per_element(int form, int op, int steps) {
  if (op == 9) return steps;
  if (op == 1) return 2;
  return form == F_FE && op != 8 ? 2 : 1;
}

template <class C>
int f12_batch(int form, int op, int arg, size_t n, const uint8_t* a, const uint8_t* b, const u32* e4, int nbits, int steps, uint8_t* out, i32* raw) {
  typedef FX<C> E;
  constexpr size_t GTB = 12 * C::FP_BYTES;
  const bool fx_all = form == F_256 && ((op >= 0 && op <= 9));
  const bool fx_mul_only = (form == F_128 || form == F_1W || form == F_2W) && (op == 0 || op == 9);
  const bool fe_ok = form == F_FE && ((op >= 0 && op <= 11) && op != 1);
  if (!(fx_all || fx_mul_only || fe_ok)) return -1;
  if (op == 1 && (arg < 0 || arg > 4)) return -1;
  if (op == 9 && (steps < 1 || steps > 64 || arg < 0 || arg > 1)) return -1;
  if (op == 7 && (nbits < 1 || nbits > 128 || !((e4[(nbits - 1) >> 5] >> ((nbits - 1) & 31)) & 1u))) return -1;
  if (n == 0) return 0;
  if (n > 65535) return -1;
  const int nout = results_per_element(form, op, steps);
  const size_t ob = n * nout * GTB, rb = form == F_FE ? 0 : n * nout * E::SLOT * sizeof(i32);
  DevBufs d;
  uint8_t* da = (uint8_t*)d.get(n * GTB);
  uint8_t* db = (uint8_t*)d.get(n * GTB);
  u32* de = (u32*)d.get(4 * sizeof(u32));
  uint8_t* dout = (uint8_t*)d.get(ob);
  i32* draw = (i32*)d.get(rb);
  u32* dsink = (u32*)d.get(n * sizeof(u32));
  d.up(da, a, n * GTB);
  d.up(db, b, n * GTB);
  d.up(de, e4, 4 * sizeof(u32));
  if (d.err == hipSuccess) d.err = hipMemset(dout, 0, ob);
  if (d.err == hipSuccess && rb) d.err = hipMemset(draw, 0, rb);
  if (d.err == hipSuccess) {
    const unsigned g = (unsigned)n;
    if (form == F_256) k_dh_fx<C, F_256><<<g, 256, E::LDS_BYTES_PAIR>>>(op, arg, da, db, de, nbits, steps, nout, dout, draw, dsink);
    else if (form == F_128) k_dh_fx<C, F_128><<<g, 128, E::LDS_BYTES>>>(op, arg, da, db, de, nbits, steps, nout, dout, draw, dsink);
    else if (form == F_1W) k_dh_fx<C, F_1W><<<g, 64, E::LDS_BYTES + FX2W_EXTRA_BYTES>>>(op, arg, da, db, de, nbits, steps, nout, dout, draw, dsink);
    else if (form == F_2W) k_dh_fx<C, F_2W><<<g, 192, E::LDS_BYTES + FX2W_EXTRA_BYTES>>>(op, arg, da, db, de, nbits, steps, nout, dout, draw, dsink);
    else k_dh_fe<C><<<g, 64, FE<C>::LDS_BYTES>>>(op, arg, da, db, de, nbits, steps, nout, dout);
  }
  d.sync();
  d.down(out, dout, ob);
  if (rb) d.down(raw, draw, rb);
  return d.done();
}

// kl::finalx (batch == 0: ONE launch over `count` partials, one verdict word) or kl::finalx_batch (batch != 0: `count` instances of one
// partial each, `count` verdict words, inst_flags read per instance), with gt_out.  flags_out: the launch's flag word (FLAG_ENC).
template <class C>
int finalx_run(int batch, size_t count, int do_final_exp, const uint8_t* partials, const u32* inst_flags, uint8_t* gt_out, u32* verdicts, u32* flags_out) {
  constexpr size_t GTB = 12 * C::FP_BYTES;
  if (count == 0 || count > 65535) return -1;
  const size_t nres = batch ? count : 1;
  DevBufs d;
  uint8_t* dp = (uint8_t*)d.get(count * GTB);
  u32* dif = (u32*)d.get(count * sizeof(u32));
  uint8_t* dgt = (uint8_t*)d.get(nres * GTB);
  u32* dv = (u32*)d.get(nres * sizeof(u32));
  u32* df = (u32*)d.get(sizeof(u32));
  d.up(dp, partials, count * GTB);
  if (batch) d.up(dif, inst_flags, count * sizeof(u32));
  if (d.err == hipSuccess) d.err = hipMemset(dgt, 0, nres * GTB);
  if (d.err == hipSuccess) d.err = hipMemset(dv, 0xff, nres * sizeof(u32));
  if (d.err == hipSuccess) d.err = hipMemset(df, 0, sizeof(u32));
  if (d.err == hipSuccess) {
    if (batch) kl::finalx_batch<C>(nullptr, dp, count, dgt, dv, dif, df);
    else kl::finalx<C>(nullptr, dp, count, do_final_exp, dgt, dv, df);
  }
  d.sync();
  d.down(gt_out, dgt, nres * GTB);
  d.down(verdicts, dv, nres * sizeof(u32));
  d.down(flags_out, df, sizeof(u32));
  return d.done();
}

}  // namespace

extern "C" {
// curve 0 / 1; form, op, arg as above; a, b: n elements of GT bytes (b is read by every op: pass a again where it has no meaning);
// e4: four little-endian exponent words; out: n x results x GT bytes; raw: n x results x slot words (forms 0 .. 3; unused for form 4)
int dh_f12(int curve, int form, int op, int arg, size_t n, const uint8_t* a, const uint8_t* b, const uint32_t* e4, int nbits, int steps, uint8_t* out,
           int32_t* raw) {
  return curve == 0 ? f12_batch<BN254>(form, op, arg, n, a, b, e4, nbits, steps, out, raw)
       : curve == 1 ? f12_batch<BLS381>(form, op, arg, n, a, b, e4, nbits, steps, out, raw) : -1;
}
// results per element of dh_f12 and the words of one raw slot (0 for form 4)
int dh_f12_results(int form, int op, int steps) { return results_per_element(form, op, steps); }
int dh_f12_slot_words(int curve, int form) { return form == F_FE ? 0 : curve == 0 ? FX<BN254>::SLOT : FX<BLS381>::SLOT; }
int dh_f12_half_stride(int curve) { return curve == 0 ? FX<BN254>::HS : FX<BLS381>::HS; }
int dh_finalx(int curve, int batch, size_t count, int do_final_exp, const uint8_t* partials, const uint32_t* inst_flags, uint8_t* gt_out, uint32_t* verdicts,
              uint32_t* flags_out) {
  return curve == 0 ? finalx_run<BN254>(batch, count, do_final_exp, partials, inst_flags, gt_out, verdicts, flags_out)
       : curve == 1 ? finalx_run<BLS381>(batch, count, do_final_exp, partials, inst_flags, gt_out, verdicts, flags_out) : -1;
}
}
