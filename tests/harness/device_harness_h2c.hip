// TEST-ONLY: the alt-bn128 hash-to-G1 schedules of k_hash.hip (k_h2c_bn_wide, k_h2c_bn_round<LPM>, k_h2c_bn_finish and the launcher
// kl::h2c_bn with its three hand-written schedules) compiled UNCHANGED, with the Keccak call replaced by a table lookup, so that a test
// can script which counters accept: a random message first accepts at counter k with probability 2^-(k + 1), and no message reaches
// the late rounds (tests/test_gpu_h2c_schedule.py).
//
// A scripted message is 8192 bytes, 256 digests of 32 bytes: the "hash" of (prefix byte c || message) is bytes 32 c .. 32 c + 31 of the
// message.  The digest of 0xFF is both candidate 255 and the sign hash, as in the reference, where both hash 0xFF || msg
// (curves/hash.go:53-77).
//
// hashes.hpp is included first, so `#pragma once` keeps the real keccak256_legacy out of the macro's reach; every later use of the name --
// h2c.hpp's three call sites and the wide kernel's own -- picks up the script.  The unit holds k_hash.hip a second time, so it is a shared
// object of its own (libdevice_harness_h2c.so), never linked with device_harness.hip's.
#include "../../bgls_amd/csrc/hashes.hpp"

namespace bgls {
inline BGLS_FN void dh_scripted_digest(const ByteSrc& src, u32 (&out_be)[8]) {
  const uint8_t* g = src.msg + 32 * (size_t)src.pre[0];
#pragma unroll
  for (int k = 0; k < 8; ++k) out_be[k] = ((u32)g[4 * k] << 24) | ((u32)g[4 * k + 1] << 16) | ((u32)g[4 * k + 2] << 8) | (u32)g[4 * k + 3];
}
}  // namespace bgls

#define keccak256_legacy dh_scripted_digest
#include "../../bgls_amd/csrc/k_hash.hip"
#undef keccak256_legacy
#include "dev_bufs.hpp"

namespace {

constexpr size_t SCRIPT_BYTES = 8192;

__global__ void __launch_bounds__(64) k_dh_h2c_to_bytes(size_t n, const Aff<F1<BN254>>* in, uint8_t* pts, uint8_t* inf) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Aff<F1<BN254>> a = in[i];
  g1_to_bytes<BN254>(pts + i * 64, a);
  inf[i] = a.inf ? 1 : 0;
}

}  // namespace

extern "C" {
// kl::h2c_bn on n scripted messages (blob: n x 8192 bytes), `lean` as the engine passes its throughput mode.  The work lists (2 n words) and
// the 64-byte counter block are allocated and zeroed as Engine::hash_to_g1 does.  Out: n x 64 big-endian affine bytes (zeros at infinity),
// n infinity bytes, the flag word, and the sixteen words of the counter block (cn[k]: the survivors of round k; all zero for n < 256).
// Returns 0, or a HIP error as a negative int (-1: bad argument).
int dh_h2c_bn(size_t n, int lean, const uint8_t* blob, uint8_t* pts, uint8_t* inf, uint32_t* flags, uint32_t* cn) {
  typedef BN254 C;
  if (n == 0 || n >= ((size_t)1 << 20)) return -1;
  DevBufs d;
  uint8_t* dblob = (uint8_t*)d.get(n * SCRIPT_BYTES);
  uint32_t* lists = (uint32_t*)d.get(2 * n * 4);
  uint32_t* dcn = (uint32_t*)d.get(64);
  uint32_t* dflags = (uint32_t*)d.get(16);
  Aff<F1<C>>* out = (Aff<F1<C>>*)d.get(n * sizeof(Aff<F1<C>>));
  uint8_t* dpts = (uint8_t*)d.get(n * 64);
  uint8_t* dinf = (uint8_t*)d.get(n);
  d.up(dblob, blob, n * SCRIPT_BYTES);
  if (d.err == hipSuccess) d.err = hipMemset(lists, 0, 2 * n * 4);
  if (d.err == hipSuccess) d.err = hipMemset(dcn, 0, 64);
  if (d.err == hipSuccess) d.err = hipMemset(dflags, 0, 16);
  if (d.err == hipSuccess) d.err = hipMemset(out, 0, n * sizeof(Aff<F1<C>>));     // a message that no kernel writes shows as (0, 0) with inf = 0
  if (d.err == hipSuccess) {
    const MsgView mv = {dblob, nullptr, SCRIPT_BYTES, SCRIPT_BYTES};
    kl::h2c_bn(nullptr, mv, n, lists, dcn, out, dflags, lean != 0);
    k_dh_h2c_to_bytes<<<nblk(n, 64), 64>>>(n, out, dpts, dinf);
  }
  d.sync();
  d.down(pts, dpts, n * 64);
  d.down(inf, dinf, n);
  d.down(flags, dflags, 4);
  d.down(cn, dcn, 64);
  return d.done();
}
}
