// Hash inputs derived from the keys themselves, built on the device from keys that are already there (kl::key_msgs):
//   PREFIX  input i = the G2 wire bytes of key i, verbatim, followed by message i -- append(keys[i].MarshalUncompressed(), msgs[i]...),
//           the distinct-message defence (bgls/blsDistinctMessage.go:51).  k_key_prefix: KM_LANES lanes cooperate on one input and walk
//           consecutive bytes of it, so a wave's loads and stores are runs of whole rows.  Where source and destination of a piece (key
//           row, message) share their 16-byte alignment a lane moves 16 bytes per access; elsewhere the destination is cut at its own
//           dword boundaries and every dword is funnelled out of the two aligned source dwords that hold its bytes (one byte per lane only
//           for the at most three bytes in front of and behind the dwords).  Input i lies at out_off(i) = msg_off(i) - msg_off(0) + i G2B of
//           the blob, recomputed from the same offsets by every lane that writes it: a lane writes bytes of [out_off(i), out_off(i + 1))
//           only, and an input that would end beyond the blob's `cap` bytes is not written at all.  Messages in the offset form get the
//           n + 1 output offsets written beside the blob; messages of one length give a fixed-stride blob and no offsets.
//   POP     input i = the compressed form of key i and nothing else -- pubkey.Marshal(), the message of a proof of possession
//           (bgls/blsKosk.go:66): kl::compress_bn / kl::compress_bls straight into the blob, fixed stride G2B / 2; a key that does not
//           compress sets FLAG_ENC as in bgls_compress_points.
#include "dev_common.hpp"
#include "launch.hpp"
#include "../../include/bgls_hip.h"

namespace bgls {

constexpr unsigned KM_LANES = 16, KM_BLOCK = 256;      // lanes per input, threads per block (16 inputs per block, 4 per wave)

// n bytes from src to dst, any alignment of either, by the KM_LANES lanes of one group (lane = 0 .. KM_LANES - 1).  Aligned loads that
// reach beyond [src, src + n) stay inside an aligned dword that holds a byte of it; stores touch [dst, dst + n) only.
__device__ __forceinline__ void km_copy(uint8_t* dst, const uint8_t* src, size_t n, unsigned lane) {
  if (((((uintptr_t)dst) | ((uintptr_t)src)) & 15) == 0) {
    const size_t nv = n >> 4;
#pragma unroll 1
    for (size_t k = lane; k < nv; k += KM_LANES) ((uint4*)dst)[k] = ((const uint4*)src)[k];
    dst += nv << 4;
    src += nv << 4;
    n &= 15;
  }
  size_t head = (size_t)((0 - (uintptr_t)dst) & 3);
  if (head > n) head = n;
  if (lane < head) dst[lane] = src[lane];
  dst += head;
  src += head;
  n -= head;
  const size_t nd = n >> 2;
  const unsigned sh = (unsigned)((uintptr_t)src & 3) * 8;
  const uint32_t* sa = (const uint32_t*)(src - (sh >> 3));
  uint32_t* da = (uint32_t*)dst;
#pragma unroll 1
  for (size_t k = lane; k < nd; k += KM_LANES) {
    uint32_t w = sa[k];
    if (sh) w = (w >> sh) | (sa[k + 1] << (32 - sh));
    da[k] = w;
  }
  const size_t tail = n & 3;
  if (lane < tail) dst[(nd << 2) + lane] = src[(nd << 2) + lane];
}

__global__ void __launch_bounds__(KM_BLOCK) k_key_prefix(const uint8_t* keys, size_t n, MsgView mv, unsigned g2b, uint8_t* blob, size_t cap, uint64_t* out_off) {
  const size_t i = (blockIdx.x * (size_t)KM_BLOCK + threadIdx.x) / KM_LANES;
  const unsigned lane = threadIdx.x % KM_LANES;
  if (i >= n) return;
  const size_t mlen = mv.size(i);
  const size_t at = (mv.off ? (size_t)(mv.off[i] - mv.off[0]) : i * mv.len) + i * g2b;
  if (out_off && lane == 0) {
    out_off[i] = at;
    if (i + 1 == n) out_off[n] = at + g2b + mlen;
  }
  if (at > cap || g2b + mlen > cap - at) return;
  km_copy(blob + at, keys + i * g2b, g2b, lane);
  km_copy(blob + at + g2b, mv.ptr(i), mlen, lane);
}

namespace kl {
void key_msgs(hipStream_t st, int curve, int mode, const uint8_t* keys, size_t n, MsgView mv, uint8_t* blob, size_t cap, uint64_t* out_off, uint32_t* flags) {
  if (n == 0) return;
  const bool bls = curve == BGLS_CURVE_BLS12_381;
  if (mode == BGLS_KEYED_POP) {
    if (bls) compress_bls(st, BGLS_G2, keys, n, blob, flags);
    else compress_bn(st, BGLS_G2, keys, n, blob, flags);
    return;
  }
  k_key_prefix<<<nblk(n * KM_LANES, KM_BLOCK), KM_BLOCK, 0, st>>>(keys, n, mv, bls ? 192u : 128u, blob, cap, out_off);
}
}  // namespace kl
}  // namespace bgls
