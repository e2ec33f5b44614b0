// Batched accountable-subgroup multisignatures (bgls_ams_verify_batch: n AmsVerifySignature calls, bgls/blsAsmSigs.go:48-59,73-86), the
// stage that is not shared with the other batched verifications:
//   k_ams_msgs   the n + total hash inputs of a batch, one lane per input, into one blob with tight offsets (MsgView's offset form):
//                input b < n is 0x00 || m_b (getAmsH0), input n + s is 0x01 || apk_b wire bytes || decimal(signers[s]) for signer s of
//                item b (getAmsH2 over strconv.Itoa: ASCII decimal, no leading zeros, "0" for zero).  The offsets are a prefix of exact
//                lengths made on the host; a lane writes exactly the bytes between its two offsets, whatever the index says by then, so
//                no lane writes outside its input.  An item with an empty signer list gets its per-item flag word set (verdict 0).
#include "dev_common.hpp"
#include "launch.hpp"

namespace bgls {

__global__ void __launch_bounds__(64) k_ams_msgs(const uint8_t* apks, const uint32_t* signers, const uint64_t* signer_off, size_t n, size_t total, MsgView mv,
                                                 unsigned g2b, const uint64_t* hoff, uint8_t* blob, uint32_t* inst_flags) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n + total) return;
  uint8_t* o = blob + hoff[i];
  const size_t len = hoff[i + 1] - hoff[i];
  if (len == 0) return;
  if (i < n) {
    o[0] = 0x00;
    const uint8_t* m = mv.ptr(i);
#pragma unroll 1
    for (size_t k = 1; k < len; ++k) o[k] = m[k - 1];
    if (signer_off[i + 1] == signer_off[i]) inst_flags[i] = 1u;
    return;
  }
  // item of signer s: the last b < n with signer_off[b] <= s (signer_off[0] = 0, signer_off[n] = total > s)
  const size_t s = i - n;
  size_t lo = 0, hi = n;
#pragma unroll 1
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (signer_off[mid] <= s) lo = mid;
    else hi = mid;
  }
  o[0] = 0x01;
  const uint8_t* a = apks + lo * g2b;
  const size_t nkey = len - 1 < g2b ? len - 1 : g2b;
#pragma unroll 1
  for (size_t k = 0; k < nkey; ++k) o[1 + k] = a[k];
  // the low nd decimal digits of the index, most significant first (nd is the index's digit count where host and device agree)
  size_t nd = len - 1 - nkey;
  if (nd > 10) nd = 10;
  uint32_t v = signers[s];
#pragma unroll 1
  for (size_t k = nd; k > 0; --k) {
    o[1 + nkey + k - 1] = (uint8_t)('0' + v % 10u);
    v /= 10u;
  }
}

namespace kl {
void ams_msgs(hipStream_t st, const uint8_t* apks, const uint32_t* signers, const uint64_t* signer_off, size_t n, size_t total, MsgView mv, unsigned g2b,
              const uint64_t* hoff, uint8_t* blob, uint32_t* inst_flags) {
  k_ams_msgs<<<nblk(n + total, 64), 64, 0, st>>>(apks, signers, signer_off, n, total, mv, g2b, hoff, blob, inst_flags);
}
}  // namespace kl
}  // namespace bgls
