// Layout of a batch of independent aggregate verifications (bgls_verify_aggregate_batch) for ONE Miller launch: the hash points and
// keys of instance b are copied to padded positions pad_off[b] .. pad_off[b + 1] -- every instance starts on a group boundary of six
// pairings of k_miller_x60's 60-pairing block, so that a group partial never mixes two instances.  Pad slots get a G1 point at
// infinity and an all-zero key: k_miller_x60 turns both into the constant line 1, and a pad group's partial is exactly one.
#include "dev_common.hpp"
#include "launch.hpp"

namespace bgls {

// one thread per 32-bit word of a padded key; the thread of word 0 also places the hash point
template <class C>
__global__ void k_batch_scatter(const Aff<F1<C>>* g1s, const uint8_t* keys, const uint64_t* inst_off, const uint64_t* pad_off, uint32_t n_inst, size_t n_pad,
                                Aff<F1<C>>* g1_out, uint32_t* key_out) {
  constexpr int KW = 4 * C::FP_BYTES / 4;                   // words of a G2 wire key
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= n_pad * KW) return;
  const size_t s = t / KW;
  const int w = (int)(t % KW);
  uint32_t lo = 0, hi = n_inst;                             // pad_off[lo] <= s < pad_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (pad_off[mid] <= s) lo = mid;
    else hi = mid;
  }
  const size_t k = s - pad_off[lo];
  const bool real = k < inst_off[lo + 1] - inst_off[lo];
  const size_t src = inst_off[lo] + k;
  uint32_t word = 0;
  if (real) {
    const uint8_t* p = keys + src * (4 * C::FP_BYTES) + 4 * w;     // wire bytes: no alignment assumed
    word = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  }
  key_out[s * KW + w] = word;
  if (w == 0) {
    if (real) {
      g1_out[s] = g1s[src];
    } else {
      Aff<F1<C>> inf;
      memset(&inf, 0, sizeof inf);
      inf.inf = true;
      g1_out[s] = inf;
    }
  }
}

namespace kl {
template <class C>
void batch_scatter(hipStream_t st, const Aff<F1<C>>* g1s, const uint8_t* keys, const uint64_t* inst_off, const uint64_t* pad_off, size_t n_inst, size_t n_pad,
                   Aff<F1<C>>* g1_out, uint8_t* key_out) {
  constexpr size_t KW = 4 * C::FP_BYTES / 4;
  k_batch_scatter<C><<<nblk(n_pad * KW, 256), 256, 0, st>>>(g1s, keys, inst_off, pad_off, (uint32_t)n_inst, n_pad, g1_out, (uint32_t*)key_out);
}
template void batch_scatter<BN254>(hipStream_t, const Aff<F1<BN254>>*, const uint8_t*, const uint64_t*, const uint64_t*, size_t, size_t, Aff<F1<BN254>>*,
                                   uint8_t*);
template void batch_scatter<BLS381>(hipStream_t, const Aff<F1<BLS381>>*, const uint8_t*, const uint64_t*, const uint64_t*, size_t, size_t,
                                    Aff<F1<BLS381>>*, uint8_t*);
}  // namespace kl
}  // namespace bgls
