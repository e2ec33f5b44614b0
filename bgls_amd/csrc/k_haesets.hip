// Batched hashed aggregation exponents and weighted key sums (bgls_verify_multi_hae_sets: n_sets VerifyMultiSignatureWithHAE calls,
// bgls/blsHAE.go:56-58,74-93), the stages that are not shared with the plain multi-signature sets:
//   k_hae_root_seg     the BLAKE2Xb root of every set, one lane per set: one compression chain over the set's key bytes with the set's
//                      own XOF length (16 k_b) in the parameter block, as host_blake2::xb_root; sets rooted on the host are skipped and
//                      their roots copied from the uploaded list by the lanes above n_sets
//   k_hae_expand_seg   the XOF nodes of every set, one lane per 64-byte node (hashes.hpp blake2xb_node), from a node table built on the
//                      host; set b's exponents land at 16 key_off[b]
//   k_hae_wsum_main    P partial sums of t_i pk_i per set (P a power of two), one partial per lane on the carry-free limbs: each key is
//                      parsed, checked (FLAG_ENC, as the sum passes), multiplied by its 128-bit exponent (rx_g2mul.hpp jacx_mul_w4, exact
//                      for every point on the twist) and added (jacx_add); the partials leave in the library's Montgomery Jac<F2<C>> form
//                      for Engine::sum_sets_tree
#include "dev_common.hpp"
#include "hashes.hpp"
#include "rx_g2mul.hpp"
#include "launch.hpp"

namespace bgls {

__device__ __forceinline__ u64 hae_le64(const uint8_t* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const u64*>(p);
  u64 v = 0;
#pragma unroll
  for (int j = 7; j >= 0; --j) v = (v << 8) | p[j];
  return v;
}

// roots: n_sets x 8 words; host: n_host records of nine words (set index, root)
__global__ void __launch_bounds__(64) k_hae_root_seg(const uint8_t* keys, const uint64_t* key_off, size_t n_sets, unsigned g2b, size_t host_min,
                                                     const u64* host, size_t n_host, u64* roots) {
  const size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (b >= n_sets + n_host) return;
  if (b >= n_sets) {
    const u64* r = host + (b - n_sets) * 9;
#pragma unroll
    for (int k = 0; k < 8; ++k) roots[r[0] * 8 + k] = r[1 + k];
    return;
  }
  const size_t nk = key_off[b + 1] - key_off[b];
  if (nk == 0 || nk > host_min) return;                      // no exponents / rooted on the host
  const uint8_t* d = keys + key_off[b] * g2b;
  const size_t len = nk * g2b;
  const bool aligned = (reinterpret_cast<uintptr_t>(d) & 7) == 0;
  u64 h[8];
  blake2xb_root_init(h, (u32)(16 * nk));
  u64 m[16];
  size_t off = 0;
#pragma unroll 1
  for (; len - off > 128; off += 128) {
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = hae_le64(d + off + 8 * k, aligned);
    blake2b_compress(h, m, (u64)off + 128, false);
  }
  // the last non-empty block, zero-padded: keys are 64-byte multiples, so the rest is whole words
  const size_t rest = len - off;
#pragma unroll
  for (int k = 0; k < 16; ++k) m[k] = 8 * (size_t)k < rest ? hae_le64(d + off + 8 * k, aligned) : 0;
  blake2b_compress(h, m, (u64)len, true);
#pragma unroll
  for (int k = 0; k < 8; ++k) roots[b * 8 + k] = h[k];
}

// nodes[g] = (set, node index); t: 16-byte exponents at 16 key_off[set]
__global__ void __launch_bounds__(64) k_hae_expand_seg(const u64* roots, const uint2* nodes, size_t n_nodes, const uint64_t* key_off, uint8_t* t) {
  const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (g >= n_nodes) return;
  const uint2 nd = nodes[g];
  const size_t lo = key_off[nd.x];
  const u32 xof_len = (u32)(16 * (key_off[nd.x + 1] - lo));
  const u32 rest = xof_len - 64u * nd.y;
  const u32 take = rest < 64u ? rest : 64u;                  // the last node of a set with k_b mod 4 != 0 is a shorter digest, not a prefix
  u64 r[8], o[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = roots[(size_t)nd.x * 8 + k];
  blake2xb_node(r, nd.y, xof_len, take, o);
  u64* out = reinterpret_cast<u64*>(t + 16 * lo + (size_t)64 * nd.y);
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (8u * k < take) out[k] = o[k];
}

// lane g: set g / P, partial g % P over keys lo + g % P, lo + g % P + P, ...; t: 16-byte aligned
template <class C>
__global__ void __launch_bounds__(64) k_hae_wsum_main(const uint8_t* keys, const uint64_t* key_off, const uint8_t* t, size_t n_sets, unsigned P,
                                                      Jac<F2<C>>* out, uint32_t* flags) {
  constexpr size_t G2B = 4 * C::FP_BYTES;
  const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t b = g / P;
  if (b >= n_sets) return;
  const size_t lo = key_off[b], hi = key_off[b + 1];
  JacX<C> acc = jacx_inf<C>();
  bool bad = false;
#pragma unroll 1
  for (size_t k = lo + g % P; k < hi; k += P) {
    AffX<C> q;
    const bool ok = affx_from_bytes<C>(q, keys + k * G2B) && affx_on_curve<C>(q);
    if (!ok) {
      bad = true;
      continue;
    }
    const uint4 e = *reinterpret_cast<const uint4*>(t + 16 * k);        // big-endian magnitude -> little-endian words
    u32 w[4] = {__builtin_bswap32(e.w), __builtin_bswap32(e.z), __builtin_bswap32(e.y), __builtin_bswap32(e.x)};
    int top = -1;
    for (int j = 3; j >= 0 && top < 0; --j)
      if (w[j]) top = j * 32 + (31 - __clz(w[j]));
    acc = jacx_add<C>(acc, jacx_mul_w4<C>(q, w, top + 1));
  }
  if (bad) atomicOr(flags, FLAG_ENC);
  out[g] = jacx_to_mont<C>(acc);
}

namespace kl {
void hae_root_seg(hipStream_t st, const uint8_t* keys, const uint64_t* key_off, size_t n_sets, unsigned g2b, size_t host_min, const uint64_t* host,
                  size_t n_host, uint64_t* roots) {
  k_hae_root_seg<<<nblk(n_sets + n_host, 64), 64, 0, st>>>(keys, key_off, n_sets, g2b, host_min, (const u64*)host, n_host, (u64*)roots);
}
void hae_expand_seg(hipStream_t st, const uint64_t* roots, const uint32_t* nodes, size_t n_nodes, const uint64_t* key_off, uint8_t* t) {
  if (n_nodes) k_hae_expand_seg<<<nblk(n_nodes, 64), 64, 0, st>>>((const u64*)roots, (const uint2*)nodes, n_nodes, key_off, t);
}
template <class C>
void hae_wsum_main(hipStream_t st, const uint8_t* keys, const uint64_t* key_off, const uint8_t* t, size_t n_sets, unsigned P, void* out, uint32_t* flags) {
  k_hae_wsum_main<C><<<nblk(n_sets * P, 64), 64, 0, st>>>(keys, key_off, t, n_sets, P, (Jac<F2<C>>*)out, flags);
}
template void hae_wsum_main<BN254>(hipStream_t, const uint8_t*, const uint64_t*, const uint8_t*, size_t, unsigned, void*, uint32_t*);
template void hae_wsum_main<BLS381>(hipStream_t, const uint8_t*, const uint64_t*, const uint8_t*, size_t, unsigned, void*, uint32_t*);
}  // namespace kl
}  // namespace bgls
