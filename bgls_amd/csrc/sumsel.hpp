// Key sums driven by a signer bitmap over a resident key set (k_sumsel_main, k_sumpair.hip): the pure pieces -- which word of a
// bitmap row a lane sees, which windows a block takes, how many blocks a set gets -- callable from the host, so that the CPU test
// tier checks them exhaustively (tests/harness/sumsel_host.cpp, tests/test_sumsel_host.py).
//
// Bitmap: set b is a row over the key set's n keys; key i is selected iff (row[i >> 3] >> (i & 7)) & 1.  On the device a row is
// read as little-endian 32-bit words (key i is bit i & 31 of word i >> 5) at a stride that is a multiple of 4 bytes.
// A WINDOW is 2048 key positions: one word per lane of the wave.  Block c of the `per` blocks of a set takes windows
// c, c + per, c + 2 per, ...
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SUMSEL_HD __host__ __device__ __forceinline__
#else
#define SUMSEL_HD inline
#endif

namespace bgls {

constexpr unsigned SUMSEL_WINDOW = 2048;       // key positions per window: 64 lanes x 32 bits
// status bit of the planning pass (beside the FLAG_* of dev_common.hpp): a row has a bit at a position >= n
constexpr uint32_t FLAG_SUBSET_STRAY = 32u;

SUMSEL_HD size_t sumsel_windows(size_t n) { return (n + SUMSEL_WINDOW - 1) / SUMSEL_WINDOW; }

// The word lane `lane` of the wave works on in window `win`: bit j set = key win * 2048 + lane * 32 + j is to be added.  Plain mode:
// the row's word; complement mode: its inverse (the keys NOT selected).  Both with the positions >= n cleared, so no lane ever
// names a key beyond the set, whatever the row holds there.
SUMSEL_HD uint32_t sumsel_word(const uint32_t* row, size_t n, size_t win, unsigned lane, bool complement) {
  const size_t w = win * 64 + lane, base = w * 32;
  if (base >= n) return 0u;
  uint32_t v = row[w];
  if (complement) v = ~v;
  const size_t rem = n - base;
  if (rem < 32) v &= (1u << rem) - 1u;
  return v;
}

// first window of block c and the step to its next one
SUMSEL_HD size_t sumsel_first_window(unsigned c) { return c; }
SUMSEL_HD size_t sumsel_window_step(unsigned per) { return per; }

// Lane pairs per set (a power of two, 32 per one-wave block): the rule of Engine::sum_sets applied to n / 2 + 1 keys -- no mode
// ever adds more than half of the set, plus the whole-set sum -- and never more blocks than the set has windows.
inline size_t sumsel_pairs_per_set(size_t n, size_t nsets) {
  const size_t most = n / 2 + 1;
  size_t P = 32;
  while (P < 8192 && P * 4 <= most && nsets * P * 2 <= (size_t)131072 && P / 32 < sumsel_windows(n)) P *= 2;
  return P;
}

// complement mode of a row with `selected` bits among n keys: mode 0 chooses (the shorter side), 1 never, 2 always
SUMSEL_HD bool sumsel_complement(size_t selected, size_t n, int mode) {
  return mode == 1 ? false : mode == 2 ? true : 2 * selected > n;
}

#if defined(__HIPCC__)
namespace kl {
// ---- k_sumpair.hip   (the launchers of the planning pass and of the masked main pass; partials as in sumpairseg_main)
void sumsel_plan(hipStream_t st, const uint32_t* rows, size_t stride_w, size_t n, size_t nsets, int mode, uint32_t* plan, uint32_t* flags);
template <class C>
void sumsel_main(hipStream_t st, const uint8_t* recs, size_t n, const uint32_t* rows, size_t stride_w, const uint32_t* plan, const uint8_t* total, size_t nsets,
                 unsigned P, void* out);
}  // namespace kl
#endif

}  // namespace bgls
