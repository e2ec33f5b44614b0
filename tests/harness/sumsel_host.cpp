// TEST-ONLY: the pure pieces of the key sum by signer bitmap (bgls_amd/csrc/sumsel.hpp) compiled for the host, for
// tests/test_sumsel_host.py: the walk of k_sumsel_main over (block, window, lane) with the same helpers, counting how often each
// key position is named.
#include <string.h>
#include <vector>
#include "../../bgls_amd/csrc/sumsel.hpp"

using namespace bgls;

extern "C" {

// row: ceil(n / 8) bytes of a host bitmap row, repacked to whole 32-bit words as the engine stages it.  counts[i] += 1 for every time
// position i < n is named by some (block c < per, window of c, lane); *outside += 1 for every named position >= n.  Returns the windows walked.
size_t sumsel_walk(const uint8_t* row, size_t n, unsigned per, int complement, uint32_t* counts, uint64_t* outside) {
  std::vector<uint32_t> words((n + 31) / 32 + 1, 0u);
  if (n) memcpy(words.data(), row, (n + 7) / 8);
  size_t walked = 0;
  for (unsigned c = 0; c < per; ++c)
    for (size_t win = sumsel_first_window(c); win < sumsel_windows(n); win += sumsel_window_step(per), ++walked)
      for (unsigned lane = 0; lane < 64; ++lane) {
        uint32_t w = sumsel_word(words.data(), n, win, lane, complement != 0);
        const size_t base = win * SUMSEL_WINDOW + (size_t)lane * 32;
        for (; w; w &= w - 1) {
          const size_t pos = base + (size_t)__builtin_ctz(w);
          if (pos < n) counts[pos] += 1;
          else *outside += 1;
        }
      }
  return walked;
}

size_t sumsel_windows_of(size_t n) { return sumsel_windows(n); }
size_t sumsel_pairs_of(size_t n, size_t nsets) { return sumsel_pairs_per_set(n, nsets); }
int sumsel_complement_of(size_t selected, size_t n, int mode) { return sumsel_complement(selected, n, mode) ? 1 : 0; }

}  // extern "C"
