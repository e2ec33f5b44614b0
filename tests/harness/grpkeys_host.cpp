// TEST-ONLY: the pure pieces of the grouped verification over a key set (bgls_amd/csrc/grpkeys.hpp) compiled for the host, for
// tests/test_grpkeys_host.py: the walk of k_sel_count, the exclusive scan and k_sel_scatter over one bitmap row, and the walk of
// k_grp_nitems, the scan and k_grp_items over a list of group sizes with a small-group threshold -- with the same helpers.
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../bgls_amd/csrc/grpkeys.hpp"

using namespace bgls;

extern "C" {

uint32_t grpkeys_small_of(size_t k) { return grpkeys_small(k); }
size_t grpkeys_max_items_of(size_t n, size_t d, uint32_t chunk, uint32_t small) { return grpkeys_max_items(n, d, chunk, small); }

// row: row_words 32-bit words over n keys; sel: room for cap entries.  Returns the number of selected keys (k); *stray = a bit at a position >= n.
size_t grpkeys_select(const uint32_t* row, size_t row_words, size_t n, uint32_t* sel, uint32_t cap, int* stray) {
  const size_t nw = grpkeys_words(n);
  std::vector<uint32_t> cnt(nw + 1, 0), rank(nw + 1, 0);
  *stray = 0;
  for (size_t w = 0; w < row_words; ++w) {
    bool s;
    const uint32_t v = grpkeys_word(row[w], n, w, &s);
    if (s) *stray = 1;
    if (w < nw) cnt[w] = (uint32_t)__builtin_popcount(v);
  }
  for (size_t w = 0; w < nw; ++w) rank[w + 1] = rank[w] + cnt[w];
  for (size_t w = 0; w < nw; ++w) {
    bool s;
    (void)grpkeys_scatter(grpkeys_word(row[w], n, w, &s), w, rank[w], cap, sel);
  }
  return rank[nw];
}

// counts: the d group sizes in the order of their runs; small_slot[g] = 1 where the group is summed by one lane pair (its whole run), else 0.
// Items as msggroup_plan (msggroup_host.cpp).  Returns the number of items, or SIZE_MAX where they do not fit in cap.
size_t grpkeys_plan(const uint32_t* counts, size_t d, uint64_t* item_start, uint32_t* item_lo, uint32_t* item_hi, uint32_t* item_group, size_t cap,
                    uint32_t chunk, uint32_t small, uint8_t* small_slot) {
  uint64_t at = 0;
  uint32_t start = 0;
  bool fits = true;
  for (size_t g = 0; g < d; ++g) {
    item_start[g] = at;
    small_slot[g] = grpkeys_is_small(counts[g], small) ? 1 : 0;
    const uint32_t cnt = grpkeys_items_of(counts[g], chunk, small);
    for (uint32_t c = 0; c < cnt; ++c) {
      if (at + c >= cap) {
        fits = false;
        continue;
      }
      msggroup_item(start, counts[g], c, chunk, &item_lo[at + c], &item_hi[at + c]);
      item_group[at + c] = (uint32_t)g;
    }
    at += cnt;
    start += counts[g];
  }
  item_start[d] = at;
  return fits ? (size_t)at : (size_t)-1;
}

}  // extern "C"
