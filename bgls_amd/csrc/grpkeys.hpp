// Grouped aggregate verification over a resident key set by signer bitmap (bgls_verify_aggregate_grouped_h / _keys_dev): the pure pieces
// -- the word / rank arithmetic of the selection pass (k_sel_count, k_sel_scatter in k_msggroup.hip) and the split of the groups into
// SMALL ones, summed by one lane pair each (k_sumpairgrp_main, k_sumpair.hip), and the others, cut into work items as before
// (msggroup.hpp) -- callable from the host, so that the CPU test tier checks them exhaustively (tests/harness/grpkeys_host.cpp,
// tests/test_grpkeys_host.py).
//
// Selection: ONE bitmap row over the key set's n keys, read as little-endian 32-bit words: key i is bit i & 31 of word i >> 5 (the bit
// rule of the subset calls, sumsel.hpp).  cnt[w] = the popcount of word w over the positions below n; rank = the exclusive scan of cnt;
// word w then writes its selected positions, ascending, to sel[rank[w] ..]: sel[0 .. k) are the selected key indices in ascending order.
// A bit at a position >= n is never named; it is reported as stray.
//
// Small / large: a group of at most `small` keys (the threshold of bgls_set_group_small, capped at GRPKEYS_SMALL_MAX; 0 = no group) gets
// NO work item: one lane pair adds its whole run.  Every other group is tiled by items exactly as msggroup_item tiles it.  Threshold 0
// reproduces the plan of msggroup.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "msggroup.hpp"

#if defined(__HIPCC__)
#define GRPKEYS_HD __host__ __device__ __forceinline__
#else
#define GRPKEYS_HD inline
#endif

namespace bgls {

// a lane pair adds a small group serially: beyond 128 keys (one lane pair's share of a full block item) the block pass is never worse
constexpr uint32_t GRPKEYS_SMALL_MAX = 128;
GRPKEYS_HD uint32_t grpkeys_small(size_t k) { return k > GRPKEYS_SMALL_MAX ? GRPKEYS_SMALL_MAX : (uint32_t)k; }

// words of a row that hold positions below n
GRPKEYS_HD size_t grpkeys_words(size_t n) { return (n + 31) / 32; }

// word w of the row with the positions >= n cleared; *stray = the word had a bit there
GRPKEYS_HD uint32_t grpkeys_word(uint32_t v, size_t n, size_t w, bool* stray) {
  const size_t base = w * 32;
  if (base >= n) {
    *stray = v != 0;
    return 0u;
  }
  const size_t rem = n - base;
  if (rem < 32) {
    *stray = (v >> rem) != 0;
    return v & ((1u << rem) - 1u);
  }
  *stray = false;
  return v;
}

// the selected positions of (cleared) word w to sel[rank ..], ascending; nothing at or beyond cap is written.  Returns the count.
GRPKEYS_HD uint32_t grpkeys_scatter(uint32_t v, size_t w, uint32_t rank, uint32_t cap, uint32_t* sel) {
  uint32_t c = 0;
  for (uint32_t bit = 0; bit < 32; ++bit) {
    if (!((v >> bit) & 1u)) continue;
    if (rank + c < cap) sel[rank + c] = (uint32_t)(w * 32) + bit;
    ++c;
  }
  return c;
}

// a group of `count` keys is summed by one lane pair
GRPKEYS_HD bool grpkeys_is_small(uint32_t count, uint32_t small) { return count <= small; }

// work items of a group: none for a small group
GRPKEYS_HD uint32_t grpkeys_items_of(uint32_t count, uint32_t chunk, uint32_t small) {
  return grpkeys_is_small(count, small) ? 0u : msggroup_items_of(count, chunk);
}

// The bound of the item count with the small groups removed.  A group with items has more than `small` keys, so there are at most
// min(d, n / (small + 1)) of them, and sum of ceil(c / K) over them <= their number + floor(n / K).  small = 0: msggroup_max_items.
GRPKEYS_HD size_t grpkeys_max_items(size_t n, size_t d, uint32_t chunk, uint32_t small) {
  const size_t big = n / ((size_t)small + 1);
  return (d < big ? d : big) + n / chunk;
}

}  // namespace bgls
