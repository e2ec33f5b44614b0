// TEST-ONLY: the work plan of the indexed key sum (bgls_amd/csrc/msggroup.hpp) compiled for the host, for tests/test_msggroup_host.py:
// the walk of k_grp_nitems, the exclusive scan and k_grp_items over a list of group sizes with the same helpers.
#include <stddef.h>
#include <stdint.h>
#include "../../bgls_amd/csrc/msggroup.hpp"

using namespace bgls;

extern "C" {

uint32_t msggroup_chunk_of(size_t n) { return msggroup_chunk(n); }
size_t msggroup_max_items_of(size_t n, size_t d, uint32_t chunk) { return msggroup_max_items(n, d, chunk); }
uint64_t msggroup_hash_of(const uint8_t* p, size_t n, uint64_t seed) { return msg_hash64(p, n, seed); }

// counts: the d group sizes, in the order of the groups' runs in the index list; chunk: keys per item.  item_start: d + 1 entries; item_lo / item_hi / item_group:
// room for `cap` items.  Returns the number of items, or SIZE_MAX where they do not fit in cap (nothing is written past cap).
size_t msggroup_plan(const uint32_t* counts, size_t d, uint64_t* item_start, uint32_t* item_lo, uint32_t* item_hi, uint32_t* item_group, size_t cap,
                     uint32_t chunk) {
  uint64_t at = 0;
  uint32_t start = 0;
  bool fits = true;
  for (size_t g = 0; g < d; ++g) {
    item_start[g] = at;
    const uint32_t cnt = msggroup_items_of(counts[g], chunk);
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
