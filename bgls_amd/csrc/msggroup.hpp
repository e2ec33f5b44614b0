// Grouping of messages by exact bytes and the work plan of the key sum that follows an index list (k_msggroup.hip, k_sumpairidx_main in
// k_sumpair.hip; bgls_group_messages, bgls_verify_aggregate_grouped): the pure pieces -- the seeded hash that places a message in the
// open-addressing table, and the cut of every group's run of the index list into work items -- callable from the host, so that the CPU
// test tier checks the plan exhaustively (tests/harness/msggroup_host.cpp, tests/test_msggroup_host.py).
//
// Plan: the signer indices are sorted by group into one index list; group g owns the run start[g] .. start[g] + count[g].  A WORK ITEM is
// at most `chunk` = msggroup_chunk(n) consecutive positions of one group's run, added by one block (32 lane pairs) into one partial sum.  The items of
// a group are consecutive -- item_start[g] .. item_start[g] + msggroup_items_of(count[g], chunk) -- and tile its run exactly once and in order,
// so the partials of a group are a contiguous set for the join.  Every group has at least one key, so there are at most
// d + floor(n / chunk) items for d groups over n keys (sum of ceil(c / K) <= d + floor(sum of (c - 1) / K)).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MSGGROUP_HD __host__ __device__ __forceinline__
#else
#define MSGGROUP_HD inline
#endif

namespace bgls {

// Keys per work item.  The most is one block's worth at full load -- 32 lane pairs x 128 keys each, where the block tree's five levels (as
// much as ~7 keys per pair) are 5 % of the item.  A call with fewer keys takes smaller items, so that ONE large group still spreads over
// the machine: n / 2048 keys per item is the rule of Engine::sum_points_jac (2048 one-wave blocks, two per SIMD), and never fewer than
// 128 (four keys per lane pair, its other bound).  The plan depends on n alone, not on the group sizes.
constexpr uint32_t MSGGROUP_CHUNK_MAX = 4096, MSGGROUP_CHUNK_MIN = 128;
MSGGROUP_HD uint32_t msggroup_chunk(size_t n) {
  const size_t c = (n + 2047) / 2048;
  return c < MSGGROUP_CHUNK_MIN ? MSGGROUP_CHUNK_MIN : c > MSGGROUP_CHUNK_MAX ? MSGGROUP_CHUNK_MAX : (uint32_t)c;
}

// `seed`: drawn by the host per process and call (engine_core.inc dup_seed).  The slot of a record must not be predictable from its bytes: an
// unseeded FNV can be inverted, and 2^20 chosen messages that share one slot turn the scan into 2^40 probes (the reference's Go map is
// seeded per process for the same reason, bgls/bgls.go:139-150).
MSGGROUP_HD uint64_t msg_hash64(const uint8_t* p, size_t n, uint64_t seed) {
  uint64_t h = 0xcbf29ce484222325ull ^ seed;
  for (size_t i = 0; i < n; ++i) {
    h ^= p[i];
    h *= 0x100000001b3ull;
  }
  h ^= h >> 29;
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 32;
  return h;
}

// work items of a group of `count` keys
MSGGROUP_HD uint32_t msggroup_items_of(uint32_t count, uint32_t chunk) { return (count + chunk - 1) / chunk; }

// positions [*lo, *hi) of the index list that item c (c < msggroup_items_of(count, chunk)) of the group at `start` takes
MSGGROUP_HD void msggroup_item(uint32_t start, uint32_t count, uint32_t c, uint32_t chunk, uint32_t* lo, uint32_t* hi) {
  const uint32_t a = c * chunk;
  const uint32_t b = count - a < chunk ? count : a + chunk;
  *lo = start + a;
  *hi = start + b;
}

// the bound of the item count: what the item workspace is sized by before the groups are known
MSGGROUP_HD size_t msggroup_max_items(size_t n, size_t d, uint32_t chunk) { return d + n / chunk; }

}  // namespace bgls
