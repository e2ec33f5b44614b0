// Grouping of n messages by exact bytes on the device (bgls_group_messages, bgls_verify_aggregate_grouped): which messages are equal, the
// groups numbered in the order of their first occurrence, the signer indices sorted by group, the cut of every group's run into work items
// for the indexed key sum (k_sumpairidx_main, k_sumpair.hip; plan: msggroup.hpp), and the d representative messages compacted into an
// ordinary MsgView for the hashing pass.  Stages, one launch each (the host engine, Engine::group_messages, orders them):
//   k_grp_resolve   the duplicate scan's table (k_dup_check, k_hash.hip: open addressing, seeded msg_hash64, at least 2 n slots, probes
//                   without a bound, exact byte comparison) -- but a probe that meets byte-equal content records the slot instead of
//                   raising a flag: slot_of[i] = the slot message i's content lives in; first[slot] = the smallest such i (atomicMin)
//   k_grp_mark      rep[i] = 1 where i is the first occurrence of its content
//   scan            rank = exclusive scan of rep: a representative's rank is its group's number, rank[n] = d
//   k_grp_assign    representatives publish their number in their slot (the table is reused: slot -> group) and themselves in rep_idx
//   k_grp_groups    group_of[i], count[group] += 1
//   scan            start = exclusive scan of count (d + 1 offsets into the index list)
//   k_grp_scatter   idx[start[g] + cursor[g]++] = i: the index list, any order within a group (the sum does not depend on it)
//   k_grp_nitems, scan, k_grp_items      the work items {lo, hi} of every group, item_start[g] .. item_start[g + 1], and the join list: the
//                   groups of several items, one work item of the second pass each (their partials, contiguous by construction)
//   k_grp_lens, scan, k_grp_compact      the representatives' bytes, contiguous, behind d + 1 offsets (or at the fixed stride of the input)
// In front of all that, for bgls_verify_aggregate_grouped_h / _keys_dev (signers selected from a key set by ONE bitmap row; grpkeys.hpp):
//   k_sel_count, scan, k_sel_scatter     sel[0 .. k) = the selected key indices, ascending; a bit at a position >= n raises FLAG_SUBSET_STRAY.
//                   The grouping then runs over the k messages as it is: idx holds ranks, the key of position p is sel[idx[p]].
//                   With a threshold `small` the plan (k_grp_nitems) gives a group of at most that many keys no item: its sum is
//                   k_sumpairgrp_main's (k_sumpair.hip).
// After the key sum: k_grp_pick / k_grp_place put the partial of a one-item group and the joined sum of a several-item group in place.
// Contention: with all n messages equal every record meets ONE slot, ONE counter and ONE cursor.  The table word is read before it is
// CAS-ed (after the first insert everybody sees it taken), and the lanes of a wave that hold the same slot / group elect their lowest lane
// (same_key_lanes), which issues one atomic for all of them -- 64 times fewer atomics on one address where it matters, one per lane
// where all keys differ and nothing contends.
#include "dev_common.hpp"
#include "launch.hpp"
#include "msggroup.hpp"
#include "grpkeys.hpp"
#include "sumsel.hpp"

using namespace bgls;

namespace {

constexpr unsigned SCAN_T = 256, SCAN_PER = 8, SCAN_TILE = SCAN_T * SCAN_PER;      // threads per block, elements per thread, per block

// The active lanes of the wave that hold the same key as this lane, as a lane mask (0 for an inactive lane).  Every lane of the wave
// calls it: the loop is uniform, one turn per distinct key among the active lanes.
__device__ __forceinline__ unsigned long long same_key_lanes(uint32_t key, bool active) {
  unsigned long long todo = __ballot(active), mine = 0ull;
  while (todo) {
    const int leader = __ffsll(todo) - 1;
    const uint32_t k = (uint32_t)__shfl((int)key, leader, 64);
    const unsigned long long same = __ballot(active && key == k);
    if (active && key == k) mine = same;
    todo &= ~same;
  }
  return mine;
}
__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }

__device__ __forceinline__ bool msg_equal(const MsgView& mv, size_t j, const uint8_t* m, size_t len) {
  if (mv.size(j) != len) return false;
  const uint8_t* o = mv.ptr(j);
  for (size_t k = 0; k < len; ++k)
    if (o[k] != m[k]) return false;
  return true;
}

__global__ void __launch_bounds__(256) k_grp_resolve(MsgView mv, size_t n, uint32_t* table, uint32_t mask, uint32_t* first, uint32_t* slot_of, uint64_t seed) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const bool active = i < n;
  uint32_t slot = 0;
  if (active) {
    const uint8_t* m = mv.ptr(i);
    const size_t len = mv.size(i);
    slot = (uint32_t)msg_hash64(m, len, seed) & mask;
    for (;;) {                                              // the table has an empty slot at all times (>= 2 n slots): the walk ends
      uint32_t prev = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (prev == 0u) prev = atomicCAS(&table[slot], 0u, (uint32_t)i + 1u);
      if (prev == 0u || msg_equal(mv, prev - 1u, m, len)) break;
      slot = (slot + 1u) & mask;
    }
    slot_of[i] = slot;
  }
  // i grows with the lane: the lowest lane of those that share a slot holds their smallest index
  // and the word is read first: it only ever falls, so a value at or below i settles it without an atomic (a stale read costs one atomic more)
  const unsigned long long same = same_key_lanes(slot, active);
  if (active && lane_id() == (unsigned)(__ffsll(same) - 1) && __hip_atomic_load(&first[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)i)
    atomicMin(&first[slot], (uint32_t)i);
}

__global__ void __launch_bounds__(256) k_grp_mark(size_t n, const uint32_t* slot_of, const uint32_t* first, uint32_t* rep) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) rep[i] = first[slot_of[i]] == (uint32_t)i ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_grp_assign(size_t n, const uint32_t* rep, const uint32_t* rank, const uint32_t* slot_of, uint32_t* table, uint32_t* rep_idx) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n || !rep[i]) return;
  const uint32_t g = rank[i];
  table[slot_of[i]] = g;
  rep_idx[g] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) k_grp_groups(size_t n, const uint32_t* slot_of, const uint32_t* table, uint32_t* group_of, uint32_t* count) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const bool active = i < n;
  uint32_t g = 0;
  if (active) {
    g = table[slot_of[i]];
    group_of[i] = g;
  }
  const unsigned long long same = same_key_lanes(g, active);
  if (active && lane_id() == (unsigned)(__ffsll(same) - 1)) atomicAdd(&count[g], (uint32_t)__popcll(same));
}

__global__ void __launch_bounds__(256) k_grp_scatter(size_t n, const uint32_t* group_of, const uint32_t* start, uint32_t* cursor, uint32_t* idx) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const bool active = i < n;
  const uint32_t g = active ? group_of[i] : 0u;
  const unsigned long long same = same_key_lanes(g, active);
  const int leader = active ? __ffsll(same) - 1 : 0;
  uint32_t base = 0;
  if (active && lane_id() == (unsigned)leader) base = atomicAdd(&cursor[g], (uint32_t)__popcll(same));
  base = (uint32_t)__shfl((int)base, leader, 64);
  if (active) idx[start[g] + base + (uint32_t)__popcll(same & ((1ull << lane_id()) - 1ull))] = (uint32_t)i;
}

// items per group (none for a group of at most `small` keys: grpkeys.hpp), and the largest group to meta[0] (one atomic per wave)
__global__ void __launch_bounds__(256) k_grp_nitems(size_t d, const uint32_t* start, uint32_t chunk, uint32_t small, uint32_t* nitems, uint32_t* meta) {
  const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  uint32_t c = 0;
  if (g < d) {
    c = start[g + 1] - start[g];
    nitems[g] = grpkeys_items_of(c, chunk, small);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)c, s, 64);
    c = o > c ? o : c;
  }
  if (lane_id() == 0 && c) atomicMax(&meta[0], c);
}

// the items of every group; a group of several items also appends itself to the join list (meta[1] entries, any order): multi[k] = the
// group, joins[k] = {first, last + 1} of its partials -- one work item of the second pass
__global__ void __launch_bounds__(256) k_grp_items(size_t d, const uint32_t* start, const uint64_t* item_start, uint32_t chunk, uint2* items, uint2* joins,
                                                   uint32_t* multi, uint32_t* meta) {
  const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (g >= d) return;
  const uint32_t s = start[g], c = start[g + 1] - s;
  const uint64_t at = item_start[g];
  const uint32_t cnt = (uint32_t)(item_start[g + 1] - at);          // = grpkeys_items_of(c, chunk, small): 0 for a small group
  for (uint32_t k = 0; k < cnt; ++k) {
    uint32_t lo, hi;
    msggroup_item(s, c, k, chunk, &lo, &hi);
    items[at + k] = make_uint2(lo, hi);
  }
  if (cnt > 1) {
    const uint32_t pos = atomicAdd(&meta[1], 1u);
    multi[pos] = (uint32_t)g;
    joins[pos] = make_uint2((uint32_t)at, (uint32_t)at + cnt);
  }
}

// key sums to their places, 16 bytes per thread (rec_words 16-byte words per point).  k_grp_pick: group g of ONE item takes its partial,
// parts[item_start[g]]; k_grp_place: joined sum k goes to group multi[k].
__global__ void __launch_bounds__(256) k_grp_pick(size_t d, const uint64_t* item_start, const uint4* parts, unsigned rec_words, uint4* sums) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t g = t / rec_words;
  const unsigned w = (unsigned)(t % rec_words);
  if (g >= d) return;
  const uint64_t at = item_start[g];
  if (item_start[g + 1] - at == 1) sums[g * rec_words + w] = parts[at * rec_words + w];
}
__global__ void __launch_bounds__(256) k_grp_place(size_t m, const uint32_t* multi, const uint4* joined, unsigned rec_words, uint4* sums) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t k = t / rec_words;
  const unsigned w = (unsigned)(t % rec_words);
  if (k < m) sums[(size_t)multi[k] * rec_words + w] = joined[k * rec_words + w];
}

// ---- selection pass of the grouped verification over a key set (grpkeys.hpp): one bitmap row -> the selected key indices, ascending.
// k_sel_count: cnt[w] = popcount of word w below n, for the words that hold positions below n; every one of the row's row_words words
// is looked at, and a bit at a position >= n raises FLAG_SUBSET_STRAY.  The exclusive scan of cnt gives the ranks and, behind them, k.
// k_sel_scatter: word w names its positions at sel[rank[w] ..]; nothing at or beyond cap is written, whatever the row holds.
__global__ void __launch_bounds__(256) k_sel_count(const uint32_t* row, size_t row_words, size_t n, uint32_t* cnt, uint32_t* flags) {
  const size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  bool stray = false;
  if (w < row_words) {
    const uint32_t v = grpkeys_word(row[w], n, w, &stray);
    if (w < grpkeys_words(n)) cnt[w] = (uint32_t)__popc(v);
  }
  if (__ballot(stray) != 0 && lane_id() == 0) atomicOr(flags, FLAG_SUBSET_STRAY);
}
__global__ void __launch_bounds__(256) k_sel_scatter(const uint32_t* row, size_t n, const uint32_t* rank, uint32_t cap, uint32_t* sel) {
  const size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (w >= grpkeys_words(n)) return;
  bool stray;
  (void)grpkeys_scatter(grpkeys_word(row[w], n, w, &stray), w, rank[w], cap, sel);
}

__global__ void __launch_bounds__(256) k_grp_lens(MsgView mv, size_t d, const uint32_t* rep_idx, uint64_t* lens) {
  const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (g < d) lens[g] = mv.size(rep_idx[g]);
}

// eight lanes per representative; out_off == nullptr: fixed stride out_stride
__global__ void __launch_bounds__(256) k_grp_compact(MsgView mv, size_t d, const uint32_t* rep_idx, const uint64_t* out_off, size_t out_stride, uint8_t* out) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t g = t >> 3;
  if (g >= d) return;
  const size_t i = rep_idx[g];
  const uint8_t* m = mv.ptr(i);
  const size_t len = mv.size(i);
  uint8_t* o = out + (out_off ? (size_t)out_off[g] : g * out_stride);
  for (size_t k = t & 7; k < len; k += 8) o[k] = m[k];
}

// ---- device-wide exclusive scan, block scan plus offsets: k_scan_sums leaves one sum per tile of SCAN_TILE elements, k_scan_offsets (one
// block) turns them into the tiles' offsets, k_scan_apply scans each tile again behind its offset.  out has n + 1 entries: out[n] = the total.
template <class T>
__device__ __forceinline__ T block_excl_scan(T v, T* sh, T* total) {
  const unsigned t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (unsigned s = 1; s < SCAN_T; s <<= 1) {
    const T x = t >= s ? sh[t - s] : (T)0;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const T incl = sh[t];
  *total = sh[SCAN_T - 1];
  __syncthreads();
  return incl - v;
}
template <class TI, class TO>
__global__ void __launch_bounds__(SCAN_T) k_scan_sums(const TI* in, size_t n, TO* bsum) {
  __shared__ TO sh[SCAN_T];
  const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
  TO s = 0;
#pragma unroll
  for (unsigned k = 0; k < SCAN_PER; ++k)
    if (base + k < n) s += (TO)in[base + k];
  TO total;
  (void)block_excl_scan<TO>(s, sh, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
template <class TO>
__global__ void __launch_bounds__(SCAN_T) k_scan_offsets(TO* bsum, size_t nb) {
  __shared__ TO sh[SCAN_T];
  TO carry = 0;
  for (size_t base = 0; base < nb; base += SCAN_T) {
    const size_t b = base + threadIdx.x;
    const TO v = b < nb ? bsum[b] : (TO)0;
    TO total;
    const TO ex = block_excl_scan<TO>(v, sh, &total);
    if (b < nb) bsum[b] = carry + ex;
    carry += total;
  }
}
template <class TI, class TO>
__global__ void __launch_bounds__(SCAN_T) k_scan_apply(const TI* in, size_t n, const TO* bsum, TO* out) {
  __shared__ TO sh[SCAN_T];
  const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
  TO v[SCAN_PER];
  TO s = 0;
#pragma unroll
  for (unsigned k = 0; k < SCAN_PER; ++k) {
    v[k] = base + k < n ? (TO)in[base + k] : (TO)0;
    s += v[k];
  }
  TO total;
  TO run = bsum[blockIdx.x] + block_excl_scan<TO>(s, sh, &total);
#pragma unroll
  for (unsigned k = 0; k < SCAN_PER; ++k) {
    if (base + k < n) {
      out[base + k] = run;
      run += v[k];
      if (base + k == n - 1) out[n] = run;
    }
  }
}

}  // namespace

// ======================================================================= launchers
namespace bgls {
namespace kl {

size_t scan_tiles(size_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

template <class TI, class TO>
void scan_excl(hipStream_t st, const TI* in, size_t n, TO* bsum, TO* out) {
  if (n == 0) return;
  const size_t nb = scan_tiles(n);
  k_scan_sums<TI, TO><<<(unsigned)nb, SCAN_T, 0, st>>>(in, n, bsum);
  k_scan_offsets<TO><<<1, SCAN_T, 0, st>>>(bsum, nb);
  k_scan_apply<TI, TO><<<(unsigned)nb, SCAN_T, 0, st>>>(in, n, bsum, out);
}
template void scan_excl<uint32_t, uint32_t>(hipStream_t, const uint32_t*, size_t, uint32_t*, uint32_t*);
template void scan_excl<uint32_t, uint64_t>(hipStream_t, const uint32_t*, size_t, uint64_t*, uint64_t*);
template void scan_excl<uint64_t, uint64_t>(hipStream_t, const uint64_t*, size_t, uint64_t*, uint64_t*);

void grp_resolve(hipStream_t st, MsgView mv, size_t n, uint32_t* table, uint32_t mask, uint32_t* first, uint32_t* slot_of, uint64_t seed) {
  k_grp_resolve<<<nblk(n, 256), 256, 0, st>>>(mv, n, table, mask, first, slot_of, seed);
}
void grp_mark(hipStream_t st, size_t n, const uint32_t* slot_of, const uint32_t* first, uint32_t* rep) {
  k_grp_mark<<<nblk(n, 256), 256, 0, st>>>(n, slot_of, first, rep);
}
void grp_assign(hipStream_t st, size_t n, const uint32_t* rep, const uint32_t* rank, const uint32_t* slot_of, uint32_t* table, uint32_t* rep_idx) {
  k_grp_assign<<<nblk(n, 256), 256, 0, st>>>(n, rep, rank, slot_of, table, rep_idx);
}
void grp_groups(hipStream_t st, size_t n, const uint32_t* slot_of, const uint32_t* table, uint32_t* group_of, uint32_t* count) {
  k_grp_groups<<<nblk(n, 256), 256, 0, st>>>(n, slot_of, table, group_of, count);
}
void grp_scatter(hipStream_t st, size_t n, const uint32_t* group_of, const uint32_t* start, uint32_t* cursor, uint32_t* idx) {
  k_grp_scatter<<<nblk(n, 256), 256, 0, st>>>(n, group_of, start, cursor, idx);
}
void grp_nitems(hipStream_t st, size_t d, const uint32_t* start, uint32_t chunk, uint32_t small, uint32_t* nitems, uint32_t* meta) {
  k_grp_nitems<<<nblk(d, 256), 256, 0, st>>>(d, start, chunk, small, nitems, meta);
}
void sel_count(hipStream_t st, const uint32_t* row, size_t row_words, size_t n, uint32_t* cnt, uint32_t* flags) {
  k_sel_count<<<nblk(row_words, 256), 256, 0, st>>>(row, row_words, n, cnt, flags);
}
void sel_scatter(hipStream_t st, const uint32_t* row, size_t n, const uint32_t* rank, uint32_t cap, uint32_t* sel) {
  k_sel_scatter<<<nblk(grpkeys_words(n), 256), 256, 0, st>>>(row, n, rank, cap, sel);
}
void grp_items(hipStream_t st, size_t d, const uint32_t* start, const uint64_t* item_start, uint32_t chunk, void* items, void* joins, uint32_t* multi, uint32_t* meta) {
  k_grp_items<<<nblk(d, 256), 256, 0, st>>>(d, start, item_start, chunk, (uint2*)items, (uint2*)joins, multi, meta);
}
void grp_pick(hipStream_t st, size_t d, const uint64_t* item_start, const uint8_t* parts, size_t rec_bytes, uint8_t* sums) {
  k_grp_pick<<<nblk(d * (rec_bytes / 16), 256), 256, 0, st>>>(d, item_start, (const uint4*)parts, (unsigned)(rec_bytes / 16), (uint4*)sums);
}
void grp_place(hipStream_t st, size_t m, const uint32_t* multi, const uint8_t* joined, size_t rec_bytes, uint8_t* sums) {
  k_grp_place<<<nblk(m * (rec_bytes / 16), 256), 256, 0, st>>>(m, multi, (const uint4*)joined, (unsigned)(rec_bytes / 16), (uint4*)sums);
}
void grp_lens(hipStream_t st, MsgView mv, size_t d, const uint32_t* rep_idx, uint64_t* lens) {
  k_grp_lens<<<nblk(d, 256), 256, 0, st>>>(mv, d, rep_idx, lens);
}
void grp_compact(hipStream_t st, MsgView mv, size_t d, const uint32_t* rep_idx, const uint64_t* out_off, size_t out_stride, uint8_t* out) {
  k_grp_compact<<<nblk(d * 8, 256), 256, 0, st>>>(mv, d, rep_idx, out_off, out_stride, out);
}

}  // namespace kl
}  // namespace bgls
