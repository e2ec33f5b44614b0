"""CPU tier: the work plan of the indexed key sum (bgls_amd/csrc/msggroup.hpp), compiled for the host (tests/harness/msggroup_host.cpp).
For every list of group sizes -- all ones, one group of n, one group of n / 2 plus singletons, sizes around one and two work items mixed
with ones, random sizes -- the items tile every group's run of the index list exactly once and in order, no item exceeds the `chunk` keys of the call (msggroup_chunk(n): 128 to 4096), the
items of a group are consecutive (item_start), and there are at most d + floor(n / chunk) of them.  The message hash compiled for the host
is checked against a Python restatement: the table's placement rule is the duplicate scan's."""
import ctypes
import importlib.util
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness():
    spec = importlib.util.spec_from_file_location("build_harness_msggroup", os.path.join(ROOT, "tests", "harness", "build_harness_msggroup.py"))
    bh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bh)
    lib = ctypes.CDLL(bh.build())
    u8p, u32p, u64p, sz = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t
    lib.msggroup_chunk_of.restype = ctypes.c_uint32
    lib.msggroup_chunk_of.argtypes = [sz]
    lib.msggroup_max_items_of.restype = sz
    lib.msggroup_max_items_of.argtypes = [sz, sz, ctypes.c_uint32]
    lib.msggroup_hash_of.restype = ctypes.c_uint64
    lib.msggroup_hash_of.argtypes = [u8p, sz, ctypes.c_uint64]
    lib.msggroup_plan.restype = sz
    lib.msggroup_plan.argtypes = [u32p, sz, u64p, u32p, u32p, u32p, sz, ctypes.c_uint32]
    return lib


def size_lists(chunk):
    rnd = random.Random(4096)
    n = 3 * chunk + 10
    yield "all ones", [1] * 300
    yield "one group of n", [n]
    yield "one group of n / 2 plus singletons", [1] * 7 + [n // 2] + [1] * (n - n // 2 - 7)
    yield "around one and two items, mixed with ones", [1, chunk - 1, 1, 1, chunk, chunk + 1, 1, 2 * chunk + 1, 1, 2 * chunk, 1, 2 * chunk - 1]
    yield "one key", [1]
    for k in range(4):
        yield "random %d" % k, [rnd.choice([1, 1, 2, 3, 40, chunk // 2, chunk, chunk + 7, 5 * chunk + 3]) for _ in range(rnd.randrange(1, 60))]
    yield "random small", [rnd.randrange(1, 9) for _ in range(1000)]


CHUNKS = [128, 129, 512, 4096]          # the least and the most keys per item, and two between


def test_keys_per_item_follow_the_call_size(harness):
    """n / 2048 keys per item, rounded up, between 128 and 4096: one large group spreads over the machine whatever n is"""
    want = {1: 128, 4100: 128, 1 << 16: 128, 1 << 18: 128, (1 << 18) + 1: 129, 1 << 20: 512, (1 << 23) - 1: 4096, 1 << 23: 4096, (1 << 30) - 1: 4096}
    assert {n: harness.msggroup_chunk_of(n) for n in want} == want
    assert all(harness.msggroup_chunk_of(n) <= harness.msggroup_chunk_of(n + 997) for n in range(1, 1 << 24, 65521))


@pytest.mark.parametrize("chunk", CHUNKS)
def test_items_tile_every_run_once_in_order_within_chunk_and_bound(harness, chunk):
    for name, sizes in size_lists(chunk):
        d, n = len(sizes), sum(sizes)
        bound = d + n // chunk
        assert harness.msggroup_max_items_of(n, d, chunk) == bound, name
        counts = (ctypes.c_uint32 * d)(*sizes)
        start = (ctypes.c_uint64 * (d + 1))()
        lo, hi, grp = ((ctypes.c_uint32 * (bound + 1))() for _ in range(3))
        items = harness.msggroup_plan(counts, d, start, lo, hi, grp, bound, chunk)
        assert items != ctypes.c_size_t(-1).value and items <= bound, (name, "more items than d + n // CHUNK", items, bound)
        assert start[0] == 0 and start[d] == items, name
        at = 0                                              # the position in the index list the next item must begin at
        t = 0
        for g, size in enumerate(sizes):
            assert start[g] == t, (name, "the items of a group are not consecutive", g)
            end = at + size
            while at < end:
                assert t < items and grp[t] == g, (name, g, t)
                assert lo[t] == at and lo[t] < hi[t] <= end, (name, "gap, overlap or an item across two groups", g, t, lo[t], hi[t])
                assert hi[t] - lo[t] <= chunk, (name, "an item above CHUNK", t)
                at = hi[t]
                t += 1
            assert start[g + 1] == t, name
        assert t == items and at == n, name


@pytest.mark.parametrize("chunk", CHUNKS)
def test_the_item_bound_is_reached_and_the_workspace_bound_refuses_one_less(harness, chunk):
    sizes = [chunk + 1] * 5 + [1] * (chunk - 5)             # n = 6 chunk: every large group spills one key into a second item
    d, n = len(sizes), sum(sizes)
    counts = (ctypes.c_uint32 * d)(*sizes)
    start = (ctypes.c_uint64 * (d + 1))()
    lo, hi, grp = ((ctypes.c_uint32 * (d + 8))() for _ in range(3))
    assert harness.msggroup_plan(counts, d, start, lo, hi, grp, d + 8, chunk) == d + 5 <= d + n // chunk
    assert harness.msggroup_plan(counts, d, start, lo, hi, grp, d + 4, chunk) == ctypes.c_size_t(-1).value


def test_message_hash_matches_its_restatement(harness):
    M = (1 << 64) - 1

    def h64(data, seed):
        h = 0xcbf29ce484222325 ^ seed
        for b in data:
            h = ((h ^ b) * 0x100000001b3) & M
        h ^= h >> 29
        h = (h * 0xbf58476d1ce4e5b9) & M
        return h ^ (h >> 32)
    rnd = random.Random(5)
    for ln in (0, 1, 7, 32, 33, 200):
        data = rnd.randbytes(ln)
        seed = rnd.getrandbits(64)
        buf = (ctypes.c_uint8 * max(ln, 1)).from_buffer_copy(data or b"\0")
        assert harness.msggroup_hash_of(buf, ln, seed) == h64(data, seed), ln
    a = (ctypes.c_uint8 * 4).from_buffer_copy(b"abcd")
    assert harness.msggroup_hash_of(a, 4, 1) != harness.msggroup_hash_of(a, 4, 2)
