"""CPU tier: the pure pieces of the grouped verification over a key set (bgls_amd/csrc/grpkeys.hpp), compiled for the host
(tests/harness/grpkeys_host.cpp).
Selection: for set sizes around the word, the window and the scan tile and rows that are empty, full, first only, last only and random at
10 / 50 / 90 %, the selection names exactly the selected positions, each once and ascending, nothing at or beyond n, and a bit at a
position >= n is reported as stray.
Plan: for thresholds 0, 1, 8 and 128 and group sizes around the threshold and the work item, every group is either ONE small slot that
covers its whole run or is tiled by items exactly as msggroup_item tiles it, the item count stays within grpkeys_max_items, and threshold 0
is the plan of msggroup.hpp (tests/harness/msggroup_host.cpp)."""
import ctypes
import importlib.util
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4100]
THRESHOLDS = [0, 1, 8, 128]
u32p, u64p, u8p, sz, u32 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t, ctypes.c_uint32


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "harness", name + ".py"))
    bh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bh)
    return ctypes.CDLL(bh.build())


@pytest.fixture(scope="module")
def harness():
    lib = _load("build_harness_grpkeys")
    lib.grpkeys_small_of.restype = u32
    lib.grpkeys_small_of.argtypes = [sz]
    lib.grpkeys_max_items_of.restype = sz
    lib.grpkeys_max_items_of.argtypes = [sz, sz, u32, u32]
    lib.grpkeys_select.restype = sz
    lib.grpkeys_select.argtypes = [u32p, sz, sz, u32p, u32, ctypes.POINTER(ctypes.c_int)]
    lib.grpkeys_plan.restype = sz
    lib.grpkeys_plan.argtypes = [u32p, sz, u64p, u32p, u32p, u32p, sz, u32, u32, u8p]
    return lib


@pytest.fixture(scope="module")
def old_plan():
    lib = _load("build_harness_msggroup")
    lib.msggroup_plan.restype = sz
    lib.msggroup_plan.argtypes = [u32p, sz, u64p, u32p, u32p, u32p, sz, u32]
    lib.msggroup_max_items_of.restype = sz
    lib.msggroup_max_items_of.argtypes = [sz, sz, u32]
    return lib


def rows(n):
    rnd = random.Random(1000 + n)
    yield "empty", set()
    yield "full", set(range(n))
    yield "first", {0}
    yield "last", {n - 1}
    for pct in (10, 50, 90):
        yield "random %d %%" % pct, {i for i in range(n) if rnd.randrange(100) < pct}


def words_of(positions, n_words):
    w = [0] * n_words
    for i in positions:
        w[i >> 5] |= 1 << (i & 31)
    return (ctypes.c_uint32 * max(n_words, 1))(*w)


def select(lib, positions, n, extra_words=0, cap=None):
    nw = (n + 31) // 32 + extra_words
    cap = n if cap is None else cap
    sel = (ctypes.c_uint32 * (cap + 8))(*([0xDEADBEEF] * (cap + 8)))
    stray = ctypes.c_int(-1)
    k = lib.grpkeys_select(words_of(positions, nw), nw, n, sel, cap, ctypes.byref(stray))
    assert list(sel)[cap:] == [0xDEADBEEF] * 8, "written beyond the capacity"
    return k, list(sel)[:min(k, cap)], stray.value


@pytest.mark.parametrize("n", SIZES)
def test_the_selection_names_the_selected_positions_once_and_ascending(harness, n):
    for name, pos in rows(n):
        k, sel, stray = select(harness, pos, n)
        assert (k, sel, stray) == (len(pos), sorted(pos), 0), (n, name)
        assert all(i < n for i in sel)


@pytest.mark.parametrize("n", SIZES)
def test_a_bit_beyond_the_set_is_stray_and_never_named(harness, n):
    for name, pos in rows(n):
        last_word_end = ((n + 31) // 32) * 32
        strays = [[last_word_end + 5], [last_word_end + 32 + 31]] + ([[n]] if n % 32 else []) + ([[last_word_end - 1]] if n % 32 else [])
        for extra in strays:
            k, sel, stray = select(harness, set(pos) | set(extra), n, extra_words=2)
            assert (k, sel, stray) == (len(pos), sorted(pos), 1), (n, name, extra)
        k, sel, stray = select(harness, pos, n, extra_words=2)
        assert (k, sel, stray) == (len(pos), sorted(pos), 0), (n, name, "zero words beyond the set are no stray")


def test_nothing_is_written_beyond_the_capacity(harness):
    """a row that selects more keys than the caller has messages: the count tells, the list stays within its room"""
    n = 2049
    k, sel, stray = select(harness, set(range(n)), n, cap=100)
    assert (k, sel, stray) == (n, list(range(100)), 0)


def test_the_threshold_is_capped_at_128(harness):
    assert [harness.grpkeys_small_of(k) for k in (0, 1, 8, 127, 128, 129, 1 << 40, ctypes.c_size_t(-1).value)] == [0, 1, 8, 127, 128, 128, 128, 128]


def size_lists(small):
    rnd = random.Random(77 + small)
    around = sorted({max(1, small - 1), max(1, small), small + 1})
    yield "around the threshold and the item", [1] + around + [128, 129, 4096, 4097, 1]
    yield "all ones", [1] * 300
    yield "one large group", [4097]
    yield "one key", [1]
    for k in range(4):
        yield "random %d" % k, [rnd.choice([1, 1, 2, 7, 8, 9, 127, 128, 129, 4096, 4097] + around) for _ in range(rnd.randrange(1, 60))]


def plan(lib, sizes, chunk, small):
    d, n = len(sizes), sum(sizes)
    cap = d + n // chunk + 4
    counts = (ctypes.c_uint32 * d)(*sizes)
    item_start = (ctypes.c_uint64 * (d + 1))()
    lo, hi, grp = (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * cap)()
    if small is None:
        m = lib.msggroup_plan(counts, d, item_start, lo, hi, grp, cap, chunk)
        slot = None
    else:
        slot = (ctypes.c_uint8 * d)()
        m = lib.grpkeys_plan(counts, d, item_start, lo, hi, grp, cap, chunk, small, slot)
        slot = list(slot)
    assert m != ctypes.c_size_t(-1).value, "the items do not fit the bound"
    return m, list(item_start), list(zip(list(lo)[:m], list(hi)[:m], list(grp)[:m])), slot


@pytest.mark.parametrize("chunk", [128, 512, 4096])
@pytest.mark.parametrize("small", THRESHOLDS)
def test_every_group_is_one_small_slot_or_tiled_by_items(harness, small, chunk):
    for name, sizes in size_lists(small):
        d, n = len(sizes), sum(sizes)
        m, item_start, items, slot = plan(harness, sizes, chunk, small)
        assert m <= harness.grpkeys_max_items_of(n, d, chunk, small), (name, "item bound")
        assert item_start[0] == 0 and item_start[d] == m
        start = 0
        for g, c in enumerate(sizes):
            mine = items[item_start[g]:item_start[g + 1]]
            if slot[g]:
                assert c <= small and mine == [], (name, g, "a small group has its slot and no item")
            else:
                assert c > small, (name, g)
                want = [(start + a, start + min(a + chunk, c), g) for a in range(0, c, chunk)]      # msggroup_item's tiling
                assert mine == want, (name, g)
            start += c


@pytest.mark.parametrize("chunk", [128, 512, 4096])
def test_threshold_zero_is_the_old_plan(harness, old_plan, chunk):
    for name, sizes in size_lists(8):
        new = plan(harness, sizes, chunk, 0)
        old = plan(old_plan, sizes, chunk, None)
        assert new[:3] == old[:3], name
        assert new[3] == [0] * len(sizes)
        d, n = len(sizes), sum(sizes)
        assert harness.grpkeys_max_items_of(n, d, chunk, 0) == old_plan.msggroup_max_items_of(n, d, chunk)
