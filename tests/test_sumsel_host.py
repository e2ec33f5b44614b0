"""CPU tier: the pure helpers of the key sum by signer bitmap (bgls_amd/csrc/sumsel.hpp), compiled for the host
(tests/harness/sumsel_host.cpp).  For every set size around a word, a pair of words and a window, every row shape and both modes, the
union of the words over all (block, window, lane) is exactly the selected set -- or exactly its complement inside [0, n) -- and each
position is named once; nothing beyond n is ever named, whatever the row's last byte holds there."""
import ctypes
import importlib.util
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4100]


@pytest.fixture(scope="module")
def harness():
    spec = importlib.util.spec_from_file_location("build_harness_sumsel", os.path.join(ROOT, "tests", "harness", "build_harness_sumsel.py"))
    bh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bh)
    lib = ctypes.CDLL(bh.build())
    u8p, u32p, u64p, sz = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t
    lib.sumsel_walk.restype = sz
    lib.sumsel_walk.argtypes = [u8p, sz, ctypes.c_uint, ctypes.c_int, u32p, u64p]
    lib.sumsel_windows_of.restype = sz
    lib.sumsel_windows_of.argtypes = [sz]
    lib.sumsel_pairs_of.restype = sz
    lib.sumsel_pairs_of.argtypes = [sz, sz]
    lib.sumsel_complement_of.restype = ctypes.c_int
    lib.sumsel_complement_of.argtypes = [sz, sz, ctypes.c_int]
    return lib


def row_of(n, selected):
    row = bytearray((n + 7) // 8)
    for i in selected:
        row[i >> 3] |= 1 << (i & 7)
    return row


def rows(n):
    rnd = random.Random(n)
    yield "empty", set()
    yield "full", set(range(n))
    yield "first", {0}
    yield "last", {n - 1}
    for p in (0.1, 0.5, 0.9):
        yield "random %.1f" % p, {i for i in range(n) if rnd.random() < p}


def walk(lib, row, n, per, comp):
    counts = (ctypes.c_uint32 * n)()
    outside = ctypes.c_uint64(0)
    buf = (ctypes.c_uint8 * len(row)).from_buffer_copy(bytes(row))
    walked = lib.sumsel_walk(buf, n, per, comp, counts, ctypes.byref(outside))
    return list(counts), outside.value, walked


@pytest.mark.parametrize("n", NS)
def test_every_position_is_named_once_and_only_the_wanted_ones(harness, n):
    for name, sel in rows(n):
        row = row_of(n, sel)
        for comp in (0, 1):
            want = [1 if (i in sel) != bool(comp) else 0 for i in range(n)]
            for per in (1, 2, 3, 4, 16):
                counts, outside, walked = walk(harness, row, n, per, comp)
                assert outside == 0, (name, comp, per)
                assert counts == want, (name, comp, per)
                assert walked == harness.sumsel_windows_of(n), (name, comp, per)       # every window belongs to exactly one block


@pytest.mark.parametrize("n", [1, 31, 33, 63, 65, 2047, 2049, 4100])
def test_bits_beyond_n_in_the_last_byte_are_never_named(harness, n):
    """the tail mask of both modes: a stray bit (which the planning pass reports) must not reach the main pass as a key index"""
    assert n % 8
    sel = {0, n - 1}
    row = row_of(n, sel)
    row[-1] |= (0xFF << (n & 7)) & 0xFF
    for comp in (0, 1):
        counts, outside, _ = walk(harness, row, n, 2, comp)
        assert outside == 0
        assert counts == [1 if (i in sel) != bool(comp) else 0 for i in range(n)]


def test_windows_blocks_and_the_mode_rule(harness):
    lib = harness
    assert [lib.sumsel_windows_of(n) for n in (0, 1, 2048, 2049, 4100)] == [0, 1, 1, 2, 3]
    # lane pairs per set: Engine::sum_sets' rule on n / 2 + 1 keys, a power of two, at least one block, never more blocks than windows
    for n in (0, 1, 65, 2049, 4100, 1 << 12, 1 << 20):
        for nsets in (1, 12, 64, 1 << 12):
            P = lib.sumsel_pairs_of(n, nsets)
            assert P >= 32 and P & (P - 1) == 0 and P <= 8192
            assert P == 32 or (P // 2 * 4 <= n // 2 + 1 and nsets * (P // 2) * 2 <= 131072 and P // 64 < lib.sumsel_windows_of(n)), (n, nsets, P)
    assert lib.sumsel_pairs_of(1 << 12, 1 << 12) == 32 and lib.sumsel_pairs_of(1 << 20, 64) == 2048 and lib.sumsel_pairs_of(4100, 12) == 128
    # the mode: complement iff 2 * selected > n, unless forced
    for n, s, want in ((10, 5, 0), (10, 6, 1), (11, 5, 0), (11, 6, 1), (0, 0, 0), (1, 1, 1)):
        assert lib.sumsel_complement_of(s, n, 0) == want
        assert lib.sumsel_complement_of(s, n, 1) == 0 and lib.sumsel_complement_of(s, n, 2) == 1
