"""Shared by the tests of the grouped aggregate verification over a resident key set (bgls_verify_aggregate_grouped_h / _keys_dev):
instances over the key sets of tests/test_gpu_multi_subsets.py (key_set: made once per curve and size), signed by the engine's own signing
path (grouped_cases.sign), the calls in their host and device forms, and the run of one call under every small-group threshold."""
import ctypes
import random

import grouped_cases as gc
import test_gpu_multi_subsets as ms

B, out, offs = gc.B, gc.out, gc.offs
THRESHOLDS = (0, 8, 128, None)          # None: the default, whatever it is
DEFAULT_SMALL = 32


def deal(sub, group_sizes, seed, msg_len=32):
    """messages for the selected keys `sub` (ascending): group g's message goes to group_sizes[g] of them, dealt at random"""
    rnd = random.Random(seed)
    assert sum(group_sizes) == len(sub)
    distinct = []
    while len(distinct) < len(group_sizes):
        m = rnd.randbytes(msg_len)
        if m not in distinct:
            distinct.append(m)
    msgs = [distinct[g] for g, c in enumerate(group_sizes) for _ in range(c)]
    rnd.shuffle(msgs)
    return msgs


def instance(lib, cid, fp, n, sub, group_sizes, seed):
    """(handle, wire keys of the whole set, messages of the selected keys in ascending key order, aggregate signature, secret keys of the set)"""
    sks, keys, h = ms.key_set(lib, cid, fp, n)
    sub = sorted(sub)
    msgs = deal(sub, group_sizes, seed)
    return h, keys, msgs, gc.sign(lib, cid, fp, [sks[i] for i in sub], msgs), sks


def bitmap_of(n, sub, length=None):
    rows, stride = ms.rows_of(n, [sub], length)
    return bytes(rows)


def keys_host(lib, h, fp, sig, bitmap, msgs, bitmap_len=None):
    """(return code, n_groups, GT bytes) of bgls_verify_aggregate_grouped_h; bitmap None: everybody"""
    d = ctypes.c_size_t(12345)
    gt = out(12 * fp)
    rc = lib.bgls_verify_aggregate_grouped_h(h, B(sig), None if bitmap is None else B(bitmap), (len(bitmap) if bitmap is not None else 0) if bitmap_len is None else bitmap_len,
                                             B(b"".join(msgs)), offs([len(m) for m in msgs]), len(msgs), ctypes.byref(d), gt)
    return rc, d.value, bytes(gt)


def keys_dev(lib, h, fp, sig, bitmap, msgs, pad=0):
    """the same of bgls_verify_aggregate_grouped_keys_dev: the bitmap padded to whole 32-bit words, messages of one length at length + pad"""
    import torch
    n, ln = len(msgs), len(msgs[0]) if msgs else 0
    dev = lambda b: torch.frombuffer(bytearray(b or b"\0\0\0\0"), dtype=torch.uint8).to("cuda:0")
    t_sig, t_msgs = dev(sig), dev(b"".join(m + b"\x5A" * pad for m in msgs))
    t_map, map_len = None, 0
    if bitmap is not None:
        padded = bytes(bitmap) + bytes(-len(bitmap) % 4)
        t_map, map_len = dev(padded), len(padded)
        assert t_map.data_ptr() % 4 == 0
    d = ctypes.c_size_t(12345)
    gt = out(12 * fp)
    torch.cuda.synchronize()
    rc = lib.bgls_verify_aggregate_grouped_keys_dev(h, t_sig.data_ptr(), t_map.data_ptr() if t_map is not None else None, map_len, t_msgs.data_ptr(), ln, ln + pad, n,
                                                    ctypes.byref(d), gt, None)
    torch.cuda.synchronize()
    return rc, d.value, bytes(gt)


def under_thresholds(lib, fn, thresholds=THRESHOLDS):
    """fn() under bgls_set_group_small 0, 8, 128 and the default: the results are identical; returns one"""
    got = []
    try:
        for s in thresholds:
            assert lib.bgls_set_group_small(DEFAULT_SMALL if s is None else s) == 0
            got.append(fn())
    finally:
        lib.bgls_set_group_small(DEFAULT_SMALL)
    assert all(g == got[0] for g in got), "the result depends on the small-group threshold"
    return got[0]


def both_forms(lib, h, fp, sig, bitmap, msgs, want, thresholds=THRESHOLDS):
    got = under_thresholds(lib, lambda: keys_host(lib, h, fp, sig, bitmap, msgs), thresholds)
    assert got == want, ("host form", got[:2], want[:2])
    got = under_thresholds(lib, lambda: keys_dev(lib, h, fp, sig, bitmap, msgs), thresholds)
    assert got == want, ("device form", got[:2], want[:2])


def against_gathered(lib, cid, fp, h, keys, n, sub, sig, msgs, verdict, null_bitmap=False, thresholds=THRESHOLDS):
    """both forms under every threshold against the existing grouped call AND the ungrouped calls on the gathered keys"""
    gathered = ms.gather(keys, fp, sub)
    want = gc.ungrouped(lib, cid, fp, sig, gathered, msgs)
    assert want[0] == verdict, "the ungrouped call disagrees with the construction of the instance"
    assert gc.grouped_host(lib, cid, fp, sig, gathered, msgs) == want
    both_forms(lib, h, fp, sig, None if null_bitmap else bitmap_of(n, sub), msgs, want, thresholds)
    return want
