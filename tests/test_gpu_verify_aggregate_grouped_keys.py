"""GPU tier: bgls_verify_aggregate_grouped_h / _keys_dev -- grouped aggregate verification whose keys are the sub-slice of a resident key
set that ONE signer bitmap selects.  Expected values come from code the feature does not run: bgls_verify_aggregate_grouped and the
ungrouped calls (bgls_verify_aggregate(..., 1), bgls_verify_aggregate_h_gt) on the gathered keys, and at the smallest shapes the C oracle.
Every result is taken under bgls_set_group_small 0, 8, 128 and the default and must not depend on it."""
import random

import pytest

import grouped_cases as gc
import grouped_keys_cases as gk
import stale_ws_cases as cat
import test_gpu_msm as mm
import test_gpu_multi_subsets as ms

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ENCODING = -1, -2
KEYS_PREPARE = 2


def split3(k, rnd):
    """three group sizes that sum to k (k >= 3), else k ones"""
    if k < 3:
        return [1] * k
    a = rnd.randrange(1, k - 1)
    b = rnd.randrange(1, k - a)
    return [a, b, k - a - b]


def test_no_signers(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    inf, other = bytes(2 * fp), cat.gen(lib, cid, 1)
    rc, h_empty = ms.upload(lib, cid, b"", 0)
    assert rc == 0
    _, _, h33 = ms.key_set(lib, cid, fp, 33)
    try:
        for sig, verdict in ((inf, 1), (other, 0)):
            want = (verdict, 0, cat.o_agg_gt(lib, cid, sig, [], []))
            assert cat.o_verdict(cid, want[2]) == verdict
            gk.both_forms(lib, h_empty, fp, sig, None, [], want)                      # NULL bitmap on an empty set
            gk.both_forms(lib, h33, fp, sig, gk.bitmap_of(33, []), [], want)          # an empty bitmap on a 33-key set
    finally:
        lib.bgls_keys_free(h_empty)


def test_one_key_and_seven_of_33_in_three_groups_against_the_oracle(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    for n, sub, sizes in ((1, [0], [1]), (33, [2, 3, 8, 16, 24, 31, 32], [4, 2, 1])):
        h, keys, msgs, sig, _ = gk.instance(lib, cid, fp, n, sub, sizes, 500 + n)
        want = gk.against_gathered(lib, cid, fp, h, keys, n, sub, sig, msgs, 1)
        gt = cat.o_agg_gt(lib, cid, sig, cat.cut(ms.gather(keys, fp, sub), 4 * fp), msgs)
        assert want == (cat.o_verdict(cid, gt), len(sizes), gt)


@pytest.mark.parametrize("n", [33, 65, 2049])
def test_bitmap_shapes(gpu_lib, curve, n):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    rnd = random.Random(n)
    shapes = [("first", [0]), ("last", [n - 1]), ("everyone", list(range(n))), ("every other", list(range(0, n, 2))), ("all but one", [i for i in range(n) if i != n // 3])]
    shapes += [("random %d" % pct, [i for i in range(n) if rnd.randrange(100) < pct] or [n // 2]) for pct in (10, 50, 90)]
    for name, sub in shapes:
        h, keys, msgs, sig, _ = gk.instance(lib, cid, fp, n, sub, split3(len(sub), rnd), 600 + n)
        want = gk.against_gathered(lib, cid, fp, h, keys, n, sub, sig, msgs, 1)
        assert want[1] == min(3, len(sub)), name
        if name == "everyone":
            gk.both_forms(lib, h, fp, sig, None, msgs, want)                          # ... and as the NULL bitmap


def test_the_selection_scan_over_more_than_one_tile(gpu_lib, curve):
    """65 537 keys are 2 049 words of the row: the prefix sum of the per-word popcounts spans two scan tiles of 2 048"""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 65537
    rnd = random.Random(65537)
    sub = sorted({i for i in range(n) if rnd.randrange(2)} | {n - 1})                                                   # the last word's one key takes part
    k = len(sub)
    sizes = [k // 64] * 63 + [k - 63 * (k // 64)]
    h, keys, msgs, sig, _ = gk.instance(lib, cid, fp, n, sub, sizes, 700)
    assert gk.against_gathered(lib, cid, fp, h, keys, n, sub, sig, msgs, 1, thresholds=(0, None))[1] == 64


def test_lane_pair_kernel_boundaries(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 2049
    rnd = random.Random(8)
    for sizes in ([1] * 31 + [7, 8, 9] + [1, 1], [1] * 70, [1, 2, 31, 32, 33, 127, 128, 129]):
        sub = sorted(rnd.sample(range(n), sum(sizes)))
        h, keys, msgs, sig, _ = gk.instance(lib, cid, fp, n, sub, sizes, 800 + len(sizes))
        assert gk.against_gathered(lib, cid, fp, h, keys, n, sub, sig, msgs, 1)[1] == len(sizes)


def test_exceptional_points_in_one_group(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    r = mm.ORDER[cid]
    a, b, c, e = 0x1234567, 0x7654321, 0xABCDEF1, 0x13579BD
    m0, m1, m2 = b"m0" * 16, b"m1" * 16, b"m2" * 16
    # group m0 holds a twice (the doubling branch); group m1 holds b and -b, whose sum is the point at infinity (the factor 1)
    sks = [a, b, e, a, r - b, c]
    msgs = [m0, m1, m2, m0, m1, m0]
    _, keys, h = ms.key_set(lib, cid, fp, 6, sks=sks)
    sig = gc.sign(lib, cid, fp, sks, msgs)
    for thresholds in ((0,), (8,)):
        want = gk.against_gathered(lib, cid, fp, h, keys, 6, list(range(6)), sig, msgs, 1, thresholds=thresholds)
        assert want[1] == 3
        gk.both_forms(lib, h, fp, sig, None, msgs, want, thresholds)
        # the two-signer instance {b, -b}: no factor at all, and the signature is the point at infinity
        sig2 = gc.sign(lib, cid, fp, [b, r - b], [m1, m1])
        assert sig2 == bytes(2 * fp)
        want = gk.against_gathered(lib, cid, fp, h, keys, 6, [1, 4], sig2, [m1, m1], 1, thresholds=thresholds)
        assert want[1:] == (1, cat.identity(cid))


def test_block_pass_boundaries(gpu_lib, curve):
    """with the lane-pair kernel off: one key more than a work item of this call holds, and the most an item ever holds plus one (33 items
    and the join of their partials)"""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    rnd = random.Random(129)
    for n, sizes in ((2049, [129, 3, 1, 20]), (4100, [gc.CHUNK_MAX + 1, 1, 1, 1])):
        assert gc.chunk_of(sum(sizes)) == 128
        sub = sorted(rnd.sample(range(n), sum(sizes)))
        h, keys, msgs, sig, _ = gk.instance(lib, cid, fp, n, sub, sizes, 900 + n)
        assert gk.against_gathered(lib, cid, fp, h, keys, n, sub, sig, msgs, 1, thresholds=(0,))[1] == 4


def test_tampering(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 65
    rnd = random.Random(65)
    sub = sorted(rnd.sample(range(n), 40))
    sizes = [20, 12, 7, 1]
    h, keys, msgs, sig, sks = gk.instance(lib, cid, fp, n, sub, sizes, 1000)
    assert gk.against_gathered(lib, cid, fp, h, keys, n, sub, sig, msgs, 1)[1] == 4
    # a wrong signature
    other_sig = gc.sign(lib, cid, fp, [sks[0]], [b"x" * 32])
    gk.against_gathered(lib, cid, fp, h, keys, n, sub, other_sig, msgs, 0)
    # two messages of different groups swapped
    j = next(k for k in range(len(msgs)) if msgs[k] != msgs[0])
    swapped = list(msgs)
    swapped[0], swapped[j] = swapped[j], swapped[0]
    assert gk.against_gathered(lib, cid, fp, h, keys, n, sub, sig, swapped, 0)[1] == 4
    # one byte of one message changed: its key moves to a new group
    changed = list(msgs)
    at = next(k for k in range(len(msgs)) if msgs.count(msgs[k]) > 1)
    changed[at] = changed[at][:-1] + bytes([changed[at][-1] ^ 1])
    assert gk.against_gathered(lib, cid, fp, h, keys, n, sub, sig, changed, 0)[1] == 5
    # one signer deselected and a non-signer selected: the same popcount, other keys
    absent = next(i for i in range(n) if i not in sub)
    moved = sorted(set(sub[1:]) | {absent})
    gk.against_gathered(lib, cid, fp, h, keys, n, moved, sig, msgs, 0)


def test_errors_and_a_valid_call_after_each(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 33
    sub = [1, 5, 6, 20, 32]
    h, keys, msgs, sig, _ = gk.instance(lib, cid, fp, n, sub, [3, 2], 1100)
    want = gk.against_gathered(lib, cid, fp, h, keys, n, sub, sig, msgs, 1)
    good = gk.bitmap_of(n, sub)

    def still_fine():
        assert gk.keys_host(lib, h, fp, sig, good, msgs) == want
        assert gk.keys_dev(lib, h, fp, sig, good, msgs) == want

    # a bit at a position >= n: in the last byte of the row, and in a byte beyond it
    stray_in, stray_out = bytearray(good), bytearray(good + bytes(3))
    stray_in[4] |= 0x02
    stray_out[7] |= 0x80
    for bad in (bytes(stray_in), bytes(stray_out)):
        assert gk.keys_host(lib, h, fp, sig, bad, msgs)[0] == ERR_ARG
        assert gk.keys_dev(lib, h, fp, sig, bad, msgs)[0] == ERR_ARG
        still_fine()
    # a popcount other than n_msgs, in both directions; the NULL bitmap selects all 33
    for bad_sub in (sub[:-1], sub + [7]):
        assert gk.keys_host(lib, h, fp, sig, gk.bitmap_of(n, bad_sub), msgs)[0] == ERR_ARG
        assert gk.keys_dev(lib, h, fp, sig, gk.bitmap_of(n, bad_sub), msgs)[0] == ERR_ARG
        still_fine()
    assert gk.keys_host(lib, h, fp, sig, None, msgs)[0] == ERR_ARG
    assert gk.keys_dev(lib, h, fp, sig, None, msgs)[0] == ERR_ARG
    # a bitmap shorter than the set
    assert gk.keys_host(lib, h, fp, sig, good[:4], msgs)[0] == ERR_ARG
    assert gk.keys_dev(lib, h, fp, sig, good[:4], msgs)[0] == ERR_ARG
    still_fine()
    # an unknown handle
    assert gk.keys_host(lib, 0xFFFFFFF1, fp, sig, good, msgs)[0] == ERR_ARG
    assert gk.keys_dev(lib, 0xFFFFFFF1, fp, sig, good, msgs)[0] == ERR_ARG
    # a key set on two shards
    rc, h2 = ms.upload(lib, cid, keys, n, devices=(0, 0))
    assert rc == 0
    try:
        assert gk.keys_host(lib, h2, fp, sig, good, msgs)[0] == ERR_ARG
        assert gk.keys_dev(lib, h2, fp, sig, good, msgs)[0] == ERR_ARG
    finally:
        lib.bgls_keys_free(h2)
    still_fine()
    # an off-curve signature
    off_curve = bytearray(sig)
    off_curve[-1] ^= 1
    assert gk.keys_host(lib, h, fp, bytes(off_curve), good, msgs)[0] == ERR_ENCODING
    assert gk.keys_dev(lib, h, fp, bytes(off_curve), good, msgs)[0] == ERR_ENCODING
    still_fine()
    # the device form with a stride above the length
    assert gk.keys_dev(lib, h, fp, sig, good, msgs, pad=7) == want


def test_variable_length_messages_in_the_host_form(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 33
    sks, keys, h = ms.key_set(lib, cid, fp, n)
    texts = [b"", b"a", b"ab", b"a" * 200, b"ab"]
    sub = [0, 3, 4, 9, 10, 11, 17, 30, 31, 32]
    msgs = [texts[k] for k in [3, 0, 1, 2, 4, 0, 3, 3, 1, 0]]
    sig = gc.sign(lib, cid, fp, [sks[i] for i in sub], msgs)
    want = gc.ungrouped(lib, cid, fp, sig, ms.gather(keys, fp, sub), msgs)
    assert want[:2] == (1, 4)
    assert gk.under_thresholds(lib, lambda: gk.keys_host(lib, h, fp, sig, gk.bitmap_of(n, sub), msgs)) == want


def test_a_prepared_key_set_gives_the_same_bytes(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 33
    sub = [0, 2, 3, 8, 16, 24, 31, 32]
    h, keys, msgs, sig, _ = gk.instance(lib, cid, fp, n, sub, [5, 2, 1], 1200)
    rc, hp = ms.upload(lib, cid, keys, n, flags=KEYS_PREPARE)
    assert rc == 0
    try:
        plain = gk.keys_host(lib, h, fp, sig, gk.bitmap_of(n, sub), msgs)
        assert plain[:2] == (1, 3)
        assert gk.keys_host(lib, hp, fp, sig, gk.bitmap_of(n, sub), msgs) == plain
        assert gk.keys_dev(lib, hp, fp, sig, gk.bitmap_of(n, sub), msgs) == plain
    finally:
        lib.bgls_keys_free(hp)


def test_python_mirror(gpu_lib, curve):
    from bgls_amd import Altbn128, Bls12, bgls
    from bgls_amd.curves import Point
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    cv = (Altbn128, Bls12)[cid]
    n = 33
    sks, keys, _ = ms.key_set(lib, cid, fp, n)
    ks = bgls.KeySet(cv, [Point(cv, 2, k) for k in cat.cut(keys, 4 * fp)])
    try:
        sub = [30, 2, 17, 5, 9]                                                # unsorted: the messages are parallel to the list as given
        msgs = [b"x" * 20, b"y" * 20, b"x" * 20, b"z" * 20, b"y" * 20]
        agg = Point(cv, 1, gc.sign(lib, cid, fp, [sks[i] for i in sub], msgs))
        order = sorted(range(len(sub)), key=lambda j: sub[j])
        asc_msgs = [msgs[j] for j in order]
        assert bgls.VerifyAggregateSignatureGroupedBySubset(cv, agg, ks, sub, msgs) is True
        assert bgls.VerifyAggregateSignatureGroupedBySubset(cv, agg, ks, gk.bitmap_of(n, sub), asc_msgs) is True
        assert bgls.VerifyAggregateSignatureGroupedBySubset(cv, agg, ks, gk.bitmap_of(n, sub), msgs) is False
        assert bgls.VerifyAggregateSignatureGroupedBySubset(cv, agg, ks, sub, msgs[:-1]) is False
        every = [bytes([i % 3]) * 8 for i in range(n)]
        agg_all = Point(cv, 1, gc.sign(lib, cid, fp, sks, every))
        assert bgls.VerifyAggregateSignatureGroupedBySubset(cv, agg_all, ks, None, every) is True
        assert bgls.VerifyAggregateSignatureGroupedBySubset(cv, agg_all, ks, list(range(n)), every) is True
        assert bgls.VerifyAggregateSignatureGroupedBySubset(cv, agg, ks, None, every) is False
        # the Kosk form prepends 0x01 to every message
        kagg = Point(cv, 1, gc.sign(lib, cid, fp, [sks[i] for i in sub], [b"\x01" + m for m in msgs]))
        assert bgls.KoskVerifyAggregateSignatureGroupedBySubset(cv, kagg, ks, sub, msgs) is True
        assert bgls.KoskVerifyAggregateSignatureGroupedBySubset(cv, agg, ks, sub, msgs) is False
        with pytest.raises(ValueError):
            bgls.VerifyAggregateSignatureGroupedBySubset(cv, agg, ks, [2, 5, 2], msgs[:3])
        with pytest.raises(TypeError):
            bgls.VerifyAggregateSignatureGroupedBySubset(cv, agg, [Point(cv, 2, k) for k in cat.cut(keys, 4 * fp)], sub, msgs)
        with pytest.raises(TypeError, match="signer-bitmap|BySubset"):
            bgls.VerifyAggregateSignatureGrouped(cv, agg, ks, msgs)
    finally:
        ks.free()
