"""GPU tier: bgls_verify_aggregate_grouped / _dev -- one hash and one pairing per distinct message, the keys of a message's signers summed
first -- against the ungrouped calls on the same inputs (bgls_verify_aggregate(..., 1) for the verdict, bgls_verify_aggregate_h_gt for the GT
bytes; grouped_cases.ungrouped), and at the smallest shapes against the C oracle: verdict, n_groups and every GT byte."""
import pytest

import grouped_cases as gc
import stale_ws_cases as cat
import test_gpu_batch_aggregate as ba
import test_gpu_msm as mm

pytestmark = pytest.mark.gpu

ERR_ENCODING = -2
MIX = [1, 2, 31, 32, 33, 127, 128, 129]


def both_forms(lib, cid, fp, sig, keys, msgs, want):
    got = gc.grouped_host(lib, cid, fp, sig, keys, msgs)
    assert got == want, ("host form", got[:2], want[:2])
    got = gc.grouped_dev(lib, cid, fp, sig, keys, msgs)
    assert got == want, ("device form", got[:2], want[:2])


def against_ungrouped(lib, cid, fp, sig, keys, msgs, verdict):
    want = gc.ungrouped(lib, cid, fp, sig, keys, msgs)
    assert want[0] == verdict, "the ungrouped call disagrees with the construction of the instance"
    both_forms(lib, cid, fp, sig, keys, msgs, want)
    return want


def test_no_signers(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    inf = bytes(2 * fp)
    other = cat.gen(lib, cid, 1)
    for sig, verdict in ((inf, 1), (other, 0)):
        assert ba.single(lib, cid, fp, sig, b"", [], 1) == verdict
        want = (verdict, 0, cat.o_agg_gt(lib, cid, sig, [], []))
        assert cat.o_verdict(cid, want[2]) == verdict
        both_forms(lib, cid, fp, sig, b"", [], want)


def test_one_signer_and_seven_signers_in_three_groups_against_the_oracle(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    for sizes in ([1], [4, 2, 1]):
        keys, msgs, sig, _, _ = gc.make_instance(lib, cid, fp, sizes, 40 + len(sizes))
        want = against_ungrouped(lib, cid, fp, sig, keys, msgs, 1)
        gt = cat.o_agg_gt(lib, cid, sig, cat.cut(keys, 4 * fp), msgs)
        assert want == (cat.o_verdict(cid, gt), len(sizes), gt)


def test_one_message_for_everybody_equals_the_multi_signature(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    keys, msgs, sig, _, _ = gc.make_instance(lib, cid, fp, [70], 51)
    want = against_ungrouped(lib, cid, fp, sig, keys, msgs, 1)
    assert want[1] == 1
    assert lib.bgls_verify_multi(cid, gc.B(sig), gc.B(keys), 70, gc.B(msgs[0]), len(msgs[0])) == 1
    bad = cat.gen(lib, cid, 1)                                 # a valid G1 point that is not the aggregate
    assert lib.bgls_verify_multi(cid, gc.B(bad), gc.B(keys), 70, gc.B(msgs[0]), len(msgs[0])) == 0
    against_ungrouped(lib, cid, fp, bad, keys, msgs, 0)


def test_every_message_distinct(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    keys, msgs, sig, _, _ = gc.make_instance(lib, cid, fp, [1] * 70, 52)
    assert against_ungrouped(lib, cid, fp, sig, keys, msgs, 1)[1] == 70


def test_a_key_twice_and_a_key_with_its_negative_in_one_group(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    r = mm.ORDER[cid]
    a, b, c, e = 0x1234567, 0x7654321, 0xABCDEF1, 0x13579BD
    m0, m1, m2 = b"m0" * 16, b"m1" * 16, b"m2" * 16
    # group m0 holds a twice; group m1 holds b and -b, whose sum is the point at infinity: the factor 1; group m2 an ordinary signer
    sks = [a, b, e, a, r - b, c]
    msgs = [m0, m1, m2, m0, m1, m0]
    keys, sig = gc.instance_from(lib, cid, fp, sks, msgs)
    want = against_ungrouped(lib, cid, fp, sig, keys, msgs, 1)
    assert want[1] == 3
    # the whole instance is one group of a key and its negative: no factor at all, and the signature is the point at infinity
    keys2, sig2 = gc.instance_from(lib, cid, fp, [b, r - b], [m1, m1])
    assert sig2 == bytes(2 * fp)
    want = against_ungrouped(lib, cid, fp, sig2, keys2, [m1, m1], 1)
    assert want[1:] == (1, cat.identity(cid))


def test_group_size_mix_and_its_tampered_variants(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    keys, msgs, sig, _, spare = gc.make_instance(lib, cid, fp, MIX, 60 + cid)
    n = len(msgs)
    assert against_ungrouped(lib, cid, fp, sig, keys, msgs, 1)[1] == len(MIX)
    # a wrong signature
    _, _, other_sig, _, _ = gc.make_instance(lib, cid, fp, [2, 1], 61)
    against_ungrouped(lib, cid, fp, other_sig, keys, msgs, 0)
    # two messages of different groups swapped
    i = 0
    j = next(k for k in range(n) if msgs[k] != msgs[0])
    swapped = list(msgs)
    swapped[i], swapped[j] = swapped[j], swapped[i]
    assert against_ungrouped(lib, cid, fp, sig, keys, swapped, 0)[1] == len(MIX)
    # one key replaced by a spare
    at = n // 2
    wrong = keys[:at * 4 * fp] + spare + keys[(at + 1) * 4 * fp:]
    against_ungrouped(lib, cid, fp, sig, wrong, msgs, 0)
    # one byte of one message changed: its key moves to a new group
    changed = list(msgs)
    changed[n - 3] = changed[n - 3][:-1] + bytes([changed[n - 3][-1] ^ 1])
    assert against_ungrouped(lib, cid, fp, sig, keys, changed, 0)[1] == len(MIX) + 1


def test_a_group_of_one_work_item_and_one_key_more(gpu_lib, curve):
    """one key more than a work item holds in one group beside three small groups: the item boundary and the join of the group's two
    partials -- at the item size of this call (128 keys: the mix above has its 127 / 128 / 129 in one item each side of it) and, with
    the most keys an item ever holds plus one, a group of 33 items whose last holds one key"""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    small = [129, 3, 1, 20]
    assert gc.chunk_of(sum(small)) == 128
    keys, msgs, sig, _, _ = gc.make_instance(lib, cid, fp, small, 75 + cid)
    assert against_ungrouped(lib, cid, fp, sig, keys, msgs, 1)[1] == 4
    keys, msgs, sig, _, _ = gc.make_instance(lib, cid, fp, [gc.CHUNK_MAX + 1, 3, 1, 20], 70 + cid)
    assert gc.chunk_of(len(msgs)) == 128
    assert against_ungrouped(lib, cid, fp, sig, keys, msgs, 1)[1] == 4
    changed = list(msgs)
    changed[5] = bytes([changed[5][0] ^ 0x10]) + changed[5][1:]
    against_ungrouped(lib, cid, fp, sig, keys, changed, 0)


def test_device_form_with_a_stride_above_the_length(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    keys, msgs, sig, _, _ = gc.make_instance(lib, cid, fp, [5, 1, 3], 80)
    want = gc.ungrouped(lib, cid, fp, sig, keys, msgs)
    assert want[0] == 1
    assert gc.grouped_dev(lib, cid, fp, sig, keys, msgs, pad=7) == want


def test_variable_length_messages(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    texts = [b"", b"a", b"ab", b"a" * 200, b"ab"]
    order = [3, 0, 1, 2, 4, 0, 3, 3, 1, 0]
    msgs = [texts[k] for k in order]
    sks = [0x1111 + 77 * k for k in range(len(msgs))]
    keys, sig = gc.instance_from(lib, cid, fp, sks, msgs)
    want = gc.ungrouped(lib, cid, fp, sig, keys, msgs)
    assert want[:2] == (1, 4)
    assert gc.grouped_host(lib, cid, fp, sig, keys, msgs) == want


def test_an_off_curve_key_anywhere_is_an_encoding_error(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    keys, msgs, sig, _, _ = gc.make_instance(lib, cid, fp, [40, 2, 30], 90)
    n = len(msgs)
    for at in (0, n // 2, n - 1):
        bad = bytearray(keys)
        bad[(at + 1) * 4 * fp - 1] ^= 1
        bad = bytes(bad)
        assert ba.single(lib, cid, fp, sig, bad, msgs, 1) == ERR_ENCODING
        assert gc.grouped_host(lib, cid, fp, sig, bad, msgs)[0] == ERR_ENCODING, at
        assert gc.grouped_dev(lib, cid, fp, sig, bad, msgs)[0] == ERR_ENCODING, at


def test_python_mirror(gpu_lib, curve):
    from bgls_amd import Altbn128, Bls12, bgls
    from bgls_amd.curves import Point
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    cv = (Altbn128, Bls12)[cid]
    keys, msgs, sig, _, _ = gc.make_instance(lib, cid, fp, [6, 1, 9], 95)
    pts = [Point(cv, 2, k) for k in cat.cut(keys, 4 * fp)]
    agg = Point(cv, 1, sig)
    assert bgls.GroupMessages(msgs) == gc.groups_of(msgs)
    assert bgls.VerifyAggregateSignatureGrouped(cv, agg, pts, msgs) is True
    assert bgls._verify_agg(cv, agg, pts, msgs, True) is True
    bad = list(msgs)
    bad[4] = bad[4] + b"!"
    assert bgls.VerifyAggregateSignatureGrouped(cv, agg, pts, bad) is False
    assert bgls.VerifyAggregateSignatureGrouped(cv, agg, pts, msgs[:-1]) is False
    # the Kosk form prepends 0x01 to every message: a signature over the prefixed messages verifies, the plain one does not
    kkeys, ksig = gc.instance_from(lib, cid, fp, [0x999 + 5 * k for k in range(len(msgs))], [b"\x01" + m for m in msgs])
    kpts = [Point(cv, 2, k) for k in cat.cut(kkeys, 4 * fp)]
    assert bgls.KoskVerifyAggregateSignatureGrouped(cv, Point(cv, 1, ksig), kpts, msgs) is True
    assert bgls.KoskVerifyAggregateSignatureGrouped(cv, agg, pts, msgs) is False
    ks = bgls.KeySet(cv, pts)
    try:
        with pytest.raises(TypeError, match="signer-bitmap|BySubset"):
            bgls.VerifyAggregateSignatureGrouped(cv, agg, ks, msgs)
    finally:
        ks.free()
