"""GPU tier: the stale-workspace protocol of tests/test_gpu_stale_workspace.py for the aggregate verification that pairs once per distinct
message ("Workspace contract").  The calls add no workspace slot: the table and the first occurrences go to WS_TABLE,
every array of 32-bit words of the grouping to WS_MSM_LIST, the 64-bit ones to WS_SEG_OFF, the compacted messages to WS_KEYED_BLOB /
WS_KEYED_OFF, the partial sums to WS_JAC_A / WS_JAC_B, the key sums to WS_SEG_KEYS -- so what other calls left there is what they must not
read.  Per curve and per form (host, device): big then small, the fills 0x00 / 0x01 / 0xFF each followed by the small valid instance and
by the tampered one behind a fill of its own, then big again.  The small instance is seven signers in three groups, every returned byte
(verdict, n_groups, GT element) stated by the C oracle; the tampered one has one changed message byte, which moves a signer to a fourth
group; the big one is 4 100 signers in 40 groups, one of them of 3 850 signers: 31 work items and the join of their partials."""
import pytest

import grouped_cases as gc
import stale_ws_cases as cat
import test_gpu_stale_workspace as sw

pytestmark = pytest.mark.gpu

BIG = [3850] + [5] * 10 + [1] * 9 + [9] * 19 + [20]          # 40 groups, 4 100 signers
BIGGER = [gc.CHUNK_MAX + 2] + [1] * 2                                 # a group of 33 work items: the join of its partials


def stated(lib, cid, fp, sig, keys, msgs):
    gt = cat.o_agg_gt(lib, cid, sig, cat.cut(keys, 4 * fp), msgs)
    return cat.o_verdict(cid, gt), gc.groups_of(msgs)[1], gt


def build(lib, cid, device_form):
    fp = cat.FP[cid]
    assert sum(BIG) == 4100 and len(BIG) == 40
    keys, msgs, sig, _, _ = cat.memo(("grouped-small", cid), lambda: gc.make_instance(lib, cid, fp, [4, 2, 1], 300 + cid))
    bkeys, bmsgs, bsig, _, _ = cat.memo(("grouped-big", cid), lambda: gc.make_instance(lib, cid, fp, BIG, 310 + cid))
    bad = list(msgs)
    bad[3] = bad[3][:7] + bytes([bad[3][7] ^ 0x40]) + bad[3][8:]
    want = cat.memo(("grouped-want", cid), lambda: stated(lib, cid, fp, sig, keys, msgs))
    want_bad = cat.memo(("grouped-want-bad", cid), lambda: stated(lib, cid, fp, sig, keys, bad))
    assert want[:2] == (1, 3) and want_bad[:2] == (0, 4)
    form = gc.grouped_dev if device_form else gc.grouped_host
    return cat.Case(lambda: form(lib, cid, fp, sig, keys, msgs), want, lambda: form(lib, cid, fp, bsig, bkeys, bmsgs),
                    lambda: form(lib, cid, fp, sig, keys, bad), want_bad)


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "dev"])
def test_small_call_after_big_call_and_poison(gpu_lib, curve, device_form):
    lib, cid = gpu_lib, curve["id"]
    case = build(lib, cid, device_form)
    big = case.big()
    assert big[:2] == (1, 40)
    sw.run_protocol(lib, case)


def test_the_join_of_partials_after_poison(gpu_lib, curve):
    """the group above one work item: its second partial and the join's offsets lie where the fill has written"""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    keys, msgs, sig, _, _ = cat.memo(("grouped-bigger", cid), lambda: gc.make_instance(lib, cid, fp, BIGGER, 320 + cid))
    first = gc.grouped_host(lib, cid, fp, sig, keys, msgs)
    assert first[:2] == (1, 3)
    for byte in (0x01, 0xFF):
        sw.fill(lib, byte, 0)
        assert gc.grouped_host(lib, cid, fp, sig, keys, msgs) == first
        sw.fill(lib, byte, 0)
        assert gc.group_host(lib, msgs) == (0,) + gc.groups_of(msgs)
