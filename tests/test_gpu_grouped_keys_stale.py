"""GPU tier: the stale-workspace protocol of tests/test_gpu_stale_workspace.py for the grouped aggregate verification over a resident key
set ("Workspace contract").  The calls add no workspace slot: the selection goes to WS_AMS_SIGNERS, the grouping
where the list form keeps it (WS_TABLE, WS_MSM_LIST, WS_SEG_OFF, WS_KEYED_BLOB / WS_KEYED_OFF), the partial sums and the lane pairs' group
sums to WS_JAC_A / WS_JAC_B, the key sums to WS_SEG_KEYS -- so what other calls left there is what they must not read.  Per curve, per
form (host, device) and with the lane-pair kernel off and on (bgls_set_group_small 0 / 8): big then small, the fills 0x00 / 0x01 / 0xFF
each followed by the small valid instance and by the tampered one behind a fill of its own, then big again.  The small instance is seven
of 33 keys in three groups, every returned byte (verdict, n_groups, GT element) stated by the C oracle; the tampered one has one changed
message byte, which moves a signer to a fourth group; the big one is 4 096 of 4 100 keys in 40 groups, one of them of 3 850 signers."""
import pytest

import grouped_cases as gc
import grouped_keys_cases as gk
import stale_ws_cases as cat
import test_gpu_multi_subsets as ms
import test_gpu_stale_workspace as sw

pytestmark = pytest.mark.gpu

BIG = [3850] + [5] * 10 + [1] * 9 + [9] * 19 + [16]          # 40 groups, 4 096 signers
SMALL_SUB = [2, 3, 8, 16, 24, 31, 32]
ABSENT = (7, 1000, 2048, 4099)


def stated(lib, cid, fp, sig, keys, msgs):
    gt = cat.o_agg_gt(lib, cid, sig, cat.cut(keys, 4 * fp), msgs)
    return cat.o_verdict(cid, gt), gc.groups_of(msgs)[1], gt


def build(lib, cid, device_form):
    fp = cat.FP[cid]
    assert sum(BIG) == 4096 and len(BIG) == 40
    big_sub = [i for i in range(4100) if i not in ABSENT]
    h, keys, msgs, sig, _ = cat.memo(("grouped-keys-small", cid), lambda: gk.instance(lib, cid, fp, 33, SMALL_SUB, [4, 2, 1], 1300 + cid))
    bh, _, bmsgs, bsig, _ = cat.memo(("grouped-keys-big", cid), lambda: gk.instance(lib, cid, fp, 4100, big_sub, BIG, 1310 + cid))
    bad = list(msgs)
    bad[3] = bad[3][:7] + bytes([bad[3][7] ^ 0x40]) + bad[3][8:]
    gathered = ms.gather(keys, fp, SMALL_SUB)
    want = cat.memo(("grouped-keys-want", cid), lambda: stated(lib, cid, fp, sig, gathered, msgs))
    want_bad = cat.memo(("grouped-keys-want-bad", cid), lambda: stated(lib, cid, fp, sig, gathered, bad))
    assert want[:2] == (1, 3) and want_bad[:2] == (0, 4)
    form = gk.keys_dev if device_form else gk.keys_host
    row, big_row = gk.bitmap_of(33, SMALL_SUB), gk.bitmap_of(4100, big_sub)
    return cat.Case(lambda: form(lib, h, fp, sig, row, msgs), want, lambda: form(lib, bh, fp, bsig, big_row, bmsgs),
                    lambda: form(lib, h, fp, sig, row, bad), want_bad, handle=h)


@pytest.mark.parametrize("small", [0, 8])
@pytest.mark.parametrize("device_form", [False, True], ids=["host", "dev"])
def test_small_call_after_big_call_and_poison(gpu_lib, curve, device_form, small):
    lib, cid = gpu_lib, curve["id"]
    case = build(lib, cid, device_form)
    try:
        assert lib.bgls_set_group_small(small) == 0
        big = case.big()
        assert big[:2] == (1, 40)
        sw.run_protocol(lib, case)
    finally:
        lib.bgls_set_group_small(gk.DEFAULT_SMALL)
