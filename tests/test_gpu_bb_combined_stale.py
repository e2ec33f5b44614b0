"""GPU tier: the stale-workspace protocol of tests/test_gpu_stale_workspace.py for bgls_bb_verify_batch_combined and its device form
("Workspace contract").  The call adds no workspace slot; it reuses the slots of the combined multi-signature check,
of the Boneh-Boyen batch and of the Miller stages it calls, so what those calls left behind is what it must not read.  Per entry point
and per path (groups through the batched Miller stage, one group through the plain one): big then small, the fills 0x00 / 0x01 / 0xFF
each followed by the small valid instance and by the tampered one behind a fill of its own, then big again.  The small instance is seven
items in groups of three and four, every returned byte stated by the C oracle; the tampered one has one changed m; the big one is 200
items in groups that cross the 60-pairing block.  The cases are built with the catalogue's helpers and run here: the catalogue's own
parametrisation stays as it is."""
import pytest

import stale_ws_cases as cat
import test_gpu_bb_combined as bc
import test_gpu_stale_workspace as sw
from oracle import coracle

pytestmark = pytest.mark.gpu

SMALL_GROUPS, BIG_GROUPS = [3, 4], [61, 100, 39]


def oracle_gts(lib, cid, it, groups):
    """per group: prod e(rho_b sigma_b, Q_b) * e(-s_g g1, g2) on the C oracle"""
    fp, q = cat.FP[cid], cat.ORDER[cid]
    n = len(it["sig"])
    g1, g2 = cat.gen(lib, cid, 1), cat.gen(lib, cid, 2)
    rho = [int.from_bytes(c, "big") for c in cat.cut(bc.mc.want_coefficients(bc.SEED, n), 16)]
    rs = [coracle.scale_point(cid, 1, s, k) for s, k in zip(it["sig"], rho)]
    qs = [cat.o_sum(cid, 2, [coracle.scale_point(cid, 2, g2, m % q), key[:4 * fp], coracle.scale_point(cid, 2, key[4 * fp:], r)])
          for key, r, m in zip(it["key"], it["r"], it["m"])]
    gts, at = [], 0
    for c in groups:
        s = sum(rho[at:at + c])
        gts.append(cat.o_gt(cid, rs[at:at + c] + [coracle.scale_point(cid, 1, g1, (q - s % q) % q)], qs[at:at + c] + [g2]))
        at += c
    return gts


def build(lib, cid, device_form, groups_small, groups_big):
    fp = cat.FP[cid]
    it = cat.memo(("bbc", cid), lambda: bc.make_items(lib, cid, fp, 7, 2100 + cid))
    big = cat.memo(("bbc-big", cid), lambda: bc.make_items(lib, cid, fp, 200, 27 + cid))
    bad = {k: list(v) for k, v in it.items()}
    bad["m"][4] ^= 1 << 33                                   # one changed m, in the second group
    gs = groups_small or [7]
    gts, gts_bad = oracle_gts(lib, cid, it, gs), oracle_gts(lib, cid, bad, gs)
    verdicts, verdicts_bad = [cat.o_verdict(cid, g) for g in gts], [cat.o_verdict(cid, g) for g in gts_bad]
    assert verdicts == [1] * len(gs) and verdicts_bad == ([1, 0] if groups_small else [0])
    if not device_form:
        run = lambda items, g: bc.run_combined(lib, cid, fp, items, g)
    else:
        bufs = {id(x): [cat.dev_bytes(bytes(p)) for p in bc.packed(x)] for x in (it, bad, big)}

        def run(items, g):
            d = bufs[id(items)]
            ng = 1 if g is None else len(g)
            v, gt = bc.out(ng), bc.out(ng * 12 * fp)
            rc = lib.bgls_bb_verify_batch_combined_dev(cid, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(items["sig"]),
                                                       None if g is None else bc.offs(g), ng, bc.B(bc.SEED), v, gt, None)
            return rc, list(v)[:ng], bytes(gt)[:ng * 12 * fp]
    return cat.Case(lambda: run(it, groups_small), (sum(verdicts), verdicts, b"".join(gts)), lambda: run(big, groups_big),
                    lambda: run(bad, groups_small), (sum(verdicts_bad), verdicts_bad, b"".join(gts_bad)))


@pytest.mark.parametrize("one_group", [False, True], ids=["groups", "one-group"])
@pytest.mark.parametrize("device_form", [False, True], ids=["host", "dev"])
def test_small_call_after_big_call_and_poison(gpu_lib, curve, device_form, one_group):
    lib, cid = gpu_lib, curve["id"]
    case = build(lib, cid, device_form, None if one_group else SMALL_GROUPS, None if one_group else BIG_GROUPS)
    big = case.big()
    assert big[:2] == ((1, [1]) if one_group else (3, [1, 1, 1]))
    sw.run_protocol(lib, case)
