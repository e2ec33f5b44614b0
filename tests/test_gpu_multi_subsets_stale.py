"""GPU tier: the stale-workspace protocol of tests/test_gpu_stale_workspace.py for the multi-signature calls by signer bitmap
("Workspace contract").  The calls add no workspace slot: partial sums go to WS_JAC_A / WS_JAC_B, rows to WS_IN_B,
signatures to WS_IN_A, the planning table to WS_SEG_OFF, the key sums to WS_SEG_KEYS -- so what other calls left there is what they must
not read.  Per form (host, device) and per forced mode (never / always the complement): big then small, the fills 0x00 / 0x01 / 0xFF each
followed by the small valid instance and by the tampered one behind a fill of its own, then big again.  The small instance is five sets
over 65 keys, every returned byte stated by the C oracle; the tampered one has one flipped bitmap bit; the big one is 64 sets over 4100
keys.  The whole-set sum the complement mode adds is cached with the key set, not in a workspace: it is made by the first call and must
survive every fill (the fill is handed the key set's handle, so its shard records are poisoned too)."""
import random

import pytest

import stale_ws_cases as cat
import test_gpu_multi_subsets as su
import test_gpu_stale_workspace as sw

pytestmark = pytest.mark.gpu


def stated(lib, cid, fp, keys, sigs, subsets, msgs):
    """(accepted, verdicts, key sums, GT elements) of the instance on the C oracle"""
    ks = [[keys[i * 4 * fp:(i + 1) * 4 * fp] for i in sorted(sub)] for sub in subsets]
    gts = [cat.o_multi_gt(lib, cid, s, k, m) for s, k, m in zip(sigs, ks, msgs)]
    verdicts = [cat.o_verdict(cid, g) for g in gts]
    return sum(verdicts), verdicts, b"".join(cat.o_sum(cid, 2, k) for k in ks), b"".join(gts)


def build(lib, cid, device_form):
    fp = cat.FP[cid]
    n, nbig = 65, 4100
    sks, keys, h = su.key_set(lib, cid, fp, n)
    bsks, bkeys, hb = su.key_set(lib, cid, fp, nbig)
    rnd = random.Random(500 + cid)
    subsets = [[3], list(range(65)), list(range(1, 65, 2)), [], [i for i in range(65) if i not in (0, 31, 64)]]
    msgs = [rnd.randbytes(32) for _ in subsets]
    sigs = cat.memo(("subsets", cid), lambda: su.sign_subsets(lib, cid, fp, sks, subsets, msgs))
    bad = [list(s) for s in subsets]
    bad[2].append(32)                                          # one flipped bitmap bit, in set 2
    bsubsets = [[i for i in range(nbig) if rnd.random() < (0.5 if b % 2 else 0.95)] for b in range(64)]
    bmsgs = [rnd.randbytes(32) for _ in bsubsets]
    bsigs = cat.memo(("subsets-big", cid), lambda: su.sign_subsets(lib, cid, fp, bsks, bsubsets, bmsgs))
    want = cat.memo(("subsets-want", cid), lambda: stated(lib, cid, fp, keys, sigs, subsets, msgs))
    want_bad = cat.memo(("subsets-want-bad", cid), lambda: stated(lib, cid, fp, keys, sigs, bad, msgs))
    assert want[:2] == (5, [1] * 5) and want_bad[:2] == (4, [1, 1, 0, 1, 1])
    form = su.verify_dev if device_form else su.verify_host
    return cat.Case(lambda: form(lib, h, fp, n, sigs, subsets, msgs), want, lambda: form(lib, hb, fp, nbig, bsigs, bsubsets, bmsgs),
                    lambda: form(lib, h, fp, n, sigs, bad, msgs), want_bad, handle=h)


@pytest.mark.parametrize("mode", [1, 2], ids=["plain", "complement"])
@pytest.mark.parametrize("device_form", [False, True], ids=["host", "dev"])
def test_small_call_after_big_call_and_poison(gpu_lib, curve, device_form, mode):
    lib, cid = gpu_lib, curve["id"]
    case = build(lib, cid, device_form)
    try:
        assert lib.bgls_set_subset_complement(mode) == 0
        big = case.big()
        assert big[0] == 64 and big[1] == [1] * 64
        sw.run_protocol(lib, case)
    finally:
        lib.bgls_set_subset_complement(0)
