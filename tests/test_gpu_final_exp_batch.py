"""GPU tier: bgls_final_exp_batch / bgls_final_exp_batch_dev -- n independent final exponentiations with one GT element and one "is one"
mark per item.  The reference is oracle.pyref through tests/test_gpu_f12_arith.py's want_final (one cache for both files: every element
is evaluated once per session); every comparison is byte-exact.

  * the whole catalogue of tests/f12_cases.py in one call: 0 gives 0, an element of Fp6* gives one, is_one marks exactly the ones;
  * every batch size one short of, on and one past 10 items x 1, 2, 4 and 8 (the items of one to eight waves of six-lane groups), with a
    cycle of eight checked elements: the same bytes at every position as in a call of one item, and edge elements at the first slot, the
    last slot and on both sides of a ten-item boundary;
  * a non-canonical coefficient in the last item fails the whole call and leaves the host outputs as they were;
  * the device form on a stream of the caller's, and calls behind poisoned and stale workspaces, give the same bytes.
"""
import ctypes

import pytest

import f12_cases as fc
from test_gpu_f12_arith import want_final

pytestmark = pytest.mark.gpu

CIDS = [0, 1]
ERR_ENCODING = -2
SIZES = (1, 2, 5, 6, 9, 10, 11, 19, 20, 21, 39, 40, 41, 79, 80, 81, 161)
CYCLE = ("random 0", "Miller value of GT 0 (its pre-image)", "GT 0 (golden pairing)", "all p - 1", "w^1", "unitary 0 (easy part of a random element)",
         "Fp2 element", "random 1")
EDGES = ("0", "-1 = p - 1 in Fp", "position 11 = p - 1", "alternating 0 / p - 1")


def _buf(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")


def gtb(cid, tag):
    return fc.pairing(cid).gt_bytes(fc.pick(cid, tag))


def one_bytes(cid):
    return bytes(12 * fc.FB[cid] - 1) + b"\x01"


def final_exp_batch(lib, cid, items, want_gt=True, want_one=True):
    """one host call: ([GT bytes] or None, [0 / 1] or None)"""
    n, g = len(items), 12 * fc.FB[cid]
    out = (ctypes.c_uint8 * (n * g))(*([0xA5] * (n * g))) if want_gt else None
    one = (ctypes.c_uint8 * n)(*([7] * n)) if want_one else None
    rc = lib.bgls_final_exp_batch(cid, _buf(b"".join(items)), n, out, one)
    assert rc == 0, (rc, n)
    ob = bytes(out) if want_gt else None
    return ([ob[i * g:(i + 1) * g] for i in range(n)] if want_gt else None), (list(one) if want_one else None)


@pytest.mark.parametrize("cid", CIDS)
def test_catalogue_against_the_oracle(gpu_lib, cid):
    cat = fc.catalogue(cid)
    items = [fc.pairing(cid).gt_bytes(a) for _, a, _ in cat]
    want = [want_final(cid, x) for x in items]
    got, ones = final_exp_batch(gpu_lib, cid, items)
    for (t, _, cls), w, g, o in zip(cat, want, got, ones):
        assert g == w, t
        assert o == (1 if w == one_bytes(cid) else 0), t
        if "zero" in cls:
            assert w == bytes(len(w)) and o == 0, t
        if "fp6" in cls and "zero" not in cls:
            assert w == one_bytes(cid) and o == 1, t
    assert 0 < sum(ones) < len(ones)
    # either output alone
    assert final_exp_batch(gpu_lib, cid, items, want_one=False) == (got, None)
    assert final_exp_batch(gpu_lib, cid, items, want_gt=False) == (None, ones)


@pytest.mark.parametrize("cid", CIDS)
def test_every_position_of_every_batch_shape(gpu_lib, cid):
    tags = CYCLE + EDGES
    single = {}
    for t in tags:
        x = gtb(cid, t)
        got, ones = final_exp_batch(gpu_lib, cid, [x])
        assert got[0] == want_final(cid, x), t
        assert ones[0] == (1 if got[0] == one_bytes(cid) else 0), t
        single[t] = (got[0], ones[0])
    for n in SIZES:
        plan = [CYCLE[i % len(CYCLE)] for i in range(n)]
        got, ones = final_exp_batch(gpu_lib, cid, [gtb(cid, t) for t in plan])
        for i, t in enumerate(plan):
            assert (got[i], ones[i]) == single[t], (n, i, t)
        # the edge elements at the first slot, the last slot and on both sides of the first ten-item boundary
        plan[0] = EDGES[0]
        plan[n - 1] = EDGES[1] if n > 1 else plan[0]
        for slot, t in ((9, EDGES[2]), (10, EDGES[3])):
            if 0 < slot < n - 1:
                plan[slot] = t
        got, ones = final_exp_batch(gpu_lib, cid, [gtb(cid, t) for t in plan])
        for i, t in enumerate(plan):
            assert (got[i], ones[i]) == single[t], (n, i, t, "edge plan")


@pytest.mark.parametrize("cid", CIDS)
def test_a_noncanonical_coefficient_fails_the_whole_call(gpu_lib, cid):
    n, g = 11, 12 * fc.FB[cid]
    items = [gtb(cid, CYCLE[i % len(CYCLE)]) for i in range(n)]
    for pos in (0, 5, 11):
        for kind in (0, 1):
            bad = items[:-1] + [fc.noncanonical(cid, items[-1], pos, kind)]
            out = (ctypes.c_uint8 * (n * g))(*([0x5A] * (n * g)))
            one = (ctypes.c_uint8 * n)(*([0x5A] * n))
            assert gpu_lib.bgls_final_exp_batch(cid, _buf(b"".join(bad)), n, out, one) == ERR_ENCODING, (pos, kind)
            assert bytes(out) == b"\x5a" * (n * g) and bytes(one) == b"\x5a" * n, (pos, kind)
    # p - 1 is canonical
    got, _ = final_exp_batch(gpu_lib, cid, items[:-1] + [gtb(cid, "all p - 1")])
    assert got[-1] == want_final(cid, gtb(cid, "all p - 1"))


@pytest.mark.parametrize("cid", CIDS)
def test_device_form_on_a_stream_of_the_callers(gpu_lib, cid):
    import torch
    n, g = 21, 12 * fc.FB[cid]
    plan = [(CYCLE + EDGES)[i % 12] for i in range(n)]
    items = [gtb(cid, t) for t in plan]
    want, want_ones = final_exp_batch(gpu_lib, cid, items)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_in = torch.frombuffer(bytearray(b"".join(items)), dtype=torch.uint8).to(dev)
        d_out = torch.full((n * g,), 0xA5, dtype=torch.uint8, device=dev)
        d_one = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    stream.synchronize()
    assert gpu_lib.bgls_final_exp_batch_dev(cid, d_in.data_ptr(), n, d_out.data_ptr(), d_one.data_ptr(), stream.cuda_stream) == 0
    ob = bytes(d_out.cpu().numpy())
    assert [ob[i * g:(i + 1) * g] for i in range(n)] == want
    assert list(d_one.cpu().numpy()) == want_ones
    # either output alone, on the context's own stream
    d_out.fill_(0)
    d_one.fill_(9)
    torch.cuda.synchronize()
    assert gpu_lib.bgls_final_exp_batch_dev(cid, d_in.data_ptr(), n, d_out.data_ptr(), None, None) == 0
    assert gpu_lib.bgls_final_exp_batch_dev(cid, d_in.data_ptr(), n, None, d_one.data_ptr(), None) == 0
    assert bytes(d_out.cpu().numpy()) == ob and list(d_one.cpu().numpy()) == want_ones
    # a non-canonical coefficient in the last item
    bad = items[:-1] + [fc.noncanonical(cid, items[-1], 3, 0)]
    d_bad = torch.frombuffer(bytearray(b"".join(bad)), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    assert gpu_lib.bgls_final_exp_batch_dev(cid, d_bad.data_ptr(), n, d_out.data_ptr(), d_one.data_ptr(), None) == ERR_ENCODING


def _fill(lib, byte):
    filled = ctypes.c_uint64(0)
    assert lib.bgls_selftest_fill_workspaces(byte, 0, ctypes.byref(filled)) == 0
    assert filled.value > 0, "the fill touched nothing"


@pytest.mark.parametrize("cid", CIDS)
def test_poisoned_and_stale_workspaces(gpu_lib, cid):
    """tests/test_gpu_stale_workspace.py's discipline: a small call directly behind fill(0x00), behind fill(0xFF) and behind a larger call
    that left every slot full of its own values gives the bytes of a call on fresh workspaces; so does the tampered one its refusal"""
    small = [gtb(cid, t) for t in ("random 0", "0", "GT 0 (golden pairing)")]
    want = [want_final(cid, x) for x in small]
    want = (want, [1 if w == one_bytes(cid) else 0 for w in want])
    big = [gtb(cid, (CYCLE + EDGES)[i % 12]) for i in range(161)]
    bad = small[:2] + [fc.noncanonical(cid, small[2], 11, 1)]
    g = 12 * fc.FB[cid]

    def refused():
        out = (ctypes.c_uint8 * (3 * g))()
        return gpu_lib.bgls_final_exp_batch(cid, _buf(b"".join(bad)), 3, out, None) == ERR_ENCODING and not any(out)

    assert final_exp_batch(gpu_lib, cid, small) == want
    first_big = final_exp_batch(gpu_lib, cid, big)
    assert final_exp_batch(gpu_lib, cid, small) == want, "behind a larger call"
    final_exp_batch(gpu_lib, cid, big)
    assert refused(), "the tampered call behind a larger call"
    for byte in (0x00, 0xFF):
        _fill(gpu_lib, byte)
        assert final_exp_batch(gpu_lib, cid, small) == want, "behind fill(0x%02x)" % byte
        _fill(gpu_lib, byte)
        assert refused(), "the tampered call behind fill(0x%02x)" % byte
    assert final_exp_batch(gpu_lib, cid, big) == first_big
