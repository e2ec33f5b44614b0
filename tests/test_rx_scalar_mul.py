"""Host tier of the point layer: rx_jac1.hpp (jac1_dbl / jac1_madd / jac1_add / jac1_mul_w4, G1 over Fp) and rx_jac.hpp / rx_g2mul.hpp
(jacx_dbl / jacx_madd / jacx_add / jacx_mul_w4, the twists over Fp2) through the host harness's ht_rx_padd and ht_rx_pmul, which compile
them with every column accumulation checked.  Each case of tests/point_cases.py is checked three ways: the wire bytes equal the plain
reference (tests/ec_ref.py, pinned by test_ec_ref.py), no column overflowed, and every output coordinate stays below the 64 p that
rx.hpp documents for the point steps.  The scalar list is proven, by ec_ref.recode alone, to reach every branch of the chain."""
import ctypes

import pytest

import point_cases as pc
from ec_ref import FB, P

VALUE_BOUND = 64                                   # rx.hpp: "|value| stays below ~64 p everywhere in the point steps"
RAW = 88                                           # point_ops.hpp PT_RAW


def _buf(b):
    return (ctypes.c_uint8 * len(b)).from_buffer_copy(b)


def _prep(lib):
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.ht_rx_padd.argtypes = [i, i, vp, vp, vp, vp, i, vp, vp, vp]
    lib.ht_rx_pmul.argtypes = [i, i, vp, vp, i, vp, vp, vp]
    return lib


def run_add(lib, cid, group, c):
    """(rc, wire bytes, raw limbs, largest |value| / p)"""
    fb = FB[cid]
    out, raw, vm = (ctypes.c_uint8 * (2 * group * fb))(), (ctypes.c_int32 * RAW)(), ctypes.c_int64()
    za = None if c["za"] is None else _buf(c["za"].to_bytes(fb, "big"))
    zb = None if c["zb"] is None else _buf(c["zb"].to_bytes(fb, "big"))
    rc = lib.ht_rx_padd(cid, group, _buf(c["a"]), za, _buf(c["b"]), zb, c["form"], out, raw, ctypes.byref(vm))
    return rc, bytes(out), list(raw), vm.value / 65536.0


def run_mul(lib, cid, group, c):
    fb = FB[cid]
    out, raw, vm = (ctypes.c_uint8 * (2 * group * fb))(), (ctypes.c_int32 * RAW)(), ctypes.c_int64()
    rc = lib.ht_rx_pmul(cid, group, _buf(c["pt"]), (ctypes.c_uint32 * 8)(*pc.k_words(c["k"])), c["nbits"], out, raw, ctypes.byref(vm))
    return rc, bytes(out), list(raw), vm.value / 65536.0


def exact_ratio(cid, group, raw):
    """the same figure from the raw limbs with Python integers: the harness's long-double figure is checked against it"""
    n = 10 if cid == 0 else 14
    worst = 0
    for c in range(3 * group):
        worst = max(worst, abs(sum(raw[1 + c * n + i] << (28 * i) for i in range(n))))
    return worst / P[cid]


@pytest.mark.parametrize("cid,group", pc.GROUPS)
def test_additions_and_doublings(host_harness, cid, group):
    lib = _prep(host_harness)
    cases = pc.add_cases(cid, group)
    seen = set()
    worst = 0.0
    for c in cases:
        rc, got, raw, ratio = run_add(lib, cid, group, c)
        assert rc == 0, (c["tag"], rc)                                     # -3: a column overflowed
        assert got == pc.add_want(cid, group, c), c["tag"]
        assert ratio < VALUE_BOUND and abs(ratio - exact_ratio(cid, group, raw)) < 1e-3, (c["tag"], ratio)
        assert raw[0] == int(got == bytes(len(got))), c["tag"]
        worst = max(worst, ratio)
        seen.add(("after dbl " if c["form"] >= 3 else "") + c["tag"].split(":")[-1].strip() if c["form"] != 2 else "dbl")
    print("largest |value| / p over %d cases: %.3f" % (len(cases), worst))
    assert {"P + P", "P + -P", "P + P'", "P' + P", "inf + inf", "inf + P", "P + inf", "2P + -P", "dbl", "after dbl 2 (P) + 2P", "after dbl 2 (P) + -2P",
            "after dbl 2 (-P) + -2P", "after dbl 2 (P) + Q"} <= seen


@pytest.mark.parametrize("cid,group", pc.GROUPS)
def test_windowed_chain(host_harness, cid, group):
    lib = _prep(host_harness)
    cases = pc.mul_cases(cid, group)
    assert pc.events(cases) >= pc.required_events(cid, group)              # every branch of the chain is reached (recode() alone)
    worst = 0.0
    for c in cases:
        rc, got, raw, ratio = run_mul(lib, cid, group, c)
        assert rc == 0, (c["tag"], rc)
        assert got == pc.mul_want(cid, group, c), (c["tag"], hex(c["k"]), c["nbits"])
        assert ratio < VALUE_BOUND and abs(ratio - exact_ratio(cid, group, raw)) < 1e-3, (c["tag"], ratio)
        worst = max(worst, ratio)
    print("largest |value| / p over %d cases: %.3f" % (len(cases), worst))


def test_bad_points_and_arguments_are_reported(host_harness):
    lib = _prep(host_harness)
    for cid, group in pc.GROUPS:
        c = dict(pc.add_cases(cid, group)[7])
        off = bytearray(pc.mul_cases(cid, group)[0]["pt"])
        off[-1] ^= 1
        assert run_add(lib, cid, group, dict(c, a=bytes(off)))[0] == -2
        assert run_add(lib, cid, group, dict(c, form=5))[0] == -1
        assert run_add(lib, cid, group, dict(c, a=bytes(off[:len(off) // 2]) + bytes(off[:len(off) // 2]), za=0, form=0))[0] == -2
        m = dict(pc.mul_cases(cid, group)[9])
        assert run_mul(lib, cid, group, dict(m, pt=bytes(off)))[0] == -2
        assert run_mul(lib, cid, group, dict(m, nbits=257))[0] == -1


def test_mixed_addition_meets_its_addend_after_a_doubling(host_harness):
    """The finding of this tier: jac1_madd / jacx_madd compared U2 with the running point's X and S2 with its Y through a zero test that
    holds on (-3 p, 5 p), but a doubling leaves X3 = F - 2 D anywhere in (-4 p, 9 p) and Y3 = E (D - X3) - 8 C in (-8 p, p).  With the
    running point straight from a doubling and equal to the addend, the differences fell outside the window, the test missed them and the
    sum came out as infinity (forms 3 and 4 of the addition cases pin this on every base point).  On BLS12-381's order-3 point (0, 2) the
    chain's own table does it: 5 P = 4 P + P with 4 P = P.  Every k below 200 on (0, 2) and on its negative is (k mod 3) P."""
    lib = _prep(host_harness)
    from ec_ref import Curve
    cv = Curve(1, 1)
    for pt in ((0, 2), cv.neg((0, 2))):
        for k in range(200):
            rc, got, _, _ = run_mul(lib, 1, 1, {"pt": cv.to_bytes(pt), "k": k, "nbits": k.bit_length()})
            assert rc == 0 and got == cv.to_bytes([None, pt, cv.neg(pt)][k % 3]), k
