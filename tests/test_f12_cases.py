"""CPU tier of the Fp12 layer: the catalogue of tests/f12_cases.py against itself (the algebra the GPU tier's expectations rest on) and
against the host build of tower.hpp / pairing.hpp (ht_f12_op ops 0 - 8 over ALL of it: the only host coverage of tower.hpp's Fp12).
The reference is oracle.pyref (Python integers); every comparison is exact."""
import ctypes

import pytest

import f12_cases as fc
from oracle.pyref.params import CURVES

CIDS = [0, 1]


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def test_catalogue_holds_every_class():
    for cid in CIDS:
        T, p = fc.pairing(cid).T, CURVES[cid].p
        cat = fc.catalogue(cid)
        tags = [t for t, _, _ in cat]
        assert len(tags) == len(set(tags)) and 40 <= len(cat) <= 64
        assert fc.catalogue(cid) is cat and [fc.pairing(cid).gt_bytes(v) for _, v, _ in cat] == [fc.pairing(cid).gt_bytes(v) for _, v, _ in fc.catalogue.__wrapped__(cid)]
        for want in ["0", "1", "-1 = p - 1 in Fp", "Fp2 element", "Fp6 element (odd w-coefficients zero)", "all p - 1", "all 1", "alternating 0 / p - 1",
                     "unitary 0 (easy part of a random element)", "GT 0 (golden pairing)", "GT 0 inverse", "GT 0 to the r", "random 2",
                     "Fp6* element (final exponentiation 1, no pairing value)"] + ["w^%d" % k for k in range(1, 6)] + \
                    ["position %d = %s" % (j, s) for j in range(12) for s in ("1", "p - 1")]:
            assert want in tags, want
        assert T.f12_to_w(fc.pick(cid, "all p - 1")) == [(p - 1, p - 1)] * 6
        assert T.f12_to_w(fc.pick(cid, "w^1"))[1] == (1, 0) and T.f12_eq(T.f12_pow(fc.pick(cid, "w^1"), 6), T.f12_from_w([CURVES[cid].xi] + [(0, 0)] * 5))
        for t, v, cls in cat:
            w = T.f12_to_w(v)
            assert all(0 <= x < p for c in w for x in c), t
            assert ("fp6" in cls) == all(w[k] == (0, 0) for k in (1, 3, 5)), t
            assert ("zero" in cls) == fc.is_zero(cid, v), t
            # "unitary" = in the cyclotomic subgroup, a^(p^4 - p^2 + 1) = 1: where the easy part lands and where Granger-Scott squares
            cyc = not fc.is_zero(cid, v) and T.f12_eq(T.f12_mul(T.f12_frob(T.f12_frob(v, 2), 2), v), T.f12_frob(v, 2))
            assert ("unitary" in cls) == cyc, t
            assert not cyc or T.f12_is_one(T.f12_mul(v, T.f12_conj(v))), t
            if "gt" in cls:
                assert T.f12_is_one(T.f12_pow(v, CURVES[cid].r)), t
        assert T.f12_is_one(fc.pick(cid, "GT 0 to the r")) and T.f12_eq(fc.pick(cid, "GT 0 to the r - 1"), fc.pick(cid, "GT 0 inverse"))
        ex = dict(fc.pow_exponents(cid))
        assert all(0 < e < 1 << 128 for e in ex.values()) and ex["U_ABS"] == fc.u_abs(cid) and len(ex) == 3 + 2 * 7 + 2
        for nb in fc.POW_TOP_BITS:
            assert ex["top bit only, %d bits" % nb].bit_length() == nb and ex["all ones, %d bits" % nb] == (1 << nb) - 1
        assert len(fc.gt_pow_exponents(cid)) == 14
        bc = fc.binary_cases(cid)
        assert len(bc) >= len(fc.REDUCED) ** 2 + 4 * len(cat) - 1


@pytest.mark.parametrize("cid", CIDS)
def test_inverses_frobenius_and_final_exponentiation(cid):
    PR = fc.pairing(cid)
    T, c = PR.T, CURVES[cid]
    for t, a, cls in fc.catalogue(cid):
        if "zero" not in cls:
            assert T.f12_is_one(T.f12_mul(a, T.f12_inv(a))), t
        x = a
        for k in (1, 2, 3):
            x = T.f12_frob(x, 1)
            assert T.f12_eq(x, T.f12_frob(a, k)), (t, k)
    # the chain equals the plain power by (p^12 - 1) / r (two elements per curve: the power costs seconds)
    e = (c.p ** 12 - 1) // c.r
    for t in ("random 0", "all p - 1"):
        a = fc.pick(cid, t)
        assert T.f12_eq(PR.final_exp(a), T.f12_pow(a, e)), t
    # 0 is not invertible; the reference does not raise: its Fp inverse of 0 is 0, so final_exp(0) = 0, and so must the device's be
    # (all twelve coefficients 0, verdict 0)
    z = fc.zero12()
    assert fc.is_zero(cid, T.f12_inv(z)) and fc.is_zero(cid, PR.final_exp(z))
    # an element of Fp6* is no pairing value, yet its final exponentiation is 1 (p^6 - 1 divides the exponent)
    assert T.f12_is_one(PR.final_exp(fc.pick(cid, "Fp6* element (final exponentiation 1, no pairing value)")))
    assert T.f12_eq(PR.final_exp(fc.pick(cid, "Miller value of GT 0 (its pre-image)")), fc.pick(cid, "GT 0 (golden pairing)"))
    # the Granger-Scott recurrence is the square on unitary elements; gs_pow is the power there
    for t, a in fc.by_class(cid, "unitary"):
        assert T.f12_eq(fc.gs_sqr(cid, a), T.f12_sqr(a)), t
        assert T.f12_eq(fc.gs_pow(cid, a, fc.u_abs(cid)), T.f12_pow(a, fc.u_abs(cid))), t


@pytest.mark.parametrize("cid", CIDS)
def test_host_tower_over_the_whole_catalogue(host_harness, cid):
    """ht_f12_op: 0 mul, 1 sqr, 2 inv, 3 - 5 frob 1 - 3, 6 cyclotomic squaring, 7 conj, 8 final_exp.  The cyclotomic squaring is the
    square on unitary elements only; on the others the host's result pins fc.gs_sqr, the recurrence itself."""
    lib, n = host_harness, fc.FB[cid]
    PR = fc.pairing(cid)
    T = PR.T

    def run(op, a, b=None):
        o = (ctypes.c_uint8 * (12 * n))()
        assert lib.ht_f12_op(cid, op, B(PR.gt_bytes(a)), None if b is None else B(PR.gt_bytes(b)), o) == 0, op
        return bytes(o)

    for t, a, b in fc.binary_cases(cid):
        assert run(0, a, b) == PR.gt_bytes(T.f12_mul(a, b)), t
    unary = ((1, T.f12_sqr), (2, T.f12_inv), (3, lambda a: T.f12_frob(a, 1)), (4, lambda a: T.f12_frob(a, 2)), (5, lambda a: T.f12_frob(a, 3)),
             (7, T.f12_conj), (8, PR.final_exp))
    for t, a, cls in fc.catalogue(cid):
        for op, fn in unary:
            assert run(op, a, a) == PR.gt_bytes(fn(a)), (t, op)
        assert run(6, a) == PR.gt_bytes(fc.gs_sqr(cid, a)), t
        if "unitary" in cls:
            assert run(6, a) == PR.gt_bytes(T.f12_sqr(a)), t
