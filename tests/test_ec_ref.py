"""Pins tests/ec_ref.py -- the plain reference the point-layer tiers compare against (test_rx_scalar_mul.py, test_gpu_point_arith.py) --
against the Python oracle's group law (oracle.pyref.groups.Groups) and the C oracle's scalar multiplication: random points, P + P, P - P,
the small-order fixture points, scalars above the order, the wire formats; and the digit recoding model against plain integers."""
import random

import pytest

import ec_ref
import point_cases as pc
from oracle import coracle
from oracle.pyref.groups import Groups
from oracle.pyref.params import CURVES


@pytest.mark.parametrize("cid,group", pc.GROUPS)
def test_group_law_matches_the_python_oracle(cid, group):
    cv, G = ec_ref.Curve(cid, group), Groups(CURVES[cid])
    add, mul, neg, tob, on = (G.g1_add, G.g1_mul, G.g1_neg, G.g1_bytes, G.g1_on_curve) if group == 1 else (G.g2_add, G.g2_mul, G.g2_neg, G.g2_bytes, G.g2_on_curve)
    assert cv.gen == (CURVES[cid].g1 if group == 1 else CURVES[cid].g2) and ec_ref.ORDER[cid] == CURVES[cid].r and cv.p == CURVES[cid].p
    assert cv.b == (CURVES[cid].b if group == 1 else G.b2)
    rnd = random.Random(77 + 10 * cid + group)
    q = ec_ref.ORDER[cid]
    pts = [None, cv.gen] + [cv.mul(cv.gen, rnd.randrange(1, q)) for _ in range(4)]
    pts += [pt for pt, _, _ in pc.fixture_points(cid, group) + pc.special_points(cid, group)]
    for a in pts:
        assert on(a) and cv.on_curve(a)
        assert cv.to_bytes(a) == tob(a) and cv.from_bytes(tob(a)) == a
        assert cv.add(a, a) == add(a, a) == cv.dbl(a)
        assert cv.add(a, cv.neg(a)) is None and cv.neg(a) == neg(a)
        for b in pts[:8]:
            assert cv.add(a, b) == add(a, b) == cv.add(b, a)
        for k in (0, 1, 2, 3, q - 1, q, q + 1, 2 * q + 5, (1 << 256) - 1, rnd.getrandbits(256), rnd.getrandbits(128)):
            assert cv.mul(a, k) == mul(a, k), k
    for pt, order, note in pc.fixture_points(cid, group) + pc.special_points(cid, group):
        if order is not None:
            assert cv.mul(pt, order) is None and cv.mul(pt, order + 1) == pt and cv.mul(pt, (1 << 256) - 1) == cv.mul(pt, ((1 << 256) - 1) % order), note
    if (cid, group) == (1, 1):
        assert cv.order((0, 2)) == 3 and cv.on_curve((0, 2))


@pytest.mark.parametrize("cid,group", pc.GROUPS)
def test_scalar_multiplication_matches_the_c_oracle(cid, group):
    cv = ec_ref.Curve(cid, group)
    rnd = random.Random(78 + 10 * cid + group)
    q = ec_ref.ORDER[cid]
    for _ in range(6):
        pt = cv.mul(cv.gen, rnd.randrange(1, q))
        for k in (rnd.randrange(q), q - 1, 1, 0):
            assert cv.to_bytes(cv.mul(pt, k)) == coracle.scale_point(cid, group, cv.to_bytes(pt), k)


def test_recode_is_the_scalar_and_names_its_branches():
    rnd = random.Random(79)
    for order in (3, 13, 23, 10069, 5864401, ec_ref.ORDER[0], ec_ref.ORDER[1]):
        for bits in (256, 128, 37, 5, 1):
            for _ in range(40):
                k = rnd.getrandbits(bits)
                for nb in (k.bit_length(), max(0, k.bit_length() - 3), min(256, bits + 2)):
                    r, ev = ec_ref.recode(k, nb, order)
                    assert r == (k & ((1 << nb) - 1)) % order and ev <= set(ec_ref.EVENTS)
    q = ec_ref.ORDER[0]
    assert "cancel" in ec_ref.recode(q, q.bit_length(), q)[1] and "double" in ec_ref.recode(q - 2, q.bit_length(), q)[1]
    assert ec_ref.recode(5, 3, 3)[1] >= {"r_inf"} and "tab_inf" in ec_ref.recode(3, 2, 3)[1]
    assert ec_ref.recode(1, 256, q)[1] == {"dbl_inf", "digit0", "r_inf"}
    for order in (10069, 5864401):
        for ev in ("double", "cancel"):
            k = ec_ref.steer_scalar(order, ev, 1 << 200, 3)
            assert ev in ec_ref.recode(k, k.bit_length(), order)[1]


@pytest.mark.parametrize("cid,group", pc.GROUPS)
def test_the_scalar_cases_reach_every_branch(cid, group):
    """the coverage condition, from recode() alone"""
    assert pc.events(pc.mul_cases(cid, group)) >= pc.required_events(cid, group)
