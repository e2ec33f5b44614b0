"""The case lists of the point-layer tiers (TEST-ONLY): tests/test_rx_scalar_mul.py feeds them to the host harness one by one and
tests/test_gpu_point_arith.py feeds the SAME lists to the device harness in waves.  Built from tests/ec_ref.py and the fixture points
of tests/golden/subgroup_*.json alone (no project import: the GPU tier keeps the Python oracle out)."""
import json
import os
import random
import re

import ec_ref
from ec_ref import ORDER, P, Curve, recode, steer_scalar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = [(0, 1), (0, 2), (1, 1), (1, 2)]
NAME = {0: "altbn128", 1: "bls12"}
# nbits of the scalar cases: the window read crosses a 32-bit word where (4 i - 1) mod 32 > 27; the ninth word is read at 256
NBITS = [0, 1, 2, 3, 4, 5] + list(range(27, 34)) + list(range(59, 66)) + list(range(124, 130)) + list(range(252, 257))


def _fp_sqrt(a, p):
    r = pow(a, (p + 1) // 4, p)
    return r if r * r % p == a % p else None


def _f2_sqrt(a, p):
    """a square root of a = (re, im) in Fp[u] / (u^2 + 1), p = 3 mod 4, or None"""
    a0, a1 = a
    if a1 == 0:
        r = _fp_sqrt(a0, p)
        if r is not None:
            return (r, 0)
        r = _fp_sqrt(-a0 % p, p)
        return None if r is None else (0, r)
    n = _fp_sqrt((a0 * a0 + a1 * a1) % p, p)
    if n is None:
        return None
    half = pow(2, -1, p)
    for s in (n, -n):
        x0 = _fp_sqrt((a0 + s) * half % p, p)
        if x0:
            return (x0, a1 * pow(2 * x0, -1, p) % p)
    return None


def fixture_points(cid, group):
    """[(point, order or None, note)] of the fixture's points that are on the curve and outside the order-r subgroup"""
    cv = Curve(cid, group)
    fix = json.load(open(os.path.join(GOLDEN, "subgroup_%s.json" % NAME[cid])))
    out = []
    for e in fix["points" if group == 2 else "g1_points"]:
        if e.get("in_subgroup") or not e.get("on_twist", e.get("on_curve")):
            continue
        pt = cv.from_bytes(bytes.fromhex(e["pt"]))
        assert cv.on_curve(pt)
        m = re.match(r"point of order (\d+)$", e["note"])
        order = int(m.group(1)) if m else None
        if order is not None:
            assert cv.mul(pt, order) is None and pt is not None
        out.append((pt, order, e["note"]))
    return out


def special_points(cid, group):
    """points with a coordinate 0, 1 or p - 1 at a few small x (and their order where it is small): BLS12-381's G1 has (0, 2) of order 3"""
    cv = Curve(cid, group)
    p, F = P[cid], cv.F
    xs = [0, 1, p - 1, 2] if group == 1 else [(0, 0), (1, 0), (p - 1, 0), (0, 1), (0, p - 1), (1, 1)]
    out = []
    for x in xs:
        rhs = F.add(F.mul(F.mul(x, x), x), cv.b)
        y = _fp_sqrt(rhs, p) if group == 1 else _f2_sqrt(rhs, p)
        if y is None:
            continue
        pt = (x, y)
        assert cv.on_curve(pt)
        out.append((pt, cv.order(pt, 16), "x = %r" % (x,)))
    return out


def add_cases(cid, group):
    """[{a, za, b, zb, form, tag}]: a, b wire bytes, za / zb a lambda (int) or None (Z = one exactly); form 0 add, 1 madd (b affine), 2 dbl, 3 madd and 4 add with 2 a as the running point.
    Every ordered pair from {inf, P, -P, 2P, Q, P under another lambda} under lambda in {1, p - 1, 2, random} for a subgroup P, and under
    lambda in {1, random} for each fixture and special point as P."""
    cv = Curve(cid, group)
    p = P[cid]
    rnd = random.Random(4100 + 10 * cid + group)
    Q = cv.mul(cv.gen, 7)
    bases = [(cv.mul(cv.gen, 5), "5 g", [None, p - 1, 2, rnd.randrange(3, p)])]
    for pt, order, note in fixture_points(cid, group) + special_points(cid, group):
        if order is not None or note.startswith("x =") or len(bases) < 3:
            bases.append((pt, note, [None, rnd.randrange(3, p)]))
    cases = []
    for Pt, note, lams in bases:
        for lam in lams:
            lam2 = rnd.randrange(3, p)
            ops = [(None, None, "inf"), (Pt, lam, "P"), (cv.neg(Pt), lam, "-P"), (cv.dbl(Pt), lam, "2P"), (Q, lam, "Q"), (Pt, lam2, "P'")]
            for a, za, ta in ops:
                for b, zb, tb in ops:
                    tag = "%s, lambda %s: %s + %s" % (note, "1" if lam is None else hex(lam)[:12], ta, tb)
                    cases.append({"a": cv.to_bytes(a), "za": za, "b": cv.to_bytes(b), "zb": zb, "form": 0, "tag": "add " + tag})
                    if tb != "P'":
                        cases.append({"a": cv.to_bytes(a), "za": za, "b": cv.to_bytes(b), "zb": None, "form": 1, "tag": "madd " + tag})
                cases.append({"a": cv.to_bytes(a), "za": za, "b": cv.to_bytes(None), "zb": None, "form": 2, "tag": "dbl %s, %s" % (note, ta)})
            # the running point straight from a doubling (its coordinates are not reductions' outputs: X up to 9 p, Y down to -8 p) meets
            # its own value, its negative, and other points: forms 3 (2 a + b, b affine) and 4 (2 a + b, both Jacobian)
            twice = [(cv.dbl(Pt), lam2, "2P"), (cv.neg(cv.dbl(Pt)), lam2, "-2P"), (Pt, lam2, "P"), (cv.neg(Pt), lam2, "-P"), (Q, lam2, "Q"), (None, None, "inf"),
                     (cv.dbl(cv.dbl(Pt)), lam2, "4P")]
            for a, za, ta in ops[:5]:
                for b, zb, tb in twice:
                    tag = "%s, lambda %s: 2 (%s) + %s" % (note, "1" if lam is None else hex(lam)[:12], ta, tb)
                    cases.append({"a": cv.to_bytes(a), "za": za, "b": cv.to_bytes(b), "zb": None, "form": 3, "tag": "madd after dbl " + tag})
                    cases.append({"a": cv.to_bytes(a), "za": za, "b": cv.to_bytes(b), "zb": zb, "form": 4, "tag": "add after dbl " + tag})
    return cases


def add_want(cid, group, case):
    cv = Curve(cid, group)
    a, b = cv.from_bytes(case["a"]), cv.from_bytes(case["b"])
    if case["form"] == 2:
        return cv.to_bytes(cv.dbl(a))
    return cv.to_bytes(cv.add(cv.dbl(a) if case["form"] >= 3 else a, b))


def mul_cases(cid, group):
    """[{pt, k, nbits, order, tag}]: the chain gets the eight words of k and nbits; order is the point's order where it is known (for the
    coverage proof by recode()), else None.  The expected point is (k mod 2^nbits) pt."""
    cv = Curve(cid, group)
    q = ORDER[cid]
    rnd = random.Random(4200 + 10 * cid + group)
    cases = []

    def case(pt, k, nbits, order, tag):
        assert 0 <= k < 1 << 256 and 0 <= nbits <= 256
        cases.append({"pt": cv.to_bytes(pt), "k": k, "nbits": nbits, "order": order, "tag": tag})

    g = cv.gen
    k0 = rnd.getrandbits(256) | (1 << 255) | (0xF << 28) | (0xF << 60)
    for nb in NBITS:
        case(g, k0, nb, q, "g, random scalar cut to nbits = %d" % nb)          # nbits below the true length: the chain masks
        case(g, (1 << nb) - 1, nb, q, "g, 2^%d - 1" % nb)
    pats = {"0x11..": int("11" * 32, 16), "0x77..": int("77" * 32, 16), "0x88..": int("88" * 32, 16), "0xff..": (1 << 256) - 1,
            "0x87..": int("87" * 32, 16), "0x78..": int("78" * 32, 16), "top bit": 1 << 255, "1 under 256": 1}
    for name, k in pats.items():
        case(g, k, 256 if name == "1 under 256" else k.bit_length(), q, "g, " + name)
        case(g, k >> 128, 128 if name == "1 under 256" else (k >> 128).bit_length(), q, "g, 128 bits of " + name)
    for e in (4, 28, 31, 32, 33, 63, 64, 127, 128, 255):
        for k in ((1 << e) + 1, (1 << e) - 1):
            case(g, k, k.bit_length(), q, "g, 2^%d %s 1" % (e, "+" if k & 1 and k > 1 << e else "-"))
    j = 1
    while j * (q - 2) < 1 << 256:
        for k, name in ((j * q, "%d q" % j), (j * (q - 2), "%d (q - 2)" % j)):
            if k < 1 << 256:
                case(g, k, k.bit_length(), q, "g, " + name)
        j += 1
    for k, name in ((q + 1, "q + 1"), (q - 1, "q - 1")):
        case(g, k, k.bit_length(), q, "g, " + name)
    case(None, k0, 256, 1, "infinity")
    for _ in range(6):
        k = rnd.getrandbits(256)
        case(cv.mul(g, rnd.randrange(1, q)), k, k.bit_length(), q, "random subgroup point, random scalar")
    for pt, order, note in fixture_points(cid, group) + special_points(cid, group):
        small = order is not None
        for bits in (256, 128):
            for _ in range((24 if bits == 256 else 12) if small else 2):
                k = rnd.getrandbits(bits)
                case(pt, k, k.bit_length(), order, "%s, random %d-bit scalar" % (note, bits))
        if small and order > 64:
            # random scalars do not meet the addend on these: steer the last addition into it (ec_ref.steer_scalar)
            for bits in (256, 128):
                for ev in ("double", "cancel"):
                    for d in (1, 7):
                        k = steer_scalar(order, ev, (1 << (bits - 5)) + rnd.getrandbits(bits - 8), d)
                        assert k.bit_length() <= bits and ev in recode(k, k.bit_length(), order)[1]
                        case(pt, k, k.bit_length(), order, "%s, scalar steered into '%s' (%d bits)" % (note, ev, bits))
        if small:
            for k in (order, order - 1, order + 1, (1 << 256) - 1):
                case(pt, k, k.bit_length(), order, "%s, k = %d" % (note, k) if k < 1 << 64 else "%s, 2^256 - 1" % note)
    return cases


def mul_want(cid, group, case):
    cv = Curve(cid, group)
    return cv.to_bytes(cv.mul(cv.from_bytes(case["pt"]), case["k"] & ((1 << case["nbits"]) - 1)))


def required_events(cid, group):
    """tab_inf needs a point of order at most 8: BLS12-381's G1 has one, (0, 2) of order 3"""
    return set(ec_ref.EVENTS) - (set() if (cid, group) == (1, 1) else {"tab_inf"})


def events(cases):
    ev = set()
    for c in cases:
        if c["order"] is not None and c["order"] > 1:
            ev |= recode(c["k"], c["nbits"], c["order"])[1]
    return ev


def k_words(k):
    return [(k >> (32 * j)) & 0xFFFFFFFF for j in range(8)]
