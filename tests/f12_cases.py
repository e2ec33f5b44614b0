"""The case lists of the Fp12 tier (TEST-ONLY): tests/test_f12_cases.py checks them against themselves and feeds them to the host build of
tower.hpp / pairing.hpp one by one (ht_f12_op), tests/test_gpu_f12_arith.py feeds the SAME lists to the cooperative forms on the device
(tests/harness/device_harness_f12.hip) one element per block, and to the public ABI.  The reference is oracle.pyref (Tower, Pairing: Python
integers); elements travel as canonical GT bytes (Pairing.gt_bytes).  Everything is seeded: two calls give the same lists."""
import functools
import json
import os
import random

from oracle.pyref.pairing import Pairing
from oracle.pyref.params import CURVES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = {0: "altbn128", 1: "bls12"}
FB = {0: 32, 1: 48}
NL = {0: 10, 1: 14}                          # 28-bit limbs of the carry-free form (RX_NL)
POW_TOP_BITS = (32, 33, 64, 65, 96, 97, 128)


@functools.lru_cache(maxsize=None)
def pairing(cid):
    return Pairing(CURVES[cid])


def u_abs(cid):
    c = CURVES[cid]
    return c.u if cid == 0 else -c.x


def zero12():
    return (((0, 0),) * 3, ((0, 0),) * 3)


def from_fp(cid, pos):
    """the element whose twelve Fp positions are pos[0 .. 12): position 2 k + h is half h (0 real, 1 imaginary) of the w^k coefficient"""
    T = pairing(cid).T
    return T.f12_from_w([(pos[2 * k], pos[2 * k + 1]) for k in range(6)])


def easy_part(cid, a):
    T = pairing(cid).T
    f = T.f12_mul(T.f12_conj(a), T.f12_inv(a))
    return T.f12_mul(T.f12_frob(f, 2), f)


def is_zero(cid, a):
    return all(v == (0, 0) for v in pairing(cid).T.f12_to_w(a))


def gs_sqr(cid, a):
    """The Granger-Scott squaring as tower.hpp f12_cyclo_sqr and finalexp.hpp fe_cyclo_sqr state it, on ANY element: it is a^2 for a
    unitary one.  What fe_pow computes on a base that is not unitary is this recurrence, so it is the reference there (pinned to the
    host build of f12_cyclo_sqr by tests/test_f12_cases.py)."""
    T = pairing(cid).T
    e = T.f12_to_w(a)
    sq, mul, xi, add, sub = T.f2_sqr, T.f2_mul, T.f2_mulxi, T.f2_add, T.f2_sub
    three = lambda v: add(add(v, v), v)
    two = lambda v: add(v, v)
    out = [None] * 6
    for even, odd, lo, hi in ((0, 3, 0, 3), (2, 5, 1, 4), (4, 1, 2, 5)):      # outputs (even k, odd k) from the pair (e_lo, e_hi)
        t0, t1 = sq(e[lo]), sq(e[hi])
        c1 = two(mul(e[lo], e[hi]))
        out[even] = sub(three(add(xi(t1), t0)), two(e[even]))
        tt = xi(c1) if odd == 1 else c1
        out[odd] = add(three(tt), two(e[odd]))
    return T.f12_from_w(out)


def gs_pow(cid, a, e):
    """left to right with gs_sqr as the squaring: fe_pow's value on any base"""
    T = pairing(cid).T
    r = a
    for bit in bin(e)[3:]:
        r = gs_sqr(cid, r)
        if bit == "1":
            r = T.f12_mul(r, a)
    return r


@functools.lru_cache(maxsize=None)
def catalogue(cid):
    """[(tag, element, classes)]: classes is a set out of {"unitary", "gt", "fp6", "zero"}; a few dozen elements per curve"""
    PR = pairing(cid)
    T, c = PR.T, CURVES[cid]
    p = c.p
    rnd = random.Random(5100 + cid)
    rfp = lambda: rnd.randrange(p)
    out = []

    def add(tag, v, *classes):
        w = T.f12_to_w(v)                                 # "fp6" (odd w-coefficients zero) and "zero" are read off the value
        auto = {"fp6"} if all(w[k] == (0, 0) for k in (1, 3, 5)) else set()
        out.append((tag, v, frozenset(classes) - {"fp6", "zero"} | auto | ({"zero"} if all(x == (0, 0) for x in w) else set())))

    add("0", zero12(), "zero", "fp6")
    add("1", T.F12_ONE, "unitary", "gt", "fp6")
    add("-1 = p - 1 in Fp", from_fp(cid, [p - 1] + [0] * 11), "fp6")      # norm 1, yet outside the cyclotomic subgroup
    add("Fp2 element", from_fp(cid, [rfp(), rfp()] + [0] * 10), "fp6")
    f6 = [rfp() if (j // 2) % 2 == 0 else 0 for j in range(12)]
    add("Fp6 element (odd w-coefficients zero)", from_fp(cid, f6), "fp6")
    for k in range(1, 6):
        add("w^%d" % k, from_fp(cid, [1 if j == 2 * k else 0 for j in range(12)]), *(("fp6",) if k % 2 == 0 else ()))
    for j in range(12):
        for v, name in ((1, "1"), (p - 1, "p - 1")):
            cls = ("fp6",) if (j // 2) % 2 == 0 else ()
            add("position %d = %s" % (j, name), from_fp(cid, [v if i == j else 0 for i in range(12)]), *(cls + (("unitary", "gt") if (j, v) == (0, 1) else ())))
    add("all p - 1", from_fp(cid, [p - 1] * 12))
    add("all 1", from_fp(cid, [1] * 12))
    add("alternating 0 / p - 1", from_fp(cid, [0 if j % 2 == 0 else p - 1 for j in range(12)]))
    add("alternating p - 1 / 0", from_fp(cid, [p - 1 if j % 2 == 0 else 0 for j in range(12)]))
    for k in range(2):
        add("unitary %d (easy part of a random element)" % k, easy_part(cid, from_fp(cid, [rfp() for _ in range(12)])), "unitary")
    vec = json.load(open(os.path.join(GOLDEN, "vectors_%s.json" % NAME[cid])))
    for k, row in enumerate(vec["pairings"][:2]):
        g = PR.gt_from_bytes(bytes.fromhex(row["gt"]))
        add("GT %d (golden pairing)" % k, g, "unitary", "gt")
        add("GT %d inverse" % k, T.f12_conj(g), "unitary", "gt")
        if k == 0:
            add("GT 0 to the r - 1", T.f12_pow(g, c.r - 1), "unitary", "gt")
            add("GT 0 to the r", T.f12_pow(g, c.r), "unitary", "gt")
            add("Miller value of GT 0 (its pre-image)", PR.gt_from_bytes(bytes.fromhex(row["miller"])))
    add("Fp6* element (final exponentiation 1, no pairing value)", from_fp(cid, [rfp() if (j // 2) % 2 == 0 else 0 for j in range(12)]), "fp6")
    for k in range(3):
        add("random %d" % k, from_fp(cid, [rfp() for _ in range(12)]))
    return out


def pick(cid, tag):
    return next(v for t, v, _ in catalogue(cid) if t == tag)


def by_class(cid, cls):
    return [(t, v) for t, v, k in catalogue(cid) if cls in k]


REDUCED = ("0", "1", "-1 = p - 1 in Fp", "all p - 1", "w^1", "w^5", "alternating 0 / p - 1", "position 11 = p - 1", "GT 0 (golden pairing)",
           "Miller value of GT 0 (its pre-image)", "random 0")


@functools.lru_cache(maxsize=None)
def binary_cases(cid):
    """[(tag, a, b)]: every ordered pair out of the reduced list, then a x a, a x a^-1 (a invertible), a x 0 and a x 1 for every element"""
    T = pairing(cid).T
    red = [(t, pick(cid, t)) for t in REDUCED]
    out = [("%s x %s" % (ta, tb), a, b) for ta, a in red for tb, b in red]
    for t, a, cls in catalogue(cid):
        out.append(("%s squared" % t, a, a))
        if "zero" not in cls:
            out.append(("%s x its inverse" % t, a, T.f12_inv(a)))
        out.append(("%s x 0" % t, a, zero12()))
        out.append(("%s x 1" % t, a, T.F12_ONE))
    return out


def pow_exponents(cid):
    """[(tag, e)] for fx_pow / fe_pow: at most 128 bits, the top bit of e is the exponent's length"""
    out = [("1", 1), ("2", 2), ("3", 3)]
    for nb in POW_TOP_BITS:
        out.append(("top bit only, %d bits" % nb, 1 << (nb - 1)))
        out.append(("all ones, %d bits" % nb, (1 << nb) - 1))
    out.append(("U_ABS", u_abs(cid)))
    out.append(("BLS12-381's COFACTOR", CURVES[1].cofactor))
    return out


def gt_pow_exponents(cid):
    """[(tag, k, negative)] for bgls_gt_pow"""
    r = CURVES[cid].r
    ks = (("0", 0), ("1", 1), ("r - 1", r - 1), ("r", r), ("r + 1", r + 1), ("2^255", 1 << 255), ("2^256 - 1", (1 << 256) - 1))
    return [("%s%s" % ("-" if neg else "", t), k, neg) for t, k in ks for neg in (0, 1)]


def words(e, n=4):
    return [(e >> (32 * j)) & 0xFFFFFFFF for j in range(n)]


def noncanonical(cid, gt, pos, kind):
    """gt with its pos-th coefficient of the wire order (0 .. 11) replaced by p (kind 0) or by all 0xff bytes (kind 1)"""
    fb = FB[cid]
    bad = CURVES[cid].p.to_bytes(fb, "big") if kind == 0 else b"\xff" * fb
    return gt[:pos * fb] + bad + gt[(pos + 1) * fb:]
