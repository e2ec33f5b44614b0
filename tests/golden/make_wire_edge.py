#!/usr/bin/env python3
"""Generates tests/golden/wire_edge_{altbn128,bls12}.json from the Python oracle alone (oracle/pyref/wire.py, subgroup.py): compressed
encodings at every refusal rule of the two formats, with the oracle's verdict and decompression (subgroup membership included, as
UnmarshalG1 / UnmarshalG2 apply it).  Each row: group, kind (the rule it exercises), in (hex), ok, pt (uncompressed wire bytes, zeros
where refused or at infinity).  Run from the repo root: python tests/golden/make_wire_edge.py"""
import json, os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.pyref.params import BN254, BLS381
from oracle.pyref.groups import Groups
from oracle.pyref.subgroup import Subgroup
from oracle.pyref import wire


def f2_cube_root(T, p, w, rnd):
    """A cube root of w in Fp2, or None where w is no cube.  Tonelli-Shanks for cubes: p^2 - 1 = 3^s t with 3 not dividing t; w^e with
    3 e = 1 (mod t) is a root up to an element of the 3-Sylow subgroup, whose discrete logarithm is taken digit by digit."""
    if w == (0, 0):
        return (0, 0)
    n = p * p - 1
    if T.f2_pow(w, n // 3) != (1, 0):
        return None
    s, t = 0, n
    while t % 3 == 0:
        s, t = s + 1, t // 3
    while True:                                             # a generator c of the 3-Sylow subgroup, from a cubic non-residue
        g = (rnd.randrange(p), rnd.randrange(p))
        if g != (0, 0) and T.f2_pow(g, n // 3) != (1, 0):
            break
    c = T.f2_pow(g, t)
    x = T.f2_pow(w, pow(3, -1, t))
    b = T.f2_mul(T.f2_mul(T.f2_sqr(x), x), T.f2_inv(w))     # x^3 / w: in the 3-Sylow subgroup, = c^j with 3 | j
    j, cinv = 0, T.f2_inv(c)
    zeta = T.f2_pow(c, 3 ** (s - 1))                        # order 3
    for k in range(s):                                      # digit k of j: (b c^-j)^(3^(s-1-k)) = zeta^digit
        u = T.f2_pow(T.f2_mul(b, T.f2_pow(cinv, j)), 3 ** (s - 1 - k))
        d = 0 if u == (1, 0) else (1 if u == zeta else 2)
        assert u == T.f2_pow(zeta, d)
        j += d * 3 ** k
    assert j % 3 == 0
    x = T.f2_mul(x, T.f2_pow(cinv, j // 3))
    assert T.f2_mul(T.f2_sqr(x), x) == (w[0] % p, w[1] % p)
    return x


def build(cv):
    bn = cv.name == "altbn128"
    G, S = Groups(cv), Subgroup(cv)
    p, fb = cv.p, 32 if bn else 48
    rnd = random.Random(0xED6E + fb)
    rows = []
    dec = {1: wire.decompress_g1 if bn else wire.bls_decompress_g1, 2: wire.decompress_g2 if bn else wire.bls_decompress_g2}
    comp = {1: wire.compress_g1 if bn else wire.bls_compress_g1, 2: wire.compress_g2 if bn else wire.bls_compress_g2}
    to_bytes = {1: G.g1_bytes, 2: G.g2_bytes}

    def add(group, data, kind):
        data = bytes(data)
        assert len(data) == fb * group
        P, ok = dec[group](data)
        pt = to_bytes[group](P) if ok else bytes(2 * fb * group)
        row = {"group": group, "kind": kind, "in": data.hex(), "ok": bool(ok), "pt": pt.hex()}
        if group == 2:                                      # the decode before the membership test (wire.hpp's g2_decompress / _zc alone)
            Pc, okc = dec[2](data, subgroup=False)
            row["ok_curve"], row["pt_curve"] = bool(okc), (G.g2_bytes(Pc) if okc else bytes(4 * fb)).hex()
        rows.append(row)
        return ok

    def be(v):
        return v.to_bytes(fb, "big")

    def flag(b, bits):
        b = bytearray(b)
        b[0] |= bits
        return bytes(b)

    g1s = [G.g1_mul(cv.g1, k) for k in (1, 2, rnd.randrange(1, cv.r))]
    g2s = [G.g2_mul(cv.g2, k) for k in (1, 2, rnd.randrange(1, cv.r))]
    top = (1 << 255) - 1 if bn else (1 << 381) - 1          # the largest value the field bytes hold under the flag bits

    def g1_rhs(x):
        return (x * x * x + cv.b) % p

    def no_point_x1():
        x = rnd.randrange(1, p)
        while pow(g1_rhs(x), (p - 1) // 2, p) == 1 or g1_rhs(x) == 0:
            x += 1
        return x

    def no_point_x2():
        T = G.T
        while True:
            x = (rnd.randrange(p), rnd.randrange(1, p))
            a = T.f2_add(T.f2_mul(T.f2_sqr(x), x), G.b2)
            norm = (a[0] * a[0] + a[1] * a[1]) % p
            if pow(norm, (p - 1) // 2, p) == p - 1:         # the norm of a square is a square
                return x

    def g1_outside():
        while True:
            x = rnd.randrange(p)
            y = pow(g1_rhs(x), (p + 1) // 4, p)
            if y * y % p == g1_rhs(x) and G.g1_mul((x, y), cv.r) is not None:
                return (x, y)

    if bn:
        for i, P in enumerate(g1s):
            c = wire.compress_g1(P)
            assert add(1, c, "valid")
            assert add(1, bytes([c[0] ^ 0x80]) + c[1:], "valid, other sign bit: the negative")
        add(1, bytes(32), "infinity")
        add(1, flag(bytes(32), 0x80), "zero x with the sign bit: infinity")
        for f in (0, 0x80):
            assert not add(1, flag(be(p), f), "x = p")
            assert not add(1, flag(be(p + 1), f), "x = p + 1")
            assert not add(1, flag(be(top), f), "x = largest value of the field bytes")
        for _ in range(3):
            assert not add(1, be(no_point_x1()), "x with no point on the curve")
        for i, Q in enumerate(g2s):
            c = wire.compress_g2(Q)
            for fi in (0, 0x80):
                for fr in (0, 0x80):
                    d = bytes([c[0] ^ fi]) + c[1:32] + bytes([c[32] ^ fr]) + c[33:]
                    add(2, d, "valid" if not fi and not fr else ("both sign bits flipped: the negative" if fi and fr else "one sign bit flipped: not a point"))
        for fi in (0, 0x80):
            for fr in (0, 0x80):
                add(2, flag(bytes(32), fi) + flag(bytes(32), fr), "zero x, flags %02x %02x: infinity" % (fi, fr))
        c = wire.compress_g2(g2s[0])
        for v, name in ((p, "p"), (p + 1, "p + 1"), (top, "largest value of the field bytes")):
            assert not add(2, be(v) + c[32:], "x_im = " + name)
            assert not add(2, c[:32] + be(v), "x_re = " + name)
            assert not add(2, flag(be(v), 0x80) + flag(c[32:], 0x80), "x_im = " + name)
        add(2, be(0) + be(p), "x_im = 0, x_re = p")
        for _ in range(3):
            x = no_point_x2()
            assert not add(2, be(x[1]) + be(x[0]), "x with no point on the twist")
    else:
        for P in g1s:
            c = wire.bls_compress_g1(P)
            assert add(1, c, "valid")
            assert add(1, bytes([c[0] ^ 0x20]) + c[1:], "valid, other sort flag: the negative")
            assert not add(1, bytes([c[0] & 0x7F]) + c[1:], "compression flag clear")
            assert not add(1, bytes([c[0] | 0x40]) + c[1:], "infinity flag with a non-zero x")
        assert add(1, flag(bytes(48), 0xC0), "infinity")
        assert not add(1, flag(bytes(48), 0xE0), "infinity flag with the sort flag")
        assert not add(1, flag(bytes(48), 0x40), "infinity flag without the compression flag")
        assert not add(1, flag(bytes(47) + b"\x01", 0xC0), "infinity flag with a non-zero x")
        add(1, flag(bytes(48), 0x80), "x = 0")
        for f in (0x80, 0xA0):
            assert not add(1, flag(be(p), f), "x = p")
            assert not add(1, flag(be(p + 1), f), "x = p + 1")
            assert not add(1, flag(be(top), f), "x = largest value of the field bytes")
        for _ in range(3):
            assert not add(1, flag(be(no_point_x1()), 0x80), "x with no point on the curve")
        for _ in range(3):
            assert not add(1, wire.bls_compress_g1(g1_outside()), "on the curve, outside the subgroup")
        for Q in g2s:
            c = wire.bls_compress_g2(Q)
            assert add(2, c, "valid")
            assert add(2, bytes([c[0] ^ 0x20]) + c[1:], "valid, other sort flag: the negative")
            assert not add(2, bytes([c[0] & 0x7F]) + c[1:], "compression flag clear")
            assert not add(2, bytes([c[0] | 0x40]) + c[1:], "infinity flag with a non-zero x")
        assert add(2, flag(bytes(96), 0xC0), "infinity")
        assert not add(2, flag(bytes(96), 0xE0), "infinity flag with the sort flag")
        assert not add(2, flag(bytes(96), 0x40), "infinity flag without the compression flag")
        assert not add(2, flag(bytes(95) + b"\x01", 0xC0), "infinity flag with a non-zero x")
        add(2, flag(bytes(96), 0x80), "x = 0")
        c = wire.bls_compress_g2(g2s[0])
        for v, name in ((p, "p"), (p + 1, "p + 1"), (top, "largest value of the field bytes")):
            assert not add(2, flag(be(v), 0x80) + c[48:], "x_im = " + name)
            assert not add(2, c[:48] + be(v), "x_re = " + name)
        assert not add(2, c[:48] + bytes([0xFF]) * 48, "x_re = 2^384 - 1")
        for _ in range(3):
            x = no_point_x2()
            assert not add(2, flag(be(x[1]), 0x80) + be(x[0]), "x with no point on the twist")
    for _ in range(4):
        assert not add(2, comp[2](S.random_twist_point(rnd)), "on the twist, outside the subgroup")
    N = S.twist_order()
    Q = G.g2_mul(S.random_twist_point(rnd), N // cv.r)
    assert add(2, comp[2](Q), "valid: [cofactor] random")
    # Points whose y^2 lies in Fp (the a.c1 == 0 branch of the Fp2 root): y in Fp or in i Fp, x a cube root of y^2 - b' in Fp2 -- a third
    # of the candidates have one.  Bounded search: y = 0 (the 2-torsion, where -b' is a cube) and up to TRIES random y of each shape, until
    # WANT of each shape are found.  Such a point is on the twist and, but for a coincidence, outside the subgroup: the whole decode
    # refuses it at the membership test, ok_curve / pt_curve say what the decode before that test makes of every flag setting.
    T = G.T
    TRIES, WANT = 24, 2
    found = []
    for shape in ("y = 0", "y in Fp", "y in i Fp"):
        got = 0
        for _ in range(1 if shape == "y = 0" else TRIES):
            v = 0 if shape == "y = 0" else rnd.randrange(1, p)
            y = (v, 0) if shape != "y in i Fp" else (0, v)
            x = f2_cube_root(T, p, T.f2_sub(T.f2_sqr(y), G.b2), rnd)
            if x is None:
                continue
            assert G.g2_on_curve((x, y))
            found.append((shape, x, y))
            got += 1
            if got == WANT:
                break
    for shape, x, y in found:
        if bn:
            for fi in (0, 0x80):
                for fr in (0, 0x80):
                    add(2, flag(be(x[1]), fi) + flag(be(x[0]), fr), "y^2 in Fp (%s), flags %02x %02x" % (shape, fi, fr))
        else:
            for f in (0x80, 0xA0):
                add(2, flag(be(x[1]), f) + be(x[0]), "y^2 in Fp (%s), flags %02x" % (shape, f))
    return {"curve": cv.name, "y2_in_fp_found": len(found), "y2_in_fp_search": "y = 0 and up to %d random y in Fp and in i Fp each, %d wanted of each" % (TRIES, WANT),
            "cases": rows}


if __name__ == "__main__":
    for cv in (BN254, BLS381):
        doc = build(cv)
        json.dump(doc, open(os.path.join(ROOT, "tests", "golden", "wire_edge_%s.json" % cv.name), "w"), indent=1)
        print(cv.name, len(doc["cases"]), "encodings;", sum(r["ok"] for r in doc["cases"]), "accepted")
