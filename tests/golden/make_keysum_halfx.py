#!/usr/bin/env python3
"""Generates tests/golden/keysum_halfx.json from the Python oracle alone (oracle/pyref): per curve two points of the twist E'(Fp2) whose
x have the same real part and different imaginary parts ("re"), and two whose x have the same imaginary part and different real parts
("im"), as uncompressed wire bytes.  Found by a search over small x with the oracle's Fp2 square root; none of them is in the order-r
subgroup (asserted), so they are inputs for the wire-byte key sums only, which check the curve equation and not the subgroup.  Where two
such points meet in an addition of the lane-pair key sum, one lane's half of H = x2 - x1 is zero and the other's is not.
Run from the repo root: python tests/golden/make_keysum_halfx.py"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.pyref.params import BN254, BLS381
from oracle.pyref.subgroup import Subgroup

out = {}
for cv in (BN254, BLS381):
    S = Subgroup(cv)
    G, T = S.G, S.G.T

    def on_twist(x):
        rhs = T.f2_add(T.f2_mul(T.f2_sqr(x), x), G.b2)
        y = T.f2_sqrt(rhs)
        return (x, y) if y is not None and y != (0, 0) and G.g2_on_curve((x, y)) else None

    def two(xs):
        pts = []
        for x in xs:
            Q = on_twist(x)
            if Q is not None:
                assert not S.in_subgroup(Q)
                pts.append(Q)
            if len(pts) == 2:
                return pts
        raise AssertionError("search bound too small")

    re = two((3, b) for b in range(1, 64))
    im = two((a, 5) for a in range(1, 64))
    assert re[0][0][0] == re[1][0][0] and re[0][0][1] != re[1][0][1]
    assert im[0][0][1] == im[1][0][1] and im[0][0][0] != im[1][0][0]
    out[cv.name] = {"re": [G.g2_bytes(Q).hex() for Q in re], "im": [G.g2_bytes(Q).hex() for Q in im]}
    print(cv.name, [Q[0] for Q in re], [Q[0] for Q in im])
json.dump(out, open(os.path.join(ROOT, "tests", "golden", "keysum_halfx.json"), "w"), indent=1)
