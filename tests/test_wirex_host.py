"""CPU tier: the compressed wire formats on the carry-free limbs (bgls_amd/csrc/wire_x.hpp) compiled for the host with every column
accumulation checked (tests/harness/wirex_host.cpp), against the Python oracle (oracle/pyref/wire.py, subgroup.py): the Fp2 square
root at function level on every branch, psi and the membership test on the subgroup fixtures, and the whole decode of every case of
the wire fixtures and of the edge fixture (tests/golden/make_wire_edge.py).  The same source is built once more as a stand-alone
program under -fsanitize=address,undefined and run over the edge fixture (nothing loaded into Python runs under a sanitizer)."""
import ctypes
import importlib.util
import json
import os
import random
import subprocess

import pytest

from oracle.pyref import wire
from oracle.pyref.groups import Groups
from oracle.pyref.params import BN254, BLS381
from oracle.pyref.subgroup import Subgroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"
CURVES = [(0, BN254, "altbn128"), (1, BLS381, "bls12")]
IDS = ["altbn128", "bls12"]


@pytest.fixture(scope="module")
def harness():
    spec = importlib.util.spec_from_file_location("build_harness_wirex", os.path.join(ROOT, "tests", "harness", "build_harness_wirex.py"))
    bh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bh)
    lib = ctypes.CDLL(bh.build())
    u8p, sz = ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t
    for name, args in (("wirex_f2_root", [ctypes.c_int, u8p, u8p, u8p, u8p]), ("wirex_psi", [ctypes.c_int, u8p, u8p]),
                       ("wirex_in_subgroup", [ctypes.c_int, ctypes.c_int, u8p]),
                       ("wirex_decode", [ctypes.c_int, ctypes.c_int, u8p, sz, ctypes.c_int, u8p, u8p])):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = args
    return lib


def buf(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if len(b) else b"\0")


def fp_bytes(cv):
    return 32 if cv is BN254 else 48


def oracle_root(cv, a):
    """the oracle's Fp2 root of a = (re, im) followed by the final check both formats apply, or None"""
    p = cv.p
    if cv is BN254:
        r = wire.calc_complex_quad_res(a)
    else:
        r = wire._f2_sqrt381(a)
    if r is None:
        return None
    sq = ((r[0] * r[0] - r[1] * r[1]) % p, 2 * r[0] * r[1] % p)
    return r if sq == (a[0] % p, a[1] % p) else None


def root_of(lib, cid, cv, a):
    fb = fp_bytes(cv)
    rr, ri = (ctypes.c_uint8 * fb)(), (ctypes.c_uint8 * fb)()
    rc = lib.wirex_f2_root(cid, buf(a[0].to_bytes(fb, "big")), buf(a[1].to_bytes(fb, "big")), rr, ri)
    assert rc in (0, 1), "a column overflowed" if rc == -3 else rc
    return (int.from_bytes(bytes(rr), "big"), int.from_bytes(bytes(ri), "big")) if rc else None


def same_root(cv, got, want):
    """+-: the sign of the root is the format's sign rule's to choose, not the root's"""
    if got is None or want is None:
        return got is None and want is None
    p = cv.p
    return got == want or got == ((p - want[0]) % p, (p - want[1]) % p)


def f2_cases(cv):
    p = cv.p
    rnd = random.Random(0xF2 + p % 1000)
    qr = lambda v: pow(v, (p - 1) // 2, p) == 1
    sq = lambda r: ((r[0] * r[0] - r[1] * r[1]) % p, 2 * r[0] * r[1] % p)
    res = next(v for v in iter(lambda: rnd.randrange(2, p), None) if qr(v))
    non = next(v for v in iter(lambda: rnd.randrange(2, p), None) if not qr(v))
    cases = [("zero", (0, 0)), ("a in Fp, a residue", (res, 0)), ("a in Fp, a non-residue", (non, 0)), ("one", (1, 0)), ("minus one", (p - 1, 0)),
             ("i", (0, 1)), ("a0 = 0", (0, res)), ("a0 = 0, a1 a non-residue", (0, non))]
    first = fallback = nonsq = 0
    inv2 = pow(2, -1, p)
    while first < 6 or fallback < 6:
        a = sq((rnd.randrange(p), rnd.randrange(1, p)))
        if a[1] == 0:
            continue
        lam = pow((a[0] * a[0] + a[1] * a[1]) % p, (p + 1) // 4, p)
        d = (a[0] + lam) * inv2 % p
        if d == 0 or qr(d):
            if first < 6:
                cases.append(("square, first delta", a))
                first += 1
        elif fallback < 6:
            cases.append(("square, fallback delta", a))
            fallback += 1
    while nonsq < 8:
        a = (rnd.randrange(p), rnd.randrange(1, p))
        if not qr((a[0] * a[0] + a[1] * a[1]) % p):
            cases.append(("non-square", a))
            nonsq += 1
    if cv is BN254:
        # r.c0 = 0 with a1 != 0 needs a delta of 0, i.e. a0 = -+lam with lam^2 = +-(a0^2 + a1^2): the plus sign gives a1 = 0, the minus sign
        # a1^2 = -2 a0^2 -- and -2 is a non-residue (p = 7 mod 8), so no such input exists; the branch is reached through a1 = 0 only, where
        # calcComplexQuadRes returns before its test ("zero" above: r = (0, 0), accepted as the root of 0)
        assert p % 8 == 7 and not qr(p - 2)
    for _ in range(200):
        cases.append(("random square", sq((rnd.randrange(p), rnd.randrange(p)))))
    return cases


@pytest.mark.parametrize("cid,cv,name", CURVES, ids=IDS)
def test_fp2_root_on_every_branch(harness, cid, cv, name):
    kinds = set()
    for kind, a in f2_cases(cv):
        want = oracle_root(cv, a)
        got = root_of(harness, cid, cv, a)
        assert same_root(cv, got, want), (kind, a, got, want)
        kinds.add((kind, want is not None))
    assert ("square, first delta", True) in kinds and ("square, fallback delta", True) in kinds and ("non-square", False) in kinds
    # alt-bn128 takes cand(a0) untested where a.c1 = 0: a non-residue a0 is refused although i sqrt(-a0) is a root; BLS12-381 finds it
    assert ("a in Fp, a non-residue", cv is not BN254) in kinds


@pytest.mark.parametrize("cid,cv,name", CURVES, ids=IDS)
def test_psi_and_membership_on_the_subgroup_fixture(harness, cid, cv, name):
    doc = json.load(open(os.path.join(GOLDEN, "subgroup_%s.json" % name)))
    S = Subgroup(cv)
    G = S.G
    fb = fp_bytes(cv)
    seen = set()
    for row in doc["points"]:
        if not row["on_twist"]:
            continue
        pt = bytes.fromhex(row["pt"])
        rc = harness.wirex_in_subgroup(cid, 2, buf(pt))
        assert rc == (1 if row["in_subgroup"] else 0), (row["note"], rc)
        seen.add(row["in_subgroup"])
        Q = G.g2_from_bytes(pt)
        if Q is not None:
            out = (ctypes.c_uint8 * (4 * fb))()
            assert harness.wirex_psi(cid, buf(pt), out) == 0, row["note"]
            assert bytes(out) == G.g2_bytes(S.psi(Q)), row["note"]
    assert seen == {True, False}
    for row in doc["g1_points"]:
        if not row["on_curve"]:
            continue
        rc = harness.wirex_in_subgroup(cid, 1, buf(bytes.fromhex(row["pt"])))
        assert rc == (1 if row["in_subgroup"] else 0), (row["note"], rc)


def decode(lib, cid, cv, group, encs, subgroup=1):
    fb = fp_bytes(cv)
    n = len(encs)
    out, ok = (ctypes.c_uint8 * (n * 2 * group * fb))(), (ctypes.c_uint8 * n)()
    rc = lib.wirex_decode(cid, group, buf(b"".join(encs)), n, subgroup, out, ok)
    assert rc == 0, "a column overflowed" if rc == -3 else rc
    ub = 2 * group * fb
    return [bytes(out)[i * ub:(i + 1) * ub] for i in range(n)], list(ok)


def oracle_decode(cv, group, data):
    bn = cv is BN254
    f = {1: wire.decompress_g1 if bn else wire.bls_decompress_g1, 2: wire.decompress_g2 if bn else wire.bls_decompress_g2}[group]
    P, ok = f(data)
    G = Groups(cv)
    ub = 2 * group * fp_bytes(cv)
    return ((G.g1_bytes if group == 1 else G.g2_bytes)(P) if ok else bytes(ub)), bool(ok)


@pytest.mark.parametrize("cid,cv,name", CURVES, ids=IDS)
def test_whole_decode_of_the_wire_fixtures(harness, cid, cv, name):
    doc = json.load(open(os.path.join(GOLDEN, "wire_%s.json" % name)))
    for group in (1, 2):
        encs = [bytes.fromhex(r["compressed"]) for r in doc["g%d" % group]] + [bytes.fromhex(r["in"]) for r in doc["g%d_decode" % group]]
        pts, oks = decode(harness, cid, cv, group, encs)
        for e, pt, ok in zip(encs, pts, oks):
            want_pt, want_ok = oracle_decode(cv, group, e)
            assert (bool(ok), pt) == (want_ok, want_pt), (group, e.hex())
        for r, pt, ok in zip(doc["g%d" % group], pts, oks):
            assert ok == 1 and pt == bytes.fromhex(r["pt"])


def edge_cases(name):
    return json.load(open(os.path.join(GOLDEN, "wire_edge_%s.json" % name)))["cases"]


@pytest.mark.parametrize("cid,cv,name", CURVES, ids=IDS)
def test_whole_decode_of_the_edge_fixture(harness, cid, cv, name):
    cases = edge_cases(name)
    assert any(c["ok"] for c in cases) and any(not c["ok"] for c in cases)
    for group in (1, 2):
        rows = [c for c in cases if c["group"] == group]
        pts, oks = decode(harness, cid, cv, group, [bytes.fromhex(c["in"]) for c in rows])
        for c, pt, ok in zip(rows, pts, oks):
            assert (bool(ok), pt.hex()) == (c["ok"], c["pt"]), (group, c["kind"], c["in"])
    # the decode before the membership test: what the sign rules make of the points with y^2 in Fp, which the membership test then refuses
    rows = [c for c in cases if c["group"] == 2]
    pts, oks = decode(harness, cid, cv, 2, [bytes.fromhex(c["in"]) for c in rows], subgroup=0)
    for c, pt, ok in zip(rows, pts, oks):
        assert (bool(ok), pt.hex()) == (c["ok_curve"], c["pt_curve"]), (c["kind"], c["in"])
    y2 = [c for c in rows if c["kind"].startswith("y^2 in Fp")]
    doc = json.load(open(os.path.join(GOLDEN, "wire_edge_%s.json" % name)))
    assert doc["y2_in_fp_found"] >= 4 and len(y2) == doc["y2_in_fp_found"] * (4 if cv is BN254 else 2)
    # every flag setting of such a point is decided by the sign rule, both ways: some settings decode, some are refused (alt-bn128: a set
    # bit on the zero component, and y in i Fp altogether -- the reference's untested cand(a0); BLS12-381 decodes both sort flags unless y = 0)
    assert {c["ok_curve"] for c in y2} == {True, False} if cv is BN254 else any(c["ok_curve"] for c in y2)
    for shape in ("y in Fp", "y in i Fp"):                      # y = 0 is there only where -b' is a cube
        assert any("(%s)" % shape in c["kind"] for c in y2), shape


@pytest.mark.parametrize("cid,cv,name", CURVES, ids=IDS)
def test_the_edge_fixture_is_what_the_oracle_says(cid, cv, name):
    bn = cv is BN254
    for c in edge_cases(name):
        pt, ok = oracle_decode(cv, c["group"], bytes.fromhex(c["in"]))
        assert (ok, pt.hex()) == (c["ok"], c["pt"]), c["kind"]
        if c["group"] == 2:
            P, okc = (wire.decompress_g2 if bn else wire.bls_decompress_g2)(bytes.fromhex(c["in"]), subgroup=False)
            assert (bool(okc), (Groups(cv).g2_bytes(P) if okc else bytes(4 * fp_bytes(cv))).hex()) == (c["ok_curve"], c["pt_curve"]), c["kind"]


def test_edge_fixture_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "wirex_san")
    subprocess.run([CLANGXX, "-std=c++17", "-O0", "-g0", "-DWIREX_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "harness", "wirex_host.cpp"), "-o", exe], check=True, timeout=1500)
    lines, want = [], []
    for cid, cv, name in CURVES:
        for c in edge_cases(name):
            lines.append("%d %d %s" % (cid, c["group"], c["in"]))
            want.append("%d %s 0" % (1 if c["ok"] else 0, c["pt"]))
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.split("\n")[:-1] == want
