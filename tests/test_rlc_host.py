"""CPU tier of the combined check's per-set body: bgls_amd/csrc/rlc_pair.hpp (one walk over the digits of r for r H and r sigma, one
inversion for both results) compiled for the host by tests/harness/rlc_host.cpp with every column accumulation checked, against the
plain affine k P of tests/ec_ref.py on both curves.  The same program is built once more under -fsanitize=address,undefined and run
stand-alone (nothing loaded into Python runs under a sanitizer)."""
import os
import random
import subprocess

import pytest

import point_cases as pc
from ec_ref import Curve, ORDER, recode

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "harness", "rlc_host.cpp")
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"
TOP = (1 << 128) - 1


def cases(cid):
    """[(tag, H, sigma, r, mode)]: points as ec_ref holds them (None = infinity)"""
    cv = Curve(cid, 1)
    q = ORDER[cid]
    rnd = random.Random(5100 + cid)
    pt = lambda: cv.mul(cv.gen, rnd.randrange(1, q))
    out = []
    for i in range(4):
        out.append(("random %d" % i, pt(), pt(), rnd.getrandbits(128) | 1, 0))
    H, S = pt(), pt()
    out.append(("H at infinity", None, S, rnd.getrandbits(128) | 1, 0))
    out.append(("sigma at infinity", H, None, rnd.getrandbits(128) | 1, 0))
    out.append(("both at infinity", None, None, rnd.getrandbits(128) | 1, 0))
    out.append(("r = 1", H, S, 1, 0))
    out.append(("r = 2^128 - 1", H, S, TOP, 0))
    out.append(("r = 0 (not a coefficient: both results at infinity)", H, S, 0, 0))
    for i, d in ((0, 1), (0, 7), (5, 7), (17, 3), (31, 5), (31, 7)):           # a single non-zero window digit d at window i
        out.append(("single digit %d at window %d" % (d, i), H, S, d << (4 * i), 0))
    out.append(("r = 2^127 (digit -8 at window 31, the carry into window 32)", H, S, 1 << 127, 0))
    out.append(("r = 2^127 + 1 (the top bit of the top word and the bit under window 0)", H, S, (1 << 127) | 1, 0))
    out.append(("sigma = -H", H, cv.neg(H), rnd.getrandbits(128) | 1, 0))
    out.append(("sigma = H", H, H, rnd.getrandbits(128) | 1, 0))
    out.append(("even r, lowest bit set by rlc_scalar", H, S, rnd.getrandbits(128) & ~1, 1))
    out.append(("odd r through rlc_scalar", H, S, rnd.getrandbits(128) | 1, 1))
    # the exceptional scalars of the point layer's own cases: 128-bit scalars steered so that an addition of the walk meets its own
    # addend (a doubling) or its negative (infinity), and small-order points where r P is infinity -- beside an ordinary point in the
    # other slot, in both orders
    for c in pc.mul_cases(cid, 1):
        if c["k"] >> 128 or c["order"] in (None, q):
            continue
        P = cv.from_bytes(c["pt"])
        out.append((c["tag"] + " | as H", P, S, c["k"], 0))
        out.append((c["tag"] + " | as sigma", H, P, c["k"], 0))
    return out


def events(cid):
    ev = set()
    for c in pc.mul_cases(cid, 1):
        if not c["k"] >> 128 and c["order"] not in (None, ORDER[cid]) and c["order"] > 1:
            ev |= recode(c["k"], 128, c["order"])[1]                           # the walk of rlc_mul2: always 33 windows
    return ev


def run(exe, cid, cs, env=None):
    cv = Curve(cid, 1)
    text = "".join("%d %d %s %s %032x\n" % (cid, mode, cv.to_bytes(H).hex(), cv.to_bytes(S).hex(), r) for _, H, S, r, mode in cs)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(cs)
    return lines


def check(cid, cs, lines):
    cv = Curve(cid, 1)
    for (tag, H, S, r, mode), line in zip(cs, lines):
        k = r | 1 if mode else r
        want = "%s %s 0" % (cv.to_bytes(cv.mul(H, k)).hex(), cv.to_bytes(cv.mul(S, k)).hex())
        assert line == want, (cid, tag, hex(r))


@pytest.fixture(scope="module")
def rlc_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rlc") / "rlc_host")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", SRC, "-o", exe], check=True, timeout=900)
    return exe


@pytest.mark.parametrize("cid", [0, 1])
def test_pair_equals_the_plain_reference(rlc_exe, cid):
    cs = cases(cid)
    check(cid, cs, run(rlc_exe, cid, cs))


def test_the_exceptional_scalars_reach_the_exceptional_branches():
    """BLS12-381's G1 has points outside the subgroup (orders 3, 11, ...): the 128-bit steered scalars put a doubling and a cancellation
    inside the 33-window walk, and (0, 2) of order 3 makes table entries and results infinity.  alt-bn128's G1 has prime order: no
    128-bit scalar reaches those branches there, and point_cases has none.  (The general addition is what every random case takes.)"""
    assert {"double", "cancel", "tab_inf", "r_inf", "dbl_inf", "digit0"} <= events(1)
    assert events(0) == set()


def test_bad_points_are_reported(rlc_exe):
    cv = Curve(0, 1)
    off = bytearray(cv.to_bytes(cv.gen))
    off[-1] ^= 1
    p = subprocess.run([rlc_exe], input="0 0 %s %s %032x\n" % (bytes(off).hex(), cv.to_bytes(cv.gen).hex(), 3), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout == "bad\n"


def test_pair_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "rlc_host_san")
    subprocess.run([CLANGXX, "-std=c++17", "-O0", "-g0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe], check=True, timeout=900)
    for cid in (0, 1):
        cs = cases(cid)
        cs = cs[:21] + cs[21::5]                                # every plain case, every fifth of the exceptional ones
        check(cid, cs, run(exe, cid, cs))
