"""CPU tier of the combined Boneh-Boyen check's coefficient sums: bgls_amd/csrc/bb_rlc.hpp (the body of k_bb_rlc_sums: six-word lane sums
with explicit carries, a tree over the 64 lanes, a 32-byte big-endian store) compiled for the host by tests/harness/bb_rlc_host.cpp with
the wave emulated, against Python's integer sums.  The same program is built once more under -fsanitize=address,undefined and run
stand-alone (nothing loaded into Python runs under a sanitizer)."""
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "harness", "bb_rlc_host.cpp")
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"
TOP = (1 << 128) - 1


def offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


def cases():
    """[(tag, coefficients, offsets)]"""
    rnd = random.Random(7300)
    coeff = lambda n: [rnd.getrandbits(128) for _ in range(n)]           # even ones among them: the sum counts them with the lowest bit set
    out = []
    sizes = [0, 1, 63, 64, 65, 4097, 0, 0, 2]
    out.append(("empty groups and the sizes around a wave", coeff(sum(sizes)), offsets(sizes)))
    out.append(("every coefficient 2^128 - 1: the top carries", [TOP] * sum(sizes), offsets(sizes)))
    ragged = [rnd.randrange(0, 200) for _ in range(40)]
    out.append(("ragged offsets", coeff(sum(ragged)), offsets(ragged)))
    out.append(("one group over everything", coeff(1000), [0, 1000]))
    out.append(("nothing but empty groups", [], [0, 0, 0]))
    out.append(("all zero bytes: every coefficient is 1", [0] * 130, [0, 65, 130]))
    return out


def run(exe, cs):
    got = []
    for tag, r, off in cs:
        text = "%d %d\n%s\n%s\n" % (len(r), len(off) - 1, " ".join(map(str, off)), "\n".join("%032x" % x for x in r))
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (tag, p.stderr[-2000:])
        got.append(p.stdout.split())
    return got


def check(cs, got):
    for (tag, r, off), lines in zip(cs, got):
        want = ["%064x" % sum(x | 1 for x in r[off[g]:off[g + 1]]) for g in range(len(off) - 1)]
        assert lines == want, tag


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bb_rlc") / "bb_rlc_host")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", SRC, "-o", path], check=True, timeout=900)
    return path


def test_sums_equal_the_integer_sums(exe):
    cs = cases()
    check(cs, run(exe, cs))


def test_the_cases_carry_past_the_coefficients_width():
    """4097 coefficients of 2^128 - 1 sum to more than 2^140: the words above the coefficients' four are carried into, in the tree and in
    a lane's own chain (65 terms) alike"""
    tag, r, off = cases()[1]
    assert max(sum(r[off[g]:off[g + 1]]) for g in range(len(off) - 1)) >> 128 >= 4096
    assert sum(r[off[5] + 0:off[6]:64]) >> 128 >= 64


def test_sums_under_the_sanitizers(tmp_path):
    path = str(tmp_path / "bb_rlc_host_san")
    subprocess.run([CLANGXX, "-std=c++17", "-O0", "-g0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", path], check=True, timeout=900)
    cs = cases()
    check(cs, run(path, cs))
