"""CPU tier for the throughput final exponentiation (bgls_amd/csrc/finalxt.hpp, k_finalxt_batch), walked on the host by
tests/harness/host_harness_fxt.cpp: the six coefficient lanes of one group on six lock-stepped threads run the kernel's own routine
(fxt_run), with every column accumulation checked for overflow and every published entry checked against the bounds the header states
(the harness answers -3 where either breaks).  Against oracle.pyref, byte-exact, over the catalogue of tests/f12_cases.py on both curves:
the general product, the squaring, the Frobenius maps 1 .. 3, conjugation, the inversion and the whole final exponentiation."""
import ctypes
import importlib.util
import os
import subprocess

import pytest

import f12_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CIDS = [0, 1]
MUL, CONJ, FROB, INVD, SCALE = range(5)


def word(op, dst, a, b=0):
    return op | dst << 4 | a << 8 | b << 12


# a^-1 on the temporaries 0 .. 4 (both curves' files hold at least five): the norm chain as tools/gen_constants.py emits it
INVERSE = [word(CONJ, 1, 0), word(MUL, 2, 0, 1), word(FROB, 3, 2, 2), word(FROB, 4, 3, 2), word(MUL, 3, 3, 4), word(MUL, 4, 2, 3), word(INVD, 4, 4),
           word(SCALE, 3, 3, 4), word(MUL, 1, 1, 3)]


@pytest.fixture(scope="module")
def fxt():
    spec = importlib.util.spec_from_file_location("build_harness_fxt", os.path.join(ROOT, "tests", "harness", "build_harness_fxt.py"))
    bh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bh)
    return ctypes.CDLL(bh.build())


def _buf(b):
    return (ctypes.c_uint8 * len(b)).from_buffer_copy(b)


def run(lib, cid, prog, out_reg, a, b=None):
    o = (ctypes.c_uint8 * (12 * fc.FB[cid]))()
    rc = lib.ht_fxt_run(cid, _buf(a), _buf(a if b is None else b), (ctypes.c_uint32 * len(prog))(*prog), len(prog), out_reg, o)
    assert rc == 0, "code %d (-3: a column overflow or a published entry outside its stated bound; -1: a malformed program)" % rc
    return bytes(o)


def gtb(cid, a):
    return fc.pairing(cid).gt_bytes(a)


@pytest.mark.parametrize("cid", CIDS)
def test_the_generated_program_fits_its_file(fxt, cid):
    assert 5 <= fxt.ht_fxt_nt(cid) <= 8 and 250 < fxt.ht_fxt_prog_len(cid) < 500
    assert fxt.ht_fxt_run(cid, _buf(bytes(12 * fc.FB[cid])), _buf(bytes(12 * fc.FB[cid])), (ctypes.c_uint32 * 1)(word(MUL, 15, 0, 0)), 1, 0,
                          (ctypes.c_uint8 * 576)()) == -1


@pytest.mark.parametrize("cid", CIDS)
def test_general_product(fxt, cid):
    T = fc.pairing(cid).T
    for t, a, b in fc.binary_cases(cid):
        assert run(fxt, cid, [word(MUL, 2, 0, 1)], 2, gtb(cid, a), gtb(cid, b)) == gtb(cid, T.f12_mul(a, b)), t


@pytest.mark.parametrize("cid", CIDS)
def test_unary_routines(fxt, cid):
    T = fc.pairing(cid).T
    for t, a, cls in fc.catalogue(cid):
        ab = gtb(cid, a)
        assert run(fxt, cid, [word(MUL, 2, 0, 0)], 2, ab) == gtb(cid, T.f12_mul(a, a)), ("squaring", t)
        assert run(fxt, cid, [word(CONJ, 2, 0)], 2, ab) == gtb(cid, T.f12_conj(a)), ("conjugation", t)
        for k in (1, 2, 3):
            assert run(fxt, cid, [word(FROB, 2, 0, k)], 2, ab) == gtb(cid, T.f12_frob(a, k)), ("frobenius", k, t)
        # a product of a conjugate and of a Frobenius image: operands that are not carry-normalised
        assert run(fxt, cid, [word(CONJ, 1, 0), word(FROB, 2, 0, 1), word(MUL, 3, 1, 2)], 3, ab) == gtb(cid, T.f12_mul(T.f12_conj(a), T.f12_frob(a, 1))), t
        want = fc.zero12() if "zero" in cls else T.f12_inv(a)
        assert run(fxt, cid, INVERSE, 1, ab) == gtb(cid, want), ("inversion", t)


@pytest.mark.parametrize("cid", CIDS)
def test_whole_final_exponentiation(fxt, cid):
    PR = fc.pairing(cid)
    one = gtb(cid, PR.T.F12_ONE)
    for t, a, cls in fc.catalogue(cid):
        ab = gtb(cid, a)
        o = (ctypes.c_uint8 * len(ab))()
        rc = fxt.ht_fxt_final_exp(cid, _buf(ab), o)
        assert rc == 0, (t, rc)
        assert bytes(o) == PR.gt_bytes(PR.final_exp(a)), t
        if "zero" in cls:
            assert bytes(o) == bytes(len(ab)), t
        if "fp6" in cls and "zero" not in cls:
            assert bytes(o) == one, t


def test_committed_program_is_what_the_generator_emits(tmp_path):
    """tools/gen_constants.py checks the program's exponents and the size of its register file when it runs: the committed header must
    be its output (and the generator must leave the other two generated headers as they are)"""
    spec = importlib.util.spec_from_file_location("gen_constants", os.path.join(ROOT, "tools", "gen_constants.py"))
    gc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gc)
    gc.OUT = str(tmp_path / "constants_gen.hpp")
    gc.main()
    for name in ("constants_fxt_gen.hpp", "constants_gen.hpp", "constants_latx_gen.hpp"):
        assert open(tmp_path / name).read() == open(os.path.join(ROOT, "bgls_amd", "csrc", name)).read(), name


def test_stand_alone_program_for_sanitizers(tmp_path):
    """the same harness source with its own main, under the address and undefined-behaviour sanitizers: a stand-alone program, nothing
    loaded into Python"""
    exe = str(tmp_path / "fxt_main")
    src = os.path.join(ROOT, "tests", "harness", "host_harness_fxt.cpp")
    subprocess.run(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-pthread", "-DFXT_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", exe], check=True, timeout=900)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
