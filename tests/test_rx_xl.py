"""CPU tier for the XL form of k_miller_x60 (bgls_amd/csrc/miller_x.hpp: the xi of a fold's wrapped terms on the LINE, formed once by the
producers, instead of on the accumulator in every publish), walked on the host by tests/harness/host_harness_xl.cpp with every column
accumulation and every stated bound checked (BGLS_RX_CHECK):

  one group of six pairings over the whole alt-bn128 loop -- 65 doublings, 21 + 2 additions, 88 line steps -- the producers' lane pairs on two
  lock-stepped threads, the consumer's six lanes in the kernel's order.  Every coefficient the new form publishes must be the field element the
  old form publishes, at every one of the 1 + 64 + 6 * 88 publishes; the group's output after from_ux_inl must be the same bytes; and with real
  lines it must be the product of pairing.hpp's Miller values."""
import ctypes
import importlib.util
import os
import random

import pytest

from oracle.pyref.groups import Groups
from oracle.pyref.params import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = 6 * 2 * 32          # six Fp2 of eight 32-bit words


@pytest.fixture(scope="module")
def xl_harness():
    spec = importlib.util.spec_from_file_location("build_harness_xl", os.path.join(ROOT, "tests", "harness", "build_harness_xl.py"))
    bh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bh)
    return ctypes.CDLL(bh.build())


@pytest.fixture(scope="module")
def points():
    c = CURVES["altbn128"]
    G = Groups(c)
    rnd = random.Random(6029)
    g1 = b"".join(G.g1_bytes(G.g1_mul(c.g1, rnd.randrange(1, c.r))) for _ in range(6))
    g2 = b"".join(G.g2_bytes(G.g2_mul(c.g2, rnd.randrange(1, c.r))) for _ in range(6))
    return g1, g2


def walk(lib, points, present, mode):
    g1, g2 = points
    old, new, ref = (ctypes.c_uint8 * OUT)(), (ctypes.c_uint8 * OUT)(), (ctypes.c_uint8 * OUT)()
    rc = lib.ht_xl_group((ctypes.c_uint8 * len(g1)).from_buffer_copy(g1), (ctypes.c_uint8 * len(g2)).from_buffer_copy(g2),
                         (ctypes.c_uint8 * 6)(*present), mode, old, new, ref)
    assert rc == 0, ("XL walk: code %d (1 + the first publish whose coefficients differ from the old form's mod p; -3 = a column overflow or a "
                     "violated bound; -2 = bad point)" % rc)
    return bytes(old), bytes(new), bytes(ref)


def test_loop_shape(xl_harness):
    assert xl_harness.ht_xl_steps() == 88


@pytest.mark.parametrize("present", [(1, 1, 1, 1, 1, 1), (1, 0, 1, 1, 0, 1), (0, 0, 0, 0, 0, 0)], ids=["full", "constant-1-lines", "all-absent"])
def test_xl_publishes_what_the_old_form_publishes(xl_harness, points, present):
    old, new, ref = walk(xl_harness, points, present, 0)
    assert new == old, "group output after from_ux_inl differs"
    assert new == ref, "group output is not the product of pairing.hpp's Miller values"


@pytest.mark.parametrize("present", [(1, 1, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1)], ids=["full", "constant-1-line"])
def test_xl_on_worst_case_limbs(xl_harness, points, present):
    """every line entry at its bound (2.1 p / 2.1 p / 3.1 p) with all-ones low limbs: the xi copies' own bound, the folds' column budget with
    (xi L) x (plain B) wrapped terms and ux_mulxi's precondition ahead of the squaring are all checked inside the walk"""
    old, new, _ = walk(xl_harness, points, present, 1)
    assert new == old
