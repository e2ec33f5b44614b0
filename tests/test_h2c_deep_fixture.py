"""CPU tier: the mined fixture tests/golden/h2c_deep_altbn128.json (real 64-byte messages whose alt-bn128 try-and-increment first accepts
at counter 0..18, tests/golden/make_h2c_deep.py) against both oracles.  The GPU tier (test_gpu_h2c_deep.py) runs the same rows through
the wide kernel and the two round schedules."""
import os
import sys

from oracle import coracle
from oracle.pyref import h2c

from tests.conftest import load_golden


def rows():
    return load_golden("h2c_deep_altbn128.json")["rows"]


def test_fixture_covers_every_depth_twice():
    fx = load_golden("h2c_deep_altbn128.json")
    assert fx["top"] >= 16
    by = {}
    for r in fx["rows"]:
        assert len(bytes.fromhex(r["msg"])) == 64 and r["tries"] == r["counter"] + 1
        by.setdefault(r["counter"], set()).add(r["msg"])
    assert sorted(by) == list(range(fx["top"] + 1)) and all(len(v) >= 2 for v in by.values())


def test_fixture_rows_equal_the_python_oracle():
    for r in rows():
        x, y, tries = h2c.altbn_hash_to_g1(bytes.fromhex(r["msg"]))
        assert tries == r["tries"], r["counter"]
        assert (x.to_bytes(32, "big") + y.to_bytes(32, "big")).hex() == r["point"], r["counter"]


def test_fixture_rows_equal_the_c_oracle():
    for r in rows():
        m = bytes.fromhex(r["msg"])
        assert coracle.hash_to_g1(0, m).hex() == r["point"], r["counter"]
        assert coracle.bn_h2c_tries(m) == r["tries"], r["counter"]


def test_fixture_messages_are_the_generator_s():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    try:
        import make_h2c_deep
    finally:
        sys.path.pop(0)
    for r in rows():
        assert make_h2c_deep.message(r["index"]).hex() == r["msg"]
