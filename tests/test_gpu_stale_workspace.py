"""GPU tier: every public entry point against stale and poisoned device workspaces ("Workspace contract").

The engine never frees or clears its device scratch between calls: a context hands back the same allocation of each of its workspace
slots as long as it is big enough, and key-set shards keep their exchange records.  Every word a kernel reads must therefore have been
written earlier in the same call.  Fresh device memory is zeroed and zero is the encoding of the point at infinity, so on a fresh
process a missing reset, or a kernel that reads padding beyond n, goes unnoticed; after a larger call that left valid points, counts or
raised flags behind it does not.

For every case of the catalogue (tests/stale_ws_cases.py: one entry point, a small instance, a big instance of the same entry on
unrelated valid inputs; a case is ONE call of ONE entry) the steps below run in this order and stop at the first failure.  Every run of the small instance must return,
byte for byte, what the C oracle (or a committed fixture) states for it -- return code, verdicts, GT elements, points, status words --
and its tampered variant, run behind a fill (or a big call) of its own, must be refused the same way:
  1. big, then small: the slots hold valid-looking data of a larger call;
  2. bgls_selftest_fill_workspaces(0x00), small;
  3. fill(0x01), small: non-zero counters, tickets and flags; limbs that look like field elements, are not at infinity, not on the curve;
  4. fill(0xFF), small: non-canonical limbs, every flag up, the infinity bit set, counters at their maximum;
  5. big again: it must equal its first result (the grow / reallocation path after small calls).
The fill covers the whole capacity of every cached slot, the pinned result words and, with a key-set handle, the shards' exchange records.

Sizes are the smallest on each side of each path switch of the host engine (listed above the registry in stale_ws_cases.py).  Out of
scope, because only large batches reach them: REDUCE_FX_MAX (12 288 partial products: 73 728 pairings), the 8192-leaf bound of the
one-launch key-sum tree and of Engine::sum_sets' P (a million keys), the 2^17-message lean hashing schedule, the 2^18-message batched
BLS12-381 normalisation, the 4096-key side-stream fork of a lone multi-signature, XB / AB (32 768 blocks per Miller launch), and the
fall-back of a skewed bucket population in the weighted sum (it needs weights no hashed exponent has; tests/test_gpu_msm.py).

The last test reads bgls_selftest_workspace_caps and fails, naming the slot, for every workspace slot that no case of the catalogue
allocated: a feature that adds a slot must add a case."""
import ctypes
import os
import re

import pytest

import stale_ws_cases as cat

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# slots no catalogue case can allocate, and why
EXEMPT = {
    "WS_GEN_TMP": "no call site: the generator lines are built into a device table of their own (Engine::gen_lines)",
}
_ran = set()


def slot_names():
    src = open(os.path.join(ROOT, "bgls_amd", "csrc", "engine_core.inc")).read()
    body = re.search(r"enum\s*\{\s*(WS_G1S\s*=\s*0.*?)\bWS_NUM\s*\}", src, flags=re.S).group(1)
    return re.findall(r"\bWS_[A-Z0-9_]+", body)


def fill(lib, byte, handle):
    filled = ctypes.c_uint64(0)
    assert lib.bgls_selftest_fill_workspaces(byte, handle, ctypes.byref(filled)) == 0
    assert filled.value > 0, "the fill touched nothing"
    return filled.value


def check_small(lib, case, byte, after):
    """the valid instance, then the tampered one, each directly behind a fill of its own (byte None: behind the big call)"""
    got = case.small()
    assert cat.matches(got, case.want), ("valid instance", after, got, case.want)
    if case.bad is not None:
        if byte is not None:
            fill(lib, byte, case.handle)
        got = case.bad()
        assert cat.matches(got, case.want_bad), ("tampered instance", after, got, case.want_bad)


def run_protocol(lib, case):
    big = case.big()
    check_small(lib, case, None, "a big call")
    if case.bad is not None:
        case.big()
        got = case.bad()
        assert cat.matches(got, case.want_bad), ("tampered instance", "directly after a big call", got, case.want_bad)
    for byte in (0x00, 0x01, 0xFF):
        fill(lib, byte, case.handle)
        check_small(lib, case, byte, "fill(0x%02x)" % byte)
    again = case.big()
    assert again == big, "the big instance changed between its two runs"


@pytest.fixture(scope="module", autouse=True)
def _release_key_sets(gpu_lib):
    yield
    cat.free_key_sets(gpu_lib)


@pytest.mark.parametrize("name", list(cat.CASES))
def test_small_call_after_big_call_and_poison(gpu_lib, name):
    lib = gpu_lib
    _ran.add(name)                                       # started: a case that fails has still allocated its slots
    built = cat.CASES[name](lib)
    for k, case in enumerate(built if isinstance(built, list) else [built]):
        if case.setup:
            assert case.setup() == 0
        try:
            run_protocol(lib, case)
        except AssertionError as e:
            raise AssertionError("entry %d of the case: %s" % (k, e)) from e
        finally:
            if case.teardown:
                case.teardown()


def test_fill_refuses_while_a_verification_is_in_flight(gpu_lib):
    """the pinned words and workspaces of a submitted verification are that verification's: the fill refuses until it is collected"""
    import torch
    lib, cid = gpu_lib, 0
    keys, msgs, sig = cat.agg_instance(lib, cid, 3, 103, msg_len=64)
    rc, flags, part = cat.run_miller_dev(lib, cid, sig, keys, msgs, 3)
    assert (rc, flags) == (0, 0)
    t_part = cat.dev_bytes(part)
    t_flags = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.bgls_final_verify_submit_dev(cid, t_part.data_ptr(), 1, t_flags.data_ptr(), None) == 0
    filled = ctypes.c_uint64(5)
    assert lib.bgls_selftest_fill_workspaces(0xFF, 0, ctypes.byref(filled)) == -1 and filled.value == 0
    assert lib.bgls_final_verify_collect(cid) == 1
    assert fill(lib, 0xFF, 0) > 0
    assert lib.bgls_selftest_fill_workspaces(0, 12345678, None) == -1          # an unknown key set


def test_the_fill_leaves_tables_keys_and_caller_buffers_alone(gpu_lib):
    """what the fill must not touch: the device tables (generator lines, fixed-base multiples), a key set's resident keys and prepared
    lines, a caller's device buffer -- a prepared key set verifies, the generator multiples come out, the buffer keeps its bytes"""
    import torch
    lib = gpu_lib
    mine = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda:0")
    for cid, curve_name in cat.CURVES:
        case = cat.CASES["key-set-%s-3shards-prepared" % curve_name](lib)[0]
        gen_case = cat.CASES["scale-generator-%s-g2" % curve_name](lib)
        assert cat.matches(case.small(), case.want)
        caps = (ctypes.c_size_t * 64)()
        slots = lib.bgls_selftest_workspace_caps(caps, 64)
        before = sum(caps[:slots])
        total = fill(lib, 0xFF, case.handle)
        # the calling thread's context alone holds `before` bytes of workspaces; three shards hold four exchange records each
        assert total >= before + 64 + 3 * 4 * (12 * cat.FP[cid] + 16)
        assert cat.matches(case.small(), case.want) and cat.matches(gen_case.small(), gen_case.want)
        assert lib.bgls_selftest_workspace_caps(caps, 64) == slots and sum(caps[:slots]) >= before      # nothing was freed
    torch.cuda.synchronize()
    assert bytes(mine.cpu().numpy()) == b"\x5a" * 4096


def test_zz_every_workspace_slot_was_allocated(gpu_lib):
    """Completeness (meaningful when this file runs alone): every slot below WS_NUM has a capacity on the calling thread's context after
    the catalogue ran, save the written exemptions."""
    lib = gpu_lib
    names = slot_names()
    caps = (ctypes.c_size_t * (len(names) + 8))()
    assert lib.bgls_selftest_workspace_caps(caps, len(caps)) == len(names), "the slot enumeration of engine_core.inc and the library disagree"
    if _ran != set(cat.CASES):
        pytest.skip("only part of the catalogue ran in this session (a selection with -k)")
    missing = [n for i, n in enumerate(names) if caps[i] == 0 and n not in EXEMPT]
    assert not missing, "workspace slots no catalogue case allocates: " + ", ".join(missing)
    stale = [n for i, n in enumerate(names) if caps[i] != 0 and n in EXEMPT]
    assert not stale, "exempted slots that are allocated after all (drop the exemption): " + ", ".join(stale)
    assert fill(lib, 0x00, 0) >= sum(caps[:len(names)])
