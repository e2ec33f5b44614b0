"""CPU tier: bgls_set_msm_plan (the test knob of the bucket method's window width and threads per bucket) and bgls_selftest_msm_last (the
report of what the last weighted sum did) are exported with the header's signatures; the knob checks its arguments and works without a
device, the report needs one.  What the plans compute is tests/test_gpu_msm_plans.py."""
import ctypes

ERR_ARG, ERR_NO_DEVICE = -1, -4


def test_msm_plan_symbols_and_argument_checks():
    import torch
    from bgls_amd import _lib
    lib = _lib.load()
    for name in ("bgls_set_msm_plan", "bgls_selftest_msm_last"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    try:
        for c in (0,) + tuple(range(4, 14)):
            for s in (0, 1, 2, 4, 8, 16):
                assert lib.bgls_set_msm_plan(c, s) == 0, (c, s)
        for c, s in ((3, 0), (14, 0), (-1, 1), (1, 1), (256 + 7, 4), (7, 3), (7, 5), (7, 32), (7, -1), (7, 256 + 4), (0, 6)):
            assert lib.bgls_set_msm_plan(c, s) == ERR_ARG, (c, s)
            assert _lib.last_error()
    finally:
        assert lib.bgls_set_msm_plan(0, 0) == 0
    assert lib.bgls_selftest_msm_last(None) == ERR_ARG                # argument check comes first, with or without a device
    if torch.cuda.is_available():
        return
    rep = (ctypes.c_uint32 * 6)(*[77] * 6)
    assert lib.bgls_selftest_msm_last(rep) == ERR_NO_DEVICE and "device" in _lib.last_error().lower()
    assert list(rep) == [77] * 6
