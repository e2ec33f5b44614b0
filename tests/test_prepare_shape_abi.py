"""CPU tier: bgls_set_prepare_shape (the test / A-B knob of the prepared key sets' shape, include/bgls_hip.h) is exported with the
header's signature and checks its arguments without a device.  What the shapes compute is tests/test_gpu_prepared_shapes.py."""
ERR_ARG = -1


def test_prepare_shape_symbol_and_argument_checks():
    from bgls_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "bgls_set_prepare_shape") and "bgls_set_prepare_shape" in _lib.SIGNATURES
    assert lib.bgls_abi_version() == 2
    try:
        for ng, chunk in ((0, 0), (6, 1), (96, 1 << 17)):
            assert lib.bgls_set_prepare_shape(ng, chunk) == 0, (ng, chunk)
        for ng in (1, 5, 97, 1 << 40):
            assert lib.bgls_set_prepare_shape(ng, 0) == ERR_ARG, ng
            assert "ng" in _lib.last_error()
            assert lib.bgls_set_prepare_shape(ng, 64) == ERR_ARG, ng
    finally:
        assert lib.bgls_set_prepare_shape(0, 0) == 0
