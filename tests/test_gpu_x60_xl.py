"""GPU tier for the XL form of k_miller_x60<BN254W, 0, 60> (bgls_amd/csrc/miller_x.hpp: the xi of a fold's wrapped terms is applied to the
line by the producers; five line entries per hand-over; the hash points' coordinates parked in the workspace instead of LDS), forced for
every batch size with bgls_set_miller_shape(4, mode), 60-pairing block form:

  * PairingProduct (curves/curve.go:125-170) against the C oracle's GT bytes at n = 1 (one group partly filled), 59 / 60 / 61 (the block
    boundary), 121 (a ragged last block) and 129 (the first size the automatic shape sends to this kernel), one instance with a key at infinity;
  * the partial product of bgls_miller_product_dev: the latency kernel's bytes (automatic shape, n <= 128) and the same bytes in role modes 0, 1, 2;
  * an off-curve key is still an encoding error."""
import ctypes
import random

import pytest

from oracle import coracle

pytestmark = pytest.mark.gpu

CID, FP = 0, 32
SIZES = (1, 59, 60, 61, 121, 129)


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def out(n):
    return (ctypes.c_uint8 * max(1, n))()


@pytest.fixture()
def shape(gpu_lib):
    def set_shape(s, arg=8):
        assert gpu_lib.bgls_set_miller_shape(s, arg if s == 4 else 6) == 0
    yield set_shape
    assert gpu_lib.bgls_set_miller_shape(0, 6) == 0


@pytest.fixture(scope="module")
def pts(gpu_lib):
    """129 random pairs (G1, G2), made once"""
    g1, g2 = out(2 * FP), out(4 * FP)
    assert gpu_lib.bgls_generator(CID, 1, g1) == 0 and gpu_lib.bgls_generator(CID, 2, g2) == 0
    rnd = random.Random(0x60D1)
    n = max(SIZES)
    k1 = b"".join(rnd.randrange(1, 1 << 250).to_bytes(32, "big") for _ in range(n))
    k2 = b"".join(rnd.randrange(1, 1 << 250).to_bytes(32, "big") for _ in range(n))
    g1s, g2s = out(n * 2 * FP), out(n * 4 * FP)
    assert gpu_lib.bgls_scale_points(CID, 1, B(bytes(g1) * n), B(k1), None, n, g1s) == 0
    assert gpu_lib.bgls_scale_points(CID, 2, B(bytes(g2) * n), B(k2), None, n, g2s) == 0
    return bytes(g1s), bytes(g2s)


@pytest.mark.parametrize("n", SIZES)
def test_pairing_product_equals_oracle(gpu_lib, shape, pts, n):
    a, b = pts[0][:n * 2 * FP], pts[1][:n * 4 * FP]
    shape(4, 8)
    o = out(12 * FP)
    assert gpu_lib.bgls_pairing_product(CID, B(a), B(b), n, o) == 0
    assert bytes(o) == coracle.pairing_product(CID, a, b, n, threads=8), "n = %d" % n


def test_key_at_infinity_is_the_constant_line(gpu_lib, shape, pts):
    """a key at infinity (and, apart from it, a hash point at infinity) inside a group of real pairings: its line is the constant 1, whose xi
    copies are zero"""
    n = 61
    a, b = bytearray(pts[0][:n * 2 * FP]), bytearray(pts[1][:n * 4 * FP])
    b[7 * 4 * FP:8 * 4 * FP] = bytes(4 * FP)
    a[60 * 2 * FP:61 * 2 * FP] = bytes(2 * FP)
    shape(4, 8)
    o = out(12 * FP)
    assert gpu_lib.bgls_pairing_product(CID, B(a), B(b), n, o) == 0
    assert bytes(o) == coracle.pairing_product(CID, bytes(a), bytes(b), n, threads=8)


@pytest.mark.parametrize("n", SIZES)
def test_partial_product_equals_latency_kernel_and_is_the_same_in_every_role_mode(gpu_lib, shape, pts, n):
    import torch
    dev = torch.device("cuda:0")
    rnd = random.Random(9000 + n)
    keys = pts[1][:n * 4 * FP]
    msgs = b"".join(i.to_bytes(4, "big") + rnd.randbytes(60) for i in range(n))
    t_keys = torch.frombuffer(bytearray(keys), dtype=torch.uint8).to(dev)
    t_msgs = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to(dev)
    gtb = 12 * FP

    def partial():
        part = torch.zeros(gtb, dtype=torch.uint8, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        assert gpu_lib.bgls_miller_product_dev(CID, None, t_keys.data_ptr(), t_msgs.data_ptr(), 64, 64, n, 1, part.data_ptr(), flags.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert int(flags.cpu()[0]) == 0
        return bytes(part.cpu().numpy())

    got = {}
    for mode in (0, 1, 2):
        shape(4, mode)
        got[mode] = partial()
    assert got[0] == got[1] == got[2], "role modes differ at n = %d" % n
    if n <= 128:
        shape(0)                                  # automatic: k_miller_latx up to 128 pairings
        assert partial() == got[0], "throughput kernel differs from the latency kernel at n = %d" % n


def test_off_curve_key_is_an_encoding_error(gpu_lib, shape, pts):
    n = 61
    b = bytearray(pts[1][:n * 4 * FP])
    b[37 * 4 * FP + 4 * FP - 1] ^= 1
    shape(4, 8)
    o = out(12 * FP)
    assert gpu_lib.bgls_pairing_product(CID, B(pts[0][:n * 2 * FP]), B(b), n, o) < 0
