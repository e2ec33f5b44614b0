"""GPU tier: key sets from compressed keys.  bgls_decompress_points_dev (the one-pass kernel on the carry-free limbs, k_wirex.hip) over the
oracle's edge fixture (tests/golden/wire_edge_*.json, written by make_wire_edge.py from oracle/pyref alone), the wire fixtures and mixed
waves, byte for byte against the fixture and against bgls_decompress_points; bgls_keys_upload_compressed on one, two and three shards
against a set made by bgls_keys_upload from the decompressed keys -- the same keys read back, the same verdicts and GT / apk bytes from
every call on the handle; every refusal with its first index; poisoned workspaces; the Python and C++ mirrors.
Sizes: 1, 63, 64, 65 and 130 keys -- a lone lane, either side of one wave, and three blocks with a ragged last one.  The upload runs
its kernel in one launch per shard (no chunking), so there is no chunk seam to place."""
import ctypes
import json
import os
import random
import subprocess

import pytest

from oracle.pyref import wire
from oracle.pyref.groups import Groups
from oracle.pyref.params import BN254, BLS381
from oracle.pyref.subgroup import Subgroup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CURVES = [(0, "altbn128"), (1, "bls12")]
IDS = [c[1] for c in CURVES]
SIZES = [1, 63, 64, 65, 130]
ERR_ARG, ERR_ENCODING = -1, -2
NMAX = 130


def u8(b):
    b = bytes(b)
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")


def fpb(cid):
    return 32 if cid == 0 else 48


def fixture_rows(name, group):
    """(encoding, ok, uncompressed bytes) of the edge fixture and of the wire fixture's decode cases"""
    cid = 0 if name == "altbn128" else 1
    ub = 2 * group * fpb(cid)
    rows = [(bytes.fromhex(c["in"]), c["ok"], bytes.fromhex(c["pt"]), c["kind"])
            for c in json.load(open(os.path.join(GOLDEN, "wire_edge_%s.json" % name)))["cases"] if c["group"] == group]
    for c in json.load(open(os.path.join(GOLDEN, "wire_%s.json" % name)))["g%d_decode" % group]:
        rows.append((bytes.fromhex(c["in"]), bool(c["ok"]), bytes.fromhex(c["pt"]) if c["ok"] else bytes(ub), "wire fixture"))
    return rows


def decode_dev(lib, cid, group, encs):
    import torch
    n, cb = len(encs), group * fpb(cid)
    t_in = torch.tensor(list(b"".join(encs)), dtype=torch.uint8, device="cuda:0")
    t_out = torch.full((n * 2 * cb,), 0xA5, dtype=torch.uint8, device="cuda:0")
    t_ok = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.bgls_decompress_points_dev(cid, group, t_in.data_ptr(), n, t_out.data_ptr(), t_ok.data_ptr(), None) == 0
    torch.cuda.synchronize()
    out = bytes(t_out.cpu().numpy().tobytes())
    return [out[i * 2 * cb:(i + 1) * 2 * cb] for i in range(n)], list(t_ok.cpu().numpy().tolist())


def decode_host(lib, cid, group, encs):
    n, cb = len(encs), group * fpb(cid)
    out, ok = (ctypes.c_uint8 * (n * 2 * cb))(), (ctypes.c_uint8 * n)()
    assert lib.bgls_decompress_points(cid, group, u8(b"".join(encs)), n, out, ok) == 0
    out = bytes(out)
    return [out[i * 2 * cb:(i + 1) * 2 * cb] for i in range(n)], list(ok)


def check_decode(lib, cid, group, rows):
    encs = [r[0] for r in rows]
    pts, oks = decode_dev(lib, cid, group, encs)
    for i, (r, pt, ok) in enumerate(zip(rows, pts, oks)):
        assert (ok, pt) == (1 if r[1] else 0, r[2]), (i, r[3], r[0].hex())
        if not r[1]:
            assert pt == bytes(len(pt))
    assert (pts, oks) == decode_host(lib, cid, group, encs)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("cid,name", CURVES, ids=IDS)
def test_dev_decode_of_the_fixtures(gpu_lib, cid, name, group):
    check_decode(gpu_lib, cid, group, fixture_rows(name, group))


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("cid,name", CURVES, ids=IDS)
def test_dev_decode_of_mixed_waves(gpu_lib, cid, name, group):
    """one wave per refused encoding of the fixture, the refusal at lanes 0, 31 and 63 among valid points, and a ragged tail"""
    rows = fixture_rows(name, group)
    good = [r for r in rows if r[1]]
    bad = [r for r in rows if not r[1]]
    assert len(good) >= 3 and len(bad) >= 5
    batch = []
    for k, b in enumerate(bad):
        wave = [good[(k + j) % len(good)] for j in range(64)]
        for lane in (0, 31, 63):
            wave[lane] = b
        batch += wave
    batch += [good[0], bad[0]]
    check_decode(gpu_lib, cid, group, batch)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cid,name", CURVES, ids=IDS)
def test_dev_decode_at_every_size(gpu_lib, cid, name, n):
    for group in (1, 2):
        rows = fixture_rows(name, group)
        check_decode(gpu_lib, cid, group, [rows[(7 * i + n) % len(rows)] for i in range(n)])


# ---- key sets -----------------------------------------------------------------------------------------------------------
class World:
    """NMAX keys of one curve with their compressed forms, and what the verification calls need"""

    def __init__(self, lib, cid):
        self.lib, self.cid, self.fp = lib, cid, fpb(cid)
        rnd = random.Random(0xC0 + cid)
        order = (BN254 if cid == 0 else BLS381).r
        self.sks = [rnd.randrange(1, order) for _ in range(NMAX)]
        kb = u8(b"".join(s.to_bytes(32, "big") for s in self.sks))
        keys = (ctypes.c_uint8 * (NMAX * 4 * self.fp))()
        assert lib.bgls_scale_generator(cid, 2, kb, NMAX, keys) == 0
        comp = (ctypes.c_uint8 * (NMAX * 2 * self.fp))()
        assert lib.bgls_compress_points(cid, 2, keys, NMAX, comp) == 0
        self.keys, self.comp = bytes(keys), bytes(comp)
        # the reference of every read-back below: the ORACLE's UnmarshalG2 of every compressed key, computed once -- its decompression, then
        # its membership test in the endomorphism form (oracle/pyref/subgroup.py proves it equal to [r]Q = infinity; the definition costs
        # 0.13 s a key in Python big integers)
        cv = BN254 if cid == 0 else BLS381
        G, S, dec = Groups(cv), Subgroup(cv), (wire.decompress_g2 if cid == 0 else wire.bls_decompress_g2)
        pts = [dec(self.comp[i * 2 * self.fp:(i + 1) * 2 * self.fp], subgroup=False) for i in range(NMAX)]
        assert all(ok and S.in_subgroup_fast(P) for P, ok in pts)
        self.oracle_keys = b"".join(G.g2_bytes(P) for P, _ in pts)
        assert self.oracle_keys == self.keys, "the keys made on the device are not what the oracle decompresses"
        self.msgs = [rnd.randbytes(11) for _ in range(NMAX // 3)]
        self.gt = lib.bgls_gt_size(cid)

    def key(self, i):
        return self.keys[i * 4 * self.fp:(i + 1) * 4 * self.fp]

    def enc(self, i):
        return self.comp[i * 2 * self.fp:(i + 1) * 2 * self.fp]

    def sign(self, n, msgs):
        blob = b"".join(msgs)
        off = (ctypes.c_uint64 * (n + 1))()
        for i, m in enumerate(msgs):
            off[i + 1] = off[i] + len(m)
        sigs = (ctypes.c_uint8 * (n * 2 * self.fp))()
        assert self.lib.bgls_sign_batch(self.cid, u8(b"".join(s.to_bytes(32, "big") for s in self.sks[:n])), u8(blob), off, n, sigs) == 0
        agg = (ctypes.c_uint8 * (2 * self.fp))()
        assert self.lib.bgls_aggregate_points(self.cid, 1, sigs, n, agg) == 0
        return agg, u8(blob), off


@pytest.fixture(scope="module")
def worlds(gpu_lib):
    return {cid: World(gpu_lib, cid) for cid, _ in CURVES}


def upload_c(lib, cid, comp, n, devs, flags=0):
    h, bad = ctypes.c_uint64(0), ctypes.c_size_t(0xBAD)
    d = (ctypes.c_int * len(devs))(*devs)
    rc = lib.bgls_keys_upload_compressed(cid, u8(comp), n, d, len(devs), flags, ctypes.byref(h), ctypes.byref(bad))
    return rc, h.value, bad.value


def upload_u(lib, cid, keys, n, devs, flags=1):
    h = ctypes.c_uint64(0)
    d = (ctypes.c_int * len(devs))(*devs)
    assert lib.bgls_keys_upload(cid, u8(keys), n, d, len(devs), flags, ctypes.byref(h)) == 0
    return h.value


def read_keys(lib, cid, h, first, count):
    out = (ctypes.c_uint8 * max(1, count * 4 * fpb(cid)))()
    assert lib.bgls_keys_read(h, first, count, out) == 0
    return bytes(out)[:count * 4 * fpb(cid)]


def everything(w, h, n, one_device):
    """what every later call on the handle returns: (rc, bytes) per call"""
    lib, res = w.lib, []
    # aggregate verification with the GT element: distinct messages, then a wrong one
    msgs = [b"m%03d" % i for i in range(n)]
    agg, blob, off = w.sign(n, msgs)
    for tamper in (False, True):
        if tamper:
            blob[1] ^= 1
        gt = (ctypes.c_uint8 * w.gt)()
        res.append((lib.bgls_verify_aggregate_h_gt(h, agg, blob, off, n, 0, gt), bytes(gt)))
    assert res[0][0] == 1 and res[1][0] == 0
    # one message, every key
    m = b"one message"
    magg, _, _ = w.sign(n, [m] * n)
    res.append((lib.bgls_verify_multi_h(h, magg, u8(m), len(m)), b""))
    res.append((lib.bgls_verify_multi_h(h, magg, u8(m + b"!"), len(m) + 1), b""))
    assert res[2][0] == 1 and res[3][0] == 0
    if one_device:
        stride = (n + 7) // 8
        rnd = random.Random(n)
        rows = [bytes([0xFF] * (n // 8) + ([(1 << (n % 8)) - 1] if n % 8 else [])), bytes([1] + [0] * (stride - 1))]
        rows.append(bytes(rows[0][i] & rnd.randrange(256) for i in range(stride)))
        out = (ctypes.c_uint8 * (len(rows) * 4 * w.fp))()
        res.append((lib.bgls_aggregate_subsets_h(h, u8(b"".join(rows)), stride, len(rows), out), bytes(out)))
        assert res[-1][0] == 0
        gm = [w.msgs[i % 3] for i in range(n)]                  # at most three groups
        gagg, gblob, goff = w.sign(n, gm)
        gt, ng = (ctypes.c_uint8 * w.gt)(), ctypes.c_size_t(0)
        res.append((lib.bgls_verify_aggregate_grouped_h(h, gagg, None, 0, gblob, goff, n, ctypes.byref(ng), gt), bytes(gt) + bytes([ng.value])))
        assert res[-1][0] == 1 and ng.value == min(n, 3)
    return res


@pytest.mark.parametrize("devs", [[0], [0, 0], [0, 0, 0]], ids=["1shard", "2shards", "3shards"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cid,name", CURVES, ids=IDS)
def test_upload_compressed_is_the_set_of_the_decompressed_keys(gpu_lib, worlds, cid, name, n, devs):
    lib, w = gpu_lib, worlds[cid]
    rc, h, bad = upload_c(lib, cid, w.comp[:n * 2 * w.fp], n, devs)
    assert rc == 0 and bad == 0xBAD, (rc, bad)
    ref = upload_u(lib, cid, w.keys[:n * 4 * w.fp], n, devs)
    try:
        info = (ctypes.c_int(), ctypes.c_size_t(), ctypes.c_int())
        assert lib.bgls_keys_info(h, *[ctypes.byref(x) for x in info]) == 0 and (info[0].value, info[1].value, info[2].value) == (cid, n, len(devs))
        got = read_keys(lib, cid, h, 0, n)
        assert got == w.oracle_keys[:n * 4 * w.fp] == read_keys(lib, cid, ref, 0, n)
        if n > 2:                                               # a range across the shard seams, and the argument rules
            assert read_keys(lib, cid, h, 1, n - 2) == w.keys[4 * w.fp:(n - 1) * 4 * w.fp]
        assert read_keys(lib, cid, h, n, 0) == b""
        one = (ctypes.c_uint8 * (4 * w.fp))()
        assert lib.bgls_keys_read(h, n, 1, one) == ERR_ARG and lib.bgls_keys_read(h, 0, n + 1, one) == ERR_ARG
        assert lib.bgls_keys_read(h, 0, 1, None) == ERR_ARG
        assert everything(w, h, n, len(devs) == 1) == everything(w, ref, n, len(devs) == 1)
    finally:
        assert lib.bgls_keys_free(h) == 0 and lib.bgls_keys_free(ref) == 0
    assert lib.bgls_keys_read(h, 0, 0, None) == ERR_ARG          # an unknown handle


@pytest.mark.parametrize("cid,name", CURVES, ids=IDS)
def test_prepared_set_from_compressed_keys(gpu_lib, worlds, cid, name):
    lib, w, n = gpu_lib, worlds[cid], 65
    for devs in ([0], [0, 0]):
        rc, h, _ = upload_c(lib, cid, w.comp[:n * 2 * w.fp], n, devs, flags=2)
        assert rc == 0
        ref = upload_u(lib, cid, w.keys[:n * 4 * w.fp], n, devs, flags=3)
        try:
            assert read_keys(lib, cid, h, 0, n) == w.keys[:n * 4 * w.fp]
            assert everything(w, h, n, len(devs) == 1) == everything(w, ref, n, len(devs) == 1)
        finally:
            assert lib.bgls_keys_free(h) == 0 and lib.bgls_keys_free(ref) == 0


@pytest.mark.parametrize("cid,name", CURVES, ids=IDS)
def test_a_set_with_a_key_at_infinity_and_an_empty_set(gpu_lib, worlds, cid, name):
    lib, w, n = gpu_lib, worlds[cid], 65
    inf_c = bytes(2 * w.fp) if cid == 0 else bytes([0xC0]) + bytes(2 * w.fp - 1)
    comp = w.comp[:7 * 2 * w.fp] + inf_c + w.comp[8 * 2 * w.fp:n * 2 * w.fp]
    keys = w.keys[:7 * 4 * w.fp] + bytes(4 * w.fp) + w.keys[8 * 4 * w.fp:n * 4 * w.fp]
    for devs in ([0], [0, 0, 0]):
        rc, h, _ = upload_c(lib, cid, comp, n, devs)
        assert rc == 0
        ref = upload_u(lib, cid, keys, n, devs)
        try:
            assert read_keys(lib, cid, h, 0, n) == keys
            m = b"without signer 7"
            sigs = (ctypes.c_uint8 * (n * 2 * w.fp))()
            blob, off = u8(m * n), (ctypes.c_uint64 * (n + 1))(*[len(m) * i for i in range(n + 1)])
            assert lib.bgls_sign_batch(cid, u8(b"".join(s.to_bytes(32, "big") for s in w.sks[:n])), blob, off, n, sigs) == 0
            rest = bytes(sigs)[:7 * 2 * w.fp] + bytes(sigs)[8 * 2 * w.fp:]
            agg = (ctypes.c_uint8 * (2 * w.fp))()
            assert lib.bgls_aggregate_points(cid, 1, u8(rest), n - 1, agg) == 0
            assert lib.bgls_verify_multi_h(h, agg, u8(m), len(m)) == lib.bgls_verify_multi_h(ref, agg, u8(m), len(m)) == 1
        finally:
            assert lib.bgls_keys_free(h) == 0 and lib.bgls_keys_free(ref) == 0
    rc, h, bad = upload_c(lib, cid, b"", 0, [0])
    assert rc == 0 and bad == 0xBAD
    info = ctypes.c_size_t(5)
    assert lib.bgls_keys_info(h, None, ctypes.byref(info), None) == 0 and info.value == 0
    assert lib.bgls_keys_free(h) == 0


@pytest.mark.parametrize("cid,name", CURVES, ids=IDS)
def test_every_refusal_fails_the_upload_and_names_the_first_key(gpu_lib, worlds, cid, name):
    lib, w, n = gpu_lib, worlds[cid], NMAX
    cb = 2 * w.fp
    bad_rows = [r for r in fixture_rows(name, 2) if not r[1]]
    kinds = {}
    for r in bad_rows:
        kinds.setdefault(r[3], r)
    assert len(kinds) >= 6

    def with_bad(at):
        comp = bytearray(w.comp[:n * cb])
        for i, r in at:
            comp[i * cb:(i + 1) * cb] = r[0]
        return bytes(comp)

    rc, last, _ = upload_c(lib, cid, w.comp[:cb], 1, [0])
    assert rc == 0 and lib.bgls_keys_free(last) == 0
    for k, (kind, r) in enumerate(sorted(kinds.items())):
        at = (17 * k + 5) % n
        rc, h, bad = upload_c(lib, cid, with_bad([(at, r)]), n, [0])
        assert (rc, bad) == (ERR_ENCODING, at), (kind, rc, bad)
        assert lib.bgls_keys_info(last + 1, None, None, None) == ERR_ARG, "a failed upload left a handle behind"
    any_bad = bad_rows[0]
    # two shards, a refused key in each: the smallest index; three shards, only the last one holds it
    rc, h, bad = upload_c(lib, cid, with_bad([(100, any_bad), (10, bad_rows[-1])]), n, [0, 0])
    assert (rc, bad) == (ERR_ENCODING, 10)
    rc, h, bad = upload_c(lib, cid, with_bad([(120, any_bad)]), n, [0, 0, 0])
    assert (rc, bad) == (ERR_ENCODING, 120)
    rc, h, bad = upload_c(lib, cid, with_bad([(129, any_bad), (128, any_bad)]), n, [0, 0, 0])
    assert (rc, bad) == (ERR_ENCODING, 128)
    # first_bad may be NULL
    hh = ctypes.c_uint64(0)
    assert lib.bgls_keys_upload_compressed(cid, u8(with_bad([(3, any_bad)])), n, None, 1, 0, ctypes.byref(hh), None) == ERR_ENCODING
    assert lib.bgls_keys_info(last + 1, None, None, None) == ERR_ARG
    # a valid upload afterwards succeeds and takes the next handle
    rc, h, bad = upload_c(lib, cid, w.comp[:n * cb], n, [0, 0])
    assert rc == 0 and h == last + 1 and bad == 0xBAD
    assert read_keys(lib, cid, h, 0, n) == w.keys[:n * 4 * w.fp]
    assert lib.bgls_keys_free(h) == 0


@pytest.mark.parametrize("cid,name", CURVES, ids=IDS)
def test_poisoned_workspaces(gpu_lib, worlds, cid, name):
    lib, w, n = gpu_lib, worlds[cid], 65
    rows = fixture_rows(name, 2)
    batch = [rows[i % len(rows)] for i in range(n)]
    big, hb, _ = upload_c(lib, cid, w.comp, NMAX, [0])          # a larger call first: the slots hold its data
    assert big == 0 and lib.bgls_keys_free(hb) == 0
    for byte in (None, 0x00, 0x01, 0xFF):
        if byte is not None:
            filled = ctypes.c_uint64(0)
            assert lib.bgls_selftest_fill_workspaces(byte, 0, ctypes.byref(filled)) == 0 and filled.value > 0
        check_decode(lib, cid, 2, batch)
        if byte is not None:
            assert lib.bgls_selftest_fill_workspaces(byte, 0, None) == 0
        rc, h, bad = upload_c(lib, cid, w.comp[:n * 2 * w.fp], n, [0, 0])
        assert rc == 0 and bad == 0xBAD
        assert read_keys(lib, cid, h, 0, n) == w.keys[:n * 4 * w.fp]
        assert everything(w, h, n, False)[0][0] == 1
        assert lib.bgls_keys_free(h) == 0
        if byte is not None:
            assert lib.bgls_selftest_fill_workspaces(byte, 0, None) == 0
        comp = bytearray(w.comp[:n * 2 * w.fp])
        comp[40 * 2 * w.fp:41 * 2 * w.fp] = next(r[0] for r in rows if not r[1])
        assert upload_c(lib, cid, bytes(comp), n, [0])[::2] == (ERR_ENCODING, 40)


def test_python_mirror(gpu_lib, worlds):
    from bgls_amd import Altbn128, Bls12, bgls
    for curve in (Altbn128, Bls12):
        w, n = worlds[curve.id], 9
        encs = [w.enc(i) for i in range(n)]
        for keys, devices in ((encs, None), (b"".join(encs), [0, 0])):
            ks = bgls.KeySet.from_compressed(curve, keys, devices=devices)
            assert len(ks) == n and [p.raw for p in ks.keys()] == [w.key(i) for i in range(n)]
            msgs = [b"msg %d" % i for i in range(n)]
            sig = bgls.AggregateSignatures([bgls.Sign(curve, sk, m) for sk, m in zip(w.sks[:n], msgs)])
            assert bgls.VerifyAggregateSignature(curve, sig, ks, msgs) is True
            assert bgls.VerifyAggregateSignature(curve, sig, ks, msgs[::-1]) is False
            ks.free()
        ks = bgls.KeySet.from_compressed(curve, encs[:3], prepare=True)
        assert [p.raw for p in ks.keys()] == [w.key(i) for i in range(3)]
        ks.free()
        broken = list(encs)
        broken[6] = broken[6][:-1] + bytes([broken[6][-1] ^ 1])
        with pytest.raises(ValueError, match="key 6 was refused"):
            bgls.KeySet.from_compressed(curve, broken)
        assert len(bgls.KeySet.from_compressed(curve, b"")) == 0


def test_cpp_mirror(gpu_lib, tmp_path):
    exe = str(tmp_path / "test_keys_compressed")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_keys_compressed.cpp"), "-L",
                    os.path.join(ROOT, "bgls_amd"), "-lbgls_hip", "-Wl,-rpath," + os.path.join(ROOT, "bgls_amd"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
