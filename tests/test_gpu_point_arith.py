"""GPU tier of the point layer: rx_jac1.hpp (G1) and rx_jac.hpp / rx_g2mul.hpp (the twists) through the device harness's dh_padd and
dh_pmul (tests/harness/device_harness_points.hip), the batched twins of the host harness's ht_rx_padd / ht_rx_pmul.  What only the device
build has is checked here: sx_montr on the inline-asm multiply rows, the chain's per-lane table indexed dynamically (scratch), its loops
with a per-lane trip count, and its per-lane branches into the doubling or infinity -- in waves whose lanes do DIFFERENT things.

  * the whole case list of the host tier (tests/point_cases.py; the two lists have the same length, asserted): every element equals the
    plain reference (tests/ec_ref.py) byte for byte, and its raw Jacobian limbs equal the host build's limb for limb;
  * mixed waves: uniform waves of one case, one exceptional lane (small-order point, k = j q, nbits = 1, P = infinity) at lanes 0 / 31 /
    32 / 63 among random subgroup lanes, alternating lanes, a wave whose lanes all have a different nbits (4 lane + 1 .. 256), a partial
    last wave (64 k + 37 and 64 k + 1 elements): every element equals the reference and the same element run alone (n = 1).

bgls_verify_multi_hae_sets draws its 128-bit exponents from a hash, so they cannot be steered through the ABI: the 128-bit width of the
chain is covered here (the 128-bit cases of the list) and in the host tier only.  Every comparison is exact."""
import ctypes
import random

import pytest

import device_harness_lib
import point_cases as pc
from ec_ref import FB, ORDER, Curve

pytestmark = pytest.mark.gpu

RAW = 88


@pytest.fixture(scope="module")
def dh(gpu_lib):
    """loaded after the library (gpu_lib imports torch first): the process keeps one HIP runtime"""
    return device_harness_lib.load()


@pytest.fixture(scope="module")
def hh(host_harness):
    vp, i = ctypes.c_void_p, ctypes.c_int
    host_harness.ht_rx_padd.argtypes = [i, i, vp, vp, vp, vp, i, vp, vp, vp]
    host_harness.ht_rx_pmul.argtypes = [i, i, vp, vp, i, vp, vp, vp]
    return host_harness


def _buf(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")


def dev_add(dh, cid, group, cases):
    """[(ok, wire bytes, raw limbs)] of one launch"""
    n, fb = len(cases), FB[cid]
    pb = 2 * group * fb
    lam = lambda z: (z or 0).to_bytes(fb, "big")
    out, raw, ok = (ctypes.c_uint8 * (n * pb))(), (ctypes.c_int32 * (n * RAW))(), (ctypes.c_uint8 * n)()
    rc = dh.dh_padd(cid, group, n, _buf(b"".join(c["a"] for c in cases)), _buf(b"".join(lam(c["za"]) for c in cases)),
                    _buf(bytes(int(c["za"] is not None) for c in cases)), _buf(b"".join(c["b"] for c in cases)),
                    _buf(b"".join(lam(c["zb"]) for c in cases)), _buf(bytes(int(c["zb"] is not None) for c in cases)),
                    _buf(bytes(c["form"] for c in cases)), out, raw, ok)
    assert rc == 0, rc
    ob, rw = bytes(out), list(raw)
    return [(ok[i], ob[i * pb:(i + 1) * pb], rw[i * RAW:(i + 1) * RAW]) for i in range(n)]


def dev_mul(dh, cid, group, cases):
    n, pb = len(cases), 2 * group * FB[cid]
    out, raw, ok = (ctypes.c_uint8 * (n * pb))(), (ctypes.c_int32 * (n * RAW))(), (ctypes.c_uint8 * n)()
    ks = (ctypes.c_uint32 * (8 * n))(*[w for c in cases for w in pc.k_words(c["k"])])
    nb = (ctypes.c_int * n)(*[c["nbits"] for c in cases])
    rc = dh.dh_pmul(cid, group, n, _buf(b"".join(c["pt"] for c in cases)), ks, nb, out, raw, ok)
    assert rc == 0, rc
    ob, rw = bytes(out), list(raw)
    return [(ok[i], ob[i * pb:(i + 1) * pb], rw[i * RAW:(i + 1) * RAW]) for i in range(n)]


def host_add(hh, cid, group, c):
    fb = FB[cid]
    out, raw, vm = (ctypes.c_uint8 * (2 * group * fb))(), (ctypes.c_int32 * RAW)(), ctypes.c_int64()
    za = None if c["za"] is None else _buf(c["za"].to_bytes(fb, "big"))
    zb = None if c["zb"] is None else _buf(c["zb"].to_bytes(fb, "big"))
    assert hh.ht_rx_padd(cid, group, _buf(c["a"]), za, _buf(c["b"]), zb, c["form"], out, raw, ctypes.byref(vm)) == 0, c["tag"]
    return bytes(out), list(raw)


def host_mul(hh, cid, group, c):
    out, raw, vm = (ctypes.c_uint8 * (2 * group * FB[cid]))(), (ctypes.c_int32 * RAW)(), ctypes.c_int64()
    assert hh.ht_rx_pmul(cid, group, _buf(c["pt"]), (ctypes.c_uint32 * 8)(*pc.k_words(c["k"])), c["nbits"], out, raw, ctypes.byref(vm)) == 0, c["tag"]
    return bytes(out), list(raw)


@pytest.mark.parametrize("cid,group", pc.GROUPS)
def test_additions_equal_the_reference_and_the_host_limbs(dh, hh, cid, group):
    cases_host = pc.add_cases(cid, group)
    cases_gpu = pc.add_cases(cid, group)                                   # the same list, in the list's own order: neighbours differ
    assert len(cases_gpu) == len(cases_host)
    got = dev_add(dh, cid, group, cases_gpu)
    for c, (ok, wire, raw) in zip(cases_host, got):
        h_wire, h_raw = host_add(hh, cid, group, c)
        assert ok == 1 and wire == pc.add_want(cid, group, c), c["tag"]
        assert wire == h_wire and raw == h_raw, c["tag"]


@pytest.mark.parametrize("cid,group", pc.GROUPS)
def test_chain_equals_the_reference_and_the_host_limbs(dh, hh, cid, group):
    cases_host = pc.mul_cases(cid, group)
    cases_gpu = pc.mul_cases(cid, group)
    assert len(cases_gpu) == len(cases_host)
    assert pc.events(cases_gpu) >= pc.required_events(cid, group)          # every branch of the chain is reached (recode() alone)
    got = dev_mul(dh, cid, group, cases_gpu)
    for c, (ok, wire, raw) in zip(cases_host, got):
        h_wire, h_raw = host_mul(hh, cid, group, c)
        assert ok == 1 and wire == pc.mul_want(cid, group, c), (c["tag"], hex(c["k"]), c["nbits"])
        assert wire == h_wire and raw == h_raw, (c["tag"], hex(c["k"]), c["nbits"])


def mul_layouts(cid, group):
    """(cases, exceptional cases): element i runs on lane i mod 64 of wave i / 64"""
    cv = Curve(cid, group)
    q = ORDER[cid]
    rnd = random.Random(4300 + 10 * cid + group)
    pool = []
    for _ in range(24):                                                    # random subgroup lanes come from a pool: the references stay cheap
        k = rnd.getrandbits(256)
        pool.append({"pt": cv.to_bytes(cv.mul(cv.gen, rnd.randrange(1, q))), "k": k, "nbits": k.bit_length(), "order": q, "tag": "random"})
    allc = pc.mul_cases(cid, group)

    def pick(word):
        return next(c for c in allc if word in c["tag"])

    small = [c for c in allc if c["order"] is not None and 1 < c["order"] < q]
    exc = [pick("g, 1 q"), pick("g, 1 (q - 2)"), pick("g, 2^1 - 1"), pick("infinity"), pick("g, 0xff.."), pick("g, 0x87..")]
    if small:
        exc += [small[0], small[len(small) // 2], small[-1], next(c for c in small if c["nbits"] <= 128)]
        exc += [c for c in small if "steered" in c["tag"]][:4]
    cases = []

    def wave(ws, tag):
        assert len(ws) == 64
        cases.extend(dict(c, tag="%s lane %d: %s" % (tag, l, c["tag"])) for l, c in enumerate(ws))

    for e in exc:
        wave([e] * 64, "(a) uniform")
    for e in exc:
        w = [rnd.choice(pool) for _ in range(64)]
        for l in (0, 31, 32, 63):
            w[l] = e
        wave(w, "(b) exceptional among random")
    for e in exc[:6]:
        wave([e if l % 2 == 0 else rnd.choice(pool) for l in range(64)], "(c) alternating")
    for e in (small[:2] if small else exc[:2]):
        wave([rnd.choice(pool) if l % 2 == 0 else e for l in range(64)], "(c) alternating")
    for base in (pool[0], exc[0]) + ((small[0],) if small else ()):
        k = base["k"] | (1 << 255)
        wave([dict(base, k=k, nbits=min(256, 4 * l + 1), tag=base["tag"] + ", nbits %d" % min(256, 4 * l + 1)) for l in range(64)], "(d) every lane its own nbits")
    tail = [exc[l % len(exc)] if l % 5 == 0 else rnd.choice(pool) for l in range(37)]
    cases.extend(dict(c, tag="(e) partial wave lane %d: %s" % (l, c["tag"])) for l, c in enumerate(tail))
    return cases, exc


@pytest.mark.parametrize("cid,group", pc.GROUPS)
def test_chain_in_mixed_waves(dh, cid, group):
    cases, exc = mul_layouts(cid, group)
    memo = {}

    def want(c):
        key = (c["pt"], c["k"], c["nbits"])
        if key not in memo:
            memo[key] = pc.mul_want(cid, group, c)
        return memo[key]

    runs = {}
    for n in (len(cases), len(cases) - 36):                                # 64 k + 37 and 64 k + 1 elements
        got = dev_mul(dh, cid, group, cases[:n])
        for c, (ok, wire, raw) in zip(cases, got):
            assert ok == 1 and wire == want(c), (c["tag"], hex(c["k"]), c["nbits"])
            key = (c["pt"], c["k"], c["nbits"])
            assert runs.setdefault(key, raw) == raw, c["tag"]              # the same element gives the same limbs wherever it runs
    alone = {}
    for c in exc + cases[-37:] + [c for c in cases if "(d)" in c["tag"]][::7]:
        key = (c["pt"], c["k"], c["nbits"])
        if key not in alone:
            alone[key] = dev_mul(dh, cid, group, [c])[0]
            assert alone[key] == (1, want(c), runs[key]), c["tag"]


@pytest.mark.parametrize("cid,group", pc.GROUPS)
def test_additions_in_mixed_waves(dh, cid, group):
    allc = pc.add_cases(cid, group)
    rnd = random.Random(4400 + 10 * cid + group)
    plain = [c for c in allc if c["tag"].endswith(("P + Q", "Q + P", "2P + Q", "Q + 2P"))]
    exc = [c for c in allc if c["tag"].endswith(("P + P'", "P' + P", "P + -P", "inf + P", "P + inf", "inf + inf", "P + P")) or c["form"] == 2][:40]
    exc += [c for c in allc if c["form"] >= 3 and c["tag"].endswith(("2 (P) + 2P", "2 (P) + -2P", "2 (-P) + -2P", "2 (P) + inf", "2 (inf) + 2P"))][:24]
    cases = []
    for e in exc:
        cases.extend([e] * 64)
        w = [rnd.choice(plain) for _ in range(64)]
        for l in (0, 31, 32, 63):
            w[l] = e
        cases.extend(w)
        cases.extend(e if l % 2 else rnd.choice(plain) for l in range(64))
    cases.extend(exc[l % len(exc)] if l % 5 == 0 else rnd.choice(plain) for l in range(37))
    key = lambda c: (c["a"], c["za"], c["b"], c["zb"], c["form"])
    runs = {}
    for n in (len(cases), len(cases) - 36):
        for c, (ok, wire, raw) in zip(cases, dev_add(dh, cid, group, cases[:n])):
            assert ok == 1 and wire == pc.add_want(cid, group, c), c["tag"]
            assert runs.setdefault(key(c), raw) == raw, c["tag"]
    for c in exc:
        assert dev_add(dh, cid, group, [c])[0] == (1, pc.add_want(cid, group, c), runs[key(c)]), c["tag"]
