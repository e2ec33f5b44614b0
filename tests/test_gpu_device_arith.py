"""GPU tier for the field arithmetic at EDGE operands in MIXED waves, through the test-only device harness (tests/harness/device_harness.hip:
the arithmetic headers and k_hash.hip's kernels compiled for gfx950 behind batched exports).  The host tier (test_host_arith.py,
test_rx_arith.py) runs the same headers as waves of one; what only the device build has is checked here:

  * the wave-uniform exits of fp_inv_ds (__ballot(gnz != 0)) and fp_jacobi_phase (the `again` / `shrink` ballots): one slow lane
    among fast ones, alternating lanes, a = 0 lanes next to working lanes, a partial last wave -- every element must equal the
    Python value and the same element run alone;
  * the inline-asm multiply rows of rx.hpp on raw limbs: limb for limb equal to the host harness;
  * rx_sqrt_pow's lane-strided LDS table at three blocks per CU;
  * k_bls_sw_jacobi's item on the degenerate digests (t = 0, t = +-sqrt(-5)) and the three BLS12-381 combine kernels on the special
    kinds no message reaches, against the host harness and the C oracle;
  * a Miller product of the signature pair alone (n = 0) under every Miller shape.

References are plain Python integers: pow, pow(a, -1, p), Euler's criterion, Fp2 = Fp[u] / (u^2 + 1)."""
import ctypes
import os
import random

import pytest

import device_harness_lib
from oracle import coracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# base-field primes, group orders (curves/altbn128.go:480, curves/bls12_381.go:339) and the BLS12-381 G1 cofactor
P = {0: 21888242871839275222246405745257275088696311157297823662689037894645226208583,
     1: 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab}
ORDER = {0: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
         1: 52435875175126190479447740508185965837690552500527637822603658699938581184513}
H1 = 0x396c8c005555e1568c00aaab0000aaab
# BLS12-381 G1 generator (the ZCash / IETF pairing-friendly-curves one)
G1_BLS = bytes.fromhex("17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
                       "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1")
FB = {0: 32, 1: 48}
LIMBS = {0: 8, 1: 12}                        # 32-bit words


@pytest.fixture(scope="module")
def dh(gpu_lib):
    """libdevice_harness.so, rebuilt (hipcc under a timeout) when any source is newer than it.  Loaded after the library (gpu_lib imports
    torch first): the process keeps one HIP runtime."""
    return device_harness_lib.load()


def buf(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")


def jacobi(a, p):
    a %= p
    if a == 0:
        return 0
    return 1 if pow(a, (p - 1) // 2, p) == 1 else -1


def inv(a, p):
    return pow(a, -1, p) if a % p else 0


# ---------------------------------------------------------------------------------------------------------------- operands, wave layouts
def catalogue(cid, rnd):
    """0, 1, 2, 3..40, p - 1, p - 2, p - k, (p +- 1) / 2, 2^k and p - 2^k (k stepping by 7), all-ones words below the top word,
    quadratic non-residues, random values"""
    p, L = P[cid], LIMBS[cid]
    v = list(range(0, 41)) + [p - 1, p - 2] + [p - k for k in (3, 4, 5, 7, 9, 1000, 1 << 31)] + [(p - 1) // 2, (p + 1) // 2]
    for k in range(0, p.bit_length(), 7):
        v += [1 << k, p - (1 << k)]
    low = (1 << (32 * (L - 1))) - 1
    top = p >> (32 * (L - 1))
    v += [low, (1 << (32 * (L - 1))) | low, ((top - 1) << (32 * (L - 1))) | low, (1 << 32) - 1, (1 << 64) - 1]
    nr = [k for k in range(2, 200) if jacobi(k, p) < 0][:4]
    v += nr + [p - k for k in nr] + [k * k % p for k in nr]
    v += [rnd.randrange(p) for _ in range(8)]
    out = []
    for x in v:
        x %= p
        if x not in out:
            out.append(x)
    return out


def layouts(cid, edge, rnd):
    """(values, tags): element i runs on lane i mod 64 of wave i / 64.  (a) uniform waves of one edge value; (b) one edge value at lanes
    0, 31, 32 and 63 among 63 random values; (c) one slow lane (random, p - 1 or a non-residue) among 63 fast ones (0, 1 or 2^k);
    (d) alternating fast and slow lanes; (e) a partial last wave: 64 k + 37 elements in all (the caller also runs 64 k + 1)."""
    p = P[cid]
    vals, tags = [], []
    pool = [rnd.randrange(p) for _ in range(192)]            # random lanes are drawn from a pool: the references stay cheap

    def rand():
        return rnd.choice(pool)

    def wave(ws, tag):
        assert len(ws) == 64
        vals.extend(ws)
        tags.extend("%s lane %d" % (tag, l) for l in range(64))

    for e in edge:
        wave([e] * 64, "(a) uniform %#x" % e)
    for e in edge:
        w = [rand() for _ in range(64)]
        for l in (0, 31, 32, 63):
            w[l] = e
        wave(w, "(b) edge %#x among random" % e)
    nr = next(k for k in range(2, 200) if jacobi(k, p) < 0)
    fast_set = [0, 1, 1 << 100, 2]
    for fast in fast_set:
        for slow in (rand(), p - 1, p - nr, rand()):
            for at in (0, 17, 63):
                w = [fast] * 64
                w[at] = slow
                wave(w, "(c) slow %#x at %d among %#x" % (slow, at, fast))
    for fast in fast_set:
        w = [fast if l % 2 == 0 else rand() for l in range(64)]
        wave(w, "(d) alternating %#x / random" % fast)
        w = [rand() if l % 2 == 0 else fast for l in range(64)]
        wave(w, "(d) alternating random / %#x" % fast)
    tail = [0 if l % 5 == 0 else rand() for l in range(37)]
    vals.extend(tail)
    tags.extend("(e) partial wave lane %d" % l for l in range(37))
    return vals, tags


def to_be(xs, nb):
    return b"".join(x.to_bytes(nb, "big") for x in xs)


def from_be(b, nb, n):
    return [int.from_bytes(b[k * nb:(k + 1) * nb], "big") for k in range(n)]


# ---------------------------------------------------------------------------------------------------------------- Fp
FP_OPS = {0: "mul", 1: "sqr", 2: "add", 3: "sub", 4: "neg", 5: "inv", 6: "sqrt_candidate", 7: "jacobi(mont)", 8: "jacobi(plain)"}


_FP_MEMO = {}


def fp_ref(cid, op, a, b):
    """op 7 is the symbol of the Montgomery residue a R: R = 2^(32 L) is a square, so both Jacobi ops give (a / p)"""
    key = (cid, op, a, b if op in (0, 2, 3) else 0)
    if key not in _FP_MEMO:
        p = P[cid]
        f = [lambda: a * b % p, lambda: a * a % p, lambda: (a + b) % p, lambda: (a - b) % p, lambda: -a % p, lambda: inv(a, p),
             lambda: pow(a, (p + 1) // 4, p), lambda: jacobi(a, p), lambda: jacobi(a, p)][op]
        _FP_MEMO[key] = f()
    return _FP_MEMO[key]


def run_fp(dh, cid, op, av, bv):
    n, nb = len(av), FB[cid]
    o = (ctypes.c_uint8 * (n * (4 if op >= 7 else nb)))()
    assert dh.dh_fp_op(cid, op, n, buf(to_be(av, nb)), buf(to_be(bv, nb)), o) == 0
    if op >= 7:
        return list((ctypes.c_int32 * n).from_buffer(o))
    return from_be(bytes(o), nb, n)


@pytest.mark.parametrize("cid", [0, 1], ids=["altbn128", "bls12"])
def test_fp_ops_at_edge_operands_in_mixed_waves(dh, cid):
    """every Fp op of the device build at the catalogue's operands in the five wave layouts; inv(0) = 0, jacobi(0) = 0"""
    p = P[cid]
    rnd = random.Random(1000 + cid)
    edge = catalogue(cid, rnd)
    av, tags = layouts(cid, edge, rnd)
    bv = [av[(7 * i + 3) % len(av)] for i in range(len(av))]          # second operands: edge and random values, other lanes' mix
    for op in FP_OPS:
        for n in (len(av), len(av) - 36):                              # 64 k + 37 and 64 k + 1 elements
            got = run_fp(dh, cid, op, av[:n], bv[:n])
            for i in range(n):
                want = fp_ref(cid, op, av[i], bv[i])
                assert got[i] == want, "%s, %s: element %d (%s), a = %#x, b = %#x: got %#x" % (FP_OPS[op], ["bn", "bls"][cid], i, tags[i], av[i], bv[i], got[i])
    assert fp_ref(cid, 5, 0, 0) == 0 and fp_ref(cid, 7, 0, 0) == 0 and fp_ref(cid, 7, p - 1, 0) == -1


@pytest.mark.parametrize("cid", [0, 1], ids=["altbn128", "bls12"])
def test_fp_ops_do_not_depend_on_the_wave(dh, cid):
    """each catalogue value run alone (n = 1) gives what it gives in the mixed waves -- and the Python value"""
    rnd = random.Random(2000 + cid)
    edge = catalogue(cid, rnd)
    for op in (5, 6, 7, 8):
        waves = run_fp(dh, cid, op, edge, edge)
        for x, w in zip(edge, waves):
            alone = run_fp(dh, cid, op, [x], [x])[0]
            assert alone == w == fp_ref(cid, op, x, x), (FP_OPS[op], hex(x), alone, w)


def test_jacobi_slow_lane_among_zero_lanes(dh):
    """a = 0 lanes (sitting the loop out, f = p) next to ONE lane that needs all limbs for many rounds: the phase narrows only when the
    working lane fits; shifting the slow lane through every lane position of a wave"""
    for cid in (0, 1):
        p = P[cid]
        rnd = random.Random(3000 + cid)
        slows = [p - 1, rnd.randrange(p), (1 << (p.bit_length() - 1)) + 12345]
        av, want = [], []
        for s in slows:
            for at in range(64):
                w = [0] * 64
                w[at] = s
                av += w
        for op in (7, 8, 5):
            got = run_fp(dh, cid, op, av, av)
            for i, x in enumerate(av):
                assert got[i] == fp_ref(cid, op, x, x), (FP_OPS[op], cid, i, hex(x))


# ---------------------------------------------------------------------------------------------------------------- Fp2
def f2_mul(a, b, p):
    return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


def f2_inv(a, p):
    n = inv(a[0] * a[0] + a[1] * a[1], p)
    return (a[0] * n % p, -a[1] * n % p)


def f2_sqrt_ref(a, p):
    """wire.hpp f2_sqrt, step for step: (ok, root)"""
    sq = lambda x: pow(x, (p + 1) // 4, p)
    half = (p + 1) // 2
    a0, a1 = a
    if a1 == 0:
        return (True, (sq(a0), 0)) if jacobi(a0, p) >= 0 else (True, (0, sq(-a0 % p)))
    norm = (a0 * a0 + a1 * a1) % p
    lam = sq(norm)
    if lam * lam % p != norm:
        return False, None
    delta = (a0 + lam) * half % p
    if jacobi(delta, p) < 0:
        delta = (a0 - lam) * half % p
    r0 = sq(delta)
    if r0 == 0:
        return False, None
    r = (r0, inv(r0, p) * half * a1 % p)
    return f2_mul(r, r, p) == a, r


def f2_cqr_ref(a, p):
    """wire.hpp f2_complex_quad_res (calcComplexQuadRes), step for step: (ok, candidate root)"""
    sq = lambda x: pow(x, (p + 1) // 4, p)
    half = (p + 1) // 2
    a0, a1 = a
    if a1 == 0:
        return True, (sq(a0), 0)
    lam = sq((a0 * a0 + a1 * a1) % p)
    delta = (a0 + lam) * half % p
    if not (delta == 0 or jacobi(delta, p) > 0):
        delta = (a0 - lam) * half % p
    r0 = sq(delta)
    if r0 == 0:
        return False, None
    return True, (r0, inv(r0, p) * half * a1 % p)


def f2_cqr_finds_root(a, p):
    """a square of Fp2 that calcComplexQuadRes roots: not an a in Fp that is a non-residue there (its candidate is a^((p + 1) / 4), which
    g2_decompress then rejects, as the reference does)"""
    if a[1] == 0:
        return jacobi(a[0], p) >= 0
    return jacobi(a[0] * a[0] + a[1] * a[1], p) >= 0


def f2_operands(cid, rnd):
    p = P[cid]
    edge = [0, 1, 2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 64, p - (1 << 64)]
    nr = next(k for k in range(2, 200) if jacobi(k, p) < 0)
    v = []
    for e in edge + [nr, p - nr]:
        v += [(e, 0), (0, e), (e, e), (e, p - 1), (e, rnd.randrange(p))]
    for z in [(1, 1), (0, 1), (p - 1, 0), (nr, 0), (0, nr), (1, 2)] + [(rnd.randrange(p), rnd.randrange(p)) for _ in range(6)]:
        v.append(f2_mul(z, z, p))                                       # squares
    v += [(rnd.randrange(p), rnd.randrange(p)) for _ in range(6)]        # about half of them non-squares
    out = []
    for x in v:
        if x not in out:
            out.append(x)
    return out


def run_f2(dh, cid, op, av, bv):
    n, nb = len(av), FB[cid]
    o = (ctypes.c_uint8 * (n * (2 * nb + 1)))()
    enc = lambda xs: b"".join(x[0].to_bytes(nb, "big") + x[1].to_bytes(nb, "big") for x in xs)
    assert dh.dh_f2_op(cid, op, n, buf(enc(av)), buf(enc(bv)), o) == 0
    b = bytes(o)
    res = []
    for k in range(n):
        r = b[k * (2 * nb + 1):(k + 1) * (2 * nb + 1)]
        res.append((r[2 * nb] == 1, (int.from_bytes(r[:nb], "big"), int.from_bytes(r[nb:2 * nb], "big"))))
    return res


@pytest.mark.parametrize("cid", [0, 1], ids=["altbn128", "bls12"])
def test_fp2_ops_and_square_roots_at_edge_operands_in_mixed_waves(dh, cid):
    """f2_mul, f2_sqr, f2_inv and wire.hpp's two square roots (G2 decompression) at edge and (non-)square operands: uniform waves,
    the edge value at lanes 0 / 31 / 32 / 63 among random squares, one slow lane among (0, 0) / (1, 0) lanes, a partial last wave;
    each element equals its run alone"""
    p = P[cid]
    rnd = random.Random(4000 + cid)
    ops = f2_operands(cid, rnd)
    av, tags = [], []
    for e in ops:
        av += [e] * 64
        tags += ["(a) uniform"] * 64
    for e in ops[::3]:
        w = [f2_mul(z, z, p) for z in ((rnd.randrange(p), rnd.randrange(p)) for _ in range(64))]
        for l in (0, 31, 32, 63):
            w[l] = e
        av += w
        tags += ["(b) edge among random squares"] * 64
    for fast in ((0, 0), (1, 0)):
        for slow in ops[-12:]:
            w = [fast] * 64
            w[rnd.randrange(64)] = slow
            av += w
            tags += ["(c) slow lane among %s" % (fast,)] * 64
        av += [fast if l % 2 else ops[-1 - l % 12] for l in range(64)]
        tags += ["(d) alternating"] * 64
    av += ops[:37]
    tags += ["(e) partial wave"] * 37
    bv = [av[(5 * i + 1) % len(av)] for i in range(len(av))]
    for op, name in ((0, "f2_mul"), (1, "f2_sqr"), (2, "f2_inv"), (3, "f2_sqrt"), (4, "f2_complex_quad_res")):
        got = run_f2(dh, cid, op, av, bv)
        alone = {}
        for i, (a, b) in enumerate(zip(av, bv)):
            ok, r = got[i]
            if op < 3:
                want = [f2_mul(a, b, p), f2_mul(a, a, p), f2_inv(a, p)][op]
                assert ok and r == want, (name, i, tags[i], a, b, r)
                continue
            wok, wr = f2_sqrt_ref(a, p) if op == 3 else f2_cqr_ref(a, p)
            assert ok == wok, (name, "success bit", i, tags[i], a)
            if ok:
                assert r == wr, (name, "root", i, tags[i], a)
                if op == 3 or f2_cqr_finds_root(a, p):
                    assert f2_mul(r, r, p) == a, (name, "root does not square back", i, tags[i], a)
            if a in ops and a not in alone:
                alone[a] = run_f2(dh, cid, op, [a], [b])[0]
                assert alone[a][0] == ok and (not ok or alone[a][1] == r), (name, "differs alone", a)
        if op == 3:
            assert sum(1 for ok, _ in got if not ok) > 0 and sum(1 for ok, _ in got if ok) > 0


# ---------------------------------------------------------------------------------------------------------------- rx_sqrt_pow (LDS table)
@pytest.mark.parametrize("cid", [0, 1], ids=["altbn128", "bls12"])
def test_rx_sqrt_pow_lds_table_in_mixed_waves(dh, cid):
    """k_hash.hip rx_sqrt_pow<C, M1> (alt-bn128 on the nine 29-bit limbs, BLS12-381 with table entry 0 in registers), the table laid
    out lane-strided in LDS as k_bls_sw_jacobi has it: a^((p + 1) / 4) and the M1 power a^((p - 3) / 4) in every layout, and alone"""
    p = P[cid]
    nb = FB[cid]
    rnd = random.Random(5000 + cid)
    edge = catalogue(cid, rnd)
    av, tags = layouts(cid, edge, rnd)
    for m1, e in ((0, (p + 1) // 4), (1, (p - 3) // 4)):
        for n in (len(av), len(av) - 36):
            o = (ctypes.c_uint8 * (n * nb))()
            assert dh.dh_rx_sqrt(cid, m1, n, buf(to_be(av[:n], nb)), o) == 0
            got = from_be(bytes(o), nb, n)
            for i in range(n):
                assert got[i] == pow(av[i], e, p), ("M1" if m1 else "sqrt", i, tags[i], hex(av[i]))
        for x in edge[::4]:
            o = (ctypes.c_uint8 * nb)()
            assert dh.dh_rx_sqrt(cid, m1, 1, buf(to_be([x], nb)), o) == 0
            assert int.from_bytes(bytes(o), "big") == pow(x, e, p), ("alone", m1, hex(x))


# ---------------------------------------------------------------------------------------------------------------- rx.hpp raw limbs
RXG = {0: (28, 10, 0), 1: (28, 14, 1), 2: (29, 9, 0)}          # harness curve id -> (limb bits, limbs, field)


def rx_limbs(x, w, nl):
    out = [(x >> (w * k)) & ((1 << w) - 1) for k in range(nl - 1)]
    out.append(x >> (w * (nl - 1)))
    assert out[-1] < (1 << 32)
    return out


def rx_val(l, w):
    return sum(int(v) << (w * k) for k, v in enumerate(l))


def rx_cases(hid, op, rnd):
    """(arg, A, B): four Fp2 operands each, as raw limbs, in the input ranges test_rx_arith.py proves the column budget for (value
    bound vb p; "max": every limb at its bound), with edge values among them"""
    w, nl, f = RXG[hid]
    p = P[f]
    mask = (1 << w) - 1
    top_p = p >> (w * (nl - 1))
    args = {1: [sum(k << (2 * t) for t, k in enumerate(ks)) for ks in ((2, 2, 2, 0), (1, 2, 2, 1), (2, 0, 1, 2))], 3: [0, 1], 4: [0x42, 0x21]}.get(op, [0])
    out = []
    for arg in args:
        if hid == 2:
            vb = {0: 4, 2: 3, 3: 2, 4: 31 if arg == 0x42 else 8}[op]
        else:
            vb = {0: 31, 1: 31, 2: 2}[op]
        edges = [0, 1, p - 1, p, vb * p - 1, (1 << (w * (nl - 1))) - 1]
        mx = [mask] * (nl - 1) + [vb * (top_p + 1) - 1]
        kinds = ["rand"] * 6 + ["edge"] * 3 + (["max"] if op in (0, 1, 3) else [])

        def operand(kind):
            if kind == "max":
                return (mx, list(mx))
            if kind == "edge":
                return (rx_limbs(rnd.choice(edges), w, nl), rx_limbs(rnd.choice(edges), w, nl))
            return (rx_limbs(rnd.randrange(vb * p), w, nl), rx_limbs(rnd.randrange(vb * p), w, nl))

        for _ in range(3 * 64 + 37):                                        # three full waves and a partial one
            kd = rnd.choice(kinds)
            out.append((arg, [operand(kd) for _ in range(4)], [operand(kd) for _ in range(4)]))
    return out


def rx_flat(ops, nl):
    flat = []
    for re, im in ops:
        flat += list(re) + list(im)
    return flat + [0] * (8 * nl - len(flat))


@pytest.mark.parametrize("hid", [0, 1, 2], ids=["altbn128_28", "bls12_28", "altbn128_29"])
def test_rx_raw_limbs_equal_the_host_build_limb_for_limb(dh, host_harness, hid):
    """the consumer arithmetic of rx.hpp on the device (inline-asm multiply rows, rx_rows_gen.hpp) gives the host harness's limbs exactly
    -- the host build checks every column for overflow, the device build wraps silently -- and the value mod p"""
    w, nl, f = RXG[hid]
    p = P[f]
    Rinv = pow(1 << (w * nl), -1, p)
    rnd = random.Random(6000 + hid)
    xi = 9 if f == 0 else 1
    ops = [0, 2] + ([1] if hid != 2 else [3, 4])
    for op in ops:
        cases = rx_cases(hid, op, rnd)
        by_arg = {}
        for c in cases:
            by_arg.setdefault(c[0], []).append(c)
        for arg, cs in by_arg.items():
            n = len(cs)
            A = (ctypes.c_uint32 * (n * 8 * nl))(*sum((rx_flat(c[1], nl) for c in cs), []))
            Bv = (ctypes.c_uint32 * (n * 8 * nl))(*sum((rx_flat(c[2], nl) for c in cs), []))
            o = (ctypes.c_uint32 * (n * 2 * nl))()
            assert dh.dh_rx_raw(hid, op, arg, n, A, Bv, o) == 0
            for k, (_, a, b) in enumerate(cs):
                ho = (ctypes.c_uint32 * (2 * nl))()
                ovf = host_harness.ht_rx_raw(hid, op, arg, (ctypes.c_uint32 * (8 * nl))(*rx_flat(a, nl)), (ctypes.c_uint32 * (8 * nl))(*rx_flat(b, nl)), ho)
                # (op 2: the host build's check of the output's top limb is tighter than the documented bound, 3.001 p for the 29-bit form, which
                # a low-limbs-all-ones input reaches: the bound is asserted on the value below, as test_rx_arith.py does)
                assert ovf == 0 or op == 2, (hid, op, arg, k)
                dev = list(o[k * 2 * nl:(k + 1) * 2 * nl])
                assert dev == list(ho), "device limbs differ from the host build: curve %d op %d arg %#x element %d" % (hid, op, arg, k)
                r0, r1 = rx_val(dev[:nl], w), rx_val(dev[nl:], w)
                va = [(rx_val(x[0], w), rx_val(x[1], w)) for x in a]
                vb = [(rx_val(x[0], w), rx_val(x[1], w)) for x in b]
                if op == 2:
                    assert r0 % p == (xi * va[0][0] - va[0][1]) % p and r1 % p == (xi * va[0][1] + va[0][0]) % p
                    assert max(r0, r1) < (3.001 if hid == 2 else 32) * p
                    continue
                if op == 4:
                    assert r0 % p == va[0][0] % p and r1 % p == va[0][1] % p
                    continue
                if op == 0:
                    ks = [1, 1, 1, 0]
                elif op == 1:
                    ks = [(arg >> (2 * t)) & 3 for t in range(4)]
                else:
                    ks = [2, 2, 2, 0] if arg & 1 else [2, 1, 2, 1]
                re = sum(kk * (x[0] * y[0] - x[1] * y[1]) for kk, x, y in zip(ks, va, vb))
                im = sum(kk * (x[0] * y[1] + x[1] * y[0]) for kk, x, y in zip(ks, va, vb))
                assert r0 % p == re * Rinv % p and r1 % p == im * Rinv % p, (hid, op, arg, k)


@pytest.mark.parametrize("hid", [0, 1, 2], ids=["altbn128_28", "bls12_28", "altbn128_29"])
def test_rx_conversions_equal_the_host_build(dh, host_harness, hid):
    """to_ux(a R) and from_ux on the device (ops 16 / 17) against ht_rx_conv, limb for limb, and the Python value"""
    w, nl, f = RXG[hid]
    p, L, nb = P[f], LIMBS[f], FB[f]
    R = 1 << (w * nl)
    rnd = random.Random(6100 + hid)
    xs = catalogue(f, rnd)[:60] + [rnd.randrange(p) for _ in range(64 * 2 + 37 - 60)]
    n = len(xs)
    words = lambda x: [(x >> (32 * k)) & 0xffffffff for k in range(L)]
    A = (ctypes.c_uint32 * (n * 8 * nl))(*sum((words(x) + [0] * (8 * nl - L) for x in xs), []))
    o = (ctypes.c_uint32 * (n * 2 * nl))()
    assert dh.dh_rx_raw(hid, 16, 0, n, A, A, o) == 0
    lims = []
    for k, x in enumerate(xs):
        dev = list(o[k * 2 * nl:k * 2 * nl + nl])
        hl = (ctypes.c_uint32 * nl)()
        assert host_harness.ht_rx_conv(hid, 0, (ctypes.c_uint8 * nb).from_buffer_copy(x.to_bytes(nb, "big")), hl) == 0
        assert dev == list(hl), (hid, hex(x))
        assert rx_val(dev, w) % p == x * R % p
        lims.append(dev)
    # back, also from unreduced tight values below 4 p
    vals = [rx_val(l, w) for l in lims] + [p, 2 * p - 1, 3 * p + 12345, 4 * p - 1]
    lims += [rx_limbs(v, w, nl) for v in vals[n:]]
    m = len(lims)
    A = (ctypes.c_uint32 * (m * 8 * nl))(*sum((l + [0] * (7 * nl) for l in lims), []))
    o = (ctypes.c_uint32 * (m * 2 * nl))()
    assert dh.dh_rx_raw(hid, 17, 0, m, A, A, o) == 0
    for k, (l, v) in enumerate(zip(lims, vals)):
        got = sum(int(o[k * 2 * nl + j]) << (32 * j) for j in range(L))
        hb = (ctypes.c_uint8 * nb)()
        assert host_harness.ht_rx_conv(hid, 1, hb, (ctypes.c_uint32 * nl)(*l)) == 0
        assert got == int.from_bytes(bytes(hb), "big") == v * pow(R, -1, p) % p, (hid, k)


# ---------------------------------------------------------------------------------------------------------------- SW items and combine (BLS12-381)
def g1_neg(pt):
    return pt if pt == bytes(96) else coracle.scale_point(1, 1, pt, -1)


def sw_digests(rnd):
    """digests by kind: INF (t = 0), PLUS / MINUS (t = +-sqrt(-5), FT_ROOT1 / 2 -- whichever is which), SW (everything else)"""
    p = P[1]
    top = (1 << 512) - 1
    root = pow(-5 % p, (p + 1) // 4, p)
    assert root * root % p == p - 5
    inf = [0, p, p * (top // p), 5 * p]
    roots = {}
    for r in (root, p - root):
        roots[r] = [r, r + 7 * p, r + p * ((top - r) // p)]
    sw = [top, top - 1, (1 << 384) - 1, 1 << 384, (1 << 384) + 1, 1 << 511, 1, p - 1, p + 1] + [rnd.getrandbits(512) for _ in range(40)]
    return inf, roots, sw


def test_bls_sw_kinds_and_every_combine_form_on_special_digests(dh, host_harness):
    """k_bls_sw_jacobi's item on digests no message reaches, in waves that mix INF / PLUS / MINUS lanes with SW lanes: kinds and points
    equal to the host build (ht_bls_sw_x_digest).  Then the real combine kernels on those items, against the C oracle:
    k_bls_combine_raw_x and k_bls_combine_raw_batched<4> give sw_0 + sw_1 +- G1K with G1K = (h^-1 mod r) g1, k_bls_combine_x gives
    h (sw_0 + sw_1) +- g1.  Infinite sums sit at position 0, in the middle and last of a raw_batched thread's four, and one thread's
    four sums are all infinite."""
    host_harness.ht_bls_sw_x_digest.restype = ctypes.c_int
    host_harness.ht_bls_sw_x_digest.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    rnd = random.Random(7000)
    inf, roots, sw = sw_digests(rnd)

    def host_item(v):
        o = ctypes.create_string_buffer(96)
        k = host_harness.ht_bls_sw_x_digest(v.to_bytes(64, "big"), o)
        assert k in (0, 1, 2, 3), (hex(v), k)
        return k, (bytes(o.raw) if k == 3 else bytes(96))

    # which root is PLUS is the constants' business: learn it from the host build, then require both
    by_kind = {0: inf, 3: sw}
    for r, vs in roots.items():
        k = host_item(r)[0]
        assert k in (1, 2)
        by_kind[k] = vs
    assert set(by_kind) == {0, 1, 2, 3}
    pick = {k: (lambda vs: (lambda: rnd.choice(vs)))(vs) for k, vs in by_kind.items()}
    sw_iter = iter(sw * 4)
    pick[3] = lambda: next(sw_iter)
    I, PL, MI, S = 0, 1, 2, 3
    groups = [[(I, I), (S, S), (PL, S), (I, S)],                  # an infinite sum first
              [(S, S), (PL, MI), (S, S), (PL, PL)],               # ... in the middle
              [(PL, S), (S, S), (S, I), (MI, PL)],                # ... last
              [(I, I), (PL, MI), (I, I), (MI, PL)],               # all four infinite
              [(S, S), (MI, S), (PL, PL), (MI, MI)],
              [(S, PL), (I, I), (S, MI), (S, S)]]
    msgs = [m for g in groups for m in g] * 3 + [(S, S), (I, I), (PL, S)]       # 75 messages: 150 items, a partial last wave and thread
    digests = [(pick[a](), pick[b]()) for a, b in msgs]
    n = len(msgs)
    flat = b"".join(d0.to_bytes(64, "big") + d1.to_bytes(64, "big") for d0, d1 in digests)
    host = [[host_item(d) for d in pair] for pair in digests]
    g1k = coracle.scale_point(1, 1, G1_BLS, pow(H1, -1, ORDER[1]))
    assert coracle.g1_in_subgroup(1, G1_BLS) == 1 and coracle.scale_point(1, 1, g1k, H1) == G1_BLS

    def expect(pair, raw):
        swp = [pt for (k, pt) in pair if k == 3]
        g = g1k if raw else G1_BLS
        spec = [g if k == 1 else g1_neg(g) for (k, _) in pair if k in (1, 2)]
        s = coracle.aggregate_points(1, 1, b"".join(swp), len(swp)) if swp else bytes(96)
        if not raw and s != bytes(96):
            s = coracle.scale_point(1, 1, s, H1)
        pts = [s] + spec
        return coracle.aggregate_points(1, 1, b"".join(pts), len(pts))

    want_raw = [expect(pair, True) for pair in host]
    want_clr = [expect(pair, False) for pair in host]
    assert sum(w == bytes(96) for w in want_raw) >= 8
    for form, name in ((0, "k_bls_combine_raw_x"), (1, "k_bls_combine_raw_batched<4>"), (2, "k_bls_combine_x")):
        kinds = (ctypes.c_uint32 * (2 * n))()
        items = (ctypes.c_uint8 * (2 * n * 96))()
        pts = (ctypes.c_uint8 * (n * 96))()
        assert dh.dh_bls_sw(n, buf(flat), form, kinds, items, pts) == 0
        for i in range(n):
            for h in range(2):
                k, pt = host[i][h]
                assert kinds[2 * i + h] == k, (name, "kind", i, h, msgs[i])
                assert bytes(items[(2 * i + h) * 96:(2 * i + h + 1) * 96]) == pt, (name, "item point", i, h)
            want = (want_clr if form == 2 else want_raw)[i]
            assert bytes(pts[i * 96:(i + 1) * 96]) == want, "%s: message %d (%s, thread %d position %d)" % (name, i, msgs[i], i // 4, i % 4)


# ---------------------------------------------------------------------------------------------------------------- Miller product, n = 0
@pytest.mark.parametrize("cid", [0, 1], ids=["altbn128", "bls12"])
def test_miller_product_of_the_signature_pair_alone_under_every_shape(gpu_lib, cid):
    """bgls_miller_product_dev with n = 0 (an empty shard) and a signature: the partial is e(-sigma, g2)'s Miller value under the automatic
    shape and under k_miller_x60's forced shape (60- and 64-pairing forms) alike -- identical bytes, and the oracle's pairing after the
    final exponentiation"""
    import torch
    nb = FB[cid]
    rnd = random.Random(8000 + cid)
    g1, g2 = (ctypes.c_uint8 * (2 * nb))(), (ctypes.c_uint8 * (4 * nb))()
    assert gpu_lib.bgls_generator(cid, 1, g1) == 0 and gpu_lib.bgls_generator(cid, 2, g2) == 0
    k = rnd.randrange(1, ORDER[cid])
    sig = coracle.scale_point(cid, 1, bytes(g1), k)
    nsig = coracle.scale_point(cid, 1, bytes(g1), -k)
    want = coracle.pairing_product(cid, nsig, bytes(g2), 1)
    dev = torch.device("cuda:0")
    t_sig = torch.frombuffer(bytearray(sig), dtype=torch.uint8).to(dev)
    dummy = torch.zeros(4 * nb + 64, dtype=torch.uint8, device=dev)
    parts = []
    try:
        for shape, mode in ((0, 6), (4, 8), (4, 16 + 8)):
            assert gpu_lib.bgls_set_miller_shape(shape, mode) == 0
            part = torch.zeros(12 * nb, dtype=torch.uint8, device=dev)
            flags = torch.zeros(1, dtype=torch.int32, device=dev)
            rc = gpu_lib.bgls_miller_product_dev(cid, t_sig.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), 64, 64, 0, 1, part.data_ptr(),
                                                 flags.data_ptr(), None)
            assert rc == 0, "shape %d mode %d: rc %d" % (shape, mode, rc)
            torch.cuda.synchronize()
            assert int(flags.cpu()[0]) == 0
            parts.append(bytes(part.cpu().numpy()))
    finally:
        assert gpu_lib.bgls_set_miller_shape(0, 6) == 0
    assert parts[0] == parts[1] == parts[2]
    assert coracle.final_exp(cid, parts[0]) == want
