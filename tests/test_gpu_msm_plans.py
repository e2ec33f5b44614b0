"""GPU tier: the bucket-method weighted sum (k_msm.inc behind bgls_weighted_sum_dev) at every window width and split, byte for byte.

The plan of a sum is msm_plan(n): c = clamp(floor(log2 n) - 3, 4, 13) window bits, W = ceil(128 / c) windows, S threads per bucket doubling
while 16 S <= n >> c.  By size alone c = 7 .. 12 need 2^10 .. 2^15 points and S > 1 needs 2^17; bgls_set_msm_plan(c, S) forces either on a
small sum, and bgls_selftest_msm_last reports what the last sum did -- path (0 per-point below the threshold, 1 bucket method, 2 per-point
after the imbalance test), c, S, W and the histogram's largest bucket and total -- so no test here can pass by quietly taking the
per-point form.

  a. all 50 plans c = 4 .. 13 x S = 1, 2, 4, 8, 16 on one pool of 240 points with edge weights for every width (digits at the 64-bit seam of
     digit_of, the fullest top window, 2^c - 1 / 2^c), a repeated pair, an opposite pair, the point at infinity and a bucket of 40; the
     reference is the C oracle's scalar multiplications and sum, computed once per (curve, group).  At this size most partials of an
     S > 1 plan start at or past their bucket's end and must stay infinity;
  b. the natural plans at n = 2^k - 1 and 2^k, k = 7 .. 15 (c = 4 .. 12 by size), and at 2^17 (S = 2) and 2^19 (S = 8), against the closed
     form (sum w_i s_i mod r) g.  Below 2^16 the weights are balanced in every window (balanced_weights): uniform 128-bit weights fill
     the few buckets of a narrow top window past the cap at c = 6, 7, 9, 11, 12 and the library then takes the per-point form, which a
     test of its own pins (path 2, same bytes) at 512, 1024, 4096, 16384 and 32768 points;
  c. the imbalance test max(8 (n >> c), 64) at the bucket that just fits and at one point more;
  d. signed 64-bit multiplicities up to -2^63 through the bucket kernels (bgls_verify_multi_multiplicity);
  e. the argument checks of bgls_set_msm_plan.

Every test leaves msm_min = 32 and the plan (0, 0) in force, pass or fail.  Each test prints the report of every sum it ran (pytest -s)."""
import ctypes
import random

import pytest

from oracle import coracle

from test_gpu_msm import B, FP, ORDER, SIZE_MAX, gen_points, oracle_wsum, out

pytestmark = pytest.mark.gpu

ERR_ARG = -1
WIDTHS = tuple(range(4, 14))
SPLITS = (1, 2, 4, 8, 16)
CG = [(0, 1), (0, 2), (1, 1), (1, 2)]
CG_IDS = ["altbn128-g1", "altbn128-g2", "bls12-g1", "bls12-g2"]
NAMES = {0: "altbn128", 1: "bls12"}


def windows(c):
    return (128 + c - 1) // c


def natural_plan(n):
    """(c, S) of msm_plan(n), restated from its description"""
    c = min(max(n.bit_length() - 1 - 3, 4), 13)
    s = 1
    while s < 16 and 16 * s <= n >> c:
        s *= 2
    return c, s


def cap(n, c):
    """the largest bucket the bucket method accepts"""
    return max(8 * (n >> c), 64)


def top_bits(c):
    """the bits left for the top window"""
    return 128 - c * (windows(c) - 1)


def histogram(weights, c, skip=()):
    """(largest bucket, listed pairs) of the non-zero c-bit digits of the weights; the points at the indices in `skip` are infinity"""
    cnt = {}
    mask = (1 << c) - 1
    for i, w in enumerate(weights):
        if i in skip:
            continue
        for j in range(windows(c)):
            d = (w >> (j * c)) & mask
            if d:
                cnt[j, d] = cnt.get((j, d), 0) + 1
    return (max(cnt.values()) if cnt else 0), sum(cnt.values())


def balanced_weights(rnd, n, c):
    """n random 128-bit weights whose digits are balanced in EVERY window of width c.  A top window of fewer than c bits has so few
    buckets that uniform weights put n >> top_bits(c) points into each -- past the cap at c = 6, 7, 9, 11, 12 whatever the size (see
    test_uniform_weights_at_narrow_top_windows_take_the_per_point_form) -- so there only the first 8 << top_bits(c) weights get a top
    digit, eight per bucket on average, like the lower windows' 8 to 16."""
    low = c * (windows(c) - 1)
    m = n if top_bits(c) == c else min(n, 8 << top_bits(c))
    return [rnd.getrandbits(128 if i < m else low) for i in range(n)]


def last(lib):
    o = (ctypes.c_uint32 * 6)()
    assert lib.bgls_selftest_msm_last(o) == 0
    return tuple(o)


@pytest.fixture(autouse=True)
def default_plan(gpu_lib):
    try:
        yield
    finally:
        assert gpu_lib.bgls_set_msm_min(32) == 0
        assert gpu_lib.bgls_set_msm_plan(0, 0) == 0


def to_dev(pts, weights):
    import torch
    dev = torch.device("cuda:0")
    t_p = torch.frombuffer(bytearray(pts), dtype=torch.uint8).to(dev)
    t_w = torch.frombuffer(bytearray(b"".join(w.to_bytes(16, "big") for w in weights)), dtype=torch.uint8).to(dev)
    return t_p, t_w


def wsum_dev(lib, cid, group, t_p, t_w, n, msm_min, plan):
    """the sum of n resident points under msm_min and the forced plan (c, S); (bytes, bgls_selftest_msm_last's report)"""
    import torch
    size = (2 if group == 1 else 4) * FP[cid]
    t_o = torch.full((size,), 0xA5, dtype=torch.uint8, device=t_p.device)
    try:
        assert lib.bgls_set_msm_min(msm_min) == 0
        assert lib.bgls_set_msm_plan(*plan) == 0
        rc = lib.bgls_weighted_sum_dev(cid, group, t_p.data_ptr(), t_w.data_ptr(), n, t_o.data_ptr(), None)
    finally:
        lib.bgls_set_msm_min(32)
        lib.bgls_set_msm_plan(0, 0)
    assert rc == 0, rc
    return bytes(t_o.cpu().numpy()), last(lib)


def generator(lib, cid, group):
    g = out((2 if group == 1 else 4) * FP[cid])
    assert lib.bgls_generator(cid, group, g) == 0
    return bytes(g)


# ---- a. every (c, S) on one small pool ---------------------------------------------------------------------------------------------
POOL_N, BLOCK, WEIGHT_SEED = 240, 40, 0x9A7


def pool_weights(cid, group):
    """(scalars, weights, index of the infinity point) of the pool: points s_i g, the edge weights at fixed positions.  One weight
    vector serves every curve and group.  The block's common weight is random below 2^125 with bit 124 set: a top window of two or
    three bits (c = 6, 7, 9; c = 5) has three or seven buckets for a quarter or an eighth of all weights each, which leaves no room for
    40 more under the cap of 64, so the block stays out of those and is a bucket of 40 in every other window and every wider top one."""
    rnd = random.Random(WEIGHT_SEED)
    r = ORDER[cid]
    w = [0, 1, 1 << 63, (1 << 64) - 1, 1 << 64, 1 << 127, (1 << 128) - 1]
    for c in WIDTHS:
        top_bits = 128 - c * (windows(c) - 1)
        w += [(1 << c) - 1, 1 << c, ((1 << top_bits) - 1) << (c * (windows(c) - 1))]
        if 64 % c:                                                # one non-zero digit with bits on both sides of bit 64
            w.append(((1 << (c - 1)) | 1) << (c * (63 // c)))
    x = rnd.getrandbits(128)                                      # the same (point, weight) twice
    w += [x, x]
    x = rnd.getrandbits(128)                                      # a point and its negative with one weight
    w += [x, x]
    inf = len(w)                                                  # the all-zero encoding with a non-zero weight
    w.append(rnd.getrandbits(128) | 1)
    w += [rnd.getrandbits(124) | 1 << 124] * BLOCK                # one weight for a block of points
    w += [rnd.getrandbits(128) for _ in range(POOL_N - len(w))]
    rs = random.Random(0x9A70 + 10 * cid + group)
    sc = [rs.randrange(1, r) for _ in w]
    sc[inf - 3] = sc[inf - 4]
    sc[inf - 1] = r - sc[inf - 2]
    assert len(w) == len(sc) == POOL_N
    return sc, w, inf


_pools = {}


def pool(lib, cid, group):
    """the pool on the device and its sum by the oracle, built once per (curve, group) and never changed"""
    if (cid, group) not in _pools:
        size = (2 if group == 1 else 4) * FP[cid]
        sc, w, inf = pool_weights(cid, group)
        pts = bytearray(gen_points(lib, cid, group, sc))
        pts[inf * size:(inf + 1) * size] = bytes(size)
        pts = bytes(pts)
        _pools[cid, group] = (to_dev(pts, w), tuple(w), inf, oracle_wsum(cid, group, pts, w))
    return _pools[cid, group]


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("cid,group", CG, ids=CG_IDS)
def test_every_forced_plan_gives_the_oracle_bytes(gpu_lib, cid, group, c):
    lib = gpu_lib
    (t_p, t_w), w, inf, want = pool(lib, cid, group)
    largest, total = histogram(w, c, skip=(inf,))
    assert BLOCK <= largest <= cap(POOL_N, c), "the pool must take the bucket path at this width"
    for s in SPLITS:
        got, rep = wsum_dev(lib, cid, group, t_p, t_w, POOL_N, 0, (c, s))
        print("forced plan %s g%d c=%d S=%d -> path %d c %d S %d W %d largest %d total %d" % ((NAMES[cid], group, c, s) + rep))
        assert rep == (1, c, s, windows(c), largest, total), (c, s)
        assert got == want, (c, s)


# ---- b. the natural plans at their seams -------------------------------------------------------------------------------------------
def closed_form_case(lib, cid, group, n, seed, balanced_for=0):
    """points s_i g and random 128-bit weights (balanced_for = c: by balanced_weights) on the device, and (sum w_i s_i mod r) g by one
    oracle multiplication"""
    rnd = random.Random(seed)
    sc = [rnd.getrandbits(250) + 1 for _ in range(n)]             # below both group orders
    w = balanced_weights(rnd, n, balanced_for) if balanced_for else [rnd.getrandbits(128) for _ in range(n)]
    dev = to_dev(gen_points(lib, cid, group, sc), w)
    want = coracle.scale_point(cid, group, generator(lib, cid, group), sum(a * b for a, b in zip(w, sc)) % ORDER[cid])
    return dev, w, want


@pytest.mark.parametrize("k", range(7, 16))
@pytest.mark.parametrize("cid,group", CG, ids=CG_IDS)
def test_natural_plans_at_the_powers_of_two(gpu_lib, cid, group, k):
    lib = gpu_lib
    for n in ((1 << k) - 1, 1 << k):
        c, s = natural_plan(n)
        (t_p, t_w), w, want = closed_form_case(lib, cid, group, n, 0xB0B + 1000 * n + 10 * cid + group, balanced_for=c)
        assert (c, s) == ((k - 3 if n == 1 << k else max(k - 4, 4)), 1)
        got, rep = wsum_dev(lib, cid, group, t_p, t_w, n, 0, (0, 0))
        print("natural plan %s g%d n=%d -> path %d c %d S %d W %d largest %d total %d" % ((NAMES[cid], group, n) + rep))
        largest, total = histogram(w, c)
        assert largest <= cap(n, c)
        assert rep == (1, c, s, windows(c), largest, total), n
        assert got == want, n


@pytest.mark.parametrize("cid,group,lg,split", [(0, 2, 17, 2), (0, 2, 19, 8), (1, 1, 17, 2)],
                         ids=["altbn128-g2-128k", "altbn128-g2-512k", "bls12-g1-128k"])
def test_natural_split_plans(gpu_lib, cid, group, lg, split):
    """S = 2 (the partials' fold ends in the second buffer) and S = 8 (three folds) as the size alone chooses them"""
    lib, n = gpu_lib, 1 << lg
    (t_p, t_w), w, want = closed_form_case(lib, cid, group, n, 0x5EA + lg + 10 * cid + group)
    assert natural_plan(n) == (13, split)
    got, rep = wsum_dev(lib, cid, group, t_p, t_w, n, 0, (0, 0))
    print("natural plan %s g%d n=%d -> path %d c %d S %d W %d largest %d total %d" % ((NAMES[cid], group, n) + rep))
    assert rep[:4] == (1, 13, split, 10) and 0 < rep[4] <= cap(n, 13) and rep[5] <= 10 * n
    assert got == want


@pytest.mark.parametrize("cid,group", CG, ids=CG_IDS)
def test_uniform_weights_at_narrow_top_windows_take_the_per_point_form(gpu_lib, cid, group):
    """What the library does with hashed (uniform 128-bit) weights at the sizes that choose c = 6, 7, 9, 11, 12: the top window's 2, 2, 2,
    7 and 8 bits leave it buckets of n >> top_bits(c) points, above max(8 (n >> c), 64), and the sum takes the per-point form (path 2).
    Pinned, not assumed: measured on an MI355X the per-point form is the faster one there (alt-bn128 G2, n = 4096: 5.7 ms against 37 ms
    by buckets with the top window's lists of a thousand points on one thread each; n = 32768: 6.4 against 8.2 ms)."""
    lib = gpu_lib
    for n in (512, 1024, 4096, 16384, 32768):
        c, s = natural_plan(n)
        (t_p, t_w), w, want = closed_form_case(lib, cid, group, n, 0x70B + n + 10 * cid + group)
        largest, total = histogram(w, c)
        assert largest > cap(n, c) and largest < 2 * (n >> top_bits(c))
        got, rep = wsum_dev(lib, cid, group, t_p, t_w, n, 0, (0, 0))
        print("uniform weights %s g%d n=%d -> path %d c %d S %d W %d largest %d total %d" % ((NAMES[cid], group, n) + rep))
        assert rep == (2, c, s, windows(c), largest, total), n
        assert got == want, n


# ---- c. the imbalance test --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,group", CG, ids=CG_IDS)
def test_imbalance_threshold_is_exact(gpu_lib, cid, group):
    """n = 600 (c = 6, cap = max(8 * 9, 64) = 72): 72 points under one weight fill a bucket to the cap and the bucket method runs; the
    73rd sends the sum to the per-point form.  No other weight shares a digit with the common one, so the bucket is exactly that full."""
    lib, n = gpu_lib, 600
    c, s = natural_plan(n)
    full = cap(n, c)
    assert (c, s, full) == (6, 1, 72)
    rnd = random.Random(0xCA9 + 10 * cid + group)
    common = rnd.getrandbits(128) | 1
    mask = (1 << c) - 1
    lower = windows(c) - 1                                         # the others get no top digit: that window has three buckets for all of them
    draws = [rnd.getrandbits(c * lower) for _ in range(4 * n)]     # about seven in ten share no digit with the common weight
    rest = [x for x in draws if all((x >> (j * c)) & mask != (common >> (j * c)) & mask for j in range(lower))][:n - full]
    assert len(rest) == n - full
    sc = [rnd.getrandbits(250) + 1 for _ in range(n)]
    pts = gen_points(lib, cid, group, sc)
    g = generator(lib, cid, group)
    for extra, path in ((0, 1), (1, 2)):
        w = [common] * (full + extra) + rest[:n - full - extra]
        largest, total = histogram(w, c)
        assert largest == full + extra
        t_p, t_w = to_dev(pts, w)
        got, rep = wsum_dev(lib, cid, group, t_p, t_w, n, 0, (0, 0))
        print("imbalance %s g%d fullest=%d -> path %d c %d S %d W %d largest %d total %d" % ((NAMES[cid], group, largest) + rep))
        assert rep == (path, c, s, windows(c), largest, total)
        assert got == coracle.scale_point(cid, group, g, sum(a * b for a, b in zip(w, sc)) % ORDER[cid])


@pytest.mark.parametrize("c", (7, 12))
def test_forced_plan_cannot_pass_by_the_per_point_form(gpu_lib, c):
    """the pool of (a) with its bucket of 40 grown past the cap of 64: the report says path 2 where (a) demands path 1; same bytes"""
    lib, cid, group = gpu_lib, 0, 2
    size = 4 * FP[cid]
    sc, w, inf = pool_weights(cid, group)
    block = inf + 1
    assert w[block:block + BLOCK] == [w[block]] * BLOCK and w[block + BLOCK] != w[block]
    over = cap(POOL_N, c) + 1 - BLOCK
    w[block + BLOCK:block + BLOCK + over] = [w[block]] * over
    assert len(w) == POOL_N
    largest, total = histogram(w, c, skip=(inf,))
    assert largest > cap(POOL_N, c)
    pts = bytearray(gen_points(lib, cid, group, sc))
    pts[inf * size:(inf + 1) * size] = bytes(size)
    pts = bytes(pts)
    t_p, t_w = to_dev(pts, w)
    got, rep = wsum_dev(lib, cid, group, t_p, t_w, POOL_N, 0, (c, 4))
    assert rep == (2, c, 4, windows(c), largest, total)
    assert got == oracle_wsum(cid, group, pts, w)


# ---- d. signs in buckets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [0, 1], ids=["altbn128", "bls12"])
def test_signed_multiplicities_through_the_buckets(gpu_lib, cid):
    """sigma = (sum m_i sk_i mod r) H(0x01 || msg) for multiplicities at the ends of int64: accepted, refused after one multiplicity
    moves by one or one sign flips, the C oracle agrees, the bucket kernels ran, and the per-point form says the same"""
    lib, n = gpu_lib, 48
    rnd = random.Random(0xD1 + cid)
    r = ORDER[cid]
    mult = [(1 << 63) - 1, -((1 << 63) - 1), -(1 << 63), 1 << 62, -(1 << 62), 0, 1, -1]
    mult += [rnd.getrandbits(63) * (1 if i % 2 else -1) for i in range(n - len(mult))]
    sks = [rnd.randrange(1, r) for _ in range(n)]
    keys = gen_points(lib, cid, 2, sks)
    msg = b"multiplicities at the ends of int64"
    sig = coracle.scale_point(cid, 1, coracle.hash_to_g1(cid, b"\x01" + msg), sum(m * s for m, s in zip(mult, sks)) % r)
    moved = list(mult); moved[3] += 1
    flipped = list(mult); flipped[0] = -flipped[0]
    c, s = natural_plan(n)
    assert (c, s) == (4, 1)

    def verdict(m, msm_min):
        try:
            assert lib.bgls_set_msm_min(msm_min) == 0
            return lib.bgls_verify_multi_multiplicity(cid, B(sig), B(keys), (ctypes.c_int64 * n)(*m), n, B(b"\x01" + msg), 1 + len(msg))
        finally:
            lib.bgls_set_msm_min(32)

    for m, want in ((mult, 1), (moved, 0), (flipped, 0)):
        largest, total = histogram([abs(x) for x in m], c)
        assert largest <= cap(n, c)
        assert coracle.verify_multi_multiplicity(cid, sig, keys, n, m, msg) == want
        assert verdict(m, 32) == want
        rep = last(lib)
        print("multiplicities %s -> path %d c %d S %d W %d largest %d total %d" % ((NAMES[cid],) + rep))
        assert rep == (1, c, s, windows(c), largest, total)
        assert verdict(m, SIZE_MAX) == want
        assert last(lib) == (0, c, s, windows(c), 0, 0)


# ---- e. argument checks ------------------------------------------------------------------------------------------------------------
def test_plan_arguments(gpu_lib):
    lib, cid, group, n = gpu_lib, 0, 1, 40
    rnd = random.Random(0xE)
    t_p, t_w = to_dev(gen_points(lib, cid, group, [rnd.randrange(1, ORDER[cid]) for _ in range(n)]), [rnd.getrandbits(128) for _ in range(n)])

    import torch
    t_o = torch.zeros(2 * FP[cid], dtype=torch.uint8, device=t_p.device)

    def plan_in_force():
        assert lib.bgls_set_msm_min(0) == 0
        try:
            assert lib.bgls_weighted_sum_dev(cid, group, t_p.data_ptr(), t_w.data_ptr(), n, t_o.data_ptr(), None) == 0
        finally:
            lib.bgls_set_msm_min(32)
        return last(lib)[:4]

    from bgls_amd._lib import last_error
    assert lib.bgls_set_msm_plan(7, 4) == 0
    for bad in ((3, 4), (14, 4), (-1, 4), (1, 1), (1 << 8 | 7, 4), (7, 3), (7, 32), (7, -1), (7, 5), (0, 3), (3, 0), (14, 0), (7, 1 << 8 | 4)):
        assert lib.bgls_set_msm_plan(*bad) == ERR_ARG and last_error(), bad
    assert plan_in_force() == (1, 7, 4, 19)                       # the refused calls left (7, 4) in force
    assert lib.bgls_set_msm_plan(0, 8) == 0
    assert plan_in_force() == (1, 4, 8, 32)                       # the width by size, the split forced
    assert lib.bgls_set_msm_plan(9, 0) == 0
    assert plan_in_force() == (1, 9, 1, 15)
    assert lib.bgls_set_msm_plan(0, 0) == 0
    assert plan_in_force() == (1,) + natural_plan(n) + (32,)
    assert lib.bgls_selftest_msm_last(None) == ERR_ARG
