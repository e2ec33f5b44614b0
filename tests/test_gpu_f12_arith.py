"""GPU tier of the Fp12 layer: the cooperative Fp12 routines of finalx.hpp (carry-free 28-bit limbs) and finalexp.hpp (32-bit limbs) through
the device harness's dh_f12 / dh_finalx (tests/harness/device_harness_f12.hip), one element per block, each form in the block shape the
product launches it in (fx/256 as k_finalx, fx/128 as k_reduce_fx, fx/1w and fx/2w as k_miller_latx, fe/64 as k_final36 / k_gt_pow), and the
same catalogue (tests/f12_cases.py) through the public ABI: bgls_gt_mul, bgls_gt_pow, bgls_final_verify_dev.

The reference is oracle.pyref (Python integers); every comparison is byte-exact, and the five product forms must agree with each other.
The raw limbs of every carry-free result slot are checked against what the headers state:
  * rx.hpp, Sx: "|limb i| < LB * 2^24 for i < NL-1 (tight: limbs in [0, 2^28), LB = 16)" -- a product's output is tight, fx_conj's is the
    negative of one (|limb| < 2^28);
  * finalx.hpp, fx_mul: "a coefficient below 6.1 p, its xi multiple below 61 p (alt-bn128) / 12.2 p (BLS12-381)" -- as magnitudes;
  * the value of the limbs is the coefficient times R' = 2^(28 NL) mod p, and the xi slot holds xi times the plain slot.
"""
import ctypes
import functools
import random

import pytest

import device_harness_lib
import f12_cases as fc
from oracle.pyref.params import CURVES

pytestmark = pytest.mark.gpu

CIDS = [0, 1]
F_256, F_128, F_1W, F_2W, F_FE = range(5)
FX_FORMS = (F_256, F_128, F_1W, F_2W)
FORM_NAME = {F_256: "fx/256", F_128: "fx/128", F_1W: "fx/1w", F_2W: "fx/2w", F_FE: "fe/64"}
XI_BOUND = {0: 61.0, 1: 12.2}                 # finalx.hpp, fx_mul: the xi multiple of a coefficient, in units of p
COEF_BOUND = 6.1                              # the same sentence: a coefficient
ERR_ENCODING = -2


@pytest.fixture(scope="module")
def dh(gpu_lib):
    """loaded after the library (gpu_lib imports torch first): the process keeps one HIP runtime"""
    return device_harness_lib.load()


def _buf(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")


def gtb(cid, a):
    return fc.pairing(cid).gt_bytes(a)


def run(dh, cid, form, op, As, Bs=None, arg=0, e=1, steps=0):
    """one launch: [[(GT bytes, raw slot words or None)] per result] per element; As, Bs: GT bytes"""
    n, g = len(As), 12 * fc.FB[cid]
    Bs = As if Bs is None else Bs
    assert len(Bs) == n
    nres, sw = dh.dh_f12_results(form, op, steps), dh.dh_f12_slot_words(cid, form)
    out = (ctypes.c_uint8 * (n * nres * g))()
    raw = (ctypes.c_int32 * max(1, n * nres * sw))()
    rc = dh.dh_f12(cid, form, op, arg, n, _buf(b"".join(As)), _buf(b"".join(Bs)), (ctypes.c_uint32 * 4)(*fc.words(e)), e.bit_length(), steps, out, raw)
    assert rc == 0, (rc, FORM_NAME[form], op)
    ob, rw = bytes(out), list(raw)
    return [[(ob[(i * nres + k) * g:(i * nres + k + 1) * g], tuple(rw[(i * nres + k) * sw:(i * nres + k + 1) * sw]) if sw else None) for k in range(nres)]
            for i in range(n)]


def check_raw(dh, cid, raw, want, tag, tight=True):
    """the limb-range invariant and the values of one result slot (see the module docstring); want: the element (Python tuples).
    tight = False: the slot was written by fx_conj or fx_frob, which negate limb by limb (sx_neg keeps the bound, not the sign)"""
    p, N, hs = CURVES[cid].p, fc.NL[cid], dh.dh_f12_half_stride(cid)
    T = fc.pairing(cid).T
    R = pow(2, 28 * N, p)
    w = T.f12_to_w(want)
    for k in range(6):
        vals = {}
        for xi in (0, 1):
            for h in (0, 1):
                limbs = raw[(2 * k + xi) * 2 * hs + h * hs:][:N]
                if tight:
                    assert all(0 <= x < 1 << 28 for x in limbs[:-1]), (tag, k, xi, h, "tight limbs")
                else:
                    assert all(abs(x) < 1 << 28 for x in limbs[:-1]), (tag, k, xi, h, "limb bound")
                v = sum(x << (28 * i) for i, x in enumerate(limbs))
                assert abs(v) < (XI_BOUND[cid] if xi else COEF_BOUND) * p, (tag, k, xi, h, v / p)
                vals[xi, h] = v
        assert (vals[0, 0] % p, vals[0, 1] % p) == (w[k][0] * R % p, w[k][1] * R % p), (tag, k, "value")
        assert (vals[1, 0] % p, vals[1, 1] % p) == T.f2_mulxi((vals[0, 0] % p, vals[0, 1] % p)), (tag, k, "xi multiple")


@functools.lru_cache(maxsize=None)
def want_final(cid, gt):
    PR = fc.pairing(cid)
    return PR.gt_bytes(PR.final_exp(PR.gt_from_bytes(gt)))


@functools.lru_cache(maxsize=None)
def want_mul(cid, a, b):
    PR = fc.pairing(cid)
    return PR.gt_bytes(PR.T.f12_mul(PR.gt_from_bytes(a), PR.gt_from_bytes(b)))


@functools.lru_cache(maxsize=None)
def want_pow(cid, a, e, gs=False):
    PR = fc.pairing(cid)
    x = PR.gt_from_bytes(a)
    if e == 0:
        return PR.gt_bytes(PR.T.F12_ONE)
    return PR.gt_bytes(fc.gs_pow(cid, x, e) if gs else PR.T.f12_pow(x, e))


@pytest.mark.parametrize("cid", CIDS)
def test_products_in_every_form(dh, cid):
    """fx_mul (256 and 128 threads), fx_mul1, fx_mul2w, fe_mul with and without want_xi (then fe_fix_xi): the binary cases, one launch per
    form (more blocks than CUs), against the reference and against each other"""
    PR = fc.pairing(cid)
    cases = fc.binary_cases(cid)
    As, Bs = [gtb(cid, a) for _, a, _ in cases], [gtb(cid, b) for _, _, b in cases]
    want = [want_mul(cid, a, b) for a, b in zip(As, Bs)]
    seen = {}
    for form in FX_FORMS:
        got = run(dh, cid, form, 0, As, Bs)
        for (t, a, b), w, res in zip(cases, want, got):
            assert res[0][0] == w, (FORM_NAME[form], t)
            check_raw(dh, cid, res[0][1], PR.gt_from_bytes(w), (FORM_NAME[form], t))
            assert seen.setdefault(t, res[0][0]) == res[0][0], (FORM_NAME[form], t)
    for op in (0, 10):
        got = run(dh, cid, F_FE, op, As, Bs)
        for (t, a, b), w, res, ab in zip(cases, want, got, As):
            assert res[0][0] == w and seen[t] == w, ("fe/64", op, t)
            assert res[1][0] == want_mul(cid, ab, w), ("fe/64 xi multiples", op, t)


@pytest.mark.parametrize("cid", CIDS)
def test_mul_pair_aliasing(dh, cid):
    """fx_mul_pair: two different products side by side, d1 < 0, destinations that are operands (of the own and of the other product), one
    slot as both factors and destination"""
    PR = fc.pairing(cid)
    cases = fc.binary_cases(cid)[:len(fc.REDUCED) ** 2]
    As, Bs = [gtb(cid, a) for _, a, _ in cases], [gtb(cid, b) for _, _, b in cases]
    wants = {0: lambda a, b: (want_mul(cid, a, b), want_mul(cid, b, b)), 1: lambda a, b: (want_mul(cid, a, b), b),
             2: lambda a, b: (want_mul(cid, a, b), want_mul(cid, b, b)), 3: lambda a, b: (want_mul(cid, a, a), want_mul(cid, b, b)),
             4: lambda a, b: (want_mul(cid, a, b), want_mul(cid, b, a))}
    for arg, fn in wants.items():
        got = run(dh, cid, F_256, 1, As, Bs, arg=arg)
        for (t, _, _), a, b, res in zip(cases, As, Bs, got):
            w = fn(a, b)
            assert (res[0][0], res[1][0]) == w, (arg, t)
            for k in (0, 1):
                check_raw(dh, cid, res[k][1], PR.gt_from_bytes(w[k]), ("fx_mul_pair", arg, k, t))


@pytest.mark.parametrize("cid", CIDS)
def test_unary_routines(dh, cid):
    """conj, frob 1 .. 3, inverse and the final exponentiation over the whole catalogue on fx/256 and fe/64; fe_cyclo_sqr on the unitary
    elements.  The inverse and the final exponentiation of 0 are 0 (tests/test_f12_cases.py pins the reference's)."""
    PR = fc.pairing(cid)
    T = PR.T
    cat = fc.catalogue(cid)
    As = [gtb(cid, a) for _, a, _ in cat]
    ops = ((2, T.f12_conj), (3, lambda a: T.f12_frob(a, 1)), (4, lambda a: T.f12_frob(a, 2)), (5, lambda a: T.f12_frob(a, 3)), (6, T.f12_inv))
    for op, fn in ops:
        want = [fn(a) for _, a, _ in cat]
        gx, ge = run(dh, cid, F_256, op, As), run(dh, cid, F_FE, op, As)
        for (t, a, _), ab, w, rx, re in zip(cat, As, want, gx, ge):
            assert rx[0][0] == gtb(cid, w), ("fx/256", op, t)
            check_raw(dh, cid, rx[0][1], w, ("fx/256", op, t), tight=op == 6)
            assert re[0][0] == gtb(cid, w) and re[1][0] == want_mul(cid, ab, gtb(cid, w)), ("fe/64", op, t)
    uni = fc.by_class(cid, "unitary")
    Us = [gtb(cid, a) for _, a in uni]
    for (t, a), ab, res in zip(uni, Us, run(dh, cid, F_FE, 11, Us)):
        assert res[0][0] == want_mul(cid, ab, ab) and res[1][0] == want_mul(cid, ab, res[0][0]), ("fe_cyclo_sqr", t)
    gx, ge = run(dh, cid, F_256, 8, As), run(dh, cid, F_FE, 8, As)
    for (t, a, cls), ab, rx, re in zip(cat, As, gx, ge):
        w = want_final(cid, ab)
        assert rx[0][0] == w and re[0][0] == w, ("final_exp", t)
        check_raw(dh, cid, rx[0][1], PR.gt_from_bytes(w), ("fx_final_exp", t))
        if "zero" in cls:
            assert w == bytes(len(w))
        if "fp6" in cls and "zero" not in cls:
            assert w == gtb(cid, T.F12_ONE), t


@pytest.mark.parametrize("cid", CIDS)
def test_powers(dh, cid):
    """fx_pow and fe_pow: every exponent of the catalogue on unitary elements and on the all-(p - 1) element (dst != a in the harness, as
    the routines require).  fe_pow squares by Granger-Scott: on a base that is not unitary its value is that recurrence's
    (f12_cases.gs_pow, pinned to the host build of tower.hpp), not the power."""
    PR = fc.pairing(cid)
    bases = [(t, a, True) for t, a in fc.by_class(cid, "unitary") if t in ("unitary 0 (easy part of a random element)", "GT 0 (golden pairing)", "GT 1 inverse", "1")]
    assert len(bases) == 4
    bases.append(("all p - 1", fc.pick(cid, "all p - 1"), False))
    As = [gtb(cid, a) for _, a, _ in bases]
    for te, e in fc.pow_exponents(cid):
        gx, ge = run(dh, cid, F_256, 7, As, e=e), run(dh, cid, F_FE, 7, As, e=e)
        for (t, a, uni), ab, rx, re in zip(bases, As, gx, ge):
            w = want_pow(cid, ab, e)
            assert rx[0][0] == w, ("fx_pow", te, t)
            check_raw(dh, cid, rx[0][1], PR.gt_from_bytes(w), ("fx_pow", te, t))
            we = w if uni else want_pow(cid, ab, e, True)
            assert re[0][0] == we and re[1][0] == want_mul(cid, ab, we), ("fe_pow", te, t)


@pytest.mark.parametrize("cid", CIDS)
def test_chains_without_canonicalisation(dh, cid):
    """The magnitude bound of finalx.hpp: 64 squarings of the all-(p - 1) element in slot form (the output slot of one product is the input
    of the next, nothing canonicalised in between), every step against the reference and against the stated bounds; in every form (fx/2w:
    `epoch` runs to 64).  Then chains acc <- acc b over a few pairs."""
    PR = fc.pairing(cid)
    T = PR.T
    a = fc.pick(cid, "all p - 1")
    want, x = [], a
    for _ in range(64):
        x = T.f12_sqr(x)
        want.append(x)
    others = [fc.pick(cid, t) for t in ("alternating 0 / p - 1", "position 11 = p - 1", "random 0")]
    As = [gtb(cid, v) for v in [a] + others]
    for form in FX_FORMS + (F_FE,):
        got = run(dh, cid, form, 9, As, steps=64)
        for s in range(64):
            assert got[0][s][0] == gtb(cid, want[s]), (FORM_NAME[form], "step", s)
            if form != F_FE:
                check_raw(dh, cid, got[0][s][1], want[s], (FORM_NAME[form], "step", s))
        for i in range(1, len(As)):
            x = others[i - 1]
            for s in range(64):
                x = T.f12_sqr(x)
                assert got[i][s][0] == gtb(cid, x), (FORM_NAME[form], i, "step", s)
    pairs = [(fc.pick(cid, ta), fc.pick(cid, tb)) for ta, tb in (("all p - 1", "all p - 1"), ("random 0", "w^5"), ("all p - 1", "-1 = p - 1 in Fp"),
                                                               ("GT 0 (golden pairing)", "GT 0 inverse"), ("random 1", "0"))]
    for form in FX_FORMS + (F_FE,):
        got = run(dh, cid, form, 9, [gtb(cid, a) for a, _ in pairs], [gtb(cid, b) for _, b in pairs], arg=1, steps=7)
        for i, (a, b) in enumerate(pairs):
            x = a
            for s in range(7):
                x = T.f12_mul(x, b)
                assert got[i][s][0] == gtb(cid, x), (FORM_NAME[form], i, "step", s)
                if form != F_FE:
                    check_raw(dh, cid, got[i][s][1], x, (FORM_NAME[form], i, "step", s))


@pytest.mark.parametrize("cid", CIDS)
def test_launch_sizes_and_layouts(dh, cid):
    """n = 1, 2, 37 and 300 blocks (300: more blocks than CUs), the catalogue in three orders: every element's product with its successor
    equals the reference and, bytes and raw limbs, the same element run alone -- wherever it runs and whoever its neighbours are"""
    cat = fc.catalogue(cid)
    m = len(cat)
    base = [(gtb(cid, cat[i][1]), gtb(cid, cat[(i + 1) % m][1])) for i in range(m)]
    rnd = random.Random(5300 + cid)
    shuffled = base[:]
    rnd.shuffle(shuffled)
    layouts = [base, base[::-1], shuffled]
    for form in FX_FORMS + (F_FE,):
        ref = {}
        for lay in layouts:
            for n in (1, 2, 37, 300):
                items = [lay[i % m] for i in range(n)]
                got = run(dh, cid, form, 0, [a for a, _ in items], [b for _, b in items])
                for it, res in zip(items, got):
                    assert res[0][0] == want_mul(cid, *it), (FORM_NAME[form], n)
                    assert ref.setdefault(it, res) == res, (FORM_NAME[form], n)
        for it in base[::4] + [base[0], base[-1]]:
            assert run(dh, cid, form, 0, [it[0]], [it[1]])[0] == ref[it], FORM_NAME[form]
    # the whole final exponentiation at 300 blocks, the catalogue reversed
    items = [base[::-1][i % m][0] for i in range(300)]
    for form in (F_256, F_FE):
        for a, res in zip(items, run(dh, cid, form, 8, items)):
            assert res[0][0] == want_final(cid, a), FORM_NAME[form]


def finalx(dh, cid, batch, partials, do_final_exp=1, inst_flags=None):
    g, count = 12 * fc.FB[cid], len(partials)
    nres = count if batch else 1
    gt, ver, fl = (ctypes.c_uint8 * (nres * g))(), (ctypes.c_uint32 * nres)(), ctypes.c_uint32()
    fi = (ctypes.c_uint32 * count)(*(inst_flags or [0] * count))
    assert dh.dh_finalx(cid, batch, count, do_final_exp, _buf(b"".join(partials)), fi, gt, ver, ctypes.byref(fl)) == 0
    gb = bytes(gt)
    return [gb[i * g:(i + 1) * g] for i in range(nres)], list(ver), fl.value


@pytest.mark.parametrize("cid", CIDS)
def test_finalx_kernels_launched_directly(dh, cid):
    """kl::finalx (count = 1, 2, 7, with and without the final exponentiation) and kl::finalx_batch (1, 2, 300 instances, inst_flags clear
    and set): verdict word and GT bytes against the reference"""
    one = gtb(cid, fc.pairing(cid).T.F12_ONE)
    cat = [gtb(cid, a) for _, a, _ in fc.catalogue(cid)]
    pre = gtb(cid, fc.pick(cid, "Miller value of GT 0 (its pre-image)"))
    gti = gtb(cid, fc.pairing(cid).T.f12_conj(fc.pick(cid, "Miller value of GT 0 (its pre-image)")))      # a pre-image of GT 0's inverse
    f6 = gtb(cid, fc.pick(cid, "Fp6* element (final exponentiation 1, no pairing value)"))
    sets = {1: [[pre], [f6], [cat[0]], [one]], 2: [[pre, gti], [gti, pre], [f6, f6], [pre, cat[0]]],
            7: [[pre, f6, gti, one, f6, one, f6], cat[-7:], [pre, gti, pre, gti, cat[0], pre, gti]]}
    for count, groups in sets.items():
        for parts in groups:
            prod = parts[0]
            for x in parts[1:]:
                prod = want_mul(cid, prod, x)
            for fe in (0, 1):
                w = want_final(cid, prod) if fe else prod
                gt, ver, fl = finalx(dh, cid, 0, parts, fe)
                assert gt[0] == w and ver[0] == int(w == one) and fl == 0, (count, fe)
    assert finalx(dh, cid, 0, [pre, gti])[1] == [1] and finalx(dh, cid, 0, [f6])[1] == [1] and finalx(dh, cid, 0, [cat[0]])[1] == [0]
    for n in (1, 2, 300):
        items = [(cat + [f6, one])[(7 * i + 5) % (len(cat) + 2)] for i in range(n)]
        for flags in ([0] * n, [(i % 3 == 1) * (1 + i % 5) for i in range(n)]):
            gt, ver, fl = finalx(dh, cid, 1, items, inst_flags=flags)
            assert fl == 0
            for a, g, v, f in zip(items, gt, ver, flags):
                assert g == want_final(cid, a) and v == int(g == one and f == 0), n


# ---- the same catalogue through the public ABI (the shipped kernels)

def abi_gt_mul(lib, cid, a, b):
    o = (ctypes.c_uint8 * len(a))()
    return lib.bgls_gt_mul(cid, _buf(a), _buf(b), o), bytes(o)


def abi_gt_pow(lib, cid, a, k, neg):
    o = (ctypes.c_uint8 * len(a))()
    return lib.bgls_gt_pow(cid, _buf(a), _buf(k.to_bytes(32, "big")), neg, o), bytes(o)


@pytest.fixture(scope="module")
def abi(gpu_lib):
    import torch

    class A:
        lib = gpu_lib

        @staticmethod
        def final_verify(cid, parts):
            t = torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).to("cuda:0")
            flags = torch.zeros(1, dtype=torch.int32, device="cuda:0")
            return gpu_lib.bgls_final_verify_dev(cid, t.data_ptr(), len(parts), flags.data_ptr(), None)

    return A


@pytest.mark.parametrize("cid", CIDS)
def test_abi_gt_mul_over_the_binary_cases(abi, cid):
    for t, a, b in fc.binary_cases(cid):
        ab, bb = gtb(cid, a), gtb(cid, b)
        assert abi_gt_mul(abi.lib, cid, ab, bb) == (0, want_mul(cid, ab, bb)), t


@pytest.mark.parametrize("cid", CIDS)
def test_abi_gt_pow(abi, cid):
    """PointT.Mul: k = 0, 1, r - 1, r, r + 1, 2^255, 2^256 - 1, each with negative 0 and 1.  On GT elements negative = 1 is the inverse
    power.  On an element that is not unitary the documented result (include/bgls_hip.h) is the CONJUGATE of the power -- the reference
    only ever raises pairing values -- and that is what is pinned here."""
    PR = fc.pairing(cid)
    T = PR.T
    for t in ("GT 0 (golden pairing)", "GT 1 inverse", "1", "all p - 1"):
        a = fc.pick(cid, t)
        ab = gtb(cid, a)
        for te, k, neg in fc.gt_pow_exponents(cid):
            w = PR.gt_from_bytes(want_pow(cid, ab, k))
            if neg and t != "all p - 1":
                assert T.f12_is_one(T.f12_mul(T.f12_conj(w), w)) and T.f12_eq(T.f12_conj(w), T.f12_inv(w))
            assert abi_gt_pow(abi.lib, cid, ab, k, neg) == (0, gtb(cid, T.f12_conj(w) if neg else w)), (t, te)


@pytest.mark.parametrize("cid", CIDS)
def test_abi_final_verify_over_catalogue_partials(abi, cid):
    """bgls_final_verify_dev with 1, 2 and 9 partials out of the catalogue: the verdict is final_exp(product) == 1 of the reference"""
    one = gtb(cid, fc.pairing(cid).T.F12_ONE)
    g = lambda t: gtb(cid, fc.pick(cid, t))
    zero, pre, gt0 = g("0"), g("Miller value of GT 0 (its pre-image)"), g("GT 0 (golden pairing)")
    T = fc.pairing(cid).T
    gti = gtb(cid, T.f12_conj(fc.pick(cid, "Miller value of GT 0 (its pre-image)")))      # conj commutes with the power: a pre-image of GT 0's inverse
    assert want_final(cid, gti) == g("GT 0 inverse")
    f6, rn, w1 = g("Fp6* element (final exponentiation 1, no pairing value)"), g("random 0"), g("w^1")
    sets = [([f6], 1), ([zero], 0), ([one], 1), ([gt0], None), ([rn], 0), ([g("all p - 1")], None),
            ([pre, gti], 1), ([gti, pre], 1), ([zero, one], 0), ([pre, zero], 0), ([f6, g("Fp2 element")], 1), ([pre, gt0], 0), ([pre, g("GT 0 inverse")], 0), ([w1, g("w^5")], 1),
            ([pre, gti, f6, one, f6, f6, one, pre, gti], 1), ([pre, gti, f6, one, zero, f6, one, pre, gti], 0), ([pre, gti, f6, one, f6, f6, one, pre, zero], 0),
            ([pre, gti, f6, one, f6, rn, one, pre, gti], 0), ([w1] * 6 + [f6, pre, gti], 1)]
    assert {len(p) for p, _ in sets} == {1, 2, 9}
    for parts, expect in sets:
        prod = parts[0]
        for x in parts[1:]:
            prod = want_mul(cid, prod, x)
        want = int(want_final(cid, prod) == one)
        assert expect is None or expect == want
        assert abi.final_verify(cid, parts) == want, len(parts)


@pytest.mark.parametrize("cid", CIDS)
def test_abi_noncanonical_partials_are_encoding_errors(abi, cid):
    """a coefficient equal to p, or of all 0xff bytes, at each of the twelve positions of the first, the second and the last partial of a
    product (bgls_gt_mul: the 24 positions of its two operands; bgls_gt_pow: the twelve of its one): the encoding error of
    test_bad_encodings_are_errors_not_accepts, never a verdict"""
    g = lambda t: gtb(cid, fc.pick(cid, t))
    one = g("1")
    pre = fc.pick(cid, "Miller value of GT 0 (its pre-image)")
    good = [gtb(cid, pre), gtb(cid, fc.pairing(cid).T.f12_inv(pre)), one, one, one]           # verdict 1 as it stands
    assert abi.final_verify(cid, good) == 1 and abi.final_verify(cid, [one]) == 1
    for pos in range(12):
        for kind in (0, 1):
            for where in (0, 1, len(good) - 1):
                parts = list(good)
                parts[where] = fc.noncanonical(cid, parts[where], pos, kind)
                assert abi.final_verify(cid, parts) == ERR_ENCODING, (pos, kind, where)
            bad = fc.noncanonical(cid, one, pos, kind)
            # p at one position of "1" is 1 again modulo p: accepted it would verify
            assert abi.final_verify(cid, [bad]) == ERR_ENCODING, (pos, kind)
            assert abi_gt_mul(abi.lib, cid, bad, one)[0] == ERR_ENCODING and abi_gt_mul(abi.lib, cid, one, bad)[0] == ERR_ENCODING, (pos, kind)
            assert abi_gt_pow(abi.lib, cid, bad, 1, 0)[0] == ERR_ENCODING and abi_gt_pow(abi.lib, cid, bad, 3, 1)[0] == ERR_ENCODING, (pos, kind)
