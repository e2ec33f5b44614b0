"""The catalogue of tests/test_gpu_stale_workspace.py: one entry point per case, with a small instance whose every returned byte the C
oracle (oracle/coracle.py) or a committed fixture states, one tampered variant where the entry returns a verdict, and a big instance of
the same entry on unrelated valid inputs.  The instance builders are the ones of the entries' own test files; nothing here asserts
anything about the library beyond "the builder's own calls succeeded" -- the protocol and the assertions are in the test module.

A builder is a function of (lib) registered in CASES under the name pytest shows; it returns one Case, or a list of them where several
entries share their instances (every Case is ONE entry and goes through the whole protocol on its own).  Building needs the GPU (the
instances are signed by the engine), so the registry holds builders and is complete at collection time."""
import ctypes
import json
import os
import random

from oracle import coracle

import test_gpu_ams_batch as am
import test_gpu_batch_aggregate as ba
import test_gpu_bbsigs as bb
import test_gpu_distinct as di
import test_gpu_msm as mm
import test_gpu_multi_hae_sets as mh
import test_gpu_multi_sets as ms
import test_gpu_multi_sets_combined as mc

HERE = os.path.dirname(os.path.abspath(__file__))
B, out, offs = ba.B, ba.out, ba.offs
ORDER, FP = mm.ORDER, mm.FP
SIZE_MAX = ctypes.c_size_t(-1).value
CURVES = ((0, "altbn128"), (1, "bls12"))
FLAG_DUP = 1

CASES = {}          # name -> builder(lib) -> Case or list of Cases
_memo = {}          # instances shared between cases (made once, never changed)


def case(name):
    def reg(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return reg


class Case:
    """ONE call of ONE entry: small() / bad() / big() run it and return a tuple of everything it handed back; want / want_bad are tuples of the same
    shape whose entries are values, or predicates of the returned value.  handle: a key set whose exchange records the fill covers;
    setup / teardown: the switch the case pins (Miller shape, bucket threshold, ...), around the whole protocol."""

    def __init__(self, small, want, big, bad=None, want_bad=None, handle=0, setup=None, teardown=None):
        self.small, self.want, self.big, self.bad, self.want_bad = small, want, big, bad, want_bad
        self.handle, self.setup, self.teardown = handle, setup, teardown


def matches(got, want):
    return len(got) == len(want) and all(w(g) if callable(w) else g == w for g, w in zip(got, want))


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


# ---------------------------------------------------------------------------------------------------------------- oracle side
def identity(cid):
    return bytes(12 * FP[cid] - 1) + b"\x01"


def gen(lib, cid, group):
    def make():
        o = out((2 if group == 1 else 4) * FP[cid])
        assert lib.bgls_generator(cid, group, o) == 0
        return bytes(o)
    return memo(("gen", cid, group), make)


def o_neg(cid, p):
    return p if not any(p) else coracle.scale_point(cid, 1, p, ORDER[cid] - 1)


def o_sum(cid, group, pts):
    """AggregatePoints of a list of wire points on the oracle; the point at infinity (all-zero bytes) is left out"""
    pts = [p for p in pts if any(p)]
    size = (2 if group == 1 else 4) * FP[cid]
    return coracle.aggregate_points(cid, group, b"".join(pts), len(pts)) if pts else bytes(size)


def o_gt(cid, g1s, g2s):
    """the pairing product of the listed pairs on the oracle; a pair with a point at infinity is the factor 1"""
    pairs = [(a, b) for a, b in zip(g1s, g2s) if any(a) and any(b)]
    if not pairs:
        return identity(cid)
    return coracle.pairing_product(cid, b"".join(a for a, _ in pairs), b"".join(b for _, b in pairs), len(pairs), threads=8)


def o_agg_gt(lib, cid, sig, keys, hash_inputs):
    """e(-sig, g2) * prod e(H(input_i), key_i): the GT element of an aggregate verification"""
    return o_gt(cid, [coracle.hash_to_g1(cid, m) for m in hash_inputs] + [o_neg(cid, sig)], list(keys) + [gen(lib, cid, 2)])


def o_verdict(cid, gt):
    return 1 if gt == identity(cid) else 0


def cut(raw, size):
    return [raw[i:i + size] for i in range(0, len(raw), size)]


def flip(m):
    return bytes([m[0] ^ 0x20]) + m[1:] if m else b"\x01"


def points(lib, cid, group, n, seed):
    """n multiples of the generator (the engine's fixed-base path), as wire bytes, with their scalars"""
    def make():
        rnd = random.Random(seed)
        ks = [rnd.randrange(1, ORDER[cid]) for _ in range(n)]
        return ks, mm.gen_points(lib, cid, group, ks)
    return memo(("points", cid, group, n, seed), make)


def dev_bytes(data):
    import torch
    return torch.frombuffer(bytearray(data or b"\0"), dtype=torch.uint8).to(torch.device("cuda:0"))


# ------------------------------------------------------------------------------------------- aggregate / multi / pairing product
def agg_instance(lib, cid, n, seed, msg_len=32):
    def make():
        keys, msgs, sigs, _ = ba.make_batch(lib, cid, FP[cid], [n], seed, msg_len=msg_len)
        return keys, msgs, sigs[0]
    return memo(("agg", cid, n, seed, msg_len), make)


def run_agg(lib, cid, sig, keys, msgs, allow_dups=0):
    return (ba.single(lib, cid, FP[cid], sig, keys, msgs, allow_dups),)


def shape_switch(lib, shape):
    if shape is None:
        return None, None
    return (lambda: lib.bgls_set_miller_shape(4, shape)), (lambda: lib.bgls_set_miller_shape(0, 0))


def make_agg_case(cid, n, shape, allow_dups):
    def build(lib):
        keys, msgs, sig = agg_instance(lib, cid, n, 100 + n)
        bkeys, bmsgs, bsig = agg_instance(lib, cid, 1000, 7)
        bad = list(msgs)
        bad[n // 2] = flip(bad[n // 2])
        want = (coracle.verify_aggregate(cid, sig, keys, msgs, bool(allow_dups), threads=8),)
        want_bad = (coracle.verify_aggregate(cid, sig, keys, bad, bool(allow_dups), threads=8),)
        assert want == (1,) and want_bad == (0,)
        setup, teardown = shape_switch(lib, shape)
        return Case(lambda: run_agg(lib, cid, sig, keys, msgs, allow_dups), want, lambda: run_agg(lib, cid, bsig, bkeys, bmsgs, allow_dups),
                    lambda: run_agg(lib, cid, sig, keys, bad, allow_dups), want_bad, setup=setup, teardown=teardown)
    return build


def make_duprule_case(cid):
    """a valid aggregate whose second message repeats the first: refused by the duplicate rule alone, accepted without it"""
    def build(lib):
        def make():
            keys, msgs, sigs, _ = ba.make_batch(lib, cid, FP[cid], [61], 55, dup_in=[0])
            return keys, msgs, sigs[0]
        keys, msgs, sig = memo(("aggdup", cid), make)
        bkeys, bmsgs, bsig = agg_instance(lib, cid, 1000, 7)
        want = (coracle.verify_aggregate(cid, sig, keys, msgs, False, threads=8), coracle.verify_aggregate(cid, sig, keys, msgs, True, threads=8))
        assert want == (0, 1)
        return [Case(lambda: run_agg(lib, cid, sig, keys, msgs, 0), want[:1], lambda: run_agg(lib, cid, bsig, bkeys, bmsgs, 0)),
                Case(lambda: run_agg(lib, cid, sig, keys, msgs, 1), want[1:], lambda: run_agg(lib, cid, bsig, bkeys, bmsgs, 1))]
    return build


def multi_instance(lib, cid, n, seed):
    def make():
        keys, msgs, sigs, _ = ms.make_sets(lib, cid, FP[cid], [n], seed)
        return keys, msgs[0], sigs[0]
    return memo(("multi", cid, n, seed), make)


def make_multi_case(cid, n):
    def build(lib):
        keys, msg, sig = multi_instance(lib, cid, n, 200 + n)
        bkeys, bmsg, bsig = multi_instance(lib, cid, 3000, 8)
        want = (coracle.verify_multi(cid, sig, keys, n, msg),)
        want_bad = (coracle.verify_multi(cid, sig, keys, n, msg + b"x"),)
        assert want == (1,) and want_bad == (0,)
        return Case(lambda: (ms.single(lib, cid, sig, keys, n, msg),), want, lambda: (ms.single(lib, cid, bsig, bkeys, 3000, bmsg),),
                    lambda: (ms.single(lib, cid, sig, keys, n, msg + b"x"),), want_bad)
    return build


def run_pairing_product(lib, cid, g1s, g2s, n):
    gt = out(12 * FP[cid])
    rc = lib.bgls_pairing_product(cid, B(g1s), B(g2s), n, gt)
    return rc, bytes(gt)


def make_pairing_case(cid, n, shape):
    def build(lib):
        _, g1s = points(lib, cid, 1, n, 300 + n)
        _, g2s = points(lib, cid, 2, n, 400 + n)
        _, b1 = points(lib, cid, 1, 700, 9)
        _, b2 = points(lib, cid, 2, 700, 10)
        want = (0, coracle.pairing_product(cid, g1s, g2s, n, threads=8))
        setup, teardown = shape_switch(lib, shape)
        return Case(lambda: run_pairing_product(lib, cid, g1s, g2s, n), want, lambda: run_pairing_product(lib, cid, b1, b2, 700),
                    setup=setup, teardown=teardown)
    return build


def run_miller_dev(lib, cid, sig, keys, msgs, n):
    """bgls_miller_product_dev into the caller's partial and flag word: return code, flag word, partial"""
    import torch
    fp = FP[cid]
    t_sig, t_keys, t_msgs = dev_bytes(sig), dev_bytes(keys), dev_bytes(b"".join(msgs))
    part = torch.zeros(12 * fp, dtype=torch.uint8, device="cuda:0")
    flags = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rc = lib.bgls_miller_product_dev(cid, t_sig.data_ptr(), t_keys.data_ptr(), t_msgs.data_ptr(), 64, 64, n, 1, part.data_ptr(), flags.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, int(flags[0].item()), bytes(part.cpu().numpy())


def run_empty_product(lib, cid):
    """the product of no pairs and no signature: the caller's partial becomes the GT element 1"""
    import torch
    part = torch.full((12 * FP[cid],), 0x77, dtype=torch.uint8, device="cuda:0")
    flags = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rc = lib.bgls_miller_product_dev(cid, None, None, None, 64, 64, 0, 1, part.data_ptr(), flags.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, int(flags[0].item()), bytes(part.cpu().numpy())


def run_final_dev(lib, cid, parts):
    """bgls_final_verify_dev over the product of the listed partials, with a clear flag word"""
    import torch
    t_parts = dev_bytes(b"".join(parts))
    flags = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return (lib.bgls_final_verify_dev(cid, t_parts.data_ptr(), len(parts), flags.data_ptr(), None),)


def make_miller_dev_case(cid, n):
    """bgls_miller_product_dev: the partial is a Miller value, so the oracle states its final exponentiation -- 1 for the valid instance,
    the GT element of the tampered one -- and the empty product, whose partial is the GT element 1 itself"""
    def build(lib):
        keys, msgs, sig = agg_instance(lib, cid, n, 500 + n, msg_len=64)
        bkeys, bmsgs, bsig = agg_instance(lib, cid, 1000, 11, msg_len=64)
        bad = list(msgs)
        bad[n - 1] = flip(bad[n - 1])
        ks = cut(keys, 4 * FP[cid])
        gt, gt_bad = o_agg_gt(lib, cid, sig, ks, msgs), o_agg_gt(lib, cid, sig, ks, bad)
        assert gt == identity(cid) and gt_bad != gt

        def big():
            return run_miller_dev(lib, cid, bsig, bkeys, bmsgs, 1000)
        return [Case(lambda: run_miller_dev(lib, cid, sig, keys, msgs, n), (0, 0, lambda p: coracle.final_exp(cid, p) == gt), big,
                     lambda: run_miller_dev(lib, cid, sig, keys, bad, n), (0, 0, lambda p: coracle.final_exp(cid, p) == gt_bad)),
                Case(lambda: run_empty_product(lib, cid), (0, 0, identity(cid)), big)]
    return build


def make_final_verify_case(cid):
    """bgls_final_verify_dev on one partial of a valid and of a tampered 61-signer instance (made once, checked on the oracle), and on the
    product of 300 partials"""
    def build(lib):
        def make():
            keys, msgs, sig = agg_instance(lib, cid, 61, 561, msg_len=64)
            bad = [flip(msgs[0])] + msgs[1:]
            good_part, bad_part = run_miller_dev(lib, cid, sig, keys, msgs, 61), run_miller_dev(lib, cid, sig, keys, bad, 61)
            assert good_part[:2] == (0, 0) and bad_part[:2] == (0, 0)
            return good_part[2], bad_part[2]
        part, part_bad = memo(("final-parts", cid), make)
        want, want_bad = (o_verdict(cid, coracle.final_exp(cid, part)),), (o_verdict(cid, coracle.final_exp(cid, part_bad)),)
        assert (want, want_bad) == ((1,), (0,))
        return Case(lambda: run_final_dev(lib, cid, [part]), want, lambda: run_final_dev(lib, cid, [part] * 299 + [part_bad]),
                    lambda: run_final_dev(lib, cid, [part_bad]), want_bad)
    return build


def make_gt_pow_case(cid):
    def build(lib):
        fp = FP[cid]
        g = coracle.pairing_product(cid, gen(lib, cid, 1), gen(lib, cid, 2), 1)
        g5 = g
        for _ in range(4):
            g5 = coracle.gt_mul(cid, g5, g)
        _, b1 = points(lib, cid, 1, 700, 9)
        _, b2 = points(lib, cid, 2, 700, 10)

        def power(negative):
            o = out(12 * fp)
            rc = lib.bgls_gt_pow(cid, B(g), B((5).to_bytes(32, "big")), negative, o)
            return rc, bytes(o)

        def big():                                       # the entry has no size: the larger call is the one it shares WS_IN_A and the flag word with
            return run_pairing_product(lib, cid, b1, b2, 700)
        # g^-5 is the one element whose product with g^5 is 1
        return [Case(lambda: power(0), (0, g5), big), Case(lambda: power(1), (0, lambda x: coracle.gt_mul(cid, g5, x) == identity(cid)), big)]
    return build


# ----------------------------------------------------------------------------------------------------------------- hashing
def ragged_msgs(n, seed):
    rnd = random.Random(seed)
    return [rnd.randbytes(di.LENGTHS[(7 * i + seed) % len(di.LENGTHS)]) for i in range(n)]


def run_hash(lib, cid, msgs):
    o = out(len(msgs) * 2 * FP[cid])
    rc = lib.bgls_hash_to_g1(cid, B(b"".join(msgs)), offs([len(m) for m in msgs]), len(msgs), o)
    return rc, bytes(o)


def make_hash_case(cid, n):
    def build(lib):
        msgs, big = ragged_msgs(n, 600 + n), ragged_msgs(2000, 12)
        want = (0, b"".join(coracle.hash_to_g1(cid, m) for m in msgs))
        return Case(lambda: run_hash(lib, cid, msgs), want, lambda: run_hash(lib, cid, big))
    return build


def keyed_keys(lib, cid, n, seed):
    def make():
        _, raw = points(lib, cid, 2, n, seed)
        comp = out(n * 2 * FP[cid])
        assert lib.bgls_compress_points(cid, 2, B(raw), n, comp) == 0
        return cut(raw, 4 * FP[cid]), cut(bytes(comp), 2 * FP[cid])
    return memo(("keyed", cid, n, seed), make)


def run_hash_keyed(lib, cid, mode, keys, msgs):
    n = len(keys)
    o = out(n * 2 * FP[cid])
    blob, off = (None, None) if mode == 1 else (B(b"".join(msgs)), offs([len(m) for m in msgs]))
    rc = lib.bgls_hash_to_g1_keyed(cid, mode, B(b"".join(keys)), blob, off, n, o)
    return rc, bytes(o)


def make_hash_keyed_case(cid, mode, n):
    def build(lib):
        keys, comp = keyed_keys(lib, cid, n, 700 + n)
        bkeys, _ = keyed_keys(lib, cid, 1000, 13)
        msgs, bmsgs = ragged_msgs(n, 650 + n), ragged_msgs(1000, 14)
        inputs = comp if mode == 1 else [k + m for k, m in zip(keys, msgs)]
        want = (0, b"".join(coracle.hash_to_g1(cid, m) for m in inputs))
        return Case(lambda: run_hash_keyed(lib, cid, mode, keys, msgs), want, lambda: run_hash_keyed(lib, cid, mode, bkeys, bmsgs))
    return build


# ------------------------------------------------------------------------------------------------------------------ points
def run_aggregate_points(lib, cid, group, raw, n):
    o = out((2 if group == 1 else 4) * FP[cid])
    rc = lib.bgls_aggregate_points(cid, group, B(raw), n, o)
    return rc, bytes(o)


def make_aggregate_points_case(cid, group, n):
    def build(lib):
        _, raw = points(lib, cid, group, n, 800 + n)
        _, big = points(lib, cid, group, 5000, 15)
        want = (0, o_sum(cid, group, cut(raw, (2 if group == 1 else 4) * FP[cid])))          # n = 0: the point at infinity
        return Case(lambda: run_aggregate_points(lib, cid, group, raw, n), want, lambda: run_aggregate_points(lib, cid, group, big, 5000))
    return build


def make_weighted_sum_case(cid, group, msm_min):
    def build(lib):
        n = 33
        rnd = random.Random(900 + group)
        _, raw = points(lib, cid, group, n, 900 + group)
        _, big = points(lib, cid, group, 700, 16)
        w = [rnd.getrandbits(128) for _ in range(n)]
        w[6], w[7], w[8] = 0, 1, (1 << 128) - 1
        bw = [rnd.getrandbits(128) for _ in range(700)]
        want = (mm.oracle_wsum(cid, group, raw, w),)
        return Case(lambda: (mm.wsum(lib, cid, group, raw, w, msm_min),), want, lambda: (mm.wsum(lib, cid, group, big, bw, msm_min),))
    return build


def make_weighted_verify_case(cid):
    """the weighted key sums behind a verdict: bgls_verify_multi_multiplicity (signed 64-bit weights from the host), bgls_verify_multi_hae,
    bgls_verify_aggregate_hae and bgls_aggregate_signatures_hae (hashed exponents), at 33 keys -- the bucket method from 32 points;
    one case per entry, each with the 700-key instance of the same entry"""
    def build(lib):
        fp, n, r = FP[cid], 33, ORDER[cid]

        def make(count, seed):
            rnd = random.Random(seed)
            sks, keys = mh.gen_keys(lib, cid, fp, count, seed)
            mult = [rnd.randrange(-5, 1 << 40) for _ in range(count)]
            mult[1], mult[2] = -3, 0
            msg = rnd.randbytes(30)
            msgs = [rnd.randbytes(20) + bytes([i & 255, i >> 8]) for i in range(count)]
            # the Kosk forms hash 0x01 || message (bgls/blsKosk.go); the C call takes the prefixed message
            msig = coracle.scale_point(cid, 1, coracle.hash_to_g1(cid, b"\x01" + msg), sum(m * s for m, s in zip(mult, sks)) % r)
            _, sigs = run_sign(lib, cid, sks, msgs)
            agg = out(2 * fp)
            assert lib.bgls_aggregate_signatures_hae(cid, B(sigs), B(keys), count, agg) == 0
            return keys, mult, msg, msgs, msig, mh.hae_sign(lib, cid, fp, sks, keys, msg), sigs, bytes(agg)
        small, big = memo(("weighted", cid), lambda: make(n, 2300)), memo(("weighted-big", cid), lambda: make(700, 30))
        keys, mult, msg, msgs, msig, hsig, sigs, agg = small
        bad_msgs = [flip(msgs[0])] + msgs[1:]

        def multiplicity(v, msg_):
            k = len(v[1])
            return (lib.bgls_verify_multi_multiplicity(cid, B(v[4]), B(v[0]), (ctypes.c_int64 * k)(*v[1]), k, B(b"\x01" + msg_), 1 + len(msg_)),)

        def multi_hae(v, msg_):
            return (lib.bgls_verify_multi_hae(cid, B(v[5]), B(v[0]), len(v[1]), B(msg_), len(msg_)),)

        def aggregate_hae(v, msgs_):
            return (lib.bgls_verify_aggregate_hae(cid, B(v[7]), B(v[0]), B(b"".join(msgs_)), offs([len(m) for m in msgs_]), len(msgs_)),)

        def sum_hae(v):
            o = out(2 * fp)
            rc = lib.bgls_aggregate_signatures_hae(cid, B(v[6]), B(v[0]), len(v[1]), o)
            return rc, bytes(o)
        wants = [(coracle.verify_multi_multiplicity(cid, msig, keys, n, mult, m),) for m in (msg, flip(msg))]
        wants += [(coracle.verify_multi_hae(cid, hsig, keys, n, m),) for m in (msg, flip(msg))]
        wants += [(coracle.verify_aggregate_hae(cid, agg, keys, m),) for m in (msgs, bad_msgs)]
        assert wants == [(1,), (0,)] * 3
        return [Case(lambda: multiplicity(small, msg), wants[0], lambda: multiplicity(big, big[2]), lambda: multiplicity(small, flip(msg)), wants[1]),
                Case(lambda: multi_hae(small, msg), wants[2], lambda: multi_hae(big, big[2]), lambda: multi_hae(small, flip(msg)), wants[3]),
                Case(lambda: aggregate_hae(small, msgs), wants[4], lambda: aggregate_hae(big, big[3]), lambda: aggregate_hae(small, bad_msgs), wants[5]),
                Case(lambda: sum_hae(small), (0, coracle.aggregate_signatures_hae(cid, sigs, keys, n)), lambda: sum_hae(big))]
    return build


def make_scale_generator_case(cid, group):
    def build(lib):
        ks, _ = points(lib, cid, group, 5, 1000 + group)
        bks, _ = points(lib, cid, group, 2000, 17)
        g = gen(lib, cid, group)
        want = (b"".join(coracle.scale_point(cid, group, g, k) for k in ks),)
        return Case(lambda: (mm.gen_points(lib, cid, group, ks),), want, lambda: (mm.gen_points(lib, cid, group, bks),))
    return build


def run_scale_points(lib, cid, group, raw, ks, signs):
    n = len(ks)
    o = out(n * (2 if group == 1 else 4) * FP[cid])
    rc = lib.bgls_scale_points(cid, group, B(raw), B(b"".join(k.to_bytes(32, "big") for k in ks)), B(bytes(signs)), n, o)
    return rc, bytes(o)


def make_scale_points_case(cid, group):
    def build(lib):
        size = (2 if group == 1 else 4) * FP[cid]
        rnd = random.Random(1100 + group)
        _, raw = points(lib, cid, group, 5, 1100 + group)
        _, big = points(lib, cid, group, 2000, 18)
        ks, signs = [rnd.randrange(1, ORDER[cid]) for _ in range(5)], [0, 1, 0, 1, 1]
        bks, bsigns = [rnd.randrange(1, 1 << 256) for _ in range(2000)], [i & 1 for i in range(2000)]
        want = (0, b"".join(coracle.scale_point(cid, group, p, (ORDER[cid] - k) if s else k) for p, k, s in zip(cut(raw, size), ks, signs)))
        return Case(lambda: run_scale_points(lib, cid, group, raw, ks, signs), want, lambda: run_scale_points(lib, cid, group, big, bks, bsigns))
    return build


def run_sign(lib, cid, sks, msgs):
    n = len(sks)
    o = out(n * 2 * FP[cid])
    rc = lib.bgls_sign_batch(cid, B(b"".join(s.to_bytes(32, "big") for s in sks)), B(b"".join(msgs)), offs([len(m) for m in msgs]), n, o)
    return rc, bytes(o)


def make_sign_case(cid, n):
    def build(lib):
        rnd = random.Random(1200 + n)
        sks, bsks = [rnd.randrange(1, ORDER[cid]) for _ in range(n)], [rnd.randrange(1, ORDER[cid]) for _ in range(2000)]
        msgs, bmsgs = ragged_msgs(n, 1200 + n), ragged_msgs(2000, 19)
        want = (0, b"".join(coracle.scale_point(cid, 1, coracle.hash_to_g1(cid, m), s) for s, m in zip(sks, msgs)))
        return Case(lambda: run_sign(lib, cid, sks, msgs), want, lambda: run_sign(lib, cid, bsks, bmsgs))
    return build


def wire_fixture(name):
    return memo(("wire", name), lambda: json.load(open(os.path.join(HERE, "golden", "wire_%s.json" % name))))


def make_wire_case(cid, name, group):
    """bgls_compress_points and bgls_decompress_points, a case each, on the committed wire fixture of the curve (recorded from the oracle)"""
    def build(lib):
        V, key = wire_fixture(name), "g%d" % group
        cb = FP[cid] * group
        rows, drows = V[key], V[key + "_decode"]
        pts, ins = b"".join(bytes.fromhex(r["pt"]) for r in rows), b"".join(bytes.fromhex(r["in"]) for r in drows)
        _, big = points(lib, cid, group, 3000, 20)

        def compress(raw, n):
            o = out(n * cb)
            rc = lib.bgls_compress_points(cid, group, B(raw), n, o)
            return rc, bytes(o)

        def decompress(raw, n):
            o, ok = out(n * 2 * cb), out(n)
            rc = lib.bgls_decompress_points(cid, group, B(raw), n, o, ok)
            return rc, bytes(o), bytes(ok)[:n]
        big_comp = memo(("wire-big", cid, group), lambda: compress(big, 3000)[1])
        want_c = (0, b"".join(bytes.fromhex(r["compressed"]) for r in rows))
        want_d = (0, b"".join(bytes.fromhex(r["pt"]) if r["ok"] else bytes(2 * cb) for r in drows), bytes(1 if r["ok"] else 0 for r in drows))
        return [Case(lambda: compress(pts, len(rows)), want_c, lambda: compress(big, 3000)),
                Case(lambda: decompress(ins, len(drows)), want_d, lambda: decompress(big_comp, 3000))]
    return build


def make_check_points_case(cid, name, group):
    """bgls_check_points on the committed subgroup fixture (points of the group, of the curve outside it, off the curve)"""
    def build(lib):
        V = memo(("subgroup", name), lambda: json.load(open(os.path.join(HERE, "golden", "subgroup_%s.json" % name))))
        rows = V["points" if group == 2 else "g1_points"]
        pts = b"".join(bytes.fromhex(r["pt"]) for r in rows)
        _, big = points(lib, cid, group, 3000, 20)

        def run(raw, n):
            ok = out(n)
            rc = lib.bgls_check_points(cid, group, B(raw), n, ok)
            return rc, bytes(ok)[:n]
        return Case(lambda: run(pts, len(rows)), (0, bytes(1 if r["in_subgroup"] else 0 for r in rows)), lambda: run(big, 3000))
    return build


# ------------------------------------------------------------------------------------------------------------ duplicate scans
def make_dup_scan_case():
    """bgls_duplicate_scan_dev, bgls_duplicate_scan_bucket_dev (a case per bucket), bgls_digest_pack_dev and bgls_duplicate_scan_packed_dev (a
    case per bucket) on 300 records: the clean list is the valid instance, the list with a planted pair the tampered one"""
    def build(lib):
        import torch
        rnd = random.Random(1300)
        n, nb, cap, bcap = 300, 3, 200, 9000
        msgs = [rnd.randbytes(64) for _ in range(n)]
        dup = list(msgs)
        dup[250] = dup[3]

        def records(count):                                                    # no record looks like padding (bytes 1 .. 15 all zero)
            return [bytes([rnd.randrange(256), 1 + rnd.randrange(255)]) + rnd.randbytes(14) for _ in range(count)]
        recs, brecs = records(n), records(20000)
        rdup = list(recs)
        rdup[250] = rdup[3]
        owner = rdup[3][0] % nb
        big = [rnd.randbytes(64) for _ in range(20000)]

        def word():
            return torch.zeros(1, dtype=torch.int32, device="cuda:0")

        def scan(ms_):
            t, f = dev_bytes(b"".join(ms_)), word()
            rc = lib.bgls_duplicate_scan_dev(t.data_ptr(), 64, 64, len(ms_), f.data_ptr(), None)
            torch.cuda.synchronize()
            return rc, int(f.item()) & FLAG_DUP

        def bucket(rs, b):
            t, f = dev_bytes(b"".join(rs)), word()
            rc = lib.bgls_duplicate_scan_bucket_dev(t.data_ptr(), 16, 16, len(rs), b, nb, f.data_ptr(), None)
            torch.cuda.synchronize()
            return rc, int(f.item()) & FLAG_DUP

        def pack(rs, cap_):
            t, w = dev_bytes(b"".join(rs)), word()
            slots = torch.zeros(nb * cap_ * 16, dtype=torch.uint8, device="cuda:0")
            rc = lib.bgls_digest_pack_dev(t.data_ptr(), len(rs), nb, cap_, slots.data_ptr(), w.data_ptr(), None)
            torch.cuda.synchronize()
            raw = bytes(slots.cpu().numpy())
            res = [rc, int(w.item())]
            for b in range(nb):
                slot = cut(raw[b * cap_ * 16:(b + 1) * cap_ * 16], 16)
                res.append(tuple(sorted(r for r in slot if any(r[1:]))))                                    # the order within a slot is the arrival order
                res.append(all(r[0] == (b + 1) % nb for r in slot if not any(r[1:])))                       # the rest is padding of the next bucket
            return tuple(res)

        def want_pack(rs):
            return (0, 0) + tuple(x for b in range(nb) for x in (tuple(sorted(r for r in rs if r[0] % nb == b)), True))

        def slot_of(rs, b, cap_):
            """what an exchange delivers to rank b: its bucket's records, then padding of the next bucket"""
            mine = [r for r in rs if r[0] % nb == b]
            return b"".join(mine) + (bytes([(b + 1) % nb]) + bytes(15)) * (cap_ - len(mine))

        def packed(rs, b, cap_):
            recv, f = dev_bytes(slot_of(rs, b, cap_)), word()
            rc = lib.bgls_duplicate_scan_packed_dev(recv.data_ptr(), cap_, b, nb, f.data_ptr(), None)
            torch.cuda.synchronize()
            return rc, int(f.item()) & FLAG_DUP
        cases = [Case(lambda: scan(msgs), (0, 0), lambda: scan(big), lambda: scan(dup), (0, 1)),
                 Case(lambda: pack(recs, cap), want_pack(recs), lambda: pack(brecs, bcap), lambda: pack(rdup, cap), want_pack(rdup))]
        for b in range(nb):
            hit = 1 if b == owner else 0
            cases.append(Case(lambda b=b: bucket(recs, b), (0, 0), lambda b=b: bucket(brecs, b), lambda b=b: bucket(rdup, b), (0, hit)))
            cases.append(Case(lambda b=b: packed(recs, b, cap), (0, 0), lambda b=b: packed(brecs, b, bcap), lambda b=b: packed(rdup, b, cap), (0, hit)))
        return cases
    return build


# ------------------------------------------------------------------------------------------- the calls with one verdict per item
def split_sizes(items, sizes):
    res, at = [], 0
    for c in sizes:
        res.append(items[at:at + c])
        at += c
    return res


def make_aggregate_batch_case(cid):
    def build(lib):
        fp = FP[cid]
        sizes, bsizes = [0, 1, 2, 60, 61, 5], [300, 7, 1000, 129, 64, 200]
        keys, msgs, sigs, _ = memo(("aggb", cid), lambda: ba.make_batch(lib, cid, fp, sizes, 1400))
        bkeys, bmsgs, bsigs, _ = memo(("aggb-big", cid), lambda: ba.make_batch(lib, cid, fp, bsizes, 21))
        msgs = list(msgs)
        t = sum(sizes[:4]) + 17
        msgs[t] = flip(msgs[t])                                                # instance 4 is tampered
        gts = [o_agg_gt(lib, cid, s, k, m) for s, k, m in zip(sigs, split_sizes(cut(keys, 4 * fp), sizes), split_sizes(msgs, sizes))]
        verdicts = [o_verdict(cid, g) for g in gts]
        assert verdicts == [1, 1, 1, 1, 0, 1]
        return Case(lambda: ba.run_batch(lib, cid, fp, sizes, keys, msgs, sigs), (sum(verdicts), verdicts, b"".join(gts)),
                    lambda: ba.run_batch(lib, cid, fp, bsizes, bkeys, bmsgs, bsigs))
    return build


def make_multi_batch_case(cid):
    def build(lib):
        import test_gpu_batch_multi as bm
        fp = FP[cid]
        sizes, bsizes = [5, 70, 2, 129, 64, 33], [300, 40, 1000, 7, 513, 64]
        keys, aggs, msgs, _ = memo(("multib", cid), lambda: bm.instance(lib, cid, fp, sizes, 1500))
        bkeys, baggs, bmsgs, _ = memo(("multib-big", cid), lambda: bm.instance(lib, cid, fp, bsizes, 22))

        def run(aggs_, keys_, sizes_, msgs_):
            return (lib.bgls_verify_multi_batch(cid, B(aggs_), B(keys_), offs(sizes_), len(sizes_), B(b"".join(msgs_)), offs([len(m) for m in msgs_]), 0),)
        bad = [msgs[1], msgs[0]] + msgs[2:]
        aggsig = coracle.aggregate_points(cid, 1, aggs, len(sizes))
        apks = b"".join(o_sum(cid, 2, ks) for ks in split_sizes(cut(keys, 4 * fp), sizes))
        want = (coracle.verify_aggregate(cid, aggsig, apks, msgs, False, threads=8),)
        want_bad = (coracle.verify_aggregate(cid, aggsig, apks, bad, False, threads=8),)
        assert want == (1,) and want_bad == (0,)
        return Case(lambda: run(aggs, keys, sizes, msgs), want, lambda: run(baggs, bkeys, bsizes, bmsgs), lambda: run(aggs, keys, sizes, bad), want_bad)
    return build


def o_multi_gt(lib, cid, sig, keys, msg):
    return o_gt(cid, [coracle.hash_to_g1(cid, msg), o_neg(cid, sig)], [o_sum(cid, 2, keys), gen(lib, cid, 2)])


def make_multi_sets_case(cid):
    def build(lib):
        fp = FP[cid]
        sizes, bsizes = [0, 1, 2, 127, 128, 129], [300, 40, 1000, 7, 513, 64] * 6
        keys, msgs, sigs, _ = memo(("sets", cid), lambda: ms.make_sets(lib, cid, fp, sizes, 1600))
        bkeys, bmsgs, bsigs, _ = memo(("sets-big", cid), lambda: ms.make_sets(lib, cid, fp, bsizes, 23))
        msgs, sigs = list(msgs), list(sigs)
        msgs[2] = msgs[2] + b"x"                                               # set 2 is tampered
        sigs[0] = bytes(2 * fp)                                                # the empty set signs with the point at infinity
        gts = [o_multi_gt(lib, cid, s, k, m) for s, k, m in zip(sigs, split_sizes(cut(keys, 4 * fp), sizes), msgs)]
        verdicts = [o_verdict(cid, g) for g in gts]
        assert verdicts == [1, 1, 0, 1, 1, 1]
        return Case(lambda: ms.run_sets(lib, cid, fp, sizes, keys, msgs, sigs), (sum(verdicts), verdicts, b"".join(gts)),
                    lambda: ms.run_sets(lib, cid, fp, bsizes, bkeys, bmsgs, bsigs))
    return build


def make_combined_case(cid):
    """six sets in three groups, and the same sets as ONE group (group_off = NULL: the unpadded Miller path): a case each"""
    def build(lib):
        fp = FP[cid]
        sizes, groups = [1, 2, 5, 3, 1, 2], [2, 3, 1]
        bsizes, bgroups = [3, 1, 2] * 100, [61, 200, 39]
        keys, msgs, sigs, _ = memo(("comb", cid), lambda: ms.make_sets(lib, cid, fp, sizes, 1700))
        bkeys, bmsgs, bsigs, _ = memo(("comb-big", cid), lambda: ms.make_sets(lib, cid, fp, bsizes, 24))
        msgs = list(msgs)
        msgs[3] = flip(msgs[3])                                                # a set of group 1 is tampered
        r = [int.from_bytes(c, "big") for c in cut(mc.want_coefficients(mc.SEED, len(sizes)), 16)]
        rh = [coracle.scale_point(cid, 1, coracle.hash_to_g1(cid, m), k) for m, k in zip(msgs, r)]
        rs = [coracle.scale_point(cid, 1, s, k) for s, k in zip(sigs, r)]
        apks = [o_sum(cid, 2, ks) for ks in split_sizes(cut(keys, 4 * fp), sizes)]

        def group_gt(lo, hi):
            return o_gt(cid, rh[lo:hi] + [o_neg(cid, o_sum(cid, 1, rs[lo:hi]))], apks[lo:hi] + [gen(lib, cid, 2)])
        gts = [group_gt(0, 2), group_gt(2, 5), group_gt(5, 6)]
        one = group_gt(0, 6)
        verdicts = [o_verdict(cid, g) for g in gts]
        assert verdicts == [1, 0, 1] and o_verdict(cid, one) == 0
        return [Case(lambda: mc.run_combined(lib, cid, fp, sizes, keys, msgs, sigs, groups), (sum(verdicts), verdicts, b"".join(gts)),
                     lambda: mc.run_combined(lib, cid, fp, bsizes, bkeys, bmsgs, bsigs, bgroups)),
                Case(lambda: mc.run_combined(lib, cid, fp, sizes, keys, msgs, sigs, None), (0, [0], one),
                     lambda: mc.run_combined(lib, cid, fp, bsizes, bkeys, bmsgs, bsigs, None))]
    return build


def hae_sets(lib, cid, sizes, seed):
    fp = FP[cid]
    rnd = random.Random(seed)
    sks, keys = mh.gen_keys(lib, cid, fp, sum(sizes), seed)
    ksets, sk_sets = mh.split(keys, sizes, fp), split_sizes(sks, sizes)
    msgs = [rnd.randbytes(1 + rnd.randrange(40)) for _ in sizes]
    return ksets, msgs, [mh.hae_sign(lib, cid, fp, s, k, m) for s, k, m in zip(sk_sets, ksets, msgs)]


def make_hae_sets_case(cid, host_min):
    def build(lib):
        fp = FP[cid]
        sizes, bsizes = [3, 1, 5, 64, 2, 33], [128, 5, 300, 64, 17, 1] * 4
        ksets, msgs, sigs = memo(("hae", cid), lambda: hae_sets(lib, cid, sizes, 1800))
        bk, bm_, bs = memo(("hae-big", cid), lambda: hae_sets(lib, cid, bsizes, 25))
        msgs = list(msgs)
        msgs[4] = flip(msgs[4])                                                # set 4 is tampered
        apks = []
        for ks, c in zip(ksets, sizes):
            t = coracle.hae_exponents(cid, ks, c)
            apks.append(o_sum(cid, 2, [coracle.scale_point(cid, 2, k, w) for k, w in zip(cut(ks, 4 * fp), t)]))
        gts = [o_gt(cid, [coracle.hash_to_g1(cid, m), o_neg(cid, s)], [a, gen(lib, cid, 2)]) for m, s, a in zip(msgs, sigs, apks)]
        verdicts = [o_verdict(cid, g) for g in gts]
        assert verdicts == [1, 1, 1, 1, 0, 1]
        return Case(lambda: mh.run_hae(lib, cid, fp, ksets, msgs, sigs), (sum(verdicts), verdicts, b"".join(apks), b"".join(gts)),
                    lambda: mh.run_hae(lib, cid, fp, bk, bm_, bs),
                    setup=lambda: lib.bgls_set_hae_root_host_min(host_min), teardown=lambda: lib.bgls_set_hae_root_host_min(mh.HOST_MIN_DEFAULT))
    return build


def make_ams_case(cid, sum_cut):
    def build(lib):
        fp = FP[cid]
        grp = memo(("amsgroup", cid), lambda: am.Group(lib, cid, fp, 1900 + cid))

        def make():
            rnd = random.Random(1901)
            small = [am.item(grp, s, rnd.randbytes(1 + 7 * i)) for i, s in enumerate(([0], [9, 10], [99, 100, 4294967295], list(range(64)), [3, 7, 3], list(range(5))))]
            big = [am.item(grp, list(range(i, i + 1 + (37 * i) % 130)), rnd.randbytes(20)) for i in range(200)]
            return small, big
        small, big = memo(("ams", cid), make)
        small = [dict(it) for it in small]
        small[1]["msg"] = flip(small[1]["msg"])                               # item 1 is tampered
        gts = []
        for it in small:
            agg_msg = o_sum(cid, 1, [coracle.hash_to_g1(cid, am.h2_msg(it["apk"], i)) for i in it["signers"]])
            gts.append(o_gt(cid, [coracle.hash_to_g1(cid, am.h0_msg(it["msg"])), agg_msg, o_neg(cid, it["sig"])], [it["key"], it["apk"], gen(lib, cid, 2)]))
        verdicts = [o_verdict(cid, g) for g in gts]
        assert verdicts == [1, 0, 1, 1, 1, 1]
        return Case(lambda: am.run_ams(lib, cid, fp, small), (sum(verdicts), verdicts, b"".join(gts)), lambda: am.run_ams(lib, cid, fp, big),
                    setup=lambda: lib.bgls_set_ams_sum_cut(sum_cut), teardown=lambda: lib.bgls_set_ams_sum_cut(1 << 16))
    return build


def make_bb_case(cid):
    def build(lib):
        fp = FP[cid]
        it = memo(("bb", cid), lambda: bb.make_items(lib, cid, fp, 6, 2000 + cid))
        big = memo(("bb-big", cid), lambda: bb.make_items(lib, cid, fp, 700, 26))
        it = {k: list(v) for k, v in it.items()}
        it["r"][3] = (it["r"][3] + 1) % ORDER[cid]                            # item 3 is tampered
        g1, g2 = gen(lib, cid, 1), gen(lib, cid, 2)
        ref = coracle.pairing_product(cid, g1, g2, 1)
        gts = []
        for sig, key, r, m in zip(it["sig"], it["key"], it["r"], it["m"]):
            q = o_sum(cid, 2, [coracle.scale_point(cid, 2, g2, m % ORDER[cid]), key[:4 * fp], coracle.scale_point(cid, 2, key[4 * fp:], r)])
            gts.append(coracle.pairing_product(cid, sig, q, 1))
        verdicts = [1 if g == ref else 0 for g in gts]
        assert verdicts == [1, 1, 1, 0, 1, 1]
        return Case(lambda: bb.run(lib, cid, fp, it), (sum(verdicts), verdicts, gts), lambda: bb.run(lib, cid, fp, big))
    return build


def pool(lib, cid):
    return memo(("pool", cid), lambda: di.Pool(lib, cid, FP[cid]))


def distinct_batch(p, sizes, seed, equal_len):
    """len(sizes) distinct-message instances over the pool's keys (taken round the pool): the instance whose size is 61 is tampered, an
    empty instance carries a signature that is not the point at infinity"""
    rnd = random.Random(seed)
    ioff, keys, msgs, sigs = [0], [], [], []
    for size in sizes:
        idx = [(ioff[-1] + i) % di.POOL for i in range(size)]
        ms_ = [rnd.randbytes(24) for _ in idx] if equal_len else di.ragged(rnd, size, len(keys))
        sigs.append(p.aggregate(p.sign_distinct(idx, ms_)) if size else p.sign([3], [b"not infinity"])[0])
        keys += [p.keys[i] for i in idx]
        msgs += ms_
        ioff.append(ioff[-1] + size)
    t = ioff[sizes.index(61)] + 17
    msgs[t] = msgs[t][:-1] + bytes([msgs[t][-1] ^ 1]) if msgs[t] else b"\x01"
    return ioff, keys, msgs, sigs


def make_distinct_case(cid):
    """bgls_verify_aggregate_distinct (one call), bgls_verify_aggregate_distinct_batch at the six-instance shape of its own tests, and its
    device-buffer form (messages of one length: the fixed-stride view of k_key_msgs): a case each"""
    def build(lib):
        import torch
        p = pool(lib, cid)
        name, agg, keys, msgs, _ = di.distinct_cases(p, 7, 307)[0]
        bad = list(msgs)
        bad[3] = flip(bad[3])
        big_idx = [i % di.POOL for i in range(1000)]
        big_msgs = ragged_msgs(1000, 27)
        big_keys = [p.keys[i] for i in big_idx]
        big_agg = memo(("dist-big", cid), lambda: p.aggregate(p.sign_distinct(big_idx, big_msgs)))

        def one(agg_, keys_, msgs_):
            return (lib.bgls_verify_aggregate_distinct(cid, B(agg_), B(b"".join(keys_)), B(b"".join(msgs_)), di.offsets(msgs_), len(keys_)),)
        v1 = o_verdict(cid, o_agg_gt(lib, cid, agg, keys, [k + m for k, m in zip(keys, msgs)]))
        v0 = o_verdict(cid, o_agg_gt(lib, cid, agg, keys, [k + m for k, m in zip(keys, bad)]))
        assert (v1, v0) == (1, 0)
        cases = [Case(lambda: one(agg, keys, msgs), (1,), lambda: one(big_agg, big_keys, big_msgs), lambda: one(agg, keys, bad), (0,))]

        def dev(inst):
            ioff, ks, ms_, sg = inst
            bufs = [dev_bytes(b"".join(sg)), dev_bytes(b"".join(ks)), dev_bytes(b"".join(ms_))]
            torch.cuda.synchronize()
            v, gt = out(len(sg)), out(len(sg) * p.GTB)
            rc = lib.bgls_verify_aggregate_distinct_batch_dev(cid, bufs[0].data_ptr(), bufs[1].data_ptr(), (ctypes.c_uint64 * len(ioff))(*ioff), len(sg),
                                                              bufs[2].data_ptr(), 24, 24, v, gt, None)
            return rc, list(v)[:len(sg)], bytes(gt)
        for equal_len in (False, True):
            inst = memo(("distb", cid, equal_len), lambda: distinct_batch(p, di.SIZES, 61 + cid, equal_len))
            binst = memo(("distb-big", cid, equal_len), lambda: distinct_batch(p, [130, 64, 200, 61, 0, 300], 31, equal_len))
            ioff, bkeys, bmsgs, bsigs = inst
            pre = [k + m for k, m in zip(bkeys, bmsgs)]
            gts = [o_agg_gt(lib, cid, bsigs[b], bkeys[ioff[b]:ioff[b + 1]], pre[ioff[b]:ioff[b + 1]]) for b in range(len(bsigs))]
            verdicts = [o_verdict(cid, g) for g in gts]
            assert verdicts == [0, 1, 1, 1, 0, 1]
            want = (sum(verdicts), verdicts, b"".join(gts))
            if equal_len:
                cases.append(Case(lambda inst=inst: dev(inst), want, lambda binst=binst: dev(binst)))
            else:
                cases.append(Case(lambda inst=inst: di.run_batch(p, lib.bgls_verify_aggregate_distinct_batch, *inst), want,
                                  lambda binst=binst: di.run_batch(p, lib.bgls_verify_aggregate_distinct_batch, *binst)))
        return cases
    return build


def make_single_keyed_case(cid):
    """bgls_verify_single_distinct_batch, its device-buffer form (messages of one length) and bgls_check_authentication_batch: a case each,
    nine items, two of them bad (a wrong key, a wrong signature) at positions that differ between the cases"""
    def build(lib):
        import torch
        p, n = pool(lib, cid), 9
        g2 = gen(lib, cid, 2)
        big_idx = [i % di.POOL for i in range(700)]

        def items(idx, msgs_, bad_key, bad_sig, tag):
            """(signatures, keys, hash inputs' messages) with item bad_key under another key and item bad_sig under its neighbour's signature"""
            sigs = list(memo(("keyed-sigs", cid, tag), lambda: p.sign_distinct(idx, msgs_)))
            keys = [p.keys[i] for i in idx]
            if bad_key is not None:
                keys[bad_key] = p.keys[100]
                sigs[bad_sig] = sigs[bad_sig - 1]
            return sigs, keys, msgs_

        def want_for(sigs, keys, inputs):
            gts = [o_gt(cid, [coracle.hash_to_g1(cid, m), o_neg(cid, s)], [k, g2]) for s, k, m in zip(sigs, keys, inputs)]
            v = [o_verdict(cid, g) for g in gts]
            return (sum(v), v, b"".join(gts))

        def single(it):
            sigs, keys, msgs_ = it
            k = len(sigs)
            v, gt = out(k), out(k * p.GTB)
            rc = lib.bgls_verify_single_distinct_batch(cid, B(b"".join(sigs)), B(b"".join(keys)), B(b"".join(msgs_)), di.offsets(msgs_), k, v, gt)
            return rc, list(v)[:k], bytes(gt)

        def single_dev(it):
            sigs, keys, msgs_ = it
            k = len(sigs)
            bufs = [dev_bytes(b"".join(sigs)), dev_bytes(b"".join(keys)), dev_bytes(b"".join(msgs_))]
            torch.cuda.synchronize()
            v, gt = out(k), out(k * p.GTB)
            rc = lib.bgls_verify_single_distinct_batch_dev(cid, bufs[0].data_ptr(), bufs[1].data_ptr(), k, bufs[2].data_ptr(), 20, 20, v, gt, None)
            return rc, list(v)[:k], bytes(gt)

        def auth(it):
            auths, keys = it
            k = len(auths)
            v, gt = out(k), out(k * p.GTB)
            rc = lib.bgls_check_authentication_batch(cid, B(b"".join(keys)), B(b"".join(auths)), k, v, gt)
            return rc, list(v)[:k], bytes(gt)
        rnd = random.Random(2100)
        ragged9, fixed9 = ragged_msgs(n, 2100), [rnd.randbytes(20) for _ in range(n)]
        it_r = items(list(range(20, 20 + n)), ragged9, 2, 7, "ragged")
        it_f = items(list(range(60, 60 + n)), fixed9, 5, 1, "fixed")
        big_r = items(big_idx, ragged_msgs(700, 28), None, None, "big-ragged")
        big_f = items(big_idx, [rnd.randbytes(20) for _ in range(700)], None, None, "big-fixed")
        aidx = list(range(40, 40 + n))
        auths = list(memo(("auths", cid), lambda: p.sign(aidx, [p.compressed[i] for i in aidx])))
        akeys, acomp = [p.keys[i] for i in aidx], [p.compressed[i] for i in aidx]
        akeys[6], acomp[6] = p.keys[101], p.compressed[101]
        auths[3] = auths[4]
        big_auth = (memo(("auths-big", cid), lambda: p.sign(big_idx, [p.compressed[i] for i in big_idx])), [p.keys[i] for i in big_idx])
        wants = [want_for(it_r[0], it_r[1], [k + m for k, m in zip(it_r[1], ragged9)]), want_for(it_f[0], it_f[1], [k + m for k, m in zip(it_f[1], fixed9)]),
                 want_for(auths, akeys, acomp)]
        assert [w[1] for w in wants] == [[1, 1, 0, 1, 1, 1, 1, 0, 1], [1, 0, 1, 1, 1, 0, 1, 1, 1], [1, 1, 1, 0, 1, 1, 0, 1, 1]]
        return [Case(lambda: single(it_r), wants[0], lambda: single(big_r)), Case(lambda: single_dev(it_f), wants[1], lambda: single_dev(big_f)),
                Case(lambda: auth((auths, akeys)), wants[2], lambda: auth(big_auth))]
    return build


# ---------------------------------------------------------------------------------------------------------------- key sets
KEY_SETS = []        # handles uploaded by the key-set cases, released by free_key_sets


def free_key_sets(lib):
    """releases every key set a case uploaded and forgets the memoised handles"""
    while KEY_SETS:
        assert lib.bgls_keys_free(KEY_SETS.pop()) == 0
    for key in [k for k in _memo if k[0] in ("keyset", "keyset-big")]:
        del _memo[key]


def make_key_set_case(cid, shards, prepare, n=65):
    """n resident keys in `shards` shards on one device: bgls_verify_aggregate_h_gt, bgls_verify_multi_h and
    bgls_verify_aggregate_distinct_h, a case each, every one with the same entry on a 700-key set as its big instance; the fill covers the
    small set's exchange records.  n = 1 in three shards: two shards hold no key, and one of them no signature either -- its record is
    the empty product."""
    def build(lib):
        p, fp = pool(lib, cid), FP[cid]
        idx = list(range(n))
        keys = [p.keys[i] for i in idx]
        msgs = ragged_msgs(n, 2200)
        msgs = [m + bytes([i]) for i, m in enumerate(msgs)]                    # distinct: the duplicate rule stays out of it
        big_idx = [i % di.POOL for i in range(700)]
        big_keys = [p.keys[i] for i in big_idx]
        big_msgs = [m + i.to_bytes(2, "big") for i, m in enumerate(ragged_msgs(700, 29))]

        def make(ix, ms_):
            return p.aggregate(p.sign(ix, ms_)), p.aggregate(p.sign(ix, [b"one message"] * len(ix))), p.aggregate(p.sign_distinct(ix, ms_))
        agg, multi, dist = memo(("keyset-sigs", cid, n), lambda: make(idx, msgs))
        bagg, bmulti, bdist = memo(("keyset-sigs-big", cid), lambda: make(big_idx, big_msgs))

        def upload(ks):
            h = ctypes.c_uint64()
            assert lib.bgls_keys_upload(cid, B(b"".join(ks)), len(ks), di.devs(shards), shards, 1 | prepare, ctypes.byref(h)) == 0
            KEY_SETS.append(h.value)
            return h.value
        h = memo(("keyset", cid, shards, prepare, n), lambda: upload(keys))
        hb = memo(("keyset-big", cid, shards, prepare), lambda: upload(big_keys))

        def agg_gt(handle, sig, ms_):
            gt = out(12 * fp)
            rc = lib.bgls_verify_aggregate_h_gt(handle, B(sig), B(b"".join(ms_)), di.offsets(ms_), len(ms_), 0, gt)
            return rc, bytes(gt)

        def multi_h(handle, sig, one):
            return (lib.bgls_verify_multi_h(handle, B(sig), B(one), len(one)),)

        def dist_gt(handle, sig, ms_):
            gt = out(12 * fp)
            rc = lib.bgls_verify_aggregate_distinct_h(handle, B(sig), B(b"".join(ms_)), di.offsets(ms_), len(ms_), gt)
            return rc, bytes(gt)
        bad = list(msgs)
        bad[n // 2] = flip(bad[n // 2])

        def want_for(ms_, one):
            a = o_agg_gt(lib, cid, agg, keys, ms_)
            d = o_agg_gt(lib, cid, dist, keys, [k + m for k, m in zip(keys, ms_)])
            return (o_verdict(cid, a), a), (coracle.verify_multi(cid, multi, b"".join(keys), n, one),), (o_verdict(cid, d), d)
        want, want_bad = memo(("keyset-want", cid, n), lambda: (want_for(msgs, b"one message"), want_for(bad, b"another message")))
        assert [w[0] for w in want] == [1, 1, 1] and [w[0] for w in want_bad] == [0, 0, 0]
        return [Case(lambda: agg_gt(h, agg, msgs), want[0], lambda: agg_gt(hb, bagg, big_msgs), lambda: agg_gt(h, agg, bad), want_bad[0], handle=h),
                Case(lambda: multi_h(h, multi, b"one message"), want[1], lambda: multi_h(hb, bmulti, b"one message"),
                     lambda: multi_h(h, multi, b"another message"), want_bad[1], handle=h),
                Case(lambda: dist_gt(h, dist, msgs), want[2], lambda: dist_gt(hb, bdist, big_msgs), lambda: dist_gt(h, dist, bad), want_bad[2], handle=h)]
    return build


# ------------------------------------------------------------------------------------------------------------- the registry
# Sizes: the smallest on each side of each path switch of the engine (engine_core.inc / engine_verify.inc) --
#   LAT_MAX = 128 pairings (k_miller_latx / k_miller_x60): 3, 61, 129; shapes automatic, (4, 8) and (4, 16 + 8) force x60's 60- and 64-forms
#   alt-bn128 hashing, one wave per four messages / work-list rounds at 256 messages: 5, 300
#   bgls_set_msm_min 0 / SIZE_MAX at 33 points; bgls_set_ams_sum_cut default / 2; bgls_set_hae_root_host_min 0 / SIZE_MAX
#   G2 key sums, one block of lane pairs / several blocks and the one-launch tree above 128 keys: 1, 5, 300
for _cid, _name in CURVES:
    for _n in (3, 61, 129, 300):
        for _shape, _tag in ((None, "auto"), (8, "x60"), (24, "x64")):
            if _n == 300 and _shape is not None:
                continue
            case("aggregate-%s-n%d-%s" % (_name, _n, _tag))(make_agg_case(_cid, _n, _shape, 0))
    case("aggregate-%s-n61-dups-allowed" % _name)(make_agg_case(_cid, 61, None, 1))
    case("aggregate-%s-duplicate-rule" % _name)(make_duprule_case(_cid))
    for _n in (1, 5, 300):
        case("multi-%s-n%d" % (_name, _n))(make_multi_case(_cid, _n))
    for _n, _shape, _tag in ((3, None, "auto"), (61, None, "auto"), (129, None, "auto"), (61, 8, "x60"), (67, 24, "x64")):
        case("pairing-product-%s-n%d-%s" % (_name, _n, _tag))(make_pairing_case(_cid, _n, _shape))
    for _n in (3, 129):
        case("miller-product-dev-%s-n%d" % (_name, _n))(make_miller_dev_case(_cid, _n))
    case("final-verify-dev-%s" % _name)(make_final_verify_case(_cid))
    case("gt-pow-%s" % _name)(make_gt_pow_case(_cid))
    for _n in (5, 300):
        case("hash-to-g1-%s-n%d" % (_name, _n))(make_hash_case(_cid, _n))
        for _mode in (0, 1):
            case("hash-to-g1-keyed-%s-mode%d-n%d" % (_name, _mode, _n))(make_hash_keyed_case(_cid, _mode, _n))
        case("sign-batch-%s-n%d" % (_name, _n))(make_sign_case(_cid, _n))
    for _group in (1, 2):
        for _n in (0, 1, 5, 300):
            case("aggregate-points-%s-g%d-n%d" % (_name, _group, _n))(make_aggregate_points_case(_cid, _group, _n))
        for _min, _tag in ((0, "buckets"), (SIZE_MAX, "per-point")):
            case("weighted-sum-%s-g%d-%s" % (_name, _group, _tag))(make_weighted_sum_case(_cid, _group, _min))
        case("scale-generator-%s-g%d" % (_name, _group))(make_scale_generator_case(_cid, _group))
        case("scale-points-%s-g%d" % (_name, _group))(make_scale_points_case(_cid, _group))
        case("wire-%s-g%d" % (_name, _group))(make_wire_case(_cid, _name, _group))
        case("check-points-%s-g%d" % (_name, _group))(make_check_points_case(_cid, _name, _group))
    case("weighted-verify-%s" % _name)(make_weighted_verify_case(_cid))
    case("aggregate-batch-%s" % _name)(make_aggregate_batch_case(_cid))
    case("multi-batch-%s" % _name)(make_multi_batch_case(_cid))
    case("multi-sets-%s" % _name)(make_multi_sets_case(_cid))
    case("multi-sets-combined-%s" % _name)(make_combined_case(_cid))
    for _min, _tag in ((0, "host-roots"), (SIZE_MAX, "device-roots")):
        case("multi-hae-sets-%s-%s" % (_name, _tag))(make_hae_sets_case(_cid, _min))
    for _cut, _tag in ((1 << 16, "one-pass"), (2, "cut2")):
        case("ams-batch-%s-%s" % (_name, _tag))(make_ams_case(_cid, _cut))
    case("bb-batch-%s" % _name)(make_bb_case(_cid))
    case("distinct-%s" % _name)(make_distinct_case(_cid))
    case("single-keyed-batches-%s" % _name)(make_single_keyed_case(_cid))
    for _shards in (1, 3):
        for _prep, _tag in ((0, "plain"), (2, "prepared")):
            case("key-set-%s-%dshards-%s" % (_name, _shards, _tag))(make_key_set_case(_cid, _shards, _prep))
    for _prep, _tag in ((0, "plain"), (2, "prepared")):
        case("key-set-%s-1key-3shards-%s" % (_name, _tag))(make_key_set_case(_cid, 3, _prep, 1))
case("duplicate-scans")(make_dup_scan_case())
