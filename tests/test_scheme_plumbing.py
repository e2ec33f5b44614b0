"""CPU tier: the host-side plumbing of the Python scheme layer (bgls_amd/bgls.py, bbsigs.py, curves.py) against a recording fake of the
C library.  No GPU and no built library: bgls_amd._lib.load is replaced for the duration of a test by a function that returns the fake,
whose every bgls_* entry records (name, args) and answers from the test's script.  What is pinned is what goes over the ABI and what
comes back: which entry is called, with which n, offsets and blob bytes, where the verdict bytes land, and how a batch that fails as a
whole is settled -- the list a batch runner returns equals what the single calls would say.

Two things are pinned by their result only, because either behaviour is right: whether a failed batch of ONE item is sent a second time
through the same entry (the second call gives the same answer), and what KoskVerifyBatchMultiSignature does with a nil point."""
import ctypes
import hashlib
import itertools
import types

import pytest

from bgls_amd import _lib, bbsigs, bgls, curves
from bgls_amd.curves import Altbn128 as cv, Bls12 as other, G1, G2, Point, PointT


# ---- the fake ------------------------------------------------------------------------------------------------------------------
def _plain(a):
    """a ctypes array as bytes (uint8) or a list (offsets, indices), so that recorded calls compare with =="""
    if isinstance(a, ctypes.Array):
        return bytes(a) if a._type_ is ctypes.c_uint8 else list(a)
    return a


class FakeLib:
    """script[name]: what the entry answers -- an rc, or (rc, bytes written into the call's output: its last argument that is not None);
    a list is consumed one answer per call, anything else answers every call.  An entry without a script answers 0."""

    def __init__(self):
        self.calls, self.script = [], {}

    def __getattr__(self, name):
        if not name.startswith("bgls_"):
            raise AttributeError(name)

        def entry(*args):
            if name == "bgls_last_error":
                return b"scripted"
            self.calls.append((name, tuple(_plain(a) for a in args)))
            ans = self.script.get(name, 0)
            if isinstance(ans, list):
                ans = ans.pop(0)
            rc, data = ans if isinstance(ans, tuple) else (ans, b"")
            if data:
                dst = [a for a in args if a is not None][-1]
                assert len(data) <= ctypes.sizeof(dst)
                ctypes.memmove(dst, bytes(data), len(data))
            return rc
        return entry

    def to(self, name):
        return [args for n, args in self.calls if n == name]


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: f)
    return f


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def g1(i):
    return Point(cv, G1, bytes([i]) * 64)


def g2(i):
    return Point(cv, G2, bytes([i]) * 128)


FG1, FG2 = Point(other, G1, bytes(96)), Point(other, G2, bytes(192))
ORDER = cv.GetG1Order()


def B(b):
    """what _lib.buf passes for these bytes (an empty blob travels as one zero byte)"""
    return bytes(b) or b"\0"


def offs(lengths):
    return [0] + list(itertools.accumulate(lengths))


def raws(points):
    return b"".join(p.raw for p in points)


def mag(k):
    """the ABI's 32-byte magnitude of a scalar, worked out here"""
    if k < 0 or k >= 1 << 256:
        k %= ORDER
    return k.to_bytes(32, "big")


# five items: good, a foreign signature, no signature, a foreign key among good ones, good
SIGS = [g1(1), FG1, None, g1(4), g1(5)]
KEYS = [[g2(10)], [g2(20), g2(21)], [g2(30)], [g2(40), FG2, g2(42)], [g2(50), g2(51)]]
MSGS = [[b""], [b"b0", b"b1"], [b"c"], [b"d0", b"", b"d2"], [b"ee0", b""]]          # one message per key
MSG1 = [b"", b"bb", b"c", b"dddd", b"eee"]                                           # one message per set
PK1 = [g2(10), g2(20), g2(30), FG2, g2(50)]                                          # one key per item
BBSIG = [bbsigs.Signature(g1(1), -3), bbsigs.Signature(FG1, 2), None, bbsigs.Signature(g1(4), 4), bbsigs.Signature(g1(5), (1 << 256) + 9)]
BBPK = [bbsigs.Pubkey(g2(10), g2(11)), bbsigs.Pubkey(g2(20), g2(21)), bbsigs.Pubkey(g2(30), g2(31)), bbsigs.Pubkey(g2(40), FG2),
        bbsigs.Pubkey(g2(50), g2(51))]
BBMSG = [7, 8, 9, 10, -11]
HMSG = [b"", b"h1", b"h2", b"h3", b"h4"]
SUBSETS = [[0, 9], [1], [2], bytes([0x18]), [4, 8, 4]]                               # over a key set of 10: two-byte rows
ROWS = [bytes([0x01, 0x02]), bytes([0x02, 0]), bytes([0x04, 0]), bytes([0x18, 0]), bytes([0x10, 0x01])]


class _Resident(bgls.KeySet):
    """a KeySet that owns no handle: nothing to free when it goes"""

    def __del__(self):
        pass


def keyset(n=10, handle=77, curve=cv):
    ks = _Resident.__new__(_Resident)
    ks.curve, ks.n, ks.handle = curve, n, handle
    return ks


class Runner:
    """One verdict runner behind a public name.  raw(a, b, c): the call on three parallel lists; batch(good): the arguments of the ONE batch
    call over the items `good`; single: (entry, args(b)) of the single call that settles item b, None where an item is settled by a batch of
    one through the same entry; good: which of the five items go into the batch."""

    def __init__(self, name, raw, lists, entry, batch, single=None, good=(0, 4)):
        self.name, self.raw, self.lists, self.entry, self.batch, self.single, self.good = name, raw, lists, entry, batch, single, list(good)

    def __call__(self, sel):
        return self.raw(*[[col[b] for b in sel] for col in self.lists])


def _aggregate(name, fn, entry, single_entry, kosk=False, allow=None):
    pre = b"\x01" if kosk else b""
    tail = () if allow is None else (allow,)

    def batch(good):
        ms = [pre + m for b in good for m in MSGS[b]]
        return (cv.id, B(raws(SIGS[b] for b in good)), B(raws(k for b in good for k in KEYS[b])), offs(len(KEYS[b]) for b in good), len(good),
                B(b"".join(ms)), offs(map(len, ms))) + tail + (bytes(len(good)), None)

    def single(b):
        ms = [pre + m for m in MSGS[b]]
        return (cv.id, SIGS[b].raw, raws(KEYS[b]), B(b"".join(ms)), offs(map(len, ms)), len(ms)) + tail
    return Runner(name, lambda s, k, m: fn(cv, s, k, m), (SIGS, KEYS, MSGS), entry, batch, (single_entry, single))


def _multi(name, fn, entry, single_entry, extra=(), kosk=False, one_key=False):
    pre = b"\x01" if kosk else b""
    keys = [[k] for k in PK1] if one_key else KEYS

    def batch(good):
        ms = [pre + MSG1[b] for b in good]
        return (cv.id, B(raws(SIGS[b] for b in good)), B(raws(k for b in good for k in keys[b])), offs(len(keys[b]) for b in good), len(good),
                B(b"".join(ms)), offs(map(len, ms)), bytes(len(good)), None) + extra

    def single(b):
        m = pre + MSG1[b]
        return cv.id, SIGS[b].raw, raws(keys[b]), len(keys[b]), B(m), len(m)
    return Runner(name, lambda s, k, m: fn(cv, s, k, m), (SIGS, PK1 if one_key else KEYS, MSG1), entry, batch, (single_entry, single))


def _subsets(name, fn, kosk=False):
    pre = b"\x01" if kosk else b""

    def batch(good):
        ms = [pre + MSG1[b] for b in good]
        return (77, B(raws(SIGS[b] for b in good)), b"".join(ROWS[b] for b in good), 2, len(good), B(b"".join(ms)), offs(map(len, ms)),
                bytes(len(good)), None, None)
    return Runner(name, lambda s, sub, m: fn(cv, s, keyset(), sub, m), (SIGS, SUBSETS, MSG1), "bgls_verify_multi_subsets_h", batch, good=(0, 3, 4))


def _keyed(name, fn, entry, msgs):
    def batch(good):
        sg, ks = B(raws(SIGS[b] for b in good)), B(raws(PK1[b] for b in good))
        if not msgs:
            return cv.id, ks, sg, len(good), bytes(len(good)), None
        ms = [MSG1[b] for b in good]
        return cv.id, sg, ks, B(b"".join(ms)), offs(map(len, ms)), len(good), bytes(len(good)), None
    return Runner(name, fn, (SIGS, PK1, MSG1), entry, batch)


def _bb(name, fn, msgs, scalar):
    def batch(good):
        return (cv.id, raws(BBSIG[b].Sigma for b in good), b"".join(mag(BBSIG[b].R) for b in good),
                b"".join(BBPK[b].U.raw + BBPK[b].V.raw for b in good), b"".join(mag(scalar(msgs[b])) for b in good), len(good), bytes(len(good)), None)
    return Runner(name, lambda s, k, m: fn(cv, s, k, m), (BBSIG, BBPK, msgs), "bgls_bb_verify_batch", batch)


def _blake(m):
    return int.from_bytes(hashlib.blake2b(m, digest_size=32).digest(), "big") % ORDER


RUNNERS = [
    _aggregate("VerifyAggregateSignatures", bgls.VerifyAggregateSignatures, "bgls_verify_aggregate_batch", "bgls_verify_aggregate", allow=0),
    _aggregate("KoskVerifyAggregateSignatures", bgls.KoskVerifyAggregateSignatures, "bgls_verify_aggregate_batch", "bgls_verify_aggregate",
               kosk=True, allow=1),
    _multi("VerifyMultiSignatures", bgls.VerifyMultiSignatures, "bgls_verify_multi_sets", "bgls_verify_multi"),
    _multi("KoskVerifyMultiSignatures", bgls.KoskVerifyMultiSignatures, "bgls_verify_multi_sets", "bgls_verify_multi", kosk=True),
    _multi("VerifySingleSignatures", bgls.VerifySingleSignatures, "bgls_verify_multi_sets", "bgls_verify_multi", one_key=True),
    _multi("KoskVerifySingleSignatures", bgls.KoskVerifySingleSignatures, "bgls_verify_multi_sets", "bgls_verify_multi", kosk=True, one_key=True),
    _subsets("VerifyMultiSignaturesBySubset", bgls.VerifyMultiSignaturesBySubset),
    _subsets("KoskVerifyMultiSignaturesBySubset", bgls.KoskVerifyMultiSignaturesBySubset, kosk=True),
    _multi("VerifyMultiSignaturesWithHAE", bgls.VerifyMultiSignaturesWithHAE, "bgls_verify_multi_hae_sets", "bgls_verify_multi_hae", extra=(None,)),
    _keyed("DistinctMsgVerifySingleSignatures", lambda s, k, m: bgls.DistinctMsgVerifySingleSignatures(cv, s, k, m),
           "bgls_verify_single_distinct_batch", True),
    _keyed("CheckAuthentications", lambda s, k, m: bgls.CheckAuthentications(cv, k, s), "bgls_check_authentication_batch", False),
    _aggregate("DistinctMsgVerifyAggregateSignatures", bgls.DistinctMsgVerifyAggregateSignatures, "bgls_verify_aggregate_distinct_batch",
               "bgls_verify_aggregate_distinct"),
    _bb("bbsigs.VerifyBatch", bbsigs.VerifyBatch, BBMSG, lambda m: m),
    _bb("bbsigs.VerifyHashedBatch", bbsigs.VerifyHashedBatch, HMSG, _blake),
]
runners = pytest.mark.parametrize("r", RUNNERS, ids=[r.name for r in RUNNERS])


# ---- batch and settle ----------------------------------------------------------------------------------------------------------
@runners
def test_mixed_input_is_one_batch_call_over_the_good_items(fake, r):
    verdicts = [1, 0, 1][:len(r.good)]
    fake.script[r.entry] = (0, bytes(verdicts))
    got = r(range(5))
    assert fake.calls == [(r.entry, r.batch(r.good))]
    assert got == [bool(verdicts[r.good.index(b)]) if b in r.good else False for b in range(5)]


@runners
def test_failed_batch_is_settled_item_by_item_in_index_order(fake, r):
    fake.script[r.entry] = [-2, (0, b"\1"), -2] if r.single is None else -2
    if r.single:
        fake.script[r.single[0]] = [1, 0]
    got = r([4, 0])                                      # items 4 and 0 as items 0 and 1 of the call
    first = (r.entry, r.batch([4, 0]))
    if r.single:
        assert fake.calls == [first, (r.single[0], r.single[1](4)), (r.single[0], r.single[1](0))]
    else:
        assert fake.calls == [first, (r.entry, r.batch([4])), (r.entry, r.batch([0]))]
    assert got == [True, False]


@runners
def test_failed_batch_of_one(fake, r):
    """a runner with a single-call function settles the item through it; the others may or may not repeat the call (same answer)"""
    fake.script[r.entry] = -2
    if r.single:
        fake.script[r.single[0]] = 1
    got = r([4])
    assert fake.calls[0] == (r.entry, r.batch([4]))
    if r.single:
        assert fake.calls[1:] == [(r.single[0], r.single[1](4))] and got == [True]
    else:
        assert all(c == fake.calls[0] for c in fake.calls) and len(fake.calls) <= 2 and got == [False]


@runners
def test_a_batch_answer_of_zero_or_more_is_taken_as_it_is(fake, r):
    fake.script[r.entry] = (1, b"\1\1")                  # rc > 0 is no failure
    assert r([0, 4]) == [True, True] and len(fake.calls) == 1


@runners
def test_length_mismatch_empty_input_and_nothing_to_batch(fake, r):
    with pytest.raises(ValueError):
        r.raw([r.lists[0][0]], [], [])
    assert r.raw([], [], []) == []
    assert r([1, 2]) == [False, False]
    assert fake.calls == []


@pytest.mark.parametrize("r", [r for r in RUNNERS if r.name.endswith(("VerifyAggregateSignatures", "VerifyMultiSignatures", "WithHAE"))],
                         ids=lambda r: r.name)
def test_an_item_over_a_key_set_gets_the_single_calls_answer_first(fake, r):
    """a KeySet in place of a key list is not batchable: the single call answers for it, before the batch call is made"""
    col = list(r.lists[1])
    col[1] = keyset(n=2)
    sigs = [g1(1), g1(2), None, g1(4), g1(5)]
    fake.script.update({"bgls_verify_aggregate_h": 1, "bgls_verify_multi_h": 1, "bgls_verify_aggregate_distinct_h": 1, r.entry: (0, b"\0\1")})
    if r.name == "VerifyMultiSignaturesWithHAE":         # its single call knows no key set: iterating one is a TypeError, as before
        with pytest.raises(TypeError):
            r.raw(sigs, col, r.lists[2])
        return
    got = r.raw(sigs, col, r.lists[2])
    assert got == [False, True, False, False, True]
    assert [n for n, _ in fake.calls] == [{"bgls_verify_aggregate_batch": "bgls_verify_aggregate_h", "bgls_verify_multi_sets": "bgls_verify_multi_h",
                                           "bgls_verify_aggregate_distinct_batch": "bgls_verify_aggregate_distinct_h"}[r.entry], r.entry]
    assert fake.calls[0][1][0] == 77 and fake.calls[0][1][1] == g1(2).raw
    assert fake.calls[1][1] == r.batch([0, 4])


def test_subset_runner_other_curve_and_type(fake):
    assert bgls.VerifyMultiSignaturesBySubset(cv, [g1(1)], keyset(curve=other), [[0]], [b"m"]) == [False]
    with pytest.raises(TypeError):
        bgls.VerifyMultiSignaturesBySubset(cv, [g1(1)], [g2(1)], [[0]], [b"m"])
    assert fake.calls == []


# ---- AMS -----------------------------------------------------------------------------------------------------------------------
def _ams_inputs():
    apks = [g2(1), g2(2), g2(3), g2(4), g2(5), g2(6), g2(7)]
    signers = [[3, 1], [0], [0], [0], [2, 2, 9], [], [1 << 32]]
    agg_keys = [g2(11), g2(12), g2(13), FG2, g2(15), g2(16), g2(17)]
    agg_sigs = [g1(1), FG1, None, g1(4), g1(5), g1(6), g1(7)]
    msgs = [b"", b"m1", b"m2", b"m3", b"mm4", b"m5", b"m6"]
    return apks, signers, agg_keys, agg_sigs, msgs


def _ams_batch(cols, good):
    apks, signers, agg_keys, agg_sigs, msgs = cols
    ms = [msgs[b] for b in good]
    return (cv.id, raws(apks[b] for b in good), raws(agg_keys[b] for b in good), raws(agg_sigs[b] for b in good),
            [i for b in good for i in signers[b]], offs(len(signers[b]) for b in good), len(good), B(b"".join(ms)), offs(map(len, ms)),
            bytes(len(good)), None)


@pytest.fixture
def ams_single(monkeypatch):
    """AmsVerifySignature is a chain of point calls of its own: the runner's use of it is pinned with a recording stand-in"""
    seen, answers = [], {}

    def stub(curve, apk, signers, aggKey, aggSig, msg):
        seen.append((curve, apk, signers, aggKey, aggSig, msg))
        return answers.get(msg, False)
    monkeypatch.setattr(bgls, "AmsVerifySignature", stub)
    return seen, answers


def test_ams_mixed_input(fake, ams_single):
    seen, answers = ams_single
    cols = _ams_inputs()
    answers[b"m6"] = True
    fake.script["bgls_ams_verify_batch"] = (0, b"\1\0")
    got = bgls.AmsVerifySignatures(cv, *cols)
    assert fake.calls == [("bgls_ams_verify_batch", _ams_batch(cols, [0, 4]))]
    # a foreign or missing point and a signer index of 2^32 go to the single path; the empty signer list is False and goes nowhere
    assert seen == [(cv,) + tuple(c[b] for c in cols) for b in (1, 2, 3, 6)]
    assert got == [True, False, False, False, False, False, True]


def test_ams_failed_batch_and_edges(fake, ams_single):
    seen, answers = ams_single
    cols = [[c[b] for b in (4, 0)] for c in _ams_inputs()]
    answers[b"mm4"] = True
    fake.script["bgls_ams_verify_batch"] = -2
    assert bgls.AmsVerifySignatures(cv, *cols) == [True, False]
    assert fake.calls == [("bgls_ams_verify_batch", _ams_batch(cols, [0, 1]))]
    assert seen == [(cv,) + tuple(c[b] for c in cols) for b in (0, 1)]
    del fake.calls[:], seen[:]
    one = [c[:1] for c in cols]
    assert bgls.AmsVerifySignatures(cv, *one) == [True]
    assert len(fake.calls) == 1 and len(seen) == 1
    del fake.calls[:], seen[:]
    with pytest.raises(ValueError):
        bgls.AmsVerifySignatures(cv, [g2(1)], [], [], [], [])
    assert bgls.AmsVerifySignatures(cv, [], [], [], [], []) == []
    assert bgls.AmsVerifySignatures(cv, [g2(1)], [[]], [g2(2)], [g1(1)], [b"m"]) == [False]
    assert fake.calls == [] and seen == []


# ---- PairBatch -----------------------------------------------------------------------------------------------------------------
GT = [bytes([0xA0 + i]) * 384 for i in range(3)]


def test_pair_batch_mixed_input(fake):
    fake.script["bgls_pair_batch"] = (0, GT[0] + GT[1])
    got = cv.PairBatch([g1(1), FG1, None, g1(4), g1(5)], [g2(1), g2(2), g2(3), FG2, g2(5)])
    assert fake.calls == [("bgls_pair_batch", (cv.id, g1(1).raw + g1(5).raw, g2(1).raw + g2(5).raw, 2, bytes(2 * 384)))]
    assert [type(p) for p in got] == [PointT, type(None), type(None), type(None), PointT]
    assert got[0].raw == GT[0] and got[4].raw == GT[1] and got[0].curve is cv


def test_pair_batch_failed_call_is_settled_with_pair(fake):
    fake.script.update({"bgls_pair_batch": -2, "bgls_pairing_product": [(0, GT[2]), -2]})
    got = cv.PairBatch([g1(5), None, g1(1)], [g2(5), g2(9), g2(1)])
    assert fake.calls == [("bgls_pair_batch", (cv.id, g1(5).raw + g1(1).raw, g2(5).raw + g2(1).raw, 2, bytes(2 * 384))),
                          ("bgls_pairing_product", (cv.id, g1(5).raw, g2(5).raw, 1, bytes(384))),
                          ("bgls_pairing_product", (cv.id, g1(1).raw, g2(1).raw, 1, bytes(384)))]
    assert got[0].raw == GT[2] and got[1] is None and got[2] is None


def test_pair_batch_a_positive_return_is_a_failure_too(fake):
    fake.script.update({"bgls_pair_batch": 1, "bgls_pairing_product": (0, GT[1])})
    got = cv.PairBatch([g1(1)], [g2(1)])
    assert [n for n, _ in fake.calls] == ["bgls_pair_batch", "bgls_pairing_product"] and got[0].raw == GT[1]


def test_pair_batch_edges(fake):
    with pytest.raises(ValueError):
        cv.PairBatch([g1(1)], [])
    assert cv.PairBatch([], []) == []
    assert cv.PairBatch([None, FG1], [g2(1), g2(2)]) == [None, None]
    assert fake.calls == []


def test_pairing_product(fake):
    fake.script["bgls_pairing_product"] = [(0, GT[0]), 3]
    pt, ok = cv.PairingProduct([g1(1), g1(2)], [g2(1), g2(2)])
    assert ok and pt.raw == GT[0]
    assert fake.calls == [("bgls_pairing_product", (cv.id, g1(1).raw + g1(2).raw, g2(1).raw + g2(2).raw, 2, bytes(384)))]
    assert cv.PairingProduct([g1(1)], [g2(1)]) == (None, False)
    del fake.calls[:]
    for a, b in (([g1(1)], []), ([g2(1)], [g2(1)]), ([g1(1)], [g1(1)]), ([None], [g2(1)]), ([FG1], [g2(1)]), ([g1(1)], [FG2])):
        assert cv.PairingProduct(a, b) == (None, False)
    assert fake.calls == []


# ---- subsets and groups --------------------------------------------------------------------------------------------------------
def test_subset_rows():
    ks = keyset(n=10)
    assert bgls._subset_rows(ks, [[0, 9], bytes([0x18]), [4, 8, 4], b"\xff\x03", []]) == (
        bytes([0x01, 0x02, 0x18, 0x00, 0x10, 0x01, 0xff, 0x03, 0x00, 0x00]), 2)
    assert bgls._subset_rows(ks, []) == (b"", 2)
    with pytest.raises(ValueError, match="subset 1: a bitmap of 3 bytes over 10 keys"):
        bgls._subset_rows(ks, [[0], bytes(3)])
    for bad in (10, -1):
        with pytest.raises(ValueError, match="subset 0: key index %d outside the key set" % bad):
            bgls._subset_rows(ks, [[bad]])


def test_group_offsets():
    assert bgls._group_offsets(5, 2) == [0, 2, 4, 5]
    assert bgls._group_offsets(4, 2) == [0, 2, 4]
    assert bgls._group_offsets(3, 64) == [0, 3]
    assert bgls._group_offsets(5, None) == [0, 5]
    for bad in (0, -3):
        with pytest.raises(ValueError, match="group must be a positive chunk size or None"):
            bgls._group_offsets(5, bad)
    assert bbsigs._group_offsets is bgls._group_offsets


def test_aggregate_keys_by_subset(fake):
    fake.script["bgls_aggregate_subsets_h"] = [(0, g2(1).raw + g2(2).raw), -3]
    got = bgls.AggregateKeysBySubset(keyset(), [[0, 9], bytes([0x18])])
    assert fake.calls == [("bgls_aggregate_subsets_h", (77, bytes([0x01, 0x02, 0x18, 0x00]), 2, 2, bytes(256)))]
    assert [(p.curve, p.group, p.raw) for p in got] == [(cv, G2, g2(1).raw), (cv, G2, g2(2).raw)]
    with pytest.raises(ValueError, match="^bgls_aggregate_subsets_h:"):
        bgls.AggregateKeysBySubset(keyset(), [[0]])
    assert bgls.AggregateKeysBySubset(keyset(), []) == []
    with pytest.raises(TypeError):
        bgls.AggregateKeysBySubset([g2(1)], [[0]])


@pytest.mark.parametrize("kosk", [False, True])
def test_grouped_by_subset(fake, kosk):
    fn = bgls.KoskVerifyAggregateSignatureGroupedBySubset if kosk else bgls.VerifyAggregateSignatureGroupedBySubset
    pre = b"\x01" if kosk else b""
    fake.script["bgls_verify_aggregate_grouped_h"] = [1, 0, 1, -2]
    ks = keyset()
    # an index list: the messages travel in ascending key order
    assert fn(cv, g1(1), ks, [7, 2, 5], [b"seven", b"", b"five"]) is True
    ms = [pre + m for m in (b"", b"five", b"seven")]
    assert fake.calls.pop() == ("bgls_verify_aggregate_grouped_h", (77, g1(1).raw, bytes([0xa4, 0x00]), 2, B(b"".join(ms)), offs(map(len, ms)), 3, None, None))
    # a bitmap goes as it is, None as no bitmap
    assert fn(cv, g1(1), ks, bytes([0x03]), [b"a", b"bc"]) is False
    ms = [pre + b"a", pre + b"bc"]
    assert fake.calls.pop() == ("bgls_verify_aggregate_grouped_h", (77, g1(1).raw, bytes([0x03]), 1, b"".join(ms), offs(map(len, ms)), 2, None, None))
    assert fn(cv, g1(1), ks, None, [b"a"]) is True
    assert fake.calls.pop() == ("bgls_verify_aggregate_grouped_h", (77, g1(1).raw, None, 0, pre + b"a", [0, len(pre) + 1], 1, None, None))
    assert fn(cv, g1(1), ks, None, [b"a"]) is False      # rc -2
    del fake.calls[:]
    with pytest.raises(ValueError, match="a key index is repeated in the subset"):
        fn(cv, g1(1), ks, [1, 2, 1], [b"a", b"b", b"c"])
    with pytest.raises(ValueError, match="a key index lies outside the key set"):
        fn(cv, g1(1), ks, [1, 10], [b"a", b"b"])
    with pytest.raises(TypeError):
        fn(cv, g1(1), [g2(1)], None, [b"a"])
    assert fn(cv, g1(1), ks, [1, 2], [b"a"]) is False
    assert fn(cv, FG1, ks, None, [b"a"]) is False and fn(cv, None, ks, None, [b"a"]) is False
    assert fn(cv, g1(1), keyset(curve=other), None, [b"a"]) is False
    assert fake.calls == []


SEED = bytes(range(32))


def test_multi_combined(fake):
    fake.script["bgls_verify_multi_sets_combined"] = [(0, b"\1\0\1"), -2]
    sigs, keys, msgs = [g1(i) for i in range(1, 6)], [[g2(10 * i + j) for j in range(i % 3 + 1)] for i in range(5)], [b"", b"b", b"cc", b"", b"eee"]
    assert bgls.VerifyMultiSignaturesCombined(cv, sigs, keys, msgs, group=2, seed=SEED) == [True, False, True]
    assert fake.calls == [("bgls_verify_multi_sets_combined", (cv.id, raws(sigs), raws(k for ks in keys for k in ks), offs(map(len, keys)), 5,
                                                                 b"".join(msgs), offs(map(len, msgs)), [0, 2, 4, 5], 3, SEED, bytes(3), None))]
    with pytest.raises(ValueError, match="^bgls_verify_multi_sets_combined:"):
        bgls.VerifyMultiSignaturesCombined(cv, sigs, keys, msgs, seed=SEED)
    assert fake.calls[1][1][7:9] == ([0, 5], 1)
    del fake.calls[:]
    with pytest.raises(ValueError, match="seed must be 32 bytes"):
        bgls.VerifyMultiSignaturesCombined(cv, sigs, keys, msgs, seed=bytes(31))
    with pytest.raises(ValueError, match="differ in length"):
        bgls.VerifyMultiSignaturesCombined(cv, sigs, keys, msgs[:4], seed=SEED)
    for s, k in (([FG1], [[g2(1)]]), ([None], [[g2(1)]]), ([g1(1)], [[g2(1), FG2]]), ([g1(1)], [[None]])):
        with pytest.raises(ValueError, match="the combined check takes G1 / G2 Points of this curve only"):
            bgls.VerifyMultiSignaturesCombined(cv, s, k, [b"m"], seed=SEED)
    assert bgls.VerifyMultiSignaturesCombined(cv, [], [], []) == []
    assert fake.calls == []
    fake.script["bgls_verify_multi_sets_combined"] = 0
    bgls.KoskVerifyMultiSignaturesCombined(cv, sigs[:2], keys[:2], [b"", b"b"])          # a drawn seed, the Kosk prefix
    args = fake.calls[0][1]
    assert args[5:7] == (b"\x01\x01b", [0, 1, 3]) and len(args[9]) == 32


def test_bb_combined(fake):
    fake.script["bgls_bb_verify_batch_combined"] = [(0, b"\0\1"), -2]
    good = [0, 4, 0]
    sigs, pks, msgs = [BBSIG[b] for b in good], [BBPK[b] for b in good], [BBMSG[b] for b in good]
    assert bbsigs.VerifyBatchCombined(cv, sigs, pks, msgs, group=2, seed=SEED) == [False, True]
    assert fake.calls == [("bgls_bb_verify_batch_combined", (cv.id, raws(s.Sigma for s in sigs), b"".join(mag(s.R) for s in sigs),
                                                               b"".join(k.U.raw + k.V.raw for k in pks), b"".join(mag(m) for m in msgs), 3, [0, 2, 3], 2,
                                                               SEED, bytes(2), None))]
    with pytest.raises(ValueError, match="^bgls_bb_verify_batch_combined:"):
        bbsigs.VerifyBatchCombined(cv, sigs, pks, msgs, seed=SEED)
    del fake.calls[:]
    with pytest.raises(ValueError, match="seed must be 32 bytes"):
        bbsigs.VerifyBatchCombined(cv, sigs, pks, msgs, seed=bytes(33))
    with pytest.raises(ValueError, match="differ in length"):
        bbsigs.VerifyBatchCombined(cv, sigs, pks[:2], msgs, seed=SEED)
    for b in (1, 2, 3):
        with pytest.raises(ValueError, match="the combined check takes Signatures and Pubkeys made of G1 / G2 Points of this curve only"):
            bbsigs.VerifyBatchCombined(cv, [BBSIG[b]], [BBPK[b]], [1], seed=SEED)
    assert bbsigs.VerifyBatchCombined(cv, [], [], []) == []
    assert fake.calls == []
    fake.script["bgls_bb_verify_batch_combined"] = 0
    assert bbsigs.VerifyHashedBatchCombined(cv, sigs[:1], pks[:1], [b"h"], seed=SEED) == [False]
    assert fake.calls[0][1][4] == mag(_blake(b"h"))


def test_located_sends_only_the_rejected_groups_again(fake):
    sigs, keys, msgs = [g1(i) for i in range(1, 6)], [[g2(i)] for i in range(1, 6)], [b"a", b"b", b"c", b"d", b"e"]
    fake.script.update({"bgls_verify_multi_sets_combined": (0, b"\1\0\1"), "bgls_verify_multi_sets": (0, b"\0\1")})
    assert bgls.VerifyMultiSignaturesLocated(cv, sigs, keys, msgs, group=2, seed=SEED) == [True, True, False, True, True]
    assert [n for n, _ in fake.calls] == ["bgls_verify_multi_sets_combined", "bgls_verify_multi_sets"]
    assert fake.calls[1][1] == (cv.id, g1(3).raw + g1(4).raw, g2(3).raw + g2(4).raw, [0, 1, 2], 2, b"cd", [0, 1, 2], bytes(2), None)
    del fake.calls[:]
    fake.script["bgls_verify_multi_sets_combined"] = (0, b"\1")
    assert bgls.VerifyMultiSignaturesLocated(cv, sigs, keys, msgs, seed=SEED) == [True] * 5          # group = 64: one group, accepted
    assert [n for n, _ in fake.calls] == ["bgls_verify_multi_sets_combined"]


def test_bb_located_sends_only_the_rejected_groups_again(fake):
    good = [0, 4, 0, 4, 0]
    sigs, pks, msgs = [BBSIG[b] for b in good], [BBPK[b] for b in good], [BBMSG[b] for b in good]
    fake.script.update({"bgls_bb_verify_batch_combined": (0, b"\0\1\1"), "bgls_bb_verify_batch": (0, b"\1\0")})
    assert bbsigs.VerifyBatchLocated(cv, sigs, pks, msgs, group=2, seed=SEED) == [True, False, True, True, True]
    assert [n for n, _ in fake.calls] == ["bgls_bb_verify_batch_combined", "bgls_bb_verify_batch"]
    assert fake.calls[1][1][1] == g1(1).raw + g1(5).raw and fake.calls[1][1][5] == 2
    del fake.calls[:]
    assert bbsigs.VerifyHashedBatchLocated(cv, sigs, pks, [b"h"] * 5, group=2, seed=SEED) == [True, False, True, True, True]
    assert fake.calls[1][1][4] == mag(_blake(b"h")) * 2


# ---- single calls ---------------------------------------------------------------------------------------------------------------
def test_single_verify_calls(fake):
    fake.script.update({"bgls_verify_aggregate": [1, 0], "bgls_verify_multi": [1, -2], "bgls_verify_aggregate_h": 1, "bgls_verify_multi_h": 1})
    keys, msgs = [g2(1), g2(2)], [b"", b"xy"]
    assert bgls._verify_agg(cv, g1(1), keys, msgs, False) is True and bgls.KoskVerifyAggregateSignature(cv, g1(1), keys, msgs) is False
    assert fake.calls == [("bgls_verify_aggregate", (cv.id, g1(1).raw, raws(keys), b"xy", [0, 0, 2], 2, 0)),
                          ("bgls_verify_aggregate", (cv.id, g1(1).raw, raws(keys), b"\x01\x01xy", [0, 1, 4], 2, 1))]
    del fake.calls[:]
    assert bgls._verify_multi(cv, g1(1), keys, b"m") is True and bgls.KoskVerifySingleSignature(cv, g1(1), g2(1), b"m") is False
    assert fake.calls == [("bgls_verify_multi", (cv.id, g1(1).raw, raws(keys), 2, b"m", 1)), ("bgls_verify_multi", (cv.id, g1(1).raw, g2(1).raw, 1, b"\x01m", 2))]
    del fake.calls[:]
    assert bgls._verify_agg(cv, g1(1), keyset(n=2), msgs, True) is True and bgls._verify_multi(cv, g1(1), keyset(), b"m") is True
    assert fake.calls == [("bgls_verify_aggregate_h", (77, g1(1).raw, b"xy", [0, 0, 2], 2, 1)), ("bgls_verify_multi_h", (77, g1(1).raw, b"m", 1))]
    del fake.calls[:]
    for sig, ks in ((None, keys), (FG1, keys), (g1(1), [g2(1), FG2]), (g1(1), [g2(1), None]), (g1(1), keyset(n=2, curve=other)), (g2(1), keys)):
        assert bgls._verify_agg(cv, sig, ks, msgs, True) is False and bgls._verify_multi(cv, sig, ks, b"m") is False
    assert bgls._verify_agg(cv, g1(1), keys, [b"m"], True) is False
    assert fake.calls == []


def test_grouped_hae_multiplicity_and_distinct_single_calls(fake):
    keys, msgs = [g2(1), g2(2)], [b"", b"xy"]
    for name in ("bgls_verify_aggregate_grouped", "bgls_verify_aggregate_hae", "bgls_verify_multi_hae", "bgls_verify_multi_multiplicity",
                 "bgls_verify_aggregate_distinct", "bgls_verify_aggregate_distinct_h"):
        fake.script[name] = [1, 0]
    assert bgls.VerifyAggregateSignatureGrouped(cv, g1(1), keys, msgs) is True
    assert bgls.KoskVerifyAggregateSignatureGrouped(cv, g1(1), keys, msgs) is False
    assert bgls.VerifyAggregateSignatureWithHAE(cv, g1(1), keys, msgs) is True
    assert bgls.VerifyMultiSignatureWithHAE(cv, g1(1), keys, b"m") is True
    assert bgls.KoskVerifyMultiSignatureWithMultiplicity(cv, g1(1), keys, [3, -1], b"m") is True
    assert bgls.DistinctMsgVerifyAggregateSignature(cv, g1(1), keys, msgs) is True
    assert bgls.DistinctMsgVerifyAggregateSignature(cv, g1(1), keyset(n=2), msgs) is True
    assert fake.calls == [
        ("bgls_verify_aggregate_grouped", (cv.id, g1(1).raw, raws(keys), b"xy", [0, 0, 2], 2, None, None)),
        ("bgls_verify_aggregate_grouped", (cv.id, g1(1).raw, raws(keys), b"\x01\x01xy", [0, 1, 4], 2, None, None)),
        ("bgls_verify_aggregate_hae", (cv.id, g1(1).raw, raws(keys), b"xy", [0, 0, 2], 2)),
        ("bgls_verify_multi_hae", (cv.id, g1(1).raw, raws(keys), 2, b"m", 1)),
        ("bgls_verify_multi_multiplicity", (cv.id, g1(1).raw, raws(keys), [3, -1], 2, b"\x01m", 2)),
        ("bgls_verify_aggregate_distinct", (cv.id, g1(1).raw, raws(keys), b"xy", [0, 0, 2], 2)),
        ("bgls_verify_aggregate_distinct_h", (77, g1(1).raw, b"xy", [0, 0, 2], 2, None))]
    del fake.calls[:]
    with pytest.raises(TypeError):
        bgls.VerifyAggregateSignatureGrouped(cv, g1(1), keyset(n=2), msgs)
    for sig, ks in ((None, keys), (FG1, keys), (g1(1), [g2(1), FG2]), (g1(1), [None, g2(1)])):
        assert bgls.VerifyAggregateSignatureGrouped(cv, sig, ks, msgs) is False
        assert bgls.VerifyAggregateSignatureWithHAE(cv, sig, ks, msgs) is False
        assert bgls.VerifyMultiSignatureWithHAE(cv, sig, ks, b"m") is False
        assert bgls.KoskVerifyMultiSignatureWithMultiplicity(cv, sig, ks, [1, 1], b"m") is False
        assert bgls.DistinctMsgVerifyAggregateSignature(cv, sig, ks, msgs) is False
    assert bgls.KoskVerifyMultiSignatureWithMultiplicity(cv, g1(1), keys, [1], b"m") is False
    assert fake.calls == []


def test_kosk_batch_multi_signature(fake):
    fake.script["bgls_verify_multi_batch"] = [1, 0]
    sigs, keys, msgs = [g1(1), g1(2)], [[g2(1), g2(2)], [g2(3)]], [b"", b"xy"]
    assert bgls.KoskVerifyBatchMultiSignature(cv, sigs, keys, msgs) is True and bgls.KoskVerifyBatchMultiSignature(cv, sigs, keys, msgs) is False
    assert fake.calls[0] == ("bgls_verify_multi_batch", (cv.id, raws(sigs), raws(k for ks in keys for k in ks), [0, 2, 3], 2, b"\x01\x01xy", [0, 1, 4], 1))
    del fake.calls[:]
    assert bgls.KoskVerifyBatchMultiSignature(cv, [], [], []) is False
    assert bgls.KoskVerifyBatchMultiSignature(cv, sigs, keys, msgs[:1]) is False
    assert bgls.KoskVerifyBatchMultiSignature(cv, [g1(1), FG1], keys, msgs) is False
    assert bgls.KoskVerifyBatchMultiSignature(cv, sigs, [[g2(1), FG2], [g2(3)]], msgs) is False
    assert bgls.KoskVerifyBatchMultiSignature(cv, [g2(1), g1(2)], keys, msgs) is False
    try:                                                 # a nil point: False like every sibling, or the AttributeError of old
        assert bgls.KoskVerifyBatchMultiSignature(cv, [g1(1), None], keys, msgs) is False
    except AttributeError:
        pass
    assert fake.calls == []


def test_hae_exponents_and_aggregate(fake):
    fake.script.update({"bgls_hae_exponents": [(0, (5).to_bytes(16, "big") + (1 << 127).to_bytes(16, "big")), -1],
                        "bgls_aggregate_signatures_hae": [(0, g1(9).raw), -2]})
    keys, sigs = [g2(1), g2(2)], [g1(1), g1(2)]
    assert bgls.hashPubKeysToExponents(keys) == [5, 1 << 127]
    assert fake.calls.pop() == ("bgls_hae_exponents", (cv.id, raws(keys), 2, bytes(32)))
    with pytest.raises(RuntimeError, match="^bgls_hae_exponents:"):
        bgls.hashPubKeysToExponents(keys)
    del fake.calls[:]
    assert bgls.hashPubKeysToExponents([]) == []
    for bad in ([g2(1), FG2], [FG2, g2(1)], [None], [g1(1)]):
        with pytest.raises(TypeError):
            bgls.hashPubKeysToExponents(bad)
    assert fake.calls == []
    got = bgls.AggregateSignaturesWithHAE(sigs, keys)
    assert (got.curve, got.group, got.raw) == (cv, G1, g1(9).raw)
    assert fake.calls == [("bgls_aggregate_signatures_hae", (cv.id, raws(sigs), raws(keys), 2, bytes(64)))]
    assert bgls.AggregateSignaturesWithHAE(sigs, keys) is None
    del fake.calls[:]
    assert bgls.AggregateSignaturesWithHAE(sigs, keys[:1]) is None
    assert bgls.AggregateSignaturesWithHAE([g1(1), FG1], keys) is None and bgls.AggregateSignaturesWithHAE(sigs, [g2(1), FG2]) is None
    assert fake.calls == []


def test_group_messages(fake):
    fake.script["bgls_group_messages"] = [0, 5]
    assert bgls.GroupMessages([b"a", b"", b"bc"]) == ([0, 0, 0], 0)
    assert fake.calls == [("bgls_group_messages", (b"abc", [0, 1, 1, 3], 3, [0, 0, 0], fake.calls[0][1][4]))]
    with pytest.raises(RuntimeError, match="^bgls_group_messages:"):
        bgls.GroupMessages([b"a"])


def test_key_set_upload_and_read(fake):
    keys = [g2(1), g2(2)]
    ks = bgls.KeySet(cv, keys)
    assert (ks.curve, ks.n, len(ks)) == (cv, 2, 2)
    assert fake.calls[0][1][:6] == (cv.id, raws(keys), 2, None, 1, 1)
    bgls.KeySet(cv, raws(keys), devices=[3, 1], check=False)
    assert fake.calls[1][1][:6] == (cv.id, raws(keys), 2, [3, 1], 2, 0)
    fake.script.update({"bgls_keys_upload": -2, "bgls_keys_read": [(0, raws(keys)), -1]})
    with pytest.raises(ValueError, match="^bgls_keys_upload: -2"):
        bgls.KeySet(cv, keys)
    del fake.calls[:]
    got = keyset(n=2).keys()
    assert fake.calls == [("bgls_keys_read", (77, 0, 2, bytes(256)))]
    assert [(p.curve, p.group, p.raw) for p in got] == [(cv, G2, k.raw) for k in keys]
    with pytest.raises(ValueError, match="^bgls_keys_read: -1"):
        keyset(n=2).keys()
    fake.script["bgls_keys_read"] = 0
    assert keyset(n=0).keys() == []


# ---- marshalling ---------------------------------------------------------------------------------------------------------------
SCALARS = [-5, (1 << 256) + 7, 1 << 256, 3, ORDER + 1, 0, -ORDER - 2]
MAGS = [ORDER - 5, ((1 << 256) + 7) % ORDER, (1 << 256) % ORDER, 3, ORDER + 1, 0, ORDER - 2]


def test_the_magnitudes_worked_out_here():
    assert [mag(k) for k in SCALARS] == [m.to_bytes(32, "big") for m in MAGS]


def test_secret_keys_and_scalars_travel_as_32_byte_magnitudes(fake, monkeypatch):
    n = len(SCALARS)
    want = b"".join(mag(k) for k in SCALARS)
    fake.script.update({"bgls_generator": (0, b"\7"), "bgls_scale_generator": (0, raws(g2(i) for i in range(n))), "bgls_sign_batch": (0, raws(g1(i) for i in range(n)))})
    got = bgls.LoadPublicKeys(cv, SCALARS)
    assert fake.to("bgls_scale_generator") == [(cv.id, G2, want, n, bytes(128 * n))]
    assert [(p.curve, p.group, p.raw) for p in got] == [(cv, G2, g2(i).raw) for i in range(n)]
    msgs = [b"", b"a", b"", b"bcd", b"e", b"f", b""]
    for kosk in (False, True):
        ms = [(b"\x01" if kosk else b"") + m for m in msgs]
        del fake.calls[:]
        got = bgls.SignBatch(cv, SCALARS, msgs, kosk=kosk)
        assert fake.to("bgls_sign_batch") == [(cv.id, want, b"".join(ms), offs(map(len, ms)), n, bytes(64 * n))]
        assert [(p.curve, p.group, p.raw) for p in got] == [(cv, G1, g1(i).raw) for i in range(n)]
    assert bgls.SignBatch(cv, SCALARS, msgs[:2]) is None and bgls.SignBatch(cv, [], []) == [] and bgls.LoadPublicKeys(cv, []) == []
    # Boneh-Boyen: both key scalars, and the exponent of a signature
    del fake.calls[:]
    fake.script["bgls_scale_generator"] = (0, g2(8).raw + g2(9).raw)
    pk = bbsigs.LoadPublicKey(cv, -5, (1 << 256) + 7)
    assert fake.to("bgls_scale_generator") == [(cv.id, G2, mag(-5) + mag((1 << 256) + 7), 2, bytes(256))]
    assert (pk.U.raw, pk.V.raw, pk.U.group, pk.V.curve) == (g2(8).raw, g2(9).raw, G2, cv)
    del fake.calls[:]
    fake.script["bgls_scale_generator"] = (0, g1(8).raw + g1(9).raw)
    exps = iter([(11, -5), (12, (1 << 256) + 7)])
    monkeypatch.setattr(bbsigs, "_sign_exponent", lambda curve, sk, m: next(exps))
    sigs = bbsigs.SignBatch(cv, [bbsigs.Privkey(1, 2)] * 2, [3, 4])
    assert fake.to("bgls_scale_generator") == [(cv.id, G1, mag(-5) + mag((1 << 256) + 7), 2, bytes(128))]
    assert [(s.Sigma.raw, s.Sigma.group, s.R) for s in sigs] == [(g1(8).raw, G1, 11), (g1(9).raw, G1, 12)]
    with pytest.raises(ValueError):
        bbsigs.SignBatch(cv, [bbsigs.Privkey(1, 2)], [])
    fake.script["bgls_scale_generator"] = -1
    for f in (lambda: bgls.LoadPublicKeys(cv, [1]), lambda: bbsigs.LoadPublicKey(cv, 1, 2)):
        with pytest.raises(RuntimeError, match="^bgls_scale_generator:"):
            f()
    fake.script["bgls_sign_batch"] = -1
    with pytest.raises(RuntimeError, match="^bgls_sign_batch:"):
        bgls.SignBatch(cv, [1], [b"m"])


def test_point_and_gt_scalars_travel_as_sign_and_magnitude(fake):
    fake.script.update({"bgls_scale_points": (0, g1(9).raw), "bgls_gt_pow": (0, GT[1])})
    for k, sign, m in ((-5, 1, 5), (5, 0, 5), (0, 0, 0), ((1 << 256) + 7, 0, ((1 << 256) + 7) % ORDER), (-(1 << 256), 1, (1 << 256) % ORDER),
                       (ORDER + 1, 0, ORDER + 1)):
        del fake.calls[:]
        p = g1(1).Mul(k)
        assert fake.calls == [("bgls_scale_points", (cv.id, G1, g1(1).raw, m.to_bytes(32, "big"), bytes([sign]), 1, bytes(64)))]
        assert (p.curve, p.group, p.raw) == (cv, G1, g1(9).raw)
        del fake.calls[:]
        t = PointT(cv, GT[0]).Mul(k)
        assert fake.calls == [("bgls_gt_pow", (cv.id, GT[0], m.to_bytes(32, "big"), sign, bytes(384)))] and t.raw == GT[1]
    del fake.calls[:]
    fake.script["bgls_scale_points"] = (0, g2(7).raw + g2(8).raw + g2(9).raw)
    pts = [g2(1), g2(2), g2(3)]
    got = curves.ScalePoints(pts, [-(1 << 256) - 7, None, 6])
    assert fake.calls == [("bgls_scale_points", (cv.id, G2, raws(pts), (((1 << 256) + 7) % ORDER).to_bytes(32, "big") + bytes(32) + (6).to_bytes(32, "big"),
                                                   bytes([1, 2, 0]), 3, bytes(384)))]
    assert [(p.curve, p.group, p.raw) for p in got] == [(cv, G2, g2(i).raw) for i in (7, 8, 9)]
    assert curves.ScalePoints(pts, None) is pts and curves.ScalePoints(pts, [1]) is None and curves.ScalePoints([], []) == []
    fake.script["bgls_scale_points"] = -1
    with pytest.raises(RuntimeError, match="^bgls_scale_points:"):
        curves.ScalePoints(pts, [1, 2, 3])
    with pytest.raises(RuntimeError, match="^bgls_scale_points:"):
        g1(1).Mul(2)


def test_aggregate_points(fake):
    fake.script["bgls_aggregate_points"] = [(0, g2(9).raw), -1]
    got = curves.AggregatePoints([g2(1), g2(2)])
    assert fake.calls == [("bgls_aggregate_points", (cv.id, G2, g2(1).raw + g2(2).raw, 2, bytes(128)))]
    assert (got.curve, got.group, got.raw) == (cv, G2, g2(9).raw)
    with pytest.raises(RuntimeError, match="^bgls_aggregate_points:"):
        curves.AggregatePoints([g1(1)])
    with pytest.raises(ValueError):
        curves.AggregatePoints([])


def test_hash_to_g1_offsets(fake):
    msgs = [b"", b"ab", b"", bytearray(b"cde"), b""]
    fake.script["bgls_hash_to_g1"] = [(0, raws(g1(i) for i in range(5))), (0, g1(7).raw), -1]
    got = cv.HashToG1Batch(msgs)
    assert fake.calls == [("bgls_hash_to_g1", (cv.id, b"abcde", [0, 0, 2, 2, 5, 5], 5, bytes(320)))]
    assert [(p.curve, p.group, p.raw) for p in got] == [(cv, G1, g1(i).raw) for i in range(5)]
    assert cv.HashToG1(b"").raw == g1(7).raw
    assert fake.calls[1] == ("bgls_hash_to_g1", (cv.id, b"\0", [0, 0], 1, bytes(64)))
    with pytest.raises(RuntimeError, match="^bgls_hash_to_g1:"):
        cv.HashToG1Batch([b"m"])


def test_hash_to_g1_keyed_offsets(fake):
    keys = [g2(1), g2(2), g2(3)]
    fake.script["bgls_hash_to_g1_keyed"] = [(0, raws(g1(i) for i in range(3))), 0, -1]
    got = cv.HashToG1Keyed(keys, [b"", b"abc", b""])
    assert [(p.curve, p.group, p.raw) for p in got] == [(cv, G1, g1(i).raw) for i in range(3)]
    cv.HashToG1Keyed(keys)
    assert fake.calls == [("bgls_hash_to_g1_keyed", (cv.id, 0, raws(keys), b"abc", [0, 0, 3, 3], 3, bytes(192))),
                          ("bgls_hash_to_g1_keyed", (cv.id, 1, raws(keys), None, None, 3, bytes(192)))]
    with pytest.raises(RuntimeError, match="^bgls_hash_to_g1_keyed:"):
        cv.HashToG1Keyed(keys)
    del fake.calls[:]
    with pytest.raises(ValueError, match="keys and msgs differ in length"):
        cv.HashToG1Keyed(keys, [b"a"])
    for bad in ([g2(1), FG2], [None], [g1(1)]):
        with pytest.raises(ValueError, match="HashToG1Keyed takes G2 Points of this curve"):
            cv.HashToG1Keyed(bad)
    assert fake.calls == []


def test_kosk_prefix_on_the_single_path(fake):
    fake.script.update({"bgls_hash_to_g1": (0, g1(3).raw), "bgls_scale_points": (0, g1(4).raw), "bgls_verify_multi": 1})
    assert bgls.KoskSign(cv, 5, b"m").raw == g1(4).raw
    assert fake.calls[0] == ("bgls_hash_to_g1", (cv.id, b"\x01m", [0, 2], 1, bytes(64)))
    del fake.calls[:]
    assert bgls.KoskVerifyMultiSignature(cv, g1(1), [g2(1)], b"m") is True and bgls.MultiSig([g2(1)], g1(1), b"m").Verify(cv) is True
    assert bgls.KoskVerifyMultiSignatureWithMultiplicity(cv, g1(1), [g2(1)], None, bytearray(b"m")) is True
    assert fake.calls == [("bgls_verify_multi", (cv.id, g1(1).raw, g2(1).raw, 1, b"\x01m", 2))] * 3


# ---- the public surface --------------------------------------------------------------------------------------------------------
PUBLIC = {
    bgls: ['AggSig', 'AggregateKeys', 'AggregateKeysBySubset', 'AggregateSignatures', 'AggregateSignaturesWithHAE',
           'AmsAggregateMembershipKeyShares', 'AmsCombineSignatureShares', 'AmsCreateMembershipKeyShares', 'AmsCreateMembershipKeySharesKnownExp',
           'AmsCreateSignatureShare', 'AmsVerifySignature', 'AmsVerifySignatureWithSetCheck', 'AmsVerifySignatures', 'Authenticate',
           'CheckAuthentication', 'CheckAuthentications', 'DistinctMsgSign', 'DistinctMsgVerifyAggregateSignature',
           'DistinctMsgVerifyAggregateSignatures', 'DistinctMsgVerifySingleSignature', 'DistinctMsgVerifySingleSignatures', 'G1', 'G2',
           'GroupMessages', 'KeyGen', 'KeySet', 'KoskSign', 'KoskVerifyAggregateSignature', 'KoskVerifyAggregateSignatureGrouped',
           'KoskVerifyAggregateSignatureGroupedBySubset', 'KoskVerifyAggregateSignatures', 'KoskVerifyBatchMultiSignature',
           'KoskVerifyBatchMultiSignatureStepwise', 'KoskVerifyMultiSignature', 'KoskVerifyMultiSignatureWithMultiplicity',
           'KoskVerifyMultiSignatures', 'KoskVerifyMultiSignaturesBySubset', 'KoskVerifyMultiSignaturesCombined', 'KoskVerifySingleSignature',
           'KoskVerifySingleSignatures', 'LoadPublicKey', 'LoadPublicKeys', 'MultiSig', 'Sign', 'SignBatch', 'VerifyAggregateSignature',
           'VerifyAggregateSignatureGrouped', 'VerifyAggregateSignatureGroupedBySubset', 'VerifyAggregateSignatureWithHAE',
           'VerifyAggregateSignatures', 'VerifyBatchMultiSignatureWithHAE', 'VerifyMultiSignatureWithHAE', 'VerifyMultiSignatures',
           'VerifyMultiSignaturesBySubset', 'VerifyMultiSignaturesCombined', 'VerifyMultiSignaturesLocated', 'VerifyMultiSignaturesWithHAE',
           'VerifySingleSignature', 'VerifySingleSignatures', 'hashPubKeysToExponents'],
    bbsigs: ['G1', 'G2', 'KeyGen', 'LoadPublicKey', 'Privkey', 'Pubkey', 'Sign', 'SignBatch', 'SignCustHash', 'SignHashed', 'Signature', 'Verify',
             'VerifyBatch', 'VerifyBatchCombined', 'VerifyBatchLocated', 'VerifyCustHash', 'VerifyHashed', 'VerifyHashedBatch',
             'VerifyHashedBatchCombined', 'VerifyHashedBatchLocated', 'blake2b256'],
    curves: ['ALTBN128', 'AggregatePoints', 'Altbn128', 'BLS12_381', 'Bls12', 'CurveSystem', 'G1', 'G2', 'Point', 'PointT', 'ScalePoints'],
}


@pytest.mark.parametrize("mod", list(PUBLIC), ids=lambda m: m.__name__)
def test_public_names(mod):
    """the module's own public names: what it defines, and its constants (modules and names imported from a sibling are not its surface)"""
    own = sorted(n for n, v in vars(mod).items() if not n.startswith("_") and not isinstance(v, types.ModuleType)
                 and getattr(v, "__module__", mod.__name__) == mod.__name__)
    assert own == PUBLIC[mod]


def test_names_that_tests_and_tools_reach_through_the_modules():
    assert callable(bgls._verify_agg) and callable(bgls._verify_multi) and callable(bgls._subset_rows) and callable(bgls._group_offsets)
    assert bgls.AggregatePoints is curves.AggregatePoints and bgls.ScalePoints is curves.ScalePoints and bgls.Point is Point
