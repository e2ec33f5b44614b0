"""GPU tier: the G2 key sums at the exceptional cases of the group law, placed by schedule (tests/keysum_cases.py: which addition of
which level of which kernel meets equal, opposite or vanished operands is decided in advance and checked by the CPU tier against a scalar
model of the launch).  Everything is byte equality with (sum of the secret keys) g2 from the C oracle, or a verdict: through
bgls_aggregate_points / _dev (also in throughput mode), bgls_aggregate_sets, key sets (bgls_verify_multi_h, bgls_verify_multi_keys_dev,
one, two and four shards), bgls_aggregate_subsets_h in every complement mode, and the grouped verifications."""
import ctypes
import types

import pytest

import keysum_cases as kc
from oracle import coracle

pytestmark = pytest.mark.gpu


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def out(n):
    return (ctypes.c_uint8 * max(1, n))()


def offs(counts):
    o = (ctypes.c_uint64 * (len(counts) + 1))()
    for i, c in enumerate(counts):
        o[i + 1] = o[i] + c
    return o


_S = {}


def session(lib, cid, fp):
    """per curve, once: the generator, the engine's key generation behind keysum_cases.wire_keys, the expected points by scalar"""
    if cid in _S:
        return _S[cid]
    g2 = out(4 * fp)
    assert lib.bgls_generator(cid, 2, g2) == 0
    g2 = bytes(g2)
    PT, r = 4 * fp, kc.ORDER[cid]

    def scale_many(scalars):
        o = out(len(scalars) * PT)
        assert lib.bgls_scale_generator(cid, 2, B(b"".join(s.to_bytes(32, "big") for s in scalars)), len(scalars), o) == 0
        o = bytes(o)
        return [o[i * PT:(i + 1) * PT] for i in range(len(scalars))]

    points = {0: bytes(PT)}

    def point(total):
        total %= r
        if total not in points:
            points[total] = coracle.scale_point(cid, 2, g2, total)
        return points[total]

    s = types.SimpleNamespace(cid=cid, fp=fp, PT=PT, r=r, g2=g2, point=point, scale_many=scale_many, handles={},
                              keys=lambda lay: b"".join(kc.wire_keys(cid, lay, scale_many)))
    # the engine's generator against the oracle's on a few scalars: everything below rests on sk * g2 being the oracle's point
    probe = kc.pool(cid)[:3] + [1, r - 1]
    assert scale_many(probe) == [coracle.scale_point(cid, 2, g2, k) for k in probe]
    _S[cid] = s
    return s


def placed_key(case_layout, targets, r, T, stage="tree"):
    """the key the builder solved for (the last one under the operand that moved); where that key is the point at infinity, the last
    key under the target that is not; key 0 for a layout without a target"""
    if not targets:
        return 0
    tg = targets[0]
    ad = kc.find(kc.run(case_layout, r, T, stage)[0], tg)
    j = max(ad.a_keys) if tg.kind == "a_inf" else max(ad.b_keys)
    if case_layout[j] == 0:
        live = [k for k in ad.a_keys + ad.b_keys if case_layout[k]]
        j = max(live) if live else next((k for k, v in enumerate(case_layout) if v), 0)
    return j


def aggregate(lib, s, keys, n):
    o = out(s.PT)
    assert lib.bgls_aggregate_points(s.cid, 2, B(keys), n, o) == 0
    return bytes(o)


def aggregate_dev_all(lib, s, blobs):
    """bgls_aggregate_points_dev on every (keys, n) from one device buffer; the results after one synchronisation"""
    import torch
    flat = b"".join(k for k, _ in blobs)
    d_in = torch.frombuffer(bytearray(flat or b"\0"), dtype=torch.uint8).to("cuda:0")
    d_out = torch.zeros(len(blobs) * s.PT, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    at = 0
    for i, (k, n) in enumerate(blobs):
        assert lib.bgls_aggregate_points_dev(s.cid, 2, d_in.data_ptr() + at, n, d_out.data_ptr() + i * s.PT, None) == 0
        at += len(k)
    torch.cuda.synchronize()
    res = bytes(d_out.cpu().numpy().tobytes())
    return [res[i * s.PT:(i + 1) * s.PT] for i in range(len(blobs))]


def test_whole_sums(gpu_lib, curve):
    """bgls_aggregate_points and bgls_aggregate_points_dev on every layout of the catalogue, alone and in throughput mode"""
    lib, s = gpu_lib, session(gpu_lib, curve["id"], curve["fp"])
    cases = kc.catalogue(s.cid)
    blobs = [(s.keys(c.layout), c.n) for c in cases]
    want = [s.point(sum(c.layout)) for c in cases]
    for c, (k, n), w in zip(cases, blobs, want):
        if c.n <= 128:
            assert coracle.aggregate_points(s.cid, 2, k, n) == w, c.name
    assert sum(w == bytes(s.PT) for w in want) >= 6
    try:
        for mode in (0, 1):
            assert lib.bgls_set_throughput_mode(mode) == 0
            for c, (k, n), w in zip(cases, blobs, want):
                assert aggregate(lib, s, k, n) == w, (c.name, mode)
            for c, got, w in zip(cases, aggregate_dev_all(lib, s, blobs), want):
                assert got == w, (c.name, mode, "device form")
    finally:
        lib.bgls_set_throughput_mode(0)


def test_segmented_sums(gpu_lib, curve):
    """bgls_aggregate_sets: the one-block layouts as sets of one call at odd offsets (P = 32), and sets of 256 and 512 keys whose eight
    block partials are equal, opposite or vanished at every node of k_sum_coop's levels (P = 256); an empty set and a set of one
    infinity in each call"""
    lib, s = gpu_lib, session(gpu_lib, curve["id"], curve["fp"])
    for sets, P in kc.segmented_calls(s.cid):
        assert kc.seg_pairs(max(len(lay) for _, lay, _ in sets), len(sets)) == P
        flat = b"".join(s.keys(lay) for _, lay, _ in sets)
        o = out(len(sets) * s.PT)
        assert lib.bgls_aggregate_sets(s.cid, 2, B(flat), offs([len(lay) for _, lay, _ in sets]), len(sets), o) == 0
        o = bytes(o)
        for i, (name, lay, _) in enumerate(sets):
            assert o[i * s.PT:(i + 1) * s.PT] == s.point(sum(lay)), (name, P)


def test_half_equal_x(gpu_lib, curve):
    """Two twist points whose x agree in one half only, meeting in jacp_madd, at level 16 and at level 1 of the block tree: one lane's half
    of H is zero, the other's is not, and the addition is an ordinary one.  Reference: the C oracle's additions (the points are outside
    the subgroup, so there is no scalar; the CPU tier pins the oracle against the Python oracle's affine law on these layouts)."""
    lib, s = gpu_lib, session(gpu_lib, curve["id"], curve["fp"])
    lays = kc.half_equal_layouts(s.cid, kc.wire_keys(s.cid, kc.pool(s.cid)[:64], s.scale_many))
    blobs = [(b"".join(lay), len(lay)) for _, lay in lays]
    want = [coracle.aggregate_points(s.cid, 2, k, n) for k, n in blobs]
    assert all(w != bytes(s.PT) for w in want)
    for (name, _), (k, n), w in zip(lays, blobs, want):
        assert aggregate(lib, s, k, n) == w, name
    for (name, _), got, w in zip(lays, aggregate_dev_all(lib, s, blobs), want):
        assert got == w, (name, "device form")
    o = out(len(lays) * s.PT)
    assert lib.bgls_aggregate_sets(s.cid, 2, B(b"".join(k for k, _ in blobs)), offs([n for _, n in blobs]), len(lays), o) == 0
    assert bytes(o) == b"".join(want)


# ------------------------------------------------------------------------------------------------ key sets
def upload(lib, s, keys, n, shards=1):
    h = ctypes.c_uint64()
    assert lib.bgls_keys_upload(s.cid, B(keys), n, (ctypes.c_int * shards)(*([0] * shards)), shards, 0, ctypes.byref(h)) == 0
    return h.value


def handle(lib, s, c):
    """the one-shard key set of a case (flags 0: the sums then run over its sum-ready records), uploaded once"""
    if c.name not in s.handles:
        s.handles[c.name] = upload(lib, s, s.keys(c.layout), c.n)
    return s.handles[c.name]


def signatures(lib, s, cases):
    """per case (message, signature of sum sk, signature of sum sk + sk_j with j the placed key, the two verdicts to expect): 1 and 0,
    and the oracle's wherever a scalar is 0 mod r (a key sum or a signature at infinity)"""
    msgs = [("key sum " + c.name).encode().ljust(48, b".") for c in cases]
    good = [sum(c.layout) % s.r for c in cases]
    off = [c.layout[placed_key(c.layout, c.targets, s.r, c.T)] or 1 for c in cases]
    bad = [(g + d) % s.r for g, d in zip(good, off)]
    scal = good + bad
    sg = out(len(scal) * 2 * s.fp)
    assert lib.bgls_sign_batch(s.cid, B(b"".join((k or 1).to_bytes(32, "big") for k in scal)), B(b"".join(msgs + msgs)), offs([48] * len(scal)), len(scal), sg) == 0
    sg = bytes(sg)
    sigs = [sg[i * 2 * s.fp:(i + 1) * 2 * s.fp] if scal[i] else bytes(2 * s.fp) for i in range(len(scal))]
    rows = []
    for i, c in enumerate(cases):
        sig_g, sig_b = sigs[i], sigs[len(cases) + i]
        want_g, want_b = 1, 0
        if good[i] == 0 or bad[i] == 0:
            keys = s.keys(c.layout)
            want_g, want_b = (coracle.verify_multi(s.cid, x, keys, c.n, msgs[i]) for x in (sig_g, sig_b))
        rows.append((msgs[i], sig_g, sig_b, want_g, want_b))
    return rows


def verify_one_shard(lib, s, cases):
    import torch
    rows = signatures(lib, s, cases)
    d = torch.frombuffer(bytearray(b"".join(m + g + b for m, g, b, _, _ in rows)), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    step, G1 = 48 + 4 * s.fp, 2 * s.fp
    zero_totals = 0
    for i, (c, (m, sig_g, sig_b, want_g, want_b)) in enumerate(zip(cases, rows)):
        h = handle(lib, s, c)
        assert lib.bgls_verify_multi_h(h, B(sig_g), B(m), 48) == want_g, c.name
        assert lib.bgls_verify_multi_h(h, B(sig_b), B(m), 48) == want_b, (c.name, "a signature off by the placed key")
        p = d.data_ptr() + i * step
        assert lib.bgls_verify_multi_keys_dev(h, p + 48, p, 48, None) == want_g, (c.name, "device form")
        assert lib.bgls_verify_multi_keys_dev(h, p + 48 + G1, p, 48, None) == want_b, (c.name, "device form, off by the placed key")
        zero_totals += sum(c.layout) % s.r == 0
    return zero_totals


@pytest.mark.parametrize("family", ["main", "block", "tree"])
def test_key_sets_verify(gpu_lib, curve, family):
    """every whole-sum layout as a one-shard key set: the right signature is accepted, the one off by the placed key refused"""
    lib, s = gpu_lib, session(gpu_lib, curve["id"], curve["fp"])
    pick = {"main": ("main", "ragged"), "block": ("block", "block-all", "block-two"), "tree": ("tree", "tree-root")}[family]
    cases = [c for c in kc.catalogue(s.cid) if c.family in pick]
    assert sum(len([c for c in kc.catalogue(s.cid) if c.family in f]) for f in (("main", "ragged"), ("block", "block-all", "block-two"), ("tree", "tree-root"))) == len(kc.catalogue(s.cid))
    zero = verify_one_shard(lib, s, cases)
    assert zero >= (4 if family == "tree" else 1 if family == "block" else 0)


def test_key_sets_in_shards(gpu_lib, curve):
    """the layouts of two and more blocks as key sets of two and four shards on one device: the per-shard sums see other cuts"""
    lib, s = gpu_lib, session(gpu_lib, curve["id"], curve["fp"])
    cases = [c for c in kc.catalogue(s.cid) if c.n >= 256]
    rows = signatures(lib, s, cases)
    for c, (m, sig_g, sig_b, want_g, want_b) in zip(cases, rows):
        for shards in (2, 4):
            h = upload(lib, s, s.keys(c.layout), c.n, shards)
            try:
                assert lib.bgls_verify_multi_h(h, B(sig_g), B(m), 48) == want_g, (c.name, shards)
                assert lib.bgls_verify_multi_h(h, B(sig_b), B(m), 48) == want_b, (c.name, shards, "off by the placed key")
            finally:
                assert lib.bgls_keys_free(h) == 0


@pytest.mark.parametrize("family", ["main", "block"])
def test_subsets(gpu_lib, curve, family):
    """bgls_aggregate_subsets_h over the key sets of the layouts of at most 128 keys (one block, entries in key order: the whole sum's
    schedule): a row that selects the whole layout, one without the placed key, one without key 0 -- in every complement mode.  Forced
    complement turns the rows into -key + TOTAL; where the total is the point at infinity the whole-set record is an infinity entry."""
    lib, s = gpu_lib, session(gpu_lib, curve["id"], curve["fp"])
    pick = {"main": ("main", "ragged"), "block": ("block", "block-all", "block-two")}[family]
    cases = [c for c in kc.catalogue(s.cid) if c.family in pick]
    assert all(c.n <= 128 and c.T == 32 for c in cases)
    zero_totals = 0
    for c in cases:
        h, total = handle(lib, s, c), sum(c.layout) % s.r
        j = placed_key(c.layout, c.targets, s.r, c.T)
        subsets = [list(range(c.n)), [i for i in range(c.n) if i != j], list(range(1, c.n))]
        want = s.point(total) + s.point(total - c.layout[j]) + s.point(total - c.layout[0])
        stride = (c.n + 7) // 8
        rows = bytearray(stride * 3)
        for b, sub in enumerate(subsets):
            for i in sub:
                rows[b * stride + (i >> 3)] |= 1 << (i & 7)
        try:
            for mode in (0, 1, 2):
                assert lib.bgls_set_subset_complement(mode) == 0
                o = out(3 * s.PT)
                assert lib.bgls_aggregate_subsets_h(h, B(rows), stride, 3, o) == 0
                assert bytes(o) == want, (c.name, mode)
        finally:
            lib.bgls_set_subset_complement(0)
        zero_totals += total == 0
    assert family != "block" or zero_totals >= 1                      # a key set whose total is infinity, complement forced among the modes


# ------------------------------------------------------------------------------------------------ grouped
def test_grouped(gpu_lib, curve):
    """Instances of at most 64 signers (the index list is then in signer order: keysum_cases) whose groups are a block-tree layout for
    s = 16 or s = 1, K twice, K with -K, three keys with the third the sum of the first two, and two infinities:
    bgls_verify_aggregate_grouped on the wire keys, bgls_verify_aggregate_grouped_h over the key set with bgls_set_group_small at 0
    (one-item k_sumpairidx_main: block tree) and at its default (k_sumpairgrp_main: serial).  Verdicts from the C oracle, for the
    right signature and for one off by the placed key."""
    lib, s = gpu_lib, session(gpu_lib, curve["id"], curve["fp"])
    byname = {c.name: c for c in kc.catalogue(s.cid)}
    pl = kc.pool(s.cid)
    for inst, name in enumerate(("block-n32-s16-equal-pair8", "block-n32-s16-opposite-pair0", "block-n32-s1-equal-pair0", "block-n32-s1-opposite-pair0",
                                 "block-n32-s16-a_inf-pair15", "block-n32-s1-b_inf-pair0")):
        c = byname[name]
        k, k2, a, b = pl[900 + 4 * inst:904 + 4 * inst]
        groups = [list(c.layout), [k, k], [k2, s.r - k2], [a, b, (a + b) % s.r], [kc.INF, kc.INF]]
        sks = [x for g in groups for x in g]
        assert len(sks) == 41
        gm = [("grouped %d %d" % (inst, g)).encode().ljust(32, b"-") for g in range(len(groups))]
        msgs = [gm[g] for g, grp in enumerate(groups) for _ in grp]
        keys = s.keys(sks)
        sums = [sum(g) % s.r for g in groups]
        off = list(sums)
        off[0] = (off[0] + (c.layout[placed_key(c.layout, c.targets, s.r, 32)] or 1)) % s.r
        sigs = []
        for scal in (sums, off):
            live = [(x, m) for x, m in zip(scal, gm) if x]
            parts = out(len(live) * 2 * s.fp)
            assert lib.bgls_sign_batch(s.cid, B(b"".join(x.to_bytes(32, "big") for x, _ in live)), B(b"".join(m for _, m in live)), offs([32] * len(live)), len(live), parts) == 0
            agg = out(2 * s.fp)
            assert lib.bgls_aggregate_sets(s.cid, 1, parts, offs([len(live)]), 1, agg) == 0
            sigs.append(bytes(agg))
        want = [coracle.verify_aggregate(s.cid, sig, keys, msgs, allow_dups=True) for sig in sigs]
        assert want == [1, 0], (name, want)
        h = upload(lib, s, keys, len(sks))
        try:
            for sig, w in zip(sigs, want):
                d = ctypes.c_size_t(0)
                assert lib.bgls_verify_aggregate_grouped(s.cid, B(sig), B(keys), B(b"".join(msgs)), offs([32] * len(msgs)), len(msgs), ctypes.byref(d), None) == w, name
                assert d.value == len(groups)
                try:
                    for small in (0, 32):
                        assert lib.bgls_set_group_small(small) == 0
                        assert lib.bgls_verify_aggregate_grouped_h(h, B(sig), None, 0, B(b"".join(msgs)), offs([32] * len(msgs)), len(msgs), ctypes.byref(d), None) == w, (name, small)
                finally:
                    lib.bgls_set_group_small(32)
        finally:
            assert lib.bgls_keys_free(h) == 0
