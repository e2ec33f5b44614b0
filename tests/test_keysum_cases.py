"""CPU tier: the layouts of tests/keysum_cases.py sit where their names say, cover what they promise, and are pinned against the C
oracle's additions before any GPU sees them."""
import pytest

import keysum_cases as kc
from oracle import coracle


def g2(cid):
    from oracle.pyref.params import BN254, BLS381
    from oracle.pyref.groups import Groups
    cv = BN254 if cid == 0 else BLS381
    return Groups(cv).g2_bytes(cv.g2)


def oracle_scale(cid):
    g = g2(cid)
    return lambda scalars: [coracle.scale_point(cid, 2, g, s) for s in scalars]


def exceptional(lay, r, T, stage="tree"):
    return {(ad.stage, ad.level, ad.where, kc.kind_of(ad, r)) for ad in kc.run(lay, r, T, stage)[0] if kc.kind_of(ad, r) in kc.EXCEPTIONAL}


def test_the_model_on_a_hand_made_layout():
    """five keys on one block: pair 0 adds keys 0 alone ... and the levels join pair 4 into 0 (s = 4), 2 into 0 and 3 into 1 (s = 2), 1 into 0"""
    r = 101
    adds, total = kc.run([1, 2, 3, 4, 5], r, 32)
    assert total == 15
    real = [(a.stage, a.level, a.where, a.a, a.b) for a in adds if a.a_keys and a.b_keys]
    assert real == [("block", 4, 0, 1, 5), ("block", 2, 0, 6, 3), ("block", 2, 1, 2, 4), ("block", 1, 0, 9, 6)]
    assert len(adds) == 5 + 31
    # 300 keys: three blocks, pair t adds t, t + 96, ...; blocks 0 and 1 meet first, block 2 passes through to the root
    adds, total = kc.run(list(range(1, 301)), 10 ** 9, kc.whole_pairs(300))
    assert kc.whole_pairs(300) == 96 and total == 300 * 301 // 2
    assert [(a.level, a.where, a.b) for a in adds if a.stage == "main" and a.where == 5] == [(0, 5, 6), (1, 5, 102), (2, 5, 198), (3, 5, 294)]
    tree = [a for a in adds if a.stage == "tree"]
    assert [(a.level, a.where) for a in tree] == [(0, 0), (1, 0)] and min(tree[1].b_keys) == 64 and len(tree[1].b_keys) == 96
    assert kc.seg_pairs(64, 200) == 32 and kc.seg_pairs(127, 1) == 32 and kc.seg_pairs(128, 1) == 64 and kc.seg_pairs(512, 37) == 256
    assert kc.tree_nodes(5) == [(0, 0), (0, 1), (1, 0), (2, 0)] and len(kc.tree_nodes(8)) == 7


@pytest.mark.parametrize("cid", [0, 1])
def test_every_case_sits_where_its_name_says(cid):
    """the model's additions contain every target with its kind, and no exceptional addition that a target does not force"""
    r = kc.ORDER[cid]
    for c in kc.catalogue(cid):
        assert c.T == kc.whole_pairs(c.n) and len(c.layout) == c.n
        assert kc.unexplained(c.layout, r, c.T, c.targets) == [], c.name
        got = exceptional(c.layout, r, c.T)
        assert {tuple(t) for t in c.targets} <= got, c.name
        if not c.targets:
            assert got == set(), c.name
        if c.family == "block" and c.n == 64:                         # both operands are sums of at least two keys, all different
            ad = kc.find(kc.run(c.layout, r, c.T)[0], c.targets[0])
            assert len(ad.a_keys) >= 2 and len(ad.b_keys) >= 2 and len({c.layout[k] for k in ad.a_keys + ad.b_keys}) >= 3, c.name
    for (sets, P) in kc.segmented_calls(cid):
        assert P == kc.seg_pairs(max(len(s[1]) for s in sets), len(sets))
        for name, lay, targets in sets:
            assert kc.unexplained(lay, r, P, targets, "coop") == [], name
        offs = [sum(len(s[1]) for s in sets[:i]) for i in range(len(sets))]
        assert sum(1 for o in offs if o % 32) * 10 >= 9 * len(offs), "the sets should lie at offsets that are no multiples of 32"
        assert any(len(s[1]) == 0 for s in sets) and any(s[1] == [kc.INF] for s in sets)


@pytest.mark.parametrize("cid", [0, 1])
def test_the_catalogue_covers_every_place(cid):
    cases = kc.catalogue(cid)
    names = {c.name for c in cases}
    assert len(names) == len(cases)
    spots = {}
    for c in cases:
        for t in c.targets:
            spots.setdefault(c.family, set()).add((c.n,) + tuple(t))
    # main loop: every named case at in-block pairs 0, 15, 16, 31
    for t in kc.MAIN_PAIRS:
        for case in kc.MAIN_CASES:
            assert "main-%s-pair%d" % (case, t) in names
    want_main = {("second_equal", (1, "equal")), ("second_opposite", (1, "opposite")), ("second_opposite", (2, "a_inf")), ("inf_first", (1, "a_inf")),
                 ("inf_middle", (2, "b_inf")), ("inf_last", (3, "b_inf")), ("third_is_sum", (2, "equal")), ("all_equal", (1, "equal"))}
    for case, (j, kind) in want_main:
        for t in kc.MAIN_PAIRS:
            assert (128, "main", j, t, kind) in spots["main"], (case, t)
    # all_equal: the four keys of the pair are one key
    for c in cases:
        if c.name.startswith("main-all_equal"):
            t = c.targets[0].where
            assert len({c.layout[t + 32 * j] for j in range(4)}) == 1
    # block tree: every (level, kind) at pair 0, pair s - 1 and an inner pair, at n = 32 and n = 64
    for n in (32, 64):
        for s in kc.LEVELS:
            for kind in kc.EXCEPTIONAL:
                for p in {0, s - 1} | ({s // 2} if s >= 4 else set()):
                    assert (n, "block", s, p, kind) in spots["block"], (n, s, kind, p)
    for s in kc.LEVELS:
        hit = {(t[3], t[4]) for t in spots["block-all"] if t[2] == s}
        assert {p for p, _ in hit} == set(range(s)) and (s < 4 or len({k for _, k in hit}) >= 3), s
    assert len({t[2] for t in spots["block-two"]}) == 2
    # ragged blocks
    for n in kc.RAGGED:
        assert {x for x in names if x.startswith("ragged-n%d" % n) and (x + "-").startswith("ragged-n%d-" % n)} == (
            {"ragged-n1"} if n == 1 else {"ragged-n%d-equal" % n, "ragged-n%d-opposite" % n})
    # trees: every inner node (the pass-through node of W = 3 and W = 5 is the b operand of their last node) with every kind, and the root
    for n in kc.TREE_N:
        W = n // 128
        nodes, cnt, level = set(), W, 0
        while cnt > 1:
            nodes |= {(level, i) for i in range(cnt // 2)}
            cnt, level = (cnt + 1) // 2, level + 1
        assert len(nodes) == W - 1
        for level, i in nodes:
            for kind in kc.NODE_KINDS:
                assert (n, "tree", level, i, kind) in spots["tree"], (n, level, i, kind)
        assert "tree-n%d-root-infinity" % n in names
    r = kc.ORDER[cid]
    for n, passed in ((384, 2), (640, 4)):                              # the last node's b operand is the block that passed through
        c = next(c for c in cases if c.n == n and c.family == "tree-root")
        ad = kc.find(kc.run(c.layout, r, c.T)[0], c.targets[0])
        assert set(ad.b_keys) == {k for k in range(n) if (k % c.T) // 32 == passed} and kc.run(c.layout, r, c.T)[1] == 0
    # segmented: every node of the three k_sum_coop levels with every kind at 256 keys, every node at 512
    (_, P0), (call1, P1) = kc.segmented_calls(cid)
    got = {(len(lay),) + tuple(t) for _, lay, tg in call1 for t in tg}
    for level, i in kc.tree_nodes(8):
        for kind in kc.NODE_KINDS:
            assert (256, "coop", level, i, kind) in got
        assert any(g[:4] == (512, "coop", level, i) for g in got)


@pytest.mark.parametrize("cid", [0, 1])
def test_the_layouts_against_the_oracles_additions(cid):
    """(sum of the scalars) g2 equals the oracle's sequential AggregatePoints over the wire keys, for every layout"""
    r, g, PT = kc.ORDER[cid], g2(cid), 4 * kc.FP[cid]
    lays = [(c.name, c.layout) for c in kc.catalogue(cid)] + [(n, lay) for sets, _ in kc.segmented_calls(cid) for n, lay, _ in sets]
    infinities = 0
    for name, lay in lays:
        keys = b"".join(kc.wire_keys(cid, lay, oracle_scale(cid)))
        total = sum(lay) % r
        want = coracle.scale_point(cid, 2, g, total) if total else bytes(PT)
        assert coracle.aggregate_points(cid, 2, keys, len(lay)) == want, name
        infinities += total == 0
    assert infinities >= 8                                              # the roots at infinity, the empty set, the sets of one infinity


@pytest.mark.parametrize("cid", [0, 1])
def test_half_equal_x_points(cid):
    """the fixture's points are on the twist, outside the subgroup, share half of x -- and the C oracle adds such points by the generic
    law: the same bytes as the Python oracle's affine additions"""
    from oracle.pyref.params import BN254, BLS381
    from oracle.pyref.groups import Groups
    G = Groups(BN254 if cid == 0 else BLS381)
    pts = kc.half_equal_points(cid)
    (a, b), (c, d) = [[G.g2_from_bytes(x) for x in pts[k]] for k in ("re", "im")]
    assert a[0][0] == b[0][0] and a[0][1] != b[0][1] and c[0][1] == d[0][1] and c[0][0] != d[0][0]
    for q in (a, b, c, d):
        assert G.g2_on_curve(q) and coracle.g2_in_subgroup(cid, G.g2_bytes(q)) == 0
    fill = kc.wire_keys(cid, kc.pool(cid)[:64], oracle_scale(cid))
    lays = kc.half_equal_layouts(cid, fill)
    assert len(lays) == 10
    for name, lay in lays:
        want = G.g2_bytes(G.g2_sum([G.g2_from_bytes(k) for k in lay]))
        assert coracle.aggregate_points(cid, 2, b"".join(lay), len(lay)) == want, name
