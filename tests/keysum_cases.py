"""Shared by the tests of the G2 key sums at the exceptional cases of the group law (tests/test_keysum_cases.py, the CPU tier, and
tests/test_gpu_keysum_edges.py): key layouts PLACED BY SCHEDULE, and the schedule itself as a scalar model.

Every key is sk * g2, so a layout is a list of scalars mod r and a partial sum is a scalar: "equal" is the same scalar, "opposite" the
negated one, "infinity" is 0 -- and the entry 0 of a layout is the wire point at infinity (all-zero bytes).  The model replays the order
in which the kernels add, as plain Python written from the code:

  whole sum (Engine::sum_points_jac, engine_core.inc:1322-1395; bgls_aggregate_points, _dev, the per-shard sums of a key set)
      W = ceil(n / 128) one-wave blocks (engine_core.inc:1334, capped at 2048, in throughput mode 1024: far above every n used here),
      T = 32 W lane pairs.  Pair t starts at infinity and adds keys t, t + T, t + 2T, ... in that order (k_sumpair_main,
      k_sumpair.hip:165-180; jacp_madd, rx_jacpair.hpp:80-111).  In block b, level s = 16, 8, 4, 2, 1 adds the sum of in-block pair
      p + s into that of pair p, for p < s (sumpair_block_tree, k_sumpair.hip:86-162).  The W block partials go up a binary tree in
      index order, node i of a level = node 2i + node 2i + 1 of the level below, an unpaired last node passes through
      (k_sum_tree_x, k_sumtree.hip:203-236; which of the two is the accumulator of the kernel's add() is decided by arrival above the
      leaves -- "a" below is always the node with the lower index).
  segmented sum (Engine::sum_sets, engine_core.inc:1273-1317; bgls_aggregate_sets)
      P = 32 lane pairs per set, doubled while P < 8192, 4 P <= the largest set and 2 P * sets <= 131072 (engine_core.inc:1280-1281).
      Pair t of a set adds lo + t, lo + t + P, ... (k_sumpairseg_main, k_sumpair.hip:183-200), every block runs the block tree, and
      the P / 32 partials of a set are halved level by level by k_sum_coop (k_points.inc:114-122: out[i] = in[2i] + in[2i + 1]).
  subset sum (k_sumsel_main, k_sumpair.hip:305-373), for a key set of at most 2048 keys (one window, one block per row:
      sumsel_pairs_per_set, sumsel.hpp:46-51): the entries are taken 32 at a time in ascending key order, pair p takes entry p of
      each round -- a row that selects keys 0 .. n-1 is the whole sum's schedule with T = 32.  In complement mode the negated
      unselected keys come first and the whole-set sum last.
  grouped sums: the index list is filled by k_grp_scatter (k_msggroup.hip:110-120).  All signers of a call with at most 64 of them sit
      in ONE wave of that launch (thread i = signer i, 256 threads a block); the lanes of a wave that share a group take ONE cursor
      value (the lowest lane's atomicAdd) and place themselves by the count of lower lanes of the same group, so within such a call a
      group's run of the list is in signer order.  A group of one work item then runs the segmented schedule with P = 32
      (k_sumpairidx_main, k_sumpair.hip:210-227), a small group is added serially by one lane pair (k_sumpairgrp_main, :235-257).

run() returns every addition performed as Add(stage, level, where, a, b, a_keys, b_keys): stage "main" (level = the pair's j-th key,
where = the pair), "block" (level = s, where = 32 * block + p) or "tree" / "coop" (level counted from the leaves, where = the node);
a, b are the operands as scalars, a_keys / b_keys the positions of the keys under them.  place() takes targets (stage, level, where,
kind) and filler scalars and solves for the one key per target that makes that addition the wanted kind; unexplained() lists every
exceptional addition of a layout that is neither a target nor forced by one.

A change of the launch geometry (keys per block, the P rule, the order of the levels) must be mirrored here: the GPU tests would still
compare the right bytes, but the cases would no longer sit where their names say."""
import json
import os
import random
from collections import namedtuple

ORDER = {0: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
         1: 52435875175126190479447740508185965837690552500527637822603658699938581184513}
FP = {0: 32, 1: 48}
INF = 0                                   # a layout entry: the wire point at infinity
EXCEPTIONAL = ("a_inf", "b_inf", "both_inf", "equal", "opposite")
LEVELS = (16, 8, 4, 2, 1)

Add = namedtuple("Add", "stage level where a b a_keys b_keys")
Target = namedtuple("Target", "stage level where kind")
Case = namedtuple("Case", "name family n T layout targets")


def kind_of(ad, r):
    """"empty": an operand with no key under it (the start of a pair's loop, a pair or block beyond the keys) -- the structure of the
    launch, not a case of the group law an input chooses"""
    if not ad.a_keys or not ad.b_keys:
        return "empty"
    if ad.a == 0 and ad.b == 0:
        return "both_inf"
    if ad.a == 0:
        return "a_inf"
    if ad.b == 0:
        return "b_inf"
    if ad.a == ad.b:
        return "equal"
    if (ad.a + ad.b) % r == 0:
        return "opposite"
    return "ordinary"


def whole_pairs(n, throughput=False):
    """T of Engine::sum_points_jac for n G2 keys"""
    return 32 * min((n + 127) // 128, 1024 if throughput else 2048)


def seg_pairs(max_set, nsets):
    """P of Engine::sum_sets for the lane-pair kernel"""
    P = 32
    while P < 8192 and P * 4 <= max_set and nsets * P * 2 <= 131072:
        P *= 2
    return P


def run(lay, r, T, tree_stage="tree"):
    """(additions, total) of one sum of the keys `lay` on T lane pairs: main loops, block trees, the tree above the T / 32 blocks"""
    n, adds = len(lay), []
    sums = []
    for t in range(T):
        acc, keys = 0, ()
        for j, k in enumerate(range(t, n, T)):
            adds.append(Add("main", j, t, acc, lay[k] % r, keys, (k,)))
            acc, keys = (acc + lay[k]) % r, keys + (k,)
        sums.append((acc, keys))
    parts = []
    for b in range(T // 32):
        blk = sums[32 * b:32 * b + 32]
        for s in LEVELS:
            for p in range(s):
                (a, ak), (c, ck) = blk[p], blk[p + s]
                adds.append(Add("block", s, 32 * b + p, a, c, ak, ck))
                blk[p] = ((a + c) % r, ak + ck)
        parts.append(blk[0])
    level = 0
    while len(parts) > 1:
        nxt = []
        for i in range((len(parts) + 1) // 2):
            if 2 * i + 1 < len(parts):
                (a, ak), (c, ck) = parts[2 * i], parts[2 * i + 1]
                adds.append(Add(tree_stage, level, i, a, c, ak, ck))
                nxt.append(((a + c) % r, ak + ck))
            else:
                nxt.append(parts[2 * i])
        parts, level = nxt, level + 1
    return adds, (parts[0][0] if parts else 0)


def find(adds, tg):
    hit = [ad for ad in adds if (ad.stage, ad.level, ad.where) == (tg.stage, tg.level, tg.where)]
    assert len(hit) == 1, tg
    return hit[0]


def place(fill, r, T, targets, same=(), tree_stage="tree"):
    """The layout `fill` (scalars, all different) with one key per target replaced so that the target's addition has its kind.  The key
    is the last one under the operand that moves (b for equal / opposite / b_inf, a for a_inf); targets are solved in the order of the
    schedule, so a later one sees the earlier ones' keys.  same: (dst, src) positions copied before anything is solved."""
    lay = [x % r for x in fill]
    for dst, src in same:
        lay[dst] = lay[src]
    order = {(ad.stage, ad.level, ad.where): i for i, ad in enumerate(run(lay, r, T, tree_stage)[0])}
    for tg in sorted(targets, key=lambda t: order[(t.stage, t.level, t.where)]):
        ad = find(run(lay, r, T, tree_stage)[0], tg)
        assert ad.a_keys and ad.b_keys, ("the schedule gives this addition no two operands", tg)
        ka, kb = max(ad.a_keys), max(ad.b_keys)
        if tg.kind == "equal":
            lay[kb] = (lay[kb] + ad.a - ad.b) % r
        elif tg.kind == "opposite":
            lay[kb] = (lay[kb] - ad.a - ad.b) % r
        elif tg.kind in ("b_inf", "both_inf"):
            lay[kb] = (lay[kb] - ad.b) % r
        if tg.kind in ("a_inf", "both_inf"):
            lay[ka] = (lay[ka] - ad.a) % r
        assert tg.kind in EXCEPTIONAL, tg
    return lay


def unexplained(lay, r, T, targets, tree_stage="tree"):
    """The exceptional additions of the layout that are neither a target nor forced by one.  Forced: (1) an operand that is infinity can
    only be so because everything under it cancels, so exceptional additions wholly UNDER the infinite operand of a target are its cause;
    (2) a target that leaves infinity (opposite, both_inf) hands it to the one addition above it, which then has that operand at infinity.
    Raises where a target's addition does not have its kind."""
    adds = run(lay, r, T, tree_stage)[0]
    tads = [find(adds, tg) for tg in targets]
    for tg, ta in zip(targets, tads):
        assert kind_of(ta, r) == tg.kind, (tg, kind_of(ta, r))
    spots = {(tg.stage, tg.level, tg.where) for tg in targets}
    handed = {frozenset(ta.a_keys + ta.b_keys) for tg, ta in zip(targets, tads) if tg.kind in ("opposite", "both_inf")}
    left = []
    for ad in adds:                                                   # in schedule order: an infinity handed up twice is followed
        k = kind_of(ad, r)
        if k not in EXCEPTIONAL or (ad.stage, ad.level, ad.where) in spots:
            continue
        under = set(ad.a_keys) | set(ad.b_keys)
        forced = False
        for tg, ta in zip(targets, tads):
            if tg.kind in ("a_inf", "both_inf") and under <= set(ta.a_keys):
                forced = True
            if tg.kind in ("b_inf", "both_inf") and under <= set(ta.b_keys):
                forced = True
        a_h, b_h = frozenset(ad.a_keys) in handed, frozenset(ad.b_keys) in handed
        if (k == "a_inf" and a_h) or (k == "b_inf" and b_h) or (k == "both_inf" and a_h and b_h):
            forced = True
            if k == "both_inf":
                handed.add(frozenset(under))
        if not forced:
            left.append(ad)
    return left


# ------------------------------------------------------------------------------------------------ the catalogue
POOL = 1100                               # filler scalars per curve: more than the largest layout, so a layout's fillers all differ
MAIN_PAIRS = (0, 15, 16, 31)
MAIN_CASES = ("second_equal", "second_opposite", "inf_first", "inf_middle", "inf_last", "third_is_sum", "all_equal")
RAGGED = (1, 2, 3, 17, 31, 33)
TREE_N = (256, 384, 640, 1024)            # W = 2, 3, 5, 8
NODE_KINDS = ("equal", "opposite", "a_inf", "b_inf")


def pool(cid):
    rnd = random.Random(0x6B5 + cid)
    seen, out = set(), []
    while len(out) < POOL:
        s = rnd.randrange(1, ORDER[cid])
        if s not in seen and ORDER[cid] - s not in seen:
            seen.add(s)
            out.append(s)
    return out


def level_pairs(s):
    """the places of a block-tree level: pair 0, pair s - 1 and, for s >= 4, one inner pair"""
    return sorted({0, s - 1} | ({s // 2} if s >= 4 else set()))


def tree_nodes(W):
    """(level, node) of every addition of the index-order tree over W leaves"""
    out, cnt, level = [], W, 0
    while cnt > 1:
        out += [(level, i) for i in range(cnt // 2)]
        cnt, level = (cnt + 1) // 2, level + 1
    return out


def main_targets(case, t):
    """a pair of four keys (n = 128): the targets of a named main-loop case, and the positions copied first"""
    if case == "second_equal":
        return [Target("main", 1, t, "equal")], ()
    if case == "second_opposite":             # ... then two more keys: the accumulator restarts from infinity
        return [Target("main", 1, t, "opposite"), Target("main", 2, t, "a_inf")], ()
    if case == "inf_first":
        return [Target("main", 1, t, "a_inf")], ()
    if case == "inf_middle":
        return [Target("main", 2, t, "b_inf")], ()
    if case == "inf_last":
        return [Target("main", 3, t, "b_inf")], ()
    if case == "third_is_sum":
        return [Target("main", 2, t, "equal")], ()
    assert case == "all_equal"                # K + K, then 2K + K and 3K + K: one doubling, two ordinary additions
    return [Target("main", 1, t, "equal")], ((t + 64, t), (t + 96, t))


_CATALOGUE = {}


def catalogue(cid):
    """every whole-sum case of one curve, made once: the layouts of the main loop, the block tree, the ragged blocks and the trees above"""
    if cid in _CATALOGUE:
        return _CATALOGUE[cid]
    r, pl = ORDER[cid], pool(cid)
    rnd = random.Random(0xCA7 + cid)
    cases = []

    def fill(n):
        o = rnd.randrange(POOL)
        return [pl[(o + i) % POOL] for i in range(n)]

    def add(name, family, n, targets, same=()):
        T = whole_pairs(n)
        lay = place(fill(n), r, T, targets, same)
        cases.append(Case(name, family, n, T, lay, tuple(targets)))

    for t in MAIN_PAIRS:
        for case in MAIN_CASES:
            tg, same = main_targets(case, t)
            add("main-%s-pair%d" % (case, t), "main", 128, tg, same)
    for n in (32, 64):
        for s in LEVELS:
            for kind in EXCEPTIONAL:
                for p in level_pairs(s):
                    add("block-n%d-s%d-%s-pair%d" % (n, s, kind, p), "block", n, [Target("block", s, p, kind)])
    for s in LEVELS:                          # every pair of the level exceptional, the kinds mixed
        add("block-n64-s%d-every-pair" % s, "block-all", 64, [Target("block", s, p, EXCEPTIONAL[(p + s) % 5]) for p in range(s)])
    # two levels of one block: pair 3 of level 16 (keys 3, 35 | 19, 51) and pair 1 of level 4 (pairs 1, 9, 17, 25 | 5, 13, 21, 29)
    add("block-n64-two-levels", "block-two", 64, [Target("block", 16, 3, "equal"), Target("block", 4, 1, "opposite")])
    for n in RAGGED:
        first = next((ad for ad in run(fill(n), r, whole_pairs(n))[0] if ad.a_keys and ad.b_keys), None)
        if first is None:
            add("ragged-n%d" % n, "ragged", n, [])
            continue
        for kind in ("equal", "opposite"):
            add("ragged-n%d-%s" % (n, kind), "ragged", n, [Target(first.stage, first.level, first.where, kind)])
    for n in TREE_N:
        nodes = tree_nodes(n // 128)
        for level, i in nodes:
            for kind in NODE_KINDS:
                add("tree-n%d-l%d-node%d-%s" % (n, level, i, kind), "tree", n, [Target("tree", level, i, kind)])
        add("tree-n%d-root-infinity" % n, "tree-root", n, [Target("tree", nodes[-1][0], 0, "opposite")])
    _CATALOGUE[cid] = cases
    return cases


def segmented_calls(cid):
    """The calls of bgls_aggregate_sets: lists of (name, layout, targets, P).  Call 0: the one-block layouts of the catalogue (at most 64
    keys: P = 32, the whole sum's schedule), in an order that puts the sets at offsets that are no multiples of 32, with an empty set
    and a set of one infinity among them.  Call 1: sets of 256 and 512 keys on P = 256 lane pairs, eight block partials each, with equal,
    opposite and vanished partials at every node of k_sum_coop's three levels; an empty set and one infinity between them."""
    r, pl = ORDER[cid], pool(cid)
    small = [c for c in catalogue(cid) if c.n <= 64]
    small.sort(key=lambda c: (c.n not in (1, 3, 17), c.name))          # the odd sizes first: every later offset is odd
    call0 = [(c.name, c.layout, c.targets) for c in small]
    call0[3:3] = [("empty", [], ()), ("one-infinity", [INF], ())]
    P0 = seg_pairs(max(len(c[1]) for c in call0), len(call0))
    assert P0 == 32
    rnd = random.Random(0x5E6 + cid)
    spec = [(256, lv, i, kind) for lv, i in tree_nodes(8) for kind in NODE_KINDS]
    spec += [(512, lv, i, NODE_KINDS[(lv + i) % 4]) for lv, i in tree_nodes(8)]
    spec.insert(1, (1, 0, 0, "one-infinity"))                         # every later set then starts at an odd offset
    spec.insert(5, (0, 0, 0, "empty"))
    P1 = seg_pairs(512, len(spec))
    assert P1 == 256
    call1 = []
    for n, lv, i, kind in spec:
        if n < 2:
            call1.append((kind, [INF] * n, ()))
            continue
        o = rnd.randrange(POOL)
        tg = (Target("coop", lv, i, kind),)
        call1.append(("coop-n%d-l%d-node%d-%s" % (n, lv, i, kind), place([pl[(o + j) % POOL] for j in range(n)], r, P1, tg, tree_stage="coop"), tg))
    return [(call0, P0), (call1, P1)]


# ------------------------------------------------------------------------------------------------ wire keys and expected points
_WIRE = {0: {}, 1: {}}


def wire_keys(cid, scalars, scale_many):
    """the wire bytes of sk * g2 for every scalar (0: infinity), each distinct scalar scaled once per process; scale_many(list of
    scalars) -> list of wire keys is the caller's generator (the oracle in the CPU tier, the engine's in the GPU tier: the CPU tier
    has pinned the layouts against the oracle's additions)"""
    known = _WIRE[cid]
    todo = sorted({s for s in scalars if s and s not in known})
    if todo:
        known.update(zip(todo, scale_many(todo)))
    zero = bytes(4 * FP[cid])
    return [known[s] if s else zero for s in scalars]


def half_equal_points(cid):
    """tests/golden/keysum_halfx.json (make_keysum_halfx.py): on-twist points P, Q with Re(x) equal and Im(x) different, and R, S with
    Im(x) equal and Re(x) different, as wire bytes.  None of them is in the order-r subgroup: wire-byte entry points only."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keysum_halfx.json")) as f:
        rows = json.load(f)["altbn128" if cid == 0 else "bls12"]
    return {k: tuple(bytes.fromhex(h) for h in v) for k, v in rows.items()}


def half_equal_layouts(cid, fillers):
    """(name, list of wire keys) with each pair of the fixture meeting in jacp_madd (n = 64: keys p and p + 32 of one pair), at level 16
    of the block tree (n = 32: keys p and p + 16) and at level 1 (n = 2).  fillers: at least 64 wire keys of ordinary points.  In every
    meeting one lane's half of H = x2 - x1 is zero and the other's is not: an ordinary addition."""
    out = []
    for tag, (a, b) in sorted(half_equal_points(cid).items()):
        for p in (0, 31):
            lay = list(fillers[:64])
            lay[p], lay[p + 32] = a, b
            out.append(("halfx-%s-madd-pair%d" % (tag, p), lay))
        for p in (0, 15):
            lay = list(fillers[:32])
            lay[p], lay[p + 16] = b, a
            out.append(("halfx-%s-level16-pair%d" % (tag, p), lay))
        out.append(("halfx-%s-level1" % tag, [a, b]))
    return out
