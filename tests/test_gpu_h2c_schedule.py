"""GPU tier for the alt-bn128 hash-to-G1 SCHEDULES at counters no message reaches, through the scripted-digest unit of the device harness
(tests/harness/device_harness_h2c.hip: k_hash.hip's k_h2c_bn_wide, k_h2c_bn_round<LPM>, k_h2c_bn_finish and kl::h2c_bn compiled unchanged,
with the Keccak call replaced by a lookup in the message).  A random message first accepts at counter k with probability 2^-(k + 1), so
random messages never run the wide kernel's later passes, the <64> rounds, the `last` branch or the exhausted exit; here a message IS its
256 digests (8192 bytes, the digest of prefix byte c at 32 c; the digest of 0xFF is candidate 255 and the sign hash), and the test
chooses which counters accept.

Every case runs in three forms: `wide` (n < 256, k_h2c_bn_wide: passes over counters 0..14, 15..30, ..., 239..254, 255), `middle`
(n >= 256, lean = 0: 1@0, 4@1, 32@5, then 64 from 37) and `lean` (n >= 256, lean = 1: 1@0, 1@1, 2@2, 4@4, 8@8, 32@16, then 64 from 48).
The round boundaries below are written from that documented shape, not read from the code.

Reference: a plain Python walk of the counters (x = digest mod q; accept the first counter where x^3 + 3 is a square; y = (x^3 + 3)^((q + 1) / 4),
negated when the last byte of digest 255 is odd; no counter: infinity and FLAG_HASH).  The accepting digests of a message have pairwise
distinct x, and those at the counters a case is about are used nowhere else, so the x of the result says which counter won.  Digests with x^3 mod q >= q - 3 stay out of the catalogue (the reference compares against the
unreduced x^3 + 3 there, which h2c.hpp documents it does not reproduce); x = q - 1 is such a value and has a case of its own.
y = 0 cannot occur: the curve has prime order, so no point of order two."""
import ctypes
import random

import pytest

import device_harness_lib

pytestmark = pytest.mark.gpu

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
FLAG_HASH = 4
SCRIPT = 8192
FORMS = ("wide", "middle", "lean")
# (lanes per message, first counter) of the rounds before the <64> rounds, and the first counter of those
SHAPE = {"middle": ([(1, 0), (4, 1), (32, 5)], 37), "lean": ([(1, 0), (1, 1), (2, 2), (4, 4), (8, 8), (32, 16)], 48)}


def segments(form):
    """(first, last) counter of every round (wide: pass) of the form, in order"""
    if form == "wide":
        return [(0, 14)] + [(c, min(c + 15, 255)) for c in range(15, 256, 16)]
    head, c64 = SHAPE[form]
    return [(c0, c0 + lpm - 1) for lpm, c0 in head] + [(c, min(c + 63, 255)) for c in range(c64, 256, 64)]


def test_the_segments_tile_the_counters():
    for form in FORMS:
        seg = segments(form)
        assert seg[0][0] == 0 and seg[-1][1] == 255 and all(b[0] == a[1] + 1 for a, b in zip(seg, seg[1:])), form
    assert len(segments("wide")) == 17 and len(segments("middle")) == 7 and len(segments("lean")) == 10


# ---------------------------------------------------------------------------------------------------------------- digest catalogue and model
class Catalogue:
    """Seeded digests by kind.  is_square is the memoised Euler criterion of x^3 + 3 and refuses the kept-out digests."""

    def __init__(self, seed):
        self.rnd = random.Random(seed)
        self.sq = {}
        self.used = set()
        self.fill = None
        self.pool = None
        self.rejects = {0: [], 1: []}                       # by the parity of the last byte (digest 255 is the sign hash)
        while min(len(v) for v in self.rejects.values()) < 256:
            h = self.rnd.getrandbits(256)
            if not self.kept_out(h) and not self.is_square(h):
                self.rejects[h & 1].append(h)

    def kept_out(self, h):
        return pow(h % Q, 3, Q) >= Q - 3

    def is_square(self, h):
        if h not in self.sq:
            assert not self.kept_out(h), "digest with x^3 mod q >= q - 3 in the catalogue: %x" % h
            y2 = (pow(h % Q, 3, Q) + 3) % Q
            assert y2 != 0
            self.sq[h] = pow(y2, (Q - 1) // 2, Q) == 1
        return self.sq[h]

    def accept(self, parity=None, at_least_q=False):
        """a fresh accepting digest: its x = h mod q is used by no other"""
        while True:
            h = self.rnd.getrandbits(256)
            if self.kept_out(h) or h % Q in self.used or (parity is not None and (h & 1) != parity) or (at_least_q and h < Q):
                continue
            if self.is_square(h):
                self.used.add(h % Q)
                return h

    def reject(self, parity=None):
        return self.rnd.choice(self.rejects[self.rnd.getrandbits(1) if parity is None else parity])

    def script(self, accepts, parity=None, fixed=None, tail=()):
        """the 8192 bytes of a message that accepts exactly at the counters `accepts` and `tail` (fixed: {counter: digest}, as given).
        The digests at `accepts` are fresh; those at `tail` -- counters behind the one that decides, or filler -- come from a pool of
        accepting digests, distinct within the message."""
        accepts, tail = set(accepts), list(tail)
        if self.pool is None:
            self.pool = [self.accept() for _ in range(2048)]
        pooled = dict(zip(tail, self.rnd.sample(self.pool, len(tail))))
        d = []
        for c in range(256):
            par = parity if c == 255 else None
            if fixed and c in fixed:
                d.append(fixed[c])
            elif c in accepts:
                d.append(self.accept(par))
            elif c in pooled:
                d.append(pooled[c])
            else:
                d.append(self.reject(par))
        return b"".join(h.to_bytes(32, "big") for h in d)

    def first_then_random(self, first):
        return self.script([first], tail=[c for c in range(first + 1, 256) if self.rnd.getrandbits(1)])

    def filler(self, k):
        """k messages as random messages are: every counter accepts with probability 1/2 (made once)"""
        assert k <= 320
        if self.fill is None:
            self.fill = [self.script([], tail=[c for c in range(256) if self.rnd.getrandbits(1)]) for _ in range(320)]
        return self.fill[:k]

    def model(self, script):
        """(first accepting counter or 256, the 64 bytes, the infinity byte)"""
        assert len(script) == SCRIPT
        for c in range(256):
            h = int.from_bytes(script[32 * c:32 * c + 32], "big")
            if self.is_square(h):
                x = h % Q
                y = pow((pow(x, 3, Q) + 3) % Q, (Q + 1) // 4, Q)
                assert y * y % Q == (pow(x, 3, Q) + 3) % Q and y != 0
                if script[SCRIPT - 1] & 1:
                    y = Q - y
                return c, x.to_bytes(32, "big") + y.to_bytes(32, "big"), 0
        return 256, bytes(64), 1


@pytest.fixture(scope="module")
def cat():
    return Catalogue(20261018)


@pytest.fixture(scope="module")
def h2c(gpu_lib):
    """libdevice_harness_h2c.so, loaded after the library (gpu_lib imports torch first): the process keeps one HIP runtime"""
    return device_harness_lib.load_h2c()


def buf(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")


def launch(h2c, scripts, lean):
    n = len(scripts)
    pts, inf = (ctypes.c_uint8 * (64 * n))(), (ctypes.c_uint8 * n)()
    flags, cn = (ctypes.c_uint32 * 1)(), (ctypes.c_uint32 * 16)()
    assert h2c.dh_h2c_bn(n, lean, buf(b"".join(scripts)), pts, inf, flags, cn) == 0
    raw = bytes(pts)
    return [raw[64 * i:64 * i + 64] for i in range(n)], list(inf), flags[0], list(cn)


def check_batch(cat, form, scripts, got):
    """every point, infinity byte, the flag word and the survivor counters of one launch against the model"""
    pts, inf, flags, cn = got
    want = [cat.model(s) for s in scripts]
    for i, (w, p, f) in enumerate(zip(want, pts, inf)):
        assert (p, f) == (w[1], w[2]), "%s: message %d of %d (first accepting counter %d)" % (form, i, len(scripts), w[0])
    assert flags == (FLAG_HASH if any(w[0] == 256 for w in want) else 0), form
    if form == "wide":
        assert cn == [0] * 16
        return
    seg = segments(form)
    # cn[k]: the messages still open after round k, i.e. whose first accepting counter lies beyond its last counter; the last round
    # appends nothing (it reports the exhausted messages instead)
    expect = [0] * 16
    for k, (_, last) in enumerate(seg[:-1], 1):
        expect[k] = sum(w[0] > last for w in want)
    assert cn == expect, form


def run_form(h2c, cat, form, scripts, filler=True, shuffle=1):
    """the scripts under one form, checked; returns their points in the order given.  Round forms: filler messages bring n to at least
    301 (at least 45 of them), and the batch is shuffled so that a case does not sit at the wave position its index gives it.  Wide
    form: batches of 131 and 125 (n < 256, no multiple of 4)."""
    rnd = random.Random(shuffle)
    if form == "wide":
        out, at, k = [], 0, 0
        while at < len(scripts):
            part = scripts[at:at + (131, 125)[k & 1]]
            got = launch(h2c, part, 0)
            check_batch(cat, form, part, got)
            out += got[0]
            at += len(part)
            k += 1
        return out
    batch = list(scripts) + (cat.filler(max(45, 301 - len(scripts))) if filler else [])
    order = list(range(len(batch)))
    rnd.shuffle(order)
    assert len(batch) >= 256
    got = launch(h2c, [batch[j] for j in order], 1 if form == "lean" else 0)
    check_batch(cat, form, [batch[j] for j in order], got)
    back = {j: p for j, p in zip(order, got[0])}
    return [back[j] for j in range(len(scripts))]


# ---------------------------------------------------------------------------------------------------------------- the cases
@pytest.fixture(scope="module")
def every_counter(cat):
    """first accepting counter = every value 0..255: one message that accepts there alone, one that goes on accepting at random"""
    return [cat.script([c]) for c in range(256)] + [cat.first_then_random(c) for c in range(256)]


@pytest.fixture(scope="module")
def lowest_wins(cat):
    """for every round of every form (LPM 1, 2, 4, 8, 32, 64; the wide kernel's 16 lanes): a message accepting at the first and the last
    counter of the segment, one at every counter of it, one at every counter from its first on, one at its last counter and the
    first of the next segment, and one at its last counter alone"""
    out = []
    for form in FORMS:
        for a, b in segments(form):
            out.append(cat.script([a, b]))
            out.append(cat.script(range(a, b + 1)))
            out.append(cat.script(range(a, 256)))
            out.append(cat.script([b, b + 1] if b < 255 else [b]))
            out.append(cat.script([b]))
    return out


@pytest.mark.parametrize("form", FORMS)
def test_first_accepting_counter_at_every_value(h2c, cat, every_counter, form):
    """Every c0, every segment boundary: a gap between two rounds loses the message that accepts only there, an overlap is harmless only
    if the lower round wins."""
    assert sorted(cat.model(s)[0] for s in every_counter) == sorted(list(range(256)) * 2)
    run_form(h2c, cat, form, every_counter)


@pytest.mark.parametrize("form", FORMS)
def test_lowest_accepting_counter_wins(h2c, cat, lowest_wins, form):
    run_form(h2c, cat, form, lowest_wins)


@pytest.mark.parametrize("form", FORMS)
def test_no_accepting_counter_is_infinity_and_flagged(h2c, cat, form):
    """The exhausted message gets infinity and raises FLAG_HASH; its neighbours keep their points; without it the flag word stays 0."""
    rnd = random.Random(5)
    good = [cat.first_then_random(rnd.choice((0, 1, 3, 14, 15, 16, 40, 200, 254, 255))) for _ in range(33)]
    dead = [cat.script([], parity=0), cat.script([], parity=1), cat.script([])]
    assert [cat.model(s)[0] for s in dead] == [256] * 3
    mixed = good[:5] + dead[:1] + good[5:20] + dead[1:] + good[20:]
    run_form(h2c, cat, form, mixed)
    run_form(h2c, cat, form, good)                       # (check_batch: flags == 0)
    if form == "wide":
        for n in (1, 2, 5):                              # a batch of exhausted messages alone, and next to the dead lanes of a partial wave
            got = launch(h2c, (dead * 2)[:n], 0)
            check_batch(cat, form, (dead * 2)[:n], got)
            assert got[2] == FLAG_HASH and got[1] == [1] * n


@pytest.mark.parametrize("form", FORMS)
def test_counter_255_alone_and_the_sign_from_the_same_digest(h2c, cat, form):
    """Digest 255 is candidate 255 AND the sign hash: both parities where it accepts, both where it rejects and a lower counter won."""
    scripts = []
    for parity in (0, 1):
        scripts += [cat.script([255], parity=parity) for _ in range(3)]
        scripts += [cat.script([c], parity=parity) for c in (0, 7, 14, 15, 36, 37, 47, 48, 254)]
        scripts += [cat.script([c, 255], parity=parity) for c in (0, 15, 240, 254)]
    pts = run_form(h2c, cat, form, scripts)
    for s, p in zip(scripts, pts):
        y = int.from_bytes(p[32:], "big")
        root = pow((pow(int.from_bytes(p[:32], "big"), 3, Q) + 3) % Q, (Q + 1) // 4, Q)
        assert y == (Q - root if s[-1] & 1 else root)


@pytest.mark.parametrize("form", FORMS)
def test_many_survivors(h2c, cat, form):
    """n = 300 messages that accept only at 250..255: every work list holds all n, and the <64> rounds walk 300 x 64 slots on their 8
    blocks (the earlier rounds on grids sized for the expected survivors).  Survivor counters equal n after every round."""
    rnd = random.Random(6)
    scripts = []
    for _ in range(300):
        first = rnd.randrange(250, 256)
        scripts.append(cat.script([first] + [c for c in range(first + 1, 256) if rnd.getrandbits(1)]))
    assert all(250 <= cat.model(s)[0] <= 255 for s in scripts)
    if form == "wide":
        for part in (scripts[:255], scripts[255:]):
            check_batch(cat, form, part, launch(h2c, part, 0))
        return
    got = launch(h2c, scripts, 1 if form == "lean" else 0)
    check_batch(cat, form, scripts, got)
    rounds = len(segments(form))
    assert got[3][1:rounds] == [300] * (rounds - 1)


def test_wide_form_mixed_waves(h2c, cat):
    """Four messages share a wave and leave in different passes: pass 1 (counters 0..14), pass 2 (15..30), pass 16 (239..254) and never,
    in every order of the four slots; then batch sizes 1, 2, 3, 5 and 255 of the same mix (partial last waves)."""
    import itertools
    rnd = random.Random(7)

    def kind(k):
        if k == 3:
            return cat.script([])
        a, b = ((0, 14), (15, 30), (239, 254))[k]
        return cat.first_then_random(rnd.randrange(a, b + 1))

    scripts = [kind(k) for perm in itertools.permutations(range(4)) for k in perm]
    assert len(scripts) == 96
    check_batch(cat, "wide", scripts, launch(h2c, scripts, 0))
    # pass 17 (counter 255 alone) next to the others
    scripts = [cat.script([255]), kind(0), kind(3), kind(2), kind(1), cat.script([255]), kind(2)]
    check_batch(cat, "wide", scripts, launch(h2c, scripts, 0))
    pool = [kind(k & 3) for k in range(255)]
    rnd.shuffle(pool)
    for n in (1, 2, 3, 5, 255):
        check_batch(cat, "wide", pool[:n], launch(h2c, pool[:n], 0))
        check_batch(cat, "wide", pool[-n:], launch(h2c, pool[-n:], 0))


@pytest.mark.parametrize("form", FORMS)
def test_edge_digests_at_the_accepting_counter(h2c, cat, form):
    """Edge values of the 256-bit digest (0, 1, q, q + 1, 2 q, 5 q, 2^256 - 1, random h >= q) at the counter that decides: where x^3 + 3 is a
    square the message accepts there, where it is not the edge digest is the last rejection before a fresh accepting one."""
    edges = [0, 1, Q, Q + 1, 2 * Q, 5 * Q, (1 << 256) - 1] + [cat.accept(at_least_q=True) for _ in range(3)] + [h for h in cat.rejects[0][:3] + cat.rejects[1][:3] if h >= Q]
    assert not any(cat.kept_out(h) for h in edges) and len(edges) > 10
    assert any(cat.is_square(h) for h in edges[:7]) and any(not cat.is_square(h) for h in edges[:7])
    scripts = []
    for k, h in enumerate(edges):
        for c in sorted(set((0, 4, 14, 15, 16, 36, 37, 100, 254)[k % 3::3] + (255,))):
            if cat.is_square(h) or c == 255:
                scripts.append(cat.script([], fixed={c: h}))          # (rejected at 255: exhausted)
            else:
                scripts.append(cat.script([c + 1], fixed={c: h}))
    pts = run_form(h2c, cat, form, scripts)
    # digests 1 and q + 1 are the generator's x: (1, 2) or (1, q - 2), four messages each
    assert sum(p[:32] == (1).to_bytes(32, "big") and int.from_bytes(p[32:], "big") in (2, Q - 2) for p in pts) == 8


@pytest.mark.parametrize("form", FORMS)
def test_x_equal_q_minus_one_is_compared_reduced(h2c, cat, form):
    """x = q - 1: x^3 + 3 = 2 after reduction, a square (q = 7 mod 8), so the schedules accept it, as h2c.hpp documents; the reference
    compares against the unreduced q + 2 and would walk on.  Pinned as the documented behaviour; kept out of every other case (the
    model refuses such a digest, so the expected bytes are written out here)."""
    assert pow(2, (Q - 1) // 2, Q) == 1 and cat.kept_out(Q - 1)
    scripts = []
    for c in (0, 20, 255):
        s = bytearray(cat.script([c + 1] if c < 255 else []))
        s[32 * c:32 * c + 32] = (Q - 1).to_bytes(32, "big")
        scripts.append(bytes(s))
    y = pow(2, (Q + 1) // 4, Q)
    want = [(Q - 1).to_bytes(32, "big") + (Q - y if s[-1] & 1 else y).to_bytes(32, "big") for s in scripts]
    if form == "wide":
        got = launch(h2c, scripts, 0)
    else:
        fill = cat.filler(298)
        got = launch(h2c, scripts + fill, 1 if form == "lean" else 0)
    assert got[0][:3] == want and got[1][:3] == [0, 0, 0] and got[2] == 0


@pytest.mark.parametrize("form", FORMS)
def test_position_independence(h2c, cat, every_counter, lowest_wins, form):
    """The same catalogue in two shuffled orders: the same point per message."""
    base = every_counter[::3] + lowest_wins[::2] + [cat.script([])]
    points = []
    for seed in (11, 12):
        order = list(range(len(base)))
        random.Random(seed).shuffle(order)
        pts = run_form(h2c, cat, form, [base[j] for j in order], shuffle=seed)
        back = {j: p for j, p in zip(order, pts)}
        points.append([back[j] for j in range(len(base))])
    assert points[0] == points[1]
