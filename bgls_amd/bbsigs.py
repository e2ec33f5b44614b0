"""Host-side mirror of the reference's `bbsigs` package (bbsigs/bbsigs.go, bbsigs/hashedbbsigs.go): Boneh-Boyen signatures, same
names and semantics.  Key generation and signing multiply a generator with bgls_scale_generator; verification is ONE
bgls_bb_verify_batch call for the whole batch (a single Verify is a batch of one; _marshal.settle).  The scalar arithmetic of Sign (an
inverse modulo the group order) and the blake2b-256 message hash of the hashed forms are host work, as in the reference."""
import ctypes
import hashlib
import os
import secrets
from . import _lib
from ._marshal import cat, is_point, mag32, scale_generator, settle
from .bgls import _group_offsets
from .curves import G1, G2


class Privkey:                                      # bbsigs/bbsigs.go:13-17
    __slots__ = ("X", "Y")

    def __init__(self, X, Y):
        self.X, self.Y = X, Y


class Pubkey:                                       # bbsigs/bbsigs.go:19-23
    __slots__ = ("U", "V")

    def __init__(self, U, V):
        self.U, self.V = U, V


class Signature:                                    # bbsigs/bbsigs.go:25-29
    __slots__ = ("Sigma", "R")

    def __init__(self, Sigma, R):
        self.Sigma, self.R = Sigma, R


def KeyGen(curve):                                  # bbsigs/bbsigs.go:31-39
    order = curve.GetG1Order()
    x, y = secrets.randbelow(order), secrets.randbelow(order)
    return Privkey(x, y), LoadPublicKey(curve, x, y)


def LoadPublicKey(curve, x, y):                     # bbsigs/bbsigs.go:41-45
    u, v = scale_generator(curve, G2, [x, y])
    return Pubkey(u, v)


def _sign_exponent(curve, sk, msg):
    """(r, (x + m + y r)^-1 mod order) with a fresh r; the degenerate r (y r = -(x + m)) is drawn again (bbsigs/bbsigs.go:47-66)."""
    order = curve.GetG1Order()
    while True:
        r = secrets.randbelow(order)
        if r * sk.Y == order - (sk.X + msg):
            continue
        e = (sk.Y * r + sk.X + msg) % order
        if e == 0:                                  # the same degenerate case modulo the order
            continue
        return r, pow(e, -1, order)


def Sign(curve, sk, msg):                           # bbsigs/bbsigs.go:47-66
    return SignBatch(curve, [sk], [msg])[0]


def SignBatch(curve, sks, msgs):
    """Sign for n (private key, message) pairs: the n scalar multiplications of g1 in one bgls_scale_generator call."""
    if len(sks) != len(msgs):
        raise ValueError("sks and msgs differ in length")
    rs, es = [], []
    for sk, m in zip(sks, msgs):
        r, e = _sign_exponent(curve, sk, m)
        rs.append(r)
        es.append(e)
    return [Signature(s, r) for s, r in zip(scale_generator(curve, G1, es), rs)]


def _batchable(curve, sig, pk):
    return (isinstance(sig, Signature) and isinstance(pk, Pubkey) and is_point(sig.Sigma, curve, G1)
            and is_point(pk.U, curve, G2) and is_point(pk.V, curve, G2))


def _items(curve, sigs, pks, msgs):
    """the four blobs of bgls_bb_verify_batch and its combined form: sigmas, the magnitudes of r, U || V per key, the magnitudes of m"""
    return (cat(s.Sigma for s in sigs), _lib.buf(b"".join(mag32(curve, s.R) for s in sigs)),
            _lib.buf(b"".join(k.U.raw + k.V.raw for k in pks)), _lib.buf(b"".join(mag32(curve, m) for m in msgs)))


def _verify_batch(curve, sigs, pks, msgs):
    """One bgls_bb_verify_batch call for the items made of this curve's Points (any other item is rejected, as a mismatched
    Add / Pair in the reference yields a result that never equals GetGT()); _marshal.settle."""
    if not (len(sigs) == len(pks) == len(msgs)):
        raise ValueError("sigs, pks and msgs differ in length")

    def call(items):
        verdicts = _lib.out(len(items))
        rc = _lib.load().bgls_bb_verify_batch(curve.id, *_items(curve, [sigs[b] for b in items], [pks[b] for b in items], [msgs[b] for b in items]),
                                              len(items), verdicts, None)
        return rc, verdicts

    return settle(len(sigs), lambda b: _batchable(curve, sigs[b], pks[b]), call)


def Verify(curve, sig, pk, msg):                    # bbsigs/bbsigs.go:68-73
    return _verify_batch(curve, [sig], [pk], [msg])[0]


def VerifyBatch(curve, sigs, pks, msgs):
    """len(sigs) independent Verify calls in one bgls_bb_verify_batch call: a list of bools, one per item."""
    return _verify_batch(curve, sigs, pks, msgs)


def VerifyBatchCombined(curve, sigs, pks, msgs, group=None, seed=None):
    """"Are these Boneh-Boyen signatures all valid?" under one combined check per group of consecutive items
    (bgls_bb_verify_batch_combined: the Miller loops of a group share their squarings, one final exponentiation per group instead of one
    per item).  group: an int chunk size, or None for one group over all items; seed: 32 bytes from a CSPRNG drawn AFTER the inputs are
    fixed (None draws os.urandom(32)).  Returns the list of group verdicts; a group that holds an item Verify rejects is rejected except
    with probability about 2^-127.  Every item must be made of Points of this curve; a foreign or nil point, or an encoding error
    anywhere, raises ValueError (use VerifyBatch to settle such a batch)."""
    n = len(sigs)
    if not (n == len(pks) == len(msgs)):
        raise ValueError("sigs, pks and msgs differ in length")
    if seed is None:
        seed = os.urandom(32)
    if len(seed) != 32:
        raise ValueError("seed must be 32 bytes")
    if n == 0:
        return []
    if not all(_batchable(curve, s, k) for s, k in zip(sigs, pks)):
        raise ValueError("the combined check takes Signatures and Pubkeys made of G1 / G2 Points of this curve only")
    goff = _group_offsets(n, group)
    verdicts = _lib.out(len(goff) - 1)
    rc = _lib.load().bgls_bb_verify_batch_combined(curve.id, *_items(curve, sigs, pks, msgs), n, (ctypes.c_uint64 * len(goff))(*goff), len(goff) - 1,
                                                   _lib.buf(bytes(seed)), verdicts, None)
    if rc < 0:
        raise ValueError("bgls_bb_verify_batch_combined: %s" % _lib.last_error())
    return [v == 1 for v in verdicts]


def VerifyBatchLocated(curve, sigs, pks, msgs, group=64, seed=None):
    """One verdict per item at the combined check's cost where everything is valid: ONE combined call over groups of `group` items, then
    ONE VerifyBatch call over only the items of the rejected groups; the items of accepted groups get True."""
    n = len(sigs)
    goff = _group_offsets(n, group)
    groups = VerifyBatchCombined(curve, sigs, pks, msgs, group, seed)
    out = [True] * n
    again = [b for g, ok in enumerate(groups) if not ok for b in range(goff[g], goff[g + 1])]
    if again:
        for b, v in zip(again, VerifyBatch(curve, [sigs[b] for b in again], [pks[b] for b in again], [msgs[b] for b in again])):
            out[b] = v
    return out


def blake2b256(msg, p):                             # bbsigs/hashedbbsigs.go:34-39
    return int.from_bytes(hashlib.blake2b(bytes(msg), digest_size=32).digest(), "big") % p


def SignHashed(curve, sk, msg):                     # bbsigs/hashedbbsigs.go:10-13
    return SignCustHash(curve, sk, msg, blake2b256)


def SignCustHash(curve, sk, msg, hash):             # bbsigs/hashedbbsigs.go:15-18
    return Sign(curve, sk, hash(msg, curve.GetG1Order()))


def VerifyHashed(curve, sig, pk, msg):              # bbsigs/hashedbbsigs.go:20-23
    return VerifyCustHash(curve, sig, pk, msg, blake2b256)


def VerifyCustHash(curve, sig, pk, msg, hash):      # bbsigs/hashedbbsigs.go:25-32
    return Verify(curve, sig, pk, hash(msg, curve.GetG1Order()))


def VerifyHashedBatch(curve, sigs, pks, msgs):
    """VerifyHashed for a batch: the messages are hashed on the host, the verifications are one call."""
    order = curve.GetG1Order()
    return _verify_batch(curve, sigs, pks, [blake2b256(m, order) for m in msgs])


def VerifyHashedBatchCombined(curve, sigs, pks, msgs, group=None, seed=None):
    """VerifyBatchCombined over hashed messages: blake2b256 on the host, as VerifyHashedBatch."""
    order = curve.GetG1Order()
    return VerifyBatchCombined(curve, sigs, pks, [blake2b256(m, order) for m in msgs], group, seed)


def VerifyHashedBatchLocated(curve, sigs, pks, msgs, group=64, seed=None):
    """VerifyBatchLocated over hashed messages: blake2b256 on the host, as VerifyHashedBatch."""
    order = curve.GetG1Order()
    return VerifyBatchLocated(curve, sigs, pks, [blake2b256(m, order) for m in msgs], group, seed)
