"""Host-side mirror of the reference's `bbsigs` package (bbsigs/bbsigs.go, bbsigs/hashedbbsigs.go): Boneh-Boyen signatures, same
names and semantics.  Key generation and signing multiply a generator with bgls_scale_generator; verification is ONE
bgls_bb_verify_batch call for the whole batch (a single Verify is a batch of one).  The scalar arithmetic of Sign (an inverse modulo
the group order) and the blake2b-256 message hash of the hashed forms are host work, as in the reference."""
import ctypes
import hashlib
import secrets
from . import _lib
from .curves import _reduce_scalar, Point, G1, G2


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


def _mag(curve, k):
    """A scalar as the ABI's 32-byte magnitude: negative scalars and those of 2^256 and above are reduced modulo the group order
    (as LoadPublicKeys does); every other value is passed unreduced."""
    return _reduce_scalar(curve, k if k >= 0 else k % curve.GetG1Order()).to_bytes(32, "big")


def _scale_generator(curve, group, scalars):
    n = len(scalars)
    if n == 0:
        return []
    size = len(curve.GetG1().raw) if group == G1 else len(curve.GetG2().raw)
    o = _lib.out(n * size)
    rc = _lib.load().bgls_scale_generator(curve.id, group, _lib.buf(b"".join(_mag(curve, k) for k in scalars)), n, o)
    if rc != 0:
        raise RuntimeError("bgls_scale_generator: %s" % _lib.last_error())
    raw = bytes(o)
    return [Point(curve, group, raw[i * size:(i + 1) * size]) for i in range(n)]


def KeyGen(curve):                                  # bbsigs/bbsigs.go:31-39
    order = curve.GetG1Order()
    x, y = secrets.randbelow(order), secrets.randbelow(order)
    return Privkey(x, y), LoadPublicKey(curve, x, y)


def LoadPublicKey(curve, x, y):                     # bbsigs/bbsigs.go:41-45
    u, v = _scale_generator(curve, G2, [x, y])
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
    return [Signature(s, r) for s, r in zip(_scale_generator(curve, G1, es), rs)]


def _batchable(curve, sig, pk):
    return (isinstance(sig, Signature) and isinstance(pk, Pubkey) and isinstance(sig.Sigma, Point) and sig.Sigma.curve is curve
            and sig.Sigma.group == G1 and all(isinstance(p, Point) and p.curve is curve and p.group == G2 for p in (pk.U, pk.V)))


def _verify_batch(curve, sigs, pks, msgs):
    """One bgls_bb_verify_batch call for the items made of this curve's Points (any other item is rejected, as a mismatched
    Add / Pair in the reference yields a result that never equals GetGT()).  A call that fails as a whole (an encoding error
    somewhere in the batch) is settled item by item."""
    if not (len(sigs) == len(pks) == len(msgs)):
        raise ValueError("sigs, pks and msgs differ in length")
    out = [False] * len(sigs)
    batch = [b for b in range(len(sigs)) if _batchable(curve, sigs[b], pks[b])]
    if not batch:
        return out
    n = len(batch)
    verdicts = (ctypes.c_uint8 * n)()
    rc = _lib.load().bgls_bb_verify_batch(curve.id, _lib.buf(b"".join(sigs[b].Sigma.raw for b in batch)),
                                          _lib.buf(b"".join(_mag(curve, sigs[b].R) for b in batch)),
                                          _lib.buf(b"".join(pks[b].U.raw + pks[b].V.raw for b in batch)),
                                          _lib.buf(b"".join(_mag(curve, msgs[b]) for b in batch)), n, verdicts, None)
    if rc < 0 and n > 1:
        for b in batch:
            out[b] = _verify_batch(curve, [sigs[b]], [pks[b]], [msgs[b]])[0]
        return out
    for i, b in enumerate(batch):
        out[b] = rc >= 0 and verdicts[i] == 1
    return out


def Verify(curve, sig, pk, msg):                    # bbsigs/bbsigs.go:68-73
    return _verify_batch(curve, [sig], [pk], [msg])[0]


def VerifyBatch(curve, sigs, pks, msgs):
    """len(sigs) independent Verify calls in one bgls_bb_verify_batch call: a list of bools, one per item."""
    return _verify_batch(curve, sigs, pks, msgs)


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
