"""What curves.py, bgls.py and bbsigs.py share in front of the C ABI: the Point test, prefix offsets, point blobs, 32-byte scalar
magnitudes, and the one batch-and-settle runner behind every call that returns a verdict per item."""
import ctypes
from itertools import accumulate
from . import _lib, curves              # curves imports this module while it is being imported itself: Point is looked up at call time


def is_point(p, curve, group):
    return isinstance(p, curves.Point) and p.curve is curve and p.group == group


def all_points(ps, curve, group):
    return all(is_point(p, curve, group) for p in ps)


def prefix_u64(lengths):
    """len + 1 prefix sums, as the ABI's key_off / inst_off / msg_off / signer_off arrays"""
    sums = list(accumulate(lengths, initial=0))
    return (ctypes.c_uint64 * len(sums))(*sums)


def msgs_arg(ms):
    """(msg_blob, msg_off) of a list of bytes"""
    return _lib.buf(b"".join(ms)), prefix_u64(len(m) for m in ms)


def cat(points):
    return _lib.buf(b"".join(p.raw for p in points))


def split_points(curve, group, raw, n):
    size = curve._pt_size(group)
    return [curves.Point(curve, group, raw[i * size:(i + 1) * size]) for i in range(n)]


def mag32(curve, k):
    """A scalar as the ABI's 32-byte magnitude.  The reference multiplies by the exact big.Int; on points of order r (every validated
    Point, every GT element) a negative scalar or one of 2^256 and above acts as its residue modulo the group order, so those are reduced
    modulo GetG1Order() -- in every path, never modulo 2^256; every other value is passed unreduced."""
    return (k % curve.GetG1Order() if k < 0 or k >= 1 << 256 else k).to_bytes(32, "big")


def scale_generator(curve, group, scalars):
    """scalars[i] times the generator of `group` in one bgls_scale_generator call"""
    n = len(scalars)
    if n == 0:
        return []
    o = _lib.out(n * len(curve._gen(group).raw))
    rc = _lib.load().bgls_scale_generator(curve.id, group, _lib.buf(b"".join(mag32(curve, k) for k in scalars)), n, o)
    if rc != 0:
        raise RuntimeError("bgls_scale_generator: %s" % _lib.last_error())
    return split_points(curve, group, bytes(o), n)


def settle(n, batchable, call, single=None):
    """The verdicts of n items, equal to what n single calls would say, from ONE batch call where that is possible.

    batchable(b): item b is made of this curve's Points and can travel in a batch.  call(items) -> (rc, verdicts) sends the items of an
    index list in one C call.  single(b) -> bool is the single call's answer for item b; None where a nil or foreign point is simply False
    and the single call is a batch of one.

    The rule: the items that are not batchable are answered first, one by one (single, or False).  The others go into one call.  If it
    fails as a whole (rc < 0: an encoding or hashing error somewhere in the batch), each of its items is settled alone, in index order:
    through single, or through call([b]).  A failed batch of ONE item without a single is False: sending it again would fail again."""
    out = [False] * n
    batch = []
    for b in range(n):
        if batchable(b):
            batch.append(b)
        elif single is not None:
            out[b] = single(b)
    if not batch:
        return out
    rc, verdicts = call(batch)
    for i, b in enumerate(batch):
        if rc >= 0:
            out[b] = verdicts[i] == 1
        elif single is not None:
            out[b] = single(b)
        elif len(batch) > 1:
            rc1, v1 = call([b])
            out[b] = rc1 >= 0 and v1[0] == 1
    return out
