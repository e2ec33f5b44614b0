"""Host-side mirror of the reference's `bgls` scheme functions on the hot path
(bgls/bgls.go, bgls/blsKosk.go), same names and semantics, each routed to ONE batch C call.  The calls that return one verdict per
item are a predicate, a closure that marshals a list of items, and _marshal.settle, which states the batch-and-settle rule once."""
import ctypes
import os
import secrets
from . import _lib
from ._marshal import all_points, cat, is_point, mag32, msgs_arg, prefix_u64, scale_generator, settle, split_points
from .curves import AggregatePoints, ScalePoints, Point, G1, G2


def KeyGen(curve):                                   # bgls/bgls.go:30-37
    x = secrets.randbelow(curve.GetG1Order())
    return x, LoadPublicKey(curve, x), None


def LoadPublicKey(curve, sk):                        # bgls/bgls.go:40-43
    return curve.GetG2().Mul(sk)


def Sign(curve, sk, msg):                            # bgls/bgls.go:46-56
    return curve.HashToG1(msg).Mul(sk)


def _kosk1(msg):                                     # the proof-of-possession schemes sign and verify 0x01 || msg (bgls/blsKosk.go:73-77)
    return b"\x01" + bytes(msg)


def _kosk(msgs):
    return [_kosk1(m) for m in msgs]


def KoskSign(curve, sk, msg):                        # bgls/blsKosk.go:73-77
    return Sign(curve, sk, _kosk1(msg))


def AggregateSignatures(sigs):                       # bgls/bgls.go:123-125
    return AggregatePoints(sigs)


def AggregateKeys(keys):                             # bgls/bgls.go:129-131
    return AggregatePoints(keys)


class KeySet:
    """n public keys resident on the GPU(s) behind a bgls_keys_t handle (include/bgls_hip.h): what a []Point of public
    keys becomes in the Go shim.  Accepted wherever the Verify* functions take `keys`.  check = the construction-time
    validation of MakeG2Point / UnmarshalG2 (subgroup membership included); devices = one entry per shard."""

    def __init__(self, curve, keys, devices=None, check=True):
        raw = b"".join(k.raw for k in keys) if keys and isinstance(keys[0], Point) else bytes(keys)
        n = len(raw) // (4 * curve.fp_bytes)
        h = ctypes.c_uint64()
        devs = list(devices) if devices else None     # NULL + one shard: the process' default device (bgls_init / bgls_select_device), as in the C++ and Go mirrors
        rc = _lib.load().bgls_keys_upload(curve.id, _lib.buf(raw), n, (ctypes.c_int * len(devs))(*devs) if devs else None, len(devs) if devs else 1,
                                          1 if check else 0, ctypes.byref(h))
        if rc != 0:
            raise ValueError("bgls_keys_upload: %d %s" % (rc, _lib.last_error()))
        self.curve, self.n, self.handle = curve, n, h.value

    @classmethod
    def from_compressed(cls, curve, keys, devices=None, prepare=False):
        """A key set from compressed keys (Point.Marshal: 64 / 96 bytes each; bytes or a list of encodings), decoded and validated on the
        device(s) in one pass as UnmarshalG2 does (bgls_keys_upload_compressed).  ValueError names the first refused key."""
        raw = bytes(keys) if isinstance(keys, (bytes, bytearray, memoryview)) else b"".join(bytes(k) for k in keys)
        cb = 2 * curve.fp_bytes
        if len(raw) % cb:
            raise ValueError("compressed keys: %d bytes is not a multiple of %d" % (len(raw), cb))
        n = len(raw) // cb
        h, bad = ctypes.c_uint64(), ctypes.c_size_t(n)
        devs = list(devices) if devices else None
        rc = _lib.load().bgls_keys_upload_compressed(curve.id, _lib.buf(raw), n, (ctypes.c_int * len(devs))(*devs) if devs else None, len(devs) if devs else 1,
                                                     2 if prepare else 0, ctypes.byref(h), ctypes.byref(bad))
        if rc == -2 and bad.value < n:
            raise ValueError("bgls_keys_upload_compressed: key %d was refused: %s" % (bad.value, _lib.last_error()))
        if rc != 0:
            raise ValueError("bgls_keys_upload_compressed: %d %s" % (rc, _lib.last_error()))
        self = cls.__new__(cls)
        self.curve, self.n, self.handle = curve, n, h.value
        return self

    def keys(self):
        """the set's keys as Points, read back from the device(s) (bgls_keys_read)"""
        out = _lib.out(self.n * 4 * self.curve.fp_bytes)
        rc = _lib.load().bgls_keys_read(self.handle, 0, self.n, out)
        if rc != 0:
            raise ValueError("bgls_keys_read: %d %s" % (rc, _lib.last_error()))
        return split_points(self.curve, G2, bytes(out), self.n)

    def __len__(self):
        return self.n

    def free(self):
        if self.handle:
            _lib.load().bgls_keys_free(self.handle)
            self.handle = 0

    def __del__(self):                                # the Go shim's runtime.SetFinalizer
        try:
            self.free()
        except Exception:
            pass


def _verify_agg(curve, aggsig, keys, msgs, allow_duplicates):
    if len(keys) != len(msgs):                       # bgls/bgls.go:95-97
        return False
    if not is_point(aggsig, curve, G1):
        return False
    if isinstance(keys, KeySet):
        if keys.curve is not curve:
            return False
        return _lib.load().bgls_verify_aggregate_h(keys.handle, _lib.buf(aggsig.raw), *msgs_arg([bytes(m) for m in msgs]), len(msgs),
                                                   1 if allow_duplicates else 0) == 1
    if not all_points(keys, curve, G2):
        return False
    rc = _lib.load().bgls_verify_aggregate(curve.id, _lib.buf(aggsig.raw), cat(keys), *msgs_arg([bytes(m) for m in msgs]), len(msgs),
                                           1 if allow_duplicates else 0)
    return rc == 1                                   # every failure collapses to false (bgls.go:115-118)


def VerifyAggregateSignature(curve, aggsig, keys, msgs):      # bgls/bgls.go:82-84
    return _verify_agg(curve, aggsig, keys, msgs, False)


def KoskVerifyAggregateSignature(curve, aggsig, keys, msgs):  # bgls/blsKosk.go:100-106
    return _verify_agg(curve, aggsig, keys, _kosk(msgs), True)


def GroupMessages(msgs):
    """(group_of, n_groups): group_of[i] is the number of the group of msgs[i]; two messages share a group iff their bytes are equal, and
    groups are numbered in the order of their first occurrence (bgls_group_messages: the grouping runs on the device)."""
    ms = [bytes(m) for m in msgs]
    n = len(ms)
    group_of = (ctypes.c_uint32 * max(n, 1))()
    n_groups = ctypes.c_size_t(0)
    rc = _lib.load().bgls_group_messages(*msgs_arg(ms), n, group_of, ctypes.byref(n_groups))
    if rc != 0:
        raise RuntimeError("bgls_group_messages: %d %s" % (rc, _lib.last_error()))
    return list(group_of)[:n], n_groups.value


def VerifyAggregateSignatureGrouped(curve, aggsig, keys, msgs):
    """KoskVerifyAggregateSignature's body (verifyAggSig with allowDuplicates = true, bgls/blsKosk.go:100-106) with one hash and one
    pairing per DISTINCT message: the keys of the signers of one message are summed first (bgls_verify_aggregate_grouped).  Same verdict
    as _verify_agg(..., True); messages are grouped by exact bytes; there is no duplicate rule.  keys: a list of G2 Points -- for a
    resident KeySet use VerifyAggregateSignatureGroupedBySubset (or, for one message per set, the signer-bitmap calls
    VerifyMultiSignaturesBySubset, AggregateKeysBySubset)."""
    if isinstance(keys, KeySet):
        raise TypeError("VerifyAggregateSignatureGrouped takes a list of keys; over a KeySet use VerifyAggregateSignatureGroupedBySubset "
                        "(or the signer-bitmap calls VerifyMultiSignaturesBySubset / AggregateKeysBySubset)")
    if len(keys) != len(msgs):                       # bgls/bgls.go:95-97
        return False
    if not (is_point(aggsig, curve, G1) and all_points(keys, curve, G2)):
        return False
    rc = _lib.load().bgls_verify_aggregate_grouped(curve.id, _lib.buf(aggsig.raw), cat(keys), *msgs_arg([bytes(m) for m in msgs]), len(msgs), None, None)
    return rc == 1                                   # every failure collapses to false (bgls.go:115-118)


def KoskVerifyAggregateSignatureGrouped(curve, aggsig, keys, msgs):  # bgls/blsKosk.go:100-106
    return VerifyAggregateSignatureGrouped(curve, aggsig, keys, _kosk(msgs))


def VerifyAggregateSignatureGroupedBySubset(curve, aggsig, keyset, subset, msgs):
    """VerifyAggregateSignatureGrouped whose keys are a sub-slice of a resident KeySet (bgls_verify_aggregate_grouped_h): nothing of a key
    travels.  subset: None (every key; msgs[i] belongs to key i), a bytes bitmap (key i selected iff (bitmap[i >> 3] >> (i & 7)) & 1; msgs in
    ascending key order) or a list of key indices, msgs parallel to the list as given -- a repeated index is a ValueError.  Every failure
    of the call collapses to False (bgls.go:115-118)."""
    if not isinstance(keyset, KeySet):
        raise TypeError("VerifyAggregateSignatureGroupedBySubset takes a KeySet")
    n = len(keyset)
    ms = [bytes(m) for m in msgs]
    if subset is None:
        bitmap = None
    elif isinstance(subset, (bytes, bytearray, memoryview)):
        bitmap = bytes(subset)
    else:
        idx = [int(i) for i in subset]
        if len(set(idx)) != len(idx):
            raise ValueError("a key index is repeated in the subset")
        if any(not 0 <= i < n for i in idx):
            raise ValueError("a key index lies outside the key set")
        if len(idx) != len(ms):                      # bgls/bgls.go:95-97
            return False
        order = sorted(range(len(idx)), key=lambda j: idx[j])
        ms = [ms[j] for j in order]
        bitmap = _subset_rows(keyset, [idx])[0]
    if keyset.curve is not curve or not is_point(aggsig, curve, G1):
        return False
    rc = _lib.load().bgls_verify_aggregate_grouped_h(keyset.handle, _lib.buf(aggsig.raw), None if bitmap is None else _lib.buf(bitmap),
                                                     0 if bitmap is None else len(bitmap), *msgs_arg(ms), len(ms), None, None)
    return rc == 1


def KoskVerifyAggregateSignatureGroupedBySubset(curve, aggsig, keyset, subset, msgs):  # bgls/blsKosk.go:100-106
    return VerifyAggregateSignatureGroupedBySubset(curve, aggsig, keyset, subset, _kosk(msgs))


def _set_ok(curve, sig, keys):
    """a G1 signature and a list of G2 keys of this curve: what the batch entries over sets of keys take"""
    return is_point(sig, curve, G1) and not isinstance(keys, KeySet) and all_points(keys, curve, G2)


def _sets_call(entry, curve, sigs, keys, msgs, before=(), after=(None,)):
    """settle()'s call(items) for the batch entries over sets of keys (bgls_verify_aggregate_batch, _distinct_batch, bgls_verify_multi_sets,
    _hae_sets): the signatures, the keys keys[b] and the messages msgs[b] (a list) of the items in order, key_off / inst_off counting
    keys; before / after: what the entry takes around `verdicts`."""
    def call(items):
        verdicts = _lib.out(len(items))
        rc = getattr(_lib.load(), entry)(curve.id, cat(sigs[b] for b in items), cat(k for b in items for k in keys[b]),
                                         prefix_u64(len(keys[b]) for b in items), len(items),
                                         *msgs_arg([bytes(m) for b in items for m in msgs[b]]), *before, verdicts, *after)
        return rc, verdicts
    return call


def _verify_agg_batch(curve, aggsigs, keys_per_instance, msgs_per_instance, allow_duplicates):
    """One bgls_verify_aggregate_batch call for every instance made of Points of this curve; an instance that is not (mismatched lengths,
    a foreign point, a KeySet) gets what _verify_agg says about it alone (_marshal.settle)."""
    if not (len(aggsigs) == len(keys_per_instance) == len(msgs_per_instance)):
        raise ValueError("aggsigs, keys_per_instance and msgs_per_instance differ in length")
    return settle(len(aggsigs),
                  lambda b: _set_ok(curve, aggsigs[b], keys_per_instance[b]) and len(keys_per_instance[b]) == len(msgs_per_instance[b]),
                  _sets_call("bgls_verify_aggregate_batch", curve, aggsigs, keys_per_instance, msgs_per_instance, before=(1 if allow_duplicates else 0,)),
                  lambda b: _verify_agg(curve, aggsigs[b], keys_per_instance[b], msgs_per_instance[b], allow_duplicates))


def VerifyAggregateSignatures(curve, aggsigs, keys_per_instance, msgs_per_instance):
    """len(aggsigs) independent VerifyAggregateSignature calls (bgls/bgls.go:82-84) in one batch: a list of bools, one per instance."""
    return _verify_agg_batch(curve, aggsigs, keys_per_instance, msgs_per_instance, False)


def KoskVerifyAggregateSignatures(curve, aggsigs, keys_per_instance, msgs_per_instance):
    """The batch of KoskVerifyAggregateSignature calls (bgls/blsKosk.go:100-106): 0x01 prepended to every message, duplicates allowed."""
    return _verify_agg_batch(curve, aggsigs, keys_per_instance, [_kosk(ms) for ms in msgs_per_instance], True)


def _verify_multi(curve, aggsig, keys, msg):                  # bgls/bgls.go:89-92
    if not is_point(aggsig, curve, G1):
        return False                                 # a nil / foreign aggsig is `false`, never an exception
    if isinstance(keys, KeySet):
        if keys.curve is not curve:
            return False
        return _lib.load().bgls_verify_multi_h(keys.handle, _lib.buf(aggsig.raw), _lib.buf(msg), len(msg)) == 1
    if not all_points(keys, curve, G2):
        return False
    rc = _lib.load().bgls_verify_multi(curve.id, _lib.buf(aggsig.raw), cat(keys), len(keys), _lib.buf(msg), len(msg))
    return rc == 1


def VerifySingleSignature(curve, sig, pubkey, msg):           # bgls/bgls.go:59-70
    return _verify_multi(curve, sig, [pubkey], bytes(msg))


def KoskVerifySingleSignature(curve, sig, pubkey, msg):       # bgls/blsKosk.go:86-90
    return VerifySingleSignature(curve, sig, pubkey, _kosk1(msg))


def KoskVerifyMultiSignature(curve, aggsig, keys, msg):       # bgls/blsKosk.go:117-120
    return _verify_multi(curve, aggsig, keys, _kosk1(msg))


def _verify_multi_sets(curve, aggsigs, keys_per_set, msgs):
    """One bgls_verify_multi_sets call for every set made of Points of this curve; a set that is not (a nil or foreign signature, a
    foreign key, a KeySet) gets what _verify_multi says about it alone (_marshal.settle)."""
    if not (len(aggsigs) == len(keys_per_set) == len(msgs)):
        raise ValueError("aggsigs, keys_per_set and msgs differ in length")
    return settle(len(aggsigs), lambda b: _set_ok(curve, aggsigs[b], keys_per_set[b]),
                  _sets_call("bgls_verify_multi_sets", curve, aggsigs, keys_per_set, [[m] for m in msgs]),
                  lambda b: _verify_multi(curve, aggsigs[b], keys_per_set[b], bytes(msgs[b])))


def VerifyMultiSignatures(curve, aggsigs, pubkeys, msgs):
    """len(aggsigs) independent verifyMultiSignature calls (bgls/bgls.go:89-92) in one batch: a list of bools, one per set."""
    return _verify_multi_sets(curve, aggsigs, pubkeys, msgs)


def KoskVerifyMultiSignatures(curve, aggsigs, pubkeys, msgs):
    """len(aggsigs) independent KoskVerifyMultiSignature calls (bgls/blsKosk.go:117-120) in one batch: 0x01 prepended to every message,
    a list of bools, one per set (pubkeys[b]: the signers of msgs[b])."""
    return _verify_multi_sets(curve, aggsigs, pubkeys, _kosk(msgs))


def _subset_rows(keyset, subsets):
    """The bitmap rows of `subsets` over a KeySet, ceil(n / 8) bytes each: a subset is a list of key indices (each below len(keyset), a
    repeated index counts once) or a bytes bitmap (key i selected iff (row[i >> 3] >> (i & 7)) & 1, at most ceil(n / 8) bytes)."""
    n = len(keyset)
    stride = (n + 7) // 8
    rows = bytearray(stride * len(subsets))
    for b, sub in enumerate(subsets):
        if isinstance(sub, (bytes, bytearray, memoryview)):
            sub = bytes(sub)
            if len(sub) > stride:
                raise ValueError("subset %d: a bitmap of %d bytes over %d keys" % (b, len(sub), n))
            rows[b * stride:b * stride + len(sub)] = sub
        else:
            for i in sub:
                if not 0 <= i < n:
                    raise ValueError("subset %d: key index %d outside the key set" % (b, i))
                rows[b * stride + (i >> 3)] |= 1 << (i & 7)
    return bytes(rows), stride


def AggregateKeysBySubset(keyset, subsets):
    """AggregateKeys (bgls/bgls.go:129-131) over len(subsets) sub-slices of a resident KeySet in one bgls_aggregate_subsets_h call: a list
    of G2 Points.  Nothing of a key travels: a subset is an index list or a bytes bitmap over the registered keys."""
    if not isinstance(keyset, KeySet):
        raise TypeError("AggregateKeysBySubset takes a KeySet")
    if not subsets:
        return []
    curve = keyset.curve
    rows, stride = _subset_rows(keyset, subsets)
    out = _lib.out(len(subsets) * 4 * curve.fp_bytes)
    rc = _lib.load().bgls_aggregate_subsets_h(keyset.handle, _lib.buf(rows), stride, len(subsets), out)
    if rc != 0:
        raise ValueError("bgls_aggregate_subsets_h: %d %s" % (rc, _lib.last_error()))
    return split_points(curve, G2, bytes(out), len(subsets))


def VerifyMultiSignaturesBySubset(curve, aggsigs, keyset, subsets, msgs):
    """len(aggsigs) independent verifyMultiSignature calls (bgls/bgls.go:89-92) whose signers are sub-slices of ONE resident KeySet -- a
    MultiSig{keys, sig, msg} over registered keys is one row -- in one bgls_verify_multi_subsets_h call: a list of bools, one per set.  A
    nil or foreign signature is False without a call; a call that fails as a whole (an off-curve signature, an exhausted hash) is settled
    set by set through calls of one row (_marshal.settle)."""
    if not isinstance(keyset, KeySet):
        raise TypeError("VerifyMultiSignaturesBySubset takes a KeySet")
    if not (len(aggsigs) == len(subsets) == len(msgs)):
        raise ValueError("aggsigs, subsets and msgs differ in length")
    if keyset.curve is not curve:
        return [False] * len(aggsigs)

    def call(items):
        rows, stride = _subset_rows(keyset, [subsets[b] for b in items])
        verdicts = _lib.out(len(items))
        rc = _lib.load().bgls_verify_multi_subsets_h(keyset.handle, cat(aggsigs[b] for b in items), _lib.buf(rows), stride, len(items),
                                                     *msgs_arg([bytes(msgs[b]) for b in items]), verdicts, None, None)
        return rc, verdicts

    return settle(len(aggsigs), lambda b: is_point(aggsigs[b], curve, G1), call)


def KoskVerifyMultiSignaturesBySubset(curve, aggsigs, keyset, subsets, msgs):
    """The same for KoskVerifyMultiSignature (bgls/blsKosk.go:117-120): 0x01 prepended to every message."""
    return VerifyMultiSignaturesBySubset(curve, aggsigs, keyset, subsets, _kosk(msgs))


def _group_offsets(n, group):
    """n_groups + 1 offsets of consecutive chunks of `group` sets (None: one group)"""
    if group is None:
        return [0, n]
    if int(group) < 1:
        raise ValueError("group must be a positive chunk size or None")
    return list(range(0, n, int(group))) + [n]


def VerifyMultiSignaturesCombined(curve, aggsigs, pubkeys, msgs, group=None, seed=None):
    """"Are these multi-signatures all valid?" under one combined check per group of consecutive sets (bgls_verify_multi_sets_combined:
    one final exponentiation per group instead of one per set).  group: an int chunk size, or None for one group over all sets;
    seed: 32 bytes from a CSPRNG drawn AFTER the inputs are fixed (None draws os.urandom(32)).  Returns the list of group verdicts; a
    group that holds a set bgls_verify_multi rejects is rejected except with probability about 2^-127.  Every set must be made of
    Points of this curve; an encoding or hashing error anywhere raises ValueError (use VerifyMultiSignatures to settle such a batch)."""
    n = len(aggsigs)
    if not (n == len(pubkeys) == len(msgs)):
        raise ValueError("aggsigs, pubkeys and msgs differ in length")
    if seed is None:
        seed = os.urandom(32)
    if len(seed) != 32:
        raise ValueError("seed must be 32 bytes")
    if n == 0:
        return []
    if not all(is_point(sig, curve, G1) and all_points(keys, curve, G2) for sig, keys in zip(aggsigs, pubkeys)):
        raise ValueError("the combined check takes G1 / G2 Points of this curve only")
    goff = _group_offsets(n, group)
    verdicts = _lib.out(len(goff) - 1)
    rc = _lib.load().bgls_verify_multi_sets_combined(curve.id, cat(aggsigs), cat(k for keys in pubkeys for k in keys),
                                                     prefix_u64(len(keys) for keys in pubkeys), n, *msgs_arg([bytes(m) for m in msgs]),
                                                     (ctypes.c_uint64 * len(goff))(*goff), len(goff) - 1, _lib.buf(bytes(seed)), verdicts, None)
    if rc < 0:
        raise ValueError("bgls_verify_multi_sets_combined: %s" % _lib.last_error())
    return [v == 1 for v in verdicts]


def KoskVerifyMultiSignaturesCombined(curve, aggsigs, pubkeys, msgs, group=None, seed=None):
    """VerifyMultiSignaturesCombined with 0x01 prepended to every message (bgls/blsKosk.go:117-120)."""
    return VerifyMultiSignaturesCombined(curve, aggsigs, pubkeys, _kosk(msgs), group, seed)


def VerifyMultiSignaturesLocated(curve, aggsigs, pubkeys, msgs, group=64, seed=None):
    """One verdict per set at the combined check's cost where everything is valid: ONE combined call over groups of `group` sets, then
    ONE VerifyMultiSignatures call over only the sets of the rejected groups; the sets of accepted groups get True."""
    n = len(aggsigs)
    goff = _group_offsets(n, group)
    groups = VerifyMultiSignaturesCombined(curve, aggsigs, pubkeys, msgs, group, seed)
    out = [True] * n
    again = [b for g, ok in enumerate(groups) if not ok for b in range(goff[g], goff[g + 1])]
    if again:
        for b, v in zip(again, VerifyMultiSignatures(curve, [aggsigs[b] for b in again], [pubkeys[b] for b in again], [msgs[b] for b in again])):
            out[b] = v
    return out


def VerifySingleSignatures(curve, sigs, pubkeys, msgs):
    """len(sigs) independent VerifySingleSignature calls (bgls/bgls.go:59-70) in one batch: one key per set, a list of bools."""
    return _verify_multi_sets(curve, sigs, [[pk] for pk in pubkeys], msgs)


def KoskVerifySingleSignatures(curve, sigs, pubkeys, msgs):
    """The batch of KoskVerifySingleSignature calls (bgls/blsKosk.go:86-90): 0x01 prepended to every message."""
    return VerifySingleSignatures(curve, sigs, pubkeys, _kosk(msgs))


def KoskVerifyBatchMultiSignature(curve, aggsigs, pubkeys, msgs):      # bgls/blsKosk.go:126-133
    """aggsigs: one multi-signature per message, pubkeys[i]: the signers of message i.  One call: the key sums of all sets
    in one launch, then ONE aggregate verification over len(msgs) pairs (the reference: AggregateSignatures, len(msgs) x
    AggregateKeys, KoskVerifyAggregateSignature)."""
    if len(aggsigs) != len(pubkeys) or len(pubkeys) != len(msgs) or not msgs:
        return False
    if not (all_points(aggsigs, curve, G1) and all(all_points(ks, curve, G2) for ks in pubkeys)):
        return False
    rc = _lib.load().bgls_verify_multi_batch(curve.id, cat(aggsigs), cat(k for ks in pubkeys for k in ks), prefix_u64(len(ks) for ks in pubkeys),
                                             len(msgs), *msgs_arg(_kosk(msgs)), 1)
    return rc == 1


class AggSig:                                                 # bgls/bgls.go:22-26,73-75
    def __init__(self, keys, msgs, sig):
        self.keys, self.msgs, self.sig = keys, msgs, sig

    def Verify(self, curve):
        return VerifyAggregateSignature(curve, self.sig, self.keys, self.msgs)


class MultiSig:                                               # bgls/bgls.go:15-19, blsKosk.go:110-112
    def __init__(self, keys, sig, msg):
        self.keys, self.sig, self.msg = keys, sig, msg

    def Verify(self, curve):
        return KoskVerifyMultiSignature(curve, self.sig, self.keys, self.msg)


# ---- hashed aggregation exponents (bgls/blsHAE.go) -----------------------------------------------------------
def hashPubKeysToExponents(pubkeys):                          # bgls/blsHAE.go:80-93
    if not pubkeys:
        return []
    curve = getattr(pubkeys[0], "curve", None)
    if curve is None or not all_points(pubkeys, curve, G2):   # the C side reads n * g2_size bytes: G2 points of ONE curve only
        raise TypeError("hashPubKeysToExponents takes G2 public keys of one curve")
    o = _lib.out(16 * len(pubkeys))
    rc = _lib.load().bgls_hae_exponents(curve.id, cat(pubkeys), len(pubkeys), o)
    if rc != 0:
        raise RuntimeError("bgls_hae_exponents: %s" % _lib.last_error())
    raw = bytes(o)
    return [int.from_bytes(raw[16 * i:16 * i + 16], "big") for i in range(len(pubkeys))]


def AggregateSignaturesWithHAE(sigs, pubkeys):                # bgls/blsHAE.go:39-46
    if len(pubkeys) != len(sigs):
        return None
    if not sigs:
        return AggregatePoints(sigs)
    curve = sigs[0].curve
    if not (all_points(pubkeys, curve, G2) and all_points(sigs, curve, G1)):
        return None
    o = _lib.out(len(sigs[0].raw))
    rc = _lib.load().bgls_aggregate_signatures_hae(curve.id, cat(sigs), cat(pubkeys), len(sigs), o)
    return Point(curve, G1, bytes(o)) if rc == 0 else None


def VerifyAggregateSignatureWithHAE(curve, aggsig, pubkeys, msgs):   # bgls/blsHAE.go:49-53
    if len(pubkeys) != len(msgs) or not all_points(pubkeys, curve, G2) or not is_point(aggsig, curve, G1):
        return False
    rc = _lib.load().bgls_verify_aggregate_hae(curve.id, _lib.buf(aggsig.raw), cat(pubkeys), *msgs_arg([bytes(m) for m in msgs]), len(msgs))
    return rc == 1


def VerifyMultiSignatureWithHAE(curve, aggsig, pubkeys, msg):        # bgls/blsHAE.go:56-58
    if not all_points(pubkeys, curve, G2) or not is_point(aggsig, curve, G1):
        return False
    rc = _lib.load().bgls_verify_multi_hae(curve.id, _lib.buf(aggsig.raw), cat(pubkeys), len(pubkeys), _lib.buf(msg), len(msg))
    return rc == 1


def VerifyMultiSignaturesWithHAE(curve, aggsigs, pubkeys, msgs):
    """len(aggsigs) independent VerifyMultiSignatureWithHAE calls (bgls/blsHAE.go:56-58) in one bgls_verify_multi_hae_sets call: a list
    of bools, one per set.  A set that is not made of Points of this curve (a nil or foreign signature, a foreign key, a KeySet) gets
    what VerifyMultiSignatureWithHAE says about it alone (_marshal.settle)."""
    if not (len(aggsigs) == len(pubkeys) == len(msgs)):
        raise ValueError("aggsigs, pubkeys and msgs differ in length")
    return settle(len(aggsigs), lambda b: _set_ok(curve, aggsigs[b], pubkeys[b]),
                  _sets_call("bgls_verify_multi_hae_sets", curve, aggsigs, pubkeys, [[m] for m in msgs], after=(None, None)),
                  lambda b: VerifyMultiSignatureWithHAE(curve, aggsigs[b], pubkeys[b], bytes(msgs[b])))


def KoskVerifyMultiSignatureWithMultiplicity(curve, aggsig, keys, multiplicity, msg):   # bgls/blsKosk.go:137-150
    if multiplicity is None:
        return KoskVerifyMultiSignature(curve, aggsig, keys, msg)
    if len(keys) != len(multiplicity):
        return False
    if not all_points(keys, curve, G2) or not is_point(aggsig, curve, G1):
        return False
    m2 = _kosk1(msg)
    mult = (ctypes.c_int64 * max(1, len(keys)))(*[int(m) for m in multiplicity])
    rc = _lib.load().bgls_verify_multi_multiplicity(curve.id, _lib.buf(aggsig.raw), cat(keys), mult, len(keys), _lib.buf(m2), len(m2))
    return rc == 1


# ---- batch forms of KeyGen / Sign -------------------------------------------------------------
def LoadPublicKeys(curve, sks):
    """LoadPublicKey (bgls/bgls.go:40-43) for a list of secret keys in one call."""
    return scale_generator(curve, G2, sks)


def SignBatch(curve, sks, msgs, kosk=False):
    """Sign / KoskSign (bgls/bgls.go:46-56, bgls/blsKosk.go:73-77) for n (secret key, message) pairs in one call."""
    n = len(sks)
    if n != len(msgs):
        return None
    if n == 0:
        return []
    o = _lib.out(n * len(curve.GetG1().raw))
    rc = _lib.load().bgls_sign_batch(curve.id, _lib.buf(b"".join(mag32(curve, sk) for sk in sks)),
                                     *msgs_arg(_kosk(msgs) if kosk else [bytes(m) for m in msgs]), n, o)
    if rc != 0:
        raise RuntimeError("bgls_sign_batch: %s" % _lib.last_error())
    return split_points(curve, G1, bytes(o), n)


# ---- wrappers that are byte concatenation in front of the same path ---------------------------------------------
def DistinctMsgSign(curve, sk, msg):                          # bgls/blsDistinctMessage.go:23-34
    return Sign(curve, sk, LoadPublicKey(curve, sk).MarshalUncompressed() + bytes(msg))


def _verify_single_keyed(curve, sigs, pubkeys, msgs):
    """One bgls_verify_single_distinct_batch (msgs a list) or bgls_check_authentication_batch (msgs None) call for the items made of
    Points of this curve; a nil or foreign point is False, as the single path says.  A call that fails as a whole (an encoding or hashing
    error somewhere in the batch) is settled item by item through batches of one (_marshal.settle)."""
    n = len(sigs)
    if n != len(pubkeys) or (msgs is not None and n != len(msgs)):
        raise ValueError("sigs, pubkeys and msgs differ in length")

    def call(items):
        verdicts = _lib.out(len(items))
        sg, ks = cat(sigs[b] for b in items), cat(pubkeys[b] for b in items)
        if msgs is None:
            rc = _lib.load().bgls_check_authentication_batch(curve.id, ks, sg, len(items), verdicts, None)
        else:
            rc = _lib.load().bgls_verify_single_distinct_batch(curve.id, sg, ks, *msgs_arg([bytes(msgs[b]) for b in items]), len(items), verdicts, None)
        return rc, verdicts

    return settle(n, lambda b: is_point(sigs[b], curve, G1) and is_point(pubkeys[b], curve, G2), call)


def DistinctMsgVerifySingleSignature(curve, sig, pubkey, msg):   # bgls/blsDistinctMessage.go:37-40
    return _verify_single_keyed(curve, [sig], [pubkey], [msg])[0]


def DistinctMsgVerifySingleSignatures(curve, sigs, pubkeys, msgs):
    """len(sigs) independent DistinctMsgVerifySingleSignature calls in one batch: a list of bools.  The key bytes are put in front of
    every message on the device."""
    return _verify_single_keyed(curve, sigs, pubkeys, msgs)


def DistinctMsgVerifyAggregateSignature(curve, aggsig, keys, msgs):   # bgls/blsDistinctMessage.go:45-57
    """keys: a list of G2 Points or a KeySet.  The key bytes are put in front of every message on the device (from the resident wire
    bytes of a KeySet); there is no duplicate rule."""
    if len(keys) != len(msgs):
        return False
    if not is_point(aggsig, curve, G1):
        return False
    blob, off = msgs_arg([bytes(m) for m in msgs])
    if isinstance(keys, KeySet):
        if keys.curve is not curve:
            return False
        return _lib.load().bgls_verify_aggregate_distinct_h(keys.handle, _lib.buf(aggsig.raw), blob, off, len(msgs), None) == 1
    if not all_points(keys, curve, G2):
        return False
    return _lib.load().bgls_verify_aggregate_distinct(curve.id, _lib.buf(aggsig.raw), cat(keys), blob, off, len(msgs)) == 1


def DistinctMsgVerifyAggregateSignatures(curve, aggsigs, keys_per_instance, msgs_per_instance):
    """len(aggsigs) independent DistinctMsgVerifyAggregateSignature calls in one batch (bgls_verify_aggregate_distinct_batch): a list of
    bools, one per instance.  An instance that is not made of Points of this curve (mismatched lengths, a foreign point, a KeySet) gets
    what the single call says about it (_marshal.settle)."""
    if not (len(aggsigs) == len(keys_per_instance) == len(msgs_per_instance)):
        raise ValueError("aggsigs, keys_per_instance and msgs_per_instance differ in length")
    return settle(len(aggsigs),
                  lambda b: _set_ok(curve, aggsigs[b], keys_per_instance[b]) and len(keys_per_instance[b]) == len(msgs_per_instance[b]),
                  _sets_call("bgls_verify_aggregate_distinct_batch", curve, aggsigs, keys_per_instance, msgs_per_instance),
                  lambda b: DistinctMsgVerifyAggregateSignature(curve, aggsigs[b], keys_per_instance[b], msgs_per_instance[b]))


def Authenticate(curve, sk):                                  # bgls/blsKosk.go:44-55: a signature on the marshalled key
    return Sign(curve, sk, LoadPublicKey(curve, sk).Marshal())


def CheckAuthentication(curve, pubkey, authentication):      # bgls/blsKosk.go:59-69
    return _verify_single_keyed(curve, [authentication], [pubkey], None)[0]


def CheckAuthentications(curve, pubkeys, authentications):
    """len(pubkeys) independent CheckAuthentication calls in one batch (bgls_check_authentication_batch): a list of bools.  The compressed
    keys that the proofs of possession sign are made on the device."""
    return _verify_single_keyed(curve, authentications, pubkeys, None)


def KoskVerifyBatchMultiSignatureStepwise(curve, aggsigs, pubkeys, msgs):    # bgls/blsKosk.go:126-133, call by call as the reference writes it
    aggsig = AggregateSignatures(aggsigs)
    keys = [AggregateKeys(ks) for ks in pubkeys]
    return KoskVerifyAggregateSignature(curve, aggsig, keys, msgs)


def VerifyBatchMultiSignatureWithHAE(curve, aggsigs, aggpubkeys, msgs, allowDups):   # bgls/blsHAE.go:62-72
    """As in the reference, the random factors of the allowDups branch are applied to a throw-away copy (ScalePoints
    returns new points and the result is discarded, blsHAE.go:64-69), so both branches verify the plain aggregate."""
    if allowDups:
        ScalePoints(aggsigs, [secrets.randbelow(curve.GetG1Order()) for _ in aggsigs])
    return _verify_agg(curve, AggregateSignatures(aggsigs), aggpubkeys, msgs, True)


# ---- accountable-subgroup multisignatures (bgls/blsAsmSigs.go) -----------------------------------------------------
def _ams_h0(curve, msg):                                      # getAmsH0, blsAsmSigs.go:73-78
    return curve.HashToG1(b"\x00" + bytes(msg))


def _ams_h2(curve, apk, msg):                                 # getAmsH2, blsAsmSigs.go:80-86
    return curve.HashToG1(b"\x01" + apk.MarshalUncompressed() + bytes(msg))


def AmsCreateMembershipKeySharesKnownExp(curve, sk, apk, exp, numSigners):   # blsAsmSigs.go:23-30
    return [_ams_h2(curve, apk, str(i).encode()).Mul(sk).Mul(exp) for i in range(numSigners)]


def AmsCreateMembershipKeyShares(curve, sk, curIndex, pubkeys):              # blsAsmSigs.go:17-21
    t = hashPubKeysToExponents(pubkeys)
    apk = AggregatePoints(ScalePoints(pubkeys, t))
    return AmsCreateMembershipKeySharesKnownExp(curve, sk, apk, t[curIndex], len(pubkeys))


def AmsAggregateMembershipKeyShares(curve, shares):           # blsAsmSigs.go:32-34
    return AggregatePoints(shares)


def AmsCreateSignatureShare(curve, sk, membershipKey, msg):   # blsAsmSigs.go:36-40
    sig, _ = _ams_h0(curve, msg).Mul(sk).Add(membershipKey)
    return sig


def AmsCombineSignatureShares(pubkeys, sigs):                 # blsAsmSigs.go:42-46
    return AggregatePoints(pubkeys), AggregateSignatures(sigs)


def AmsVerifySignature(curve, apk, signers, aggKey, aggSig, msg):   # blsAsmSigs.go:48-59: a three-pairing product
    aggMsg = AggregatePoints([_ams_h2(curve, apk, str(i).encode()) for i in signers])
    pt, ok = curve.PairingProduct([_ams_h0(curve, msg), aggMsg, aggSig.Mul(-1)], [aggKey, apk, curve.GetG2()])
    return ok and pt.Equals(curve.GetGTIdentity())


def AmsVerifySignatures(curve, apks, signers, aggKeys, aggSigs, msgs):
    """len(apks) independent AmsVerifySignature calls (blsAsmSigs.go:48-59) in one bgls_ams_verify_batch call: a list of bools, one per
    item.  An item that is not made of Points of this curve (a nil or foreign signature or key) or has a signer index outside
    [0, 2^32) gets what AmsVerifySignature says about it alone; an empty signer list gives False (the reference panics) (_marshal.settle)."""
    n = len(apks)
    if not (n == len(signers) == len(aggKeys) == len(aggSigs) == len(msgs)):
        raise ValueError("apks, signers, aggKeys, aggSigs and msgs differ in length")

    def sendable(b):
        return (is_point(aggSigs[b], curve, G1) and all_points([apks[b], aggKeys[b]], curve, G2)
                and all(isinstance(i, int) and 0 <= i < 1 << 32 for i in signers[b]))

    def call(items):
        flat = [i for b in items for i in signers[b]]
        verdicts = _lib.out(len(items))
        rc = _lib.load().bgls_ams_verify_batch(curve.id, cat(apks[b] for b in items), cat(aggKeys[b] for b in items), cat(aggSigs[b] for b in items),
                                               (ctypes.c_uint32 * len(flat))(*flat), prefix_u64(len(signers[b]) for b in items), len(items),
                                               *msgs_arg([bytes(msgs[b]) for b in items]), verdicts, None)
        return rc, verdicts

    def single(b):                                   # a sendable item that was not sent has no signers
        return False if sendable(b) and len(signers[b]) == 0 else AmsVerifySignature(curve, apks[b], signers[b], aggKeys[b], aggSigs[b], bytes(msgs[b]))

    return settle(n, lambda b: sendable(b) and len(signers[b]) > 0, call, single)


def AmsVerifySignatureWithSetCheck(curve, check, apk, signers, aggKey, aggSig, msg):   # blsAsmSigs.go:61-66
    if not check(signers):
        return False
    return AmsVerifySignature(curve, apk, signers, aggKey, aggSig, msg)
