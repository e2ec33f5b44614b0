"""Shared by the tests of the grouped aggregate verification (bgls_group_messages, bgls_verify_aggregate_grouped): instances whose
messages repeat, made by the engine's own signing path as tests/test_gpu_batch_aggregate.py::make_batch makes them (bgls_scale_generator,
bgls_sign_batch, bgls_aggregate_sets; the messages are repeated BEFORE signing), the calls in their host and device forms, and the
expectation from code the grouped calls do not run: bgls_verify_aggregate(..., 1) and bgls_verify_aggregate_h_gt on the same inputs."""
import ctypes
import random

import test_gpu_batch_aggregate as ba

B, out, offs = ba.B, ba.out, ba.offs
CHUNK_MAX = 4096      # msggroup.hpp: the most keys per work item of the indexed key sum


def chunk_of(n):
    """msggroup.hpp msggroup_chunk: keys per work item in a call over n signers"""
    return min(4096, max(128, (n + 2047) // 2048))


def groups_of(msgs):
    """the specification: group numbers in the order of first occurrence, by exact bytes"""
    seen = {}
    return [seen.setdefault(bytes(m), len(seen)) for m in msgs], len(seen)


def make_instance(lib, cid, fp, group_sizes, seed, msg_len=32, shuffle=True, n_spare=1):
    """One valid aggregate over sum(group_sizes) signers: group g's message is signed by group_sizes[g] signers, the signers in a shuffled
    order.  Returns (keys, the per-signer messages, the aggregate signature, the secret keys, n_spare keys of signers outside the instance)."""
    rnd = random.Random(seed)
    n = sum(group_sizes)
    sks = [rnd.randrange(1, 1 << 250) for _ in range(n + n_spare)]
    kb = b"".join(s.to_bytes(32, "big") for s in sks)
    keys = out((n + n_spare) * 4 * fp)
    assert lib.bgls_scale_generator(cid, 2, B(kb), n + n_spare, keys) == 0
    distinct = []
    while len(distinct) < len(group_sizes):
        m = rnd.randbytes(msg_len)
        if m not in distinct:
            distinct.append(m)
    msgs = [distinct[g] for g, c in enumerate(group_sizes) for _ in range(c)]
    if shuffle:
        rnd.shuffle(msgs)
    keys = bytes(keys)
    return keys[:n * 4 * fp], msgs, sign(lib, cid, fp, sks[:n], msgs), sks[:n], keys[n * 4 * fp:]


def sign(lib, cid, fp, sks, msgs):
    """the aggregate of signer i's signature on msgs[i]"""
    n = len(sks)
    if n == 0:
        return bytes(2 * fp)
    kb = b"".join(s.to_bytes(32, "big") for s in sks)
    sigs = out(n * 2 * fp)
    assert lib.bgls_sign_batch(cid, B(kb), B(b"".join(msgs)), offs([len(m) for m in msgs]), n, sigs) == 0
    agg = out(2 * fp)
    assert lib.bgls_aggregate_sets(cid, 1, sigs, offs([n]), 1, agg) == 0
    return bytes(agg)


def group_host(lib, msgs):
    n = len(msgs)
    g = (ctypes.c_uint32 * max(n, 1))()
    d = ctypes.c_size_t(12345)
    rc = lib.bgls_group_messages(B(b"".join(msgs)), offs([len(m) for m in msgs]), n, g, ctypes.byref(d))
    return rc, list(g)[:n], d.value


def group_dev(lib, msgs, stride=None):
    """the device form on messages of one length, at `stride` (default: the length)"""
    import torch
    n, ln = len(msgs), len(msgs[0])
    stride = ln if stride is None else stride
    blob = b"".join(m + b"\xA5" * (stride - ln) for m in msgs)
    t = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).to("cuda:0")
    g = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda:0")
    d = ctypes.c_size_t(12345)
    torch.cuda.synchronize()
    rc = lib.bgls_group_messages_dev(t.data_ptr(), ln, stride, n, g.data_ptr(), ctypes.byref(d), None)
    torch.cuda.synchronize()
    return rc, [int(x) for x in g.cpu().tolist()][:n], d.value


def grouped_host(lib, cid, fp, sig, keys, msgs):
    """(return code, n_groups, GT bytes) of bgls_verify_aggregate_grouped"""
    d = ctypes.c_size_t(12345)
    gt = out(12 * fp)
    rc = lib.bgls_verify_aggregate_grouped(cid, B(sig), B(keys), B(b"".join(msgs)), offs([len(m) for m in msgs]), len(msgs), ctypes.byref(d), gt)
    return rc, d.value, bytes(gt)


def grouped_dev(lib, cid, fp, sig, keys, msgs, pad=0):
    """the same of bgls_verify_aggregate_grouped_dev: messages of one length at the stride length + pad"""
    import torch
    n, ln = len(msgs), len(msgs[0]) if msgs else 0
    dev = lambda b: torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to("cuda:0")
    t_sig, t_keys, t_msgs = dev(sig), dev(keys), dev(b"".join(m + b"\x5A" * pad for m in msgs))
    d = ctypes.c_size_t(12345)
    gt = out(12 * fp)
    torch.cuda.synchronize()
    rc = lib.bgls_verify_aggregate_grouped_dev(cid, t_sig.data_ptr(), t_keys.data_ptr(), t_msgs.data_ptr(), ln, ln + pad, n, ctypes.byref(d), gt, None)
    torch.cuda.synchronize()
    return rc, d.value, bytes(gt)


def ungrouped(lib, cid, fp, sig, keys, msgs):
    """(return code, number of distinct messages, GT bytes) from the calls this feature does not touch"""
    rc = ba.single(lib, cid, fp, sig, keys, msgs, 1)
    return rc, groups_of(msgs)[1], (ba.single_gt(lib, cid, fp, sig, keys, msgs) if rc in (0, 1) else None)


def instance_from(lib, cid, fp, sks, msgs):
    """(keys, aggregate signature) of the signers with the secret keys sks, signer i on msgs[i] -- for instances with a repeated or a negated key"""
    n = len(sks)
    keys = out(n * 4 * fp)
    assert lib.bgls_scale_generator(cid, 2, B(b"".join(s.to_bytes(32, "big") for s in sks)), n, keys) == 0
    return bytes(keys), sign(lib, cid, fp, sks, msgs)
