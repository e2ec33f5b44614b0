"""GPU tier: bgls_group_messages / bgls_group_messages_dev against a Python dict in first-occurrence order, byte for byte: the sizes
around one wave and one scan tile, all messages equal, all distinct, the empty message, messages that differ in the last byte only, a
proper prefix of another message, variable and fixed lengths, the device form at a stride above the length, and 2^16 messages over 300
values in a skewed distribution, twice (the table's seed differs per call: the result may not)."""
import random

import pytest

import grouped_cases as gc

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 257]


def check(lib, msgs, dev_stride=None):
    want, d = gc.groups_of(msgs)
    got = gc.group_host(lib, msgs)
    assert got == (0, want, d), ("host form", got[0], got[2], d)
    if dev_stride is not None:
        got = gc.group_dev(lib, msgs, dev_stride)
        assert got == (0, want, d), ("device form", got[0], got[2], d)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_equal_distinct_and_mixed(gpu_lib, n):
    rnd = random.Random(900 + n)
    check(gpu_lib, [b"one message for everybody, 32 b."] * n, dev_stride=32)            # all equal
    check(gpu_lib, [i.to_bytes(4, "big") + bytes(28) for i in range(n)], dev_stride=48)    # all distinct, stride above the length
    pool = [rnd.randbytes(rnd.randrange(0, 70)) for _ in range(max(1, n // 3))]
    check(gpu_lib, [rnd.choice(pool) for _ in range(n)])                                  # variable lengths, repeats


def test_empty_last_byte_and_prefix(gpu_lib):
    rnd = random.Random(31)
    base = rnd.randbytes(40)
    msgs = [base, b"", base[:-1] + bytes([base[-1] ^ 1]), base[:39], b"", base + b"\0", base, b"\0", b"", base[:39], bytes(40), bytes(39)]
    want, d = gc.groups_of(msgs)
    assert d == 8 and want[1] == want[4] == want[8] == 1                                   # the empty message three times among others
    check(gpu_lib, msgs)
    same_len = [base, base[:-1] + bytes([base[-1] ^ 0x80]), base, base[:-1] + bytes([base[-1] ^ 1]), base[:-1] + bytes([base[-1] ^ 0x80])]
    check(gpu_lib, same_len, dev_stride=40)
    check(gpu_lib, same_len, dev_stride=41)


def test_empty_messages_only_in_the_device_form(gpu_lib):
    got = gc.group_dev(gpu_lib, [b""] * 5, 0)
    assert got == (0, [0] * 5, 1)
    got = gc.group_dev(gpu_lib, [b""] * 70, 16)
    assert got == (0, [0] * 70, 1)


def test_no_messages(gpu_lib):
    assert gc.group_host(gpu_lib, []) == (0, [], 0)


def test_65536_messages_over_300_skewed_values_twice(gpu_lib):
    rnd = random.Random(65536)
    pool = [rnd.randbytes(32) for _ in range(300)]
    weights = [1.0 / (k + 1) ** 1.3 for k in range(300)]
    msgs = rnd.choices(pool, weights=weights, k=1 << 16)
    msgs[-300:] = pool                                                                    # every value occurs
    want, d = gc.groups_of(msgs)
    assert d == 300
    first = gc.group_dev(gpu_lib, msgs, 32)
    second = gc.group_dev(gpu_lib, msgs, 32)
    assert first == (0, want, 300)
    assert second == first
    assert gc.group_host(gpu_lib, msgs) == first
