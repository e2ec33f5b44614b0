"""Plain reference for the point layer (TEST-ONLY): the schoolbook affine group law on Python integers, over Fp for G1 and over
Fp2 = Fp[u] / (u^2 + 1) for the twists, with the curve constants of the C ABI (alt-bn128: y^2 = x^3 + 3 and the D-type twist
b' = 3 / (9 + u); BLS12-381: y^2 = x^3 + 4 and the M-type twist b' = 4 (1 + u)).  None is the point at infinity.

mul(P, k) is double-and-add on the INTEGER k: no reduction modulo any group order, so it is right for points outside the order-r
subgroup.  recode(k, nbits, order) models the signed radix-16 walk of jac1_mul_w4 / jacx_mul_w4 on a point of the given order and
returns the branch events it takes; the tests use it to PROVE that their scalars reach every branch, never as an expected value.

Imports nothing of the project: the GPU tier keeps the Python oracle out (test_gpu_device_arith.py), and the CPU tier pins this
module against oracle.pyref and the C oracle (test_ec_ref.py)."""

P = {0: 21888242871839275222246405745257275088696311157297823662689037894645226208583,
     1: 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab}
ORDER = {0: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
         1: 52435875175126190479447740508185965837690552500527637822603658699938581184513}
FB = {0: 32, 1: 48}
B1 = {0: 3, 1: 4}
G1 = {0: (1, 2),
      1: (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
          0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1)}
# (re, im)
G2 = {0: ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
           11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930,
           4082367875863433681332203403145435568316851327593401208105741076214120093531)),
      1: ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
           0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
          (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
           0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be))}

EVENTS = ("plain", "double", "cancel", "r_inf", "dbl_inf", "tab_inf", "digit0")


class Fp1:
    """Fp: elements are ints in [0, p)"""

    def __init__(self, p):
        self.p = p
        self.zero, self.one = 0, 1

    def add(self, a, b):
        return (a + b) % self.p

    def sub(self, a, b):
        return (a - b) % self.p

    def mul(self, a, b):
        return a * b % self.p

    def inv(self, a):
        return pow(a, -1, self.p)

    def small(self, k):
        return k % self.p


class Fp2:
    """Fp[u] / (u^2 + 1): elements are (re, im)"""

    def __init__(self, p):
        self.p = p
        self.zero, self.one = (0, 0), (1, 0)

    def add(self, a, b):
        return ((a[0] + b[0]) % self.p, (a[1] + b[1]) % self.p)

    def sub(self, a, b):
        return ((a[0] - b[0]) % self.p, (a[1] - b[1]) % self.p)

    def mul(self, a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % self.p, (a[0] * b[1] + a[1] * b[0]) % self.p)

    def inv(self, a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, self.p)
        return (a[0] * n % self.p, -a[1] * n % self.p)

    def small(self, k):
        return (k % self.p, 0)


class Curve:
    """y^2 = x^3 + b over Fp (group 1) or over Fp2 on the twist (group 2) of curve `cid` (0 alt-bn128, 1 BLS12-381)"""

    def __init__(self, cid, group):
        self.cid, self.group, self.p, self.fb = cid, group, P[cid], FB[cid]
        if group == 1:
            self.F = Fp1(self.p)
            self.b = B1[cid]
            self.gen = G1[cid]
        else:
            self.F = Fp2(self.p)
            self.b = self.F.mul((3, 0), self.F.inv((9, 1))) if cid == 0 else (4, 4)
            self.gen = G2[cid]
        self.size = (2 if group == 1 else 4) * self.fb

    def on_curve(self, pt):
        if pt is None:
            return True
        F = self.F
        x, y = pt
        return F.mul(y, y) == F.add(F.mul(F.mul(x, x), x), self.b)

    def neg(self, pt):
        return None if pt is None else (pt[0], self.F.sub(self.F.zero, pt[1]))

    def add(self, a, b):
        F = self.F
        if a is None:
            return b
        if b is None:
            return a
        (x1, y1), (x2, y2) = a, b
        if x1 == x2:
            if F.add(y1, y2) == F.zero:
                return None
            m = F.mul(F.mul(F.small(3), F.mul(x1, x1)), F.inv(F.add(y1, y1)))
        else:
            m = F.mul(F.sub(y2, y1), F.inv(F.sub(x2, x1)))
        x3 = F.sub(F.sub(F.mul(m, m), x1), x2)
        return (x3, F.sub(F.mul(m, F.sub(x1, x3)), y1))

    def dbl(self, a):
        return self.add(a, a)

    def mul(self, pt, k):
        """k pt for the integer k >= 0 as given (never reduced)"""
        assert k >= 0
        r = None
        for bit in bin(k)[2:] if k else "":
            r = self.add(r, r)
            if bit == "1":
                r = self.add(r, pt)
        return r

    def order(self, pt, bound=1 << 24):
        """the order of pt when it is at most `bound`, else None (a walk: for the small-order fixture points only)"""
        r, n = pt, 1
        while r is not None:
            if n >= bound:
                return None
            r = self.add(r, pt)
            n += 1
        return n

    # ---- wire bytes: G1 x || y, G2 x_im || x_re || y_im || y_re, big-endian, all zero = infinity
    def to_bytes(self, pt):
        if pt is None:
            return bytes(self.size)
        if self.group == 1:
            return pt[0].to_bytes(self.fb, "big") + pt[1].to_bytes(self.fb, "big")
        (x0, x1), (y0, y1) = pt
        return b"".join(v.to_bytes(self.fb, "big") for v in (x1, x0, y1, y0))

    def from_bytes(self, b):
        assert len(b) == self.size
        if b == bytes(self.size):
            return None
        v = [int.from_bytes(b[i:i + self.fb], "big") for i in range(0, self.size, self.fb)]
        return (v[0], v[1]) if self.group == 1 else ((v[1], v[0]), (v[3], v[2]))

    def scaled(self, pt, lam):
        """the Jacobian representative (lam^2 x, lam^3 y, lam) of pt, lam a non-zero element of Fp; field elements as this class holds them"""
        F = self.F
        l1 = F.small(lam)
        l2 = F.mul(l1, l1)
        return (F.mul(l2, pt[0]), F.mul(F.mul(l2, l1), pt[1]), l1)


def recode(k, nbits, order):
    """The walk of jac1_mul_w4 / jacx_mul_w4 over the low `nbits` bits of k, on a point of the given order (multiples of the point are
    integers modulo `order`; 0 is infinity).  Returns (k' mod order for the masked scalar k', the set of branch events):
      digit0   a zero digit: no addition                    tab_inf  the table entry |digit| P is infinity
      r_inf    the running point is infinity at an addition dbl_inf  a doubling of infinity
      double   running point == addend                      cancel   running point == -addend
      plain    the general addition"""
    ev = set()
    if nbits <= 0:
        return 0, ev
    k &= (1 << nbits) - 1
    nw = (nbits + 4) >> 2
    r = 0
    for i in range(nw - 1, -1, -1):
        if i != nw - 1:
            for _ in range(4):
                if r == 0:
                    ev.add("dbl_inf")
                r = 2 * r % order
        pos = 4 * i - 1
        b5 = (k << 1) & 31 if pos < 0 else (k >> pos) & 31
        val = (((b5 & 15) + 1) >> 1) - (b5 >> 4) * 8
        if val == 0:
            ev.add("digit0")
            continue
        q = val % order
        if q == 0:
            ev.add("tab_inf")
            continue
        if r == 0:
            ev.add("r_inf")
        elif r == q:
            ev.add("double")
        elif (r + q) % order == 0:
            ev.add("cancel")
        else:
            ev.add("plain")
        r = (r + q) % order
    return r, ev


def steer_scalar(order, event, high, low_digit):
    """k = 16 h + d (d = low_digit in 1..7, so the last window's digit is +d and no carry enters the windows above) with 16 h congruent to
    d (event 'double') or -d ('cancel') modulo `order`: the last addition of the walk meets its own addend.  h is the smallest such
    value at or above `high`; order must be odd."""
    assert 1 <= low_digit <= 7 and order % 2 == 1
    want = (low_digit if event == "double" else -low_digit) * pow(16, -1, order) % order
    h = high + (want - high) % order
    return 16 * h + low_digit
