"""Operands and integer models for the tests of the fused two-product Montgomery block (Fp::mul2 / mulsub of csrc/field.cuh,
HK_MONT2_ASM_<FIELD> of csrc/mont_asm.h): tests/test_mul2_cpu.py and tests/test_mul2_gpu.py.  A plain module with fixed seeds.

Field objects are those of tests/field_edges.py: B is the representative bound (2p on a lazy field, p otherwise)."""
import random

from tests import field_edges as fe

FIELDS = fe.FIELDS


# ---- the block, restated on integers ---------------------------------------------------------------------------------------
def mul2_columns(f, a, b, c, d):
    """The fused product-scanning recurrence on 32-bit limbs with a 96-bit column accumulator: column i holds
    sum a_j b_(i-j) + sum c_j d_(i-j) + sum m_j p_(i-j).  -> (value before any correction, largest accumulator seen)."""
    N, M32 = f.N, fe.M32
    A, Bb, C, D, P = (fe.to_limbs(x, N) for x in (a, b, c, d, f.p))
    inv = (-pow(f.p, -1, 1 << 32)) % (1 << 32)
    m, out, acc, peak = [0] * N, [0] * N, 0, 0
    for i in range(2 * N - 1):
        lo, hi = max(0, i - N + 1), min(i, N - 1)
        for j in range(lo, hi + 1):
            acc += A[j] * Bb[i - j] + C[j] * D[i - j]
            if i - j >= 0 and (i >= N or j < i):
                acc += m[j] * P[i - j]
        if i < N:
            m[i] = (acc & M32) * inv & M32
            acc += m[i] * P[0]
            assert acc & M32 == 0
        else:
            out[i - N] = acc & M32
        peak = max(peak, acc)
        acc >>= 32
    out[N - 1] = acc & M32
    return fe.from_limbs(out) + ((acc >> 32) << (32 * N)), peak       # anything above N limbs would show here


def mul2_exact(f, a, b, c, d):
    """(a b + c d + m p) / R with the one m < R that makes the division exact: what every correct reduction computes"""
    s = a * b + c * d
    m = (-s * pow(f.p, -1, f.R)) % f.R
    return (s + m * f.p) >> (32 * f.N)


def needs_correction(f):
    """lazy fields: whether p (8p / R + 1) exceeds 2p"""
    return 8 * f.p + f.R > 2 * f.R


# ---- operands -------------------------------------------------------------------------------------------------------------
def grid_values(f):
    """The eight values of the 8^4 grid.  Lazy fields: 0, 1, p - 1, p, p + 1, 2p - 1, the all-ones value nearest below 2p (no
    value next to 2^(32N - 1) is below 2p on any of these moduli: 2p < R / 2) and one random value.  Canonical fields
    (BLS12-381 Fr) hold nothing at or above p: p - 2, (p - 1) / 2 and (p + 1) / 2 stand in for p, p + 1 and 2p - 1."""
    p, B = f.p, f.B
    ones = (1 << ((B - 1).bit_length() - 1)) - 1
    rnd = random.Random("%s/mul2-grid" % f.name).randrange(B)
    if f.lazy:
        v = [0, 1, p - 1, p, p + 1, 2 * p - 1, ones, rnd]
    else:
        v = [0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, ones, rnd]
    assert len(set(v)) == 8 and all(0 <= x < B for x in v)
    return v


def tuples(f, n_random=3000, n_zero=64):
    """All 8^4 grid tuples, n_random random tuples below the bound, n_zero tuples with a b + c d = 0 (mod p) on non-zero
    operands, and (B - 1, B - 1, B - 1, B - 1 - k) for k < 16: the largest products there are.  Whether such a value lands
    in [2p, 2.52 p) on BN254 also takes a quotient m above about R / 2, which about every second k gives."""
    g = grid_values(f)
    out = [(a, b, c, d) for a in g for b in g for c in g for d in g]
    rnd = random.Random("%s/mul2-tuples" % f.name)
    out += [tuple(rnd.randrange(f.B) for _ in range(4)) for _ in range(n_random)]
    for k in range(n_zero):
        a, b, c = (rnd.randrange(1, f.p) for _ in range(3))
        d = (-a * b * pow(c, -1, f.p)) % f.p
        if f.lazy and k & 1:                                   # the same zero on non-canonical representatives
            a, d = a + f.p, d + f.p
        assert (a * b + c * d) % f.p == 0 and max(a, b, c, d) < f.B
        out.append((a, b, c, d))
    out += [(f.B - 1, f.B - 1, f.B - 1, f.B - 1 - k) for k in range(16)]
    return out


# ---- the lazy mixed add, restated on integers -------------------------------------------------------------------------------
class LazyModel:
    """The device's lazy arithmetic on a lazy field with the fused block, value for value: representatives in [0, 2p), the
    Montgomery quotient exact, add / sub reduced against 2p."""

    def __init__(self, f):
        assert f.lazy
        self.f, self.p, self.p2 = f, f.p, 2 * f.p
        self.fix = needs_correction(f)
        self.corrected = 0                                     # mul2 values that arrived in [2p, ...)

    def mul(self, a, b):
        return mul2_exact(self.f, a, b, 0, 0)

    def add(self, a, b):
        t = a + b
        return t - self.p2 if t >= self.p2 else t

    def sub(self, a, b):
        t = a - b
        return t + self.p2 if t < 0 else t

    def mulsub(self, a, b, c, d):
        t = mul2_exact(self.f, a, b, c, self.p2 - d)
        if t >= self.p2:
            assert self.fix
            self.corrected += 1
            t -= self.p2
        return t

    def is_zero(self, a):
        return a in (0, self.p)

    def madd(self, acc, q):
        """ec_madd of csrc/ec.cuh on raw (x, y, zz, zzz) and an affine (x, y); (0, 0) is the base at infinity"""
        if self.is_zero(q[0]) and self.is_zero(q[1]):
            return acc
        if self.is_zero(acc[2]):
            return (q[0], q[1], self.f.one, self.f.one)
        x1, y1, zz, zzz = acc
        pd = self.sub(self.mul(q[0], zz), x1)
        r = self.sub(self.mul(q[1], zzz), y1)
        if self.is_zero(pd):
            if not self.is_zero(r):
                return (0, 0, 0, 0)
            u = self.add(q[1], q[1])
            v = self.mul(u, u)
            w = self.mul(u, v)
            s = self.mul(q[0], v)
            xx = self.mul(q[0], q[0])
            m = self.add(self.add(xx, xx), xx)
            x3 = self.sub(self.mul(m, m), self.add(s, s))
            return (x3, self.mulsub(m, self.sub(s, x3), w, q[1]), v, w)
        pp = self.mul(pd, pd)
        ppp = self.mul(pd, pp)
        qq = self.mul(x1, pp)
        x3 = self.sub(self.sub(self.mul(r, r), ppp), self.add(qq, qq))
        return (x3, self.mulsub(r, self.sub(qq, x3), ppp, y1), self.mul(zz, pp), self.mul(zzz, ppp))


# ---- affine points on y^2 = x^3 + b over a prime field, canonical integers -------------------------------------------------
def affine_add(p, P, Q):
    """None is infinity"""
    if P is None:
        return Q
    if Q is None:
        return P
    if P[0] == Q[0]:
        if (P[1] + Q[1]) % p == 0:
            return None
        lam = 3 * P[0] * P[0] * pow(2 * P[1], -1, p) % p
    else:
        lam = (Q[1] - P[1]) * pow(Q[0] - P[0], -1, p) % p
    x = (lam * lam - P[0] - Q[0]) % p
    return x, (lam * (P[0] - x) - P[1]) % p


def random_point(p, b, rnd):
    """p = 3 (mod 4) on both curves"""
    assert p % 4 == 3
    while True:
        x = rnd.randrange(p)
        y2 = (x * x * x + b) % p
        y = pow(y2, (p + 1) // 4, p)
        if y * y % p == y2 and y:
            return x, y
