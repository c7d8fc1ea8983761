"""Deterministic operand sets for the tests of the device field arithmetic (csrc/field.cuh, csrc/mont_asm.h):
tests/test_mont_asm_cpu.py interprets the generated assembly on them, tests/test_field_device_gpu.py and
tests/test_wave_f12_gpu.py run the device build of the same code on them.  A plain module with fixed seeds.

For a field with modulus p on N 32-bit limbs, R = 2^(32 N): the representative bound B is 2p when 4p <= R (the
"lazy" fields, whose device values live in [0, 2p) while they are in registers) and p otherwise.  B is the
contract of field.cuh; no operand >= B is ever generated here (behaviour there is undefined by design).
"""
import random

from oracle.pyref.params import BN254, BLS12_381

M32 = 0xFFFFFFFF


class Field:
    def __init__(self, name, p, n):
        self.name, self.p, self.N = name, p, n
        self.R = 1 << (32 * n)
        self.lazy = 4 * p <= self.R
        self.B = 2 * p if self.lazy else p
        self.Rinv = pow(self.R, -1, p)
        self.one = self.R % p                     # Montgomery one

    def __repr__(self):
        return "Field(%s)" % self.name


# keyed as the HK_<KIND>_ASM_<FIELD> macros of mont_asm.h; the order is the field id of shim_field_op (0..3)
FIELDS = {
    "BN254_FR": Field("BN254_FR", BN254.r, 8),
    "BN254_FQ": Field("BN254_FQ", BN254.q, 8),
    "BLS12_381_FR": Field("BLS12_381_FR", BLS12_381.r, 8),
    "BLS12_381_FQ": Field("BLS12_381_FQ", BLS12_381.q, 12),
}
FIELD_IDS = {name: i for i, name in enumerate(FIELDS)}
# the Fq2 towers (field ids 4 and 5 of shim_field_op) over their base fields
FP2_BASE = {4: "BN254_FQ", 5: "BLS12_381_FQ"}


def _dedup(vals):
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def _seed(f, tag):
    return "%s/%s" % (f.name, tag)                # str seeds hash deterministically (random.seed version 2)


def edge_values(f):
    """Named edge values, plus the non-canonical representatives of 0, 1 and Montgomery one on lazy fields."""
    p, B, R, N = f.p, f.B, f.R, f.N
    v = [0, 1, 2, p - 2, p - 1, B - 2, B - 1, (p - 1) // 2, (p + 1) // 2, R % p, R * R % p,
         (1 << 32) - 1, 1 << 32, (1 << (32 * (N - 1))) - 1, 1 << (32 * (N - 1))]
    if f.lazy:
        v += [p, p + 1, p + R % p]
    assert all(0 <= x < B for x in v), f
    return _dedup(v)


def limb_patterns(f):
    """12 values whose limbs are each 0 or 0xffffffff, reduced mod B."""
    rnd = random.Random(_seed(f, "limbs"))
    N = f.N
    masks = [(1 << N) - 1, 1, 1 << (N - 1), (1 << N) - 2, (1 << (N - 1)) - 1, 0x5555 & ((1 << N) - 1),
             0xAAAA & ((1 << N) - 1)]
    while len(masks) < 12:
        m = rnd.randrange(1, 1 << N)
        if m not in masks:
            masks.append(m)
    out = []
    for m in masks:
        x = sum(M32 << (32 * i) for i in range(N) if (m >> i) & 1)
        out.append(x % f.B)
    return out


def _biased_limb(rnd):
    u = rnd.random()
    if u < 0.4:
        return M32
    if u < 0.5:
        return 0
    if u < 0.8:
        return 0xFFFF0000 | rnd.getrandbits(16)   # upper half ones
    return rnd.getrandbits(32)


def biased_randoms(f, count=40, tag="biased"):
    """Limbs drawn 40 % all-ones, 10 % zero, 30 % upper half ones, else uniform; the value then taken mod B.  This is
    the distribution that reaches the rare carries into the third accumulator word of the Montgomery products."""
    rnd = random.Random(_seed(f, tag))
    return [sum(_biased_limb(rnd) << (32 * i) for i in range(f.N)) % f.B for _ in range(count)]


def uniform_randoms(f, count=40, tag="uniform"):
    rnd = random.Random(_seed(f, tag))
    return [rnd.randrange(f.B) for _ in range(count)]


# Operand pairs that a directed search found to fire third-word carries of the MONT blocks which the sets above
# leave cold (tests/test_mont_asm_cpu.py, carry coverage).  (field) -> [(a, b), ...]
DIRECTED_PAIRS = {
    "BN254_FR": [],
    "BN254_FQ": [],
    # p[0] = 1 here, so the quotient-digit product m_i * p[0] of column i carries out of 64 bits only when the column's
    # middle word is 0xffffffff: a_i solved from the other limbs (b[0] near 2^32) for columns 2 .. 7; column 1 fires in
    # the structured set and column 0 cannot (a_0 b_0 + m_0 < 2^64)
    "BLS12_381_FR": [
        (0x2d4ddc2a25c26de570d72816d9b4aeed061a29b5344bcead46fae9a2c3d43301,
         0x3347038796f928789265a68dc43dfc6adf1a81cef2e711dbca3e9bc8fffffffc),
        (0x1cab646204481613c32b3ef7077c843e0605060c54ca402378175cad07c8a0be,
         0x6fffef197aceca27433e833e34528896336d72aad942214641dbe4c3fffffff7),
        (0x4c31a99aebddef58e6ff4dba062962b339366891d1bebbd86ed6992371cda0f6,
         0x4e4ab29058b9d1b291c693837ddb2d6220193e2a66bdb0a673ddfabefffffffa),
        (0x4a873f5638fdddf3662886e1b959bbe3f2d87e49313cb436af04e43190e4400f,
         0x507d58244034f311bd6f7e283b42f83b4c789199abc11ccb68d3a2b6fffffff0),
        (0x3793dccc75d69f91c41d769838af0326393036de09765b57adee2a9057fa699f,
         0x35f58d8485cb96f41087c0720ab0b8aabaf3000caea2d1e227d2c95ffffffffb),
        (0x2c617509b6c60147532f94468d98dad5a272da5f5d0ca9ee7418237508d53315,
         0x282266e8a7c96bcc8dc99c71fd1eea07b06b9e411ba0dc0eb16de37afffffff0),
    ],
    "BLS12_381_FQ": [],
}


def structured_values(f):
    return _dedup(edge_values(f) + limb_patterns(f) + biased_randoms(f))


def all_values(f):
    return _dedup(structured_values(f) + uniform_randoms(f))


def pair_list(f, n_random=4096):
    """All ordered pairs of the edge, limb-pattern and biased-random values, the directed pairs, and n_random uniformly
    random pairs."""
    s = structured_values(f)
    pairs = [(a, b) for a in s for b in s]
    pairs += DIRECTED_PAIRS[f.name]
    rnd = random.Random(_seed(f, "pairs"))
    pairs += [(rnd.randrange(f.B), rnd.randrange(f.B)) for _ in range(n_random)]
    return pairs


def lazy_alias_pairs(f, count=64):
    """(x, x + p) and (x + p, x) for canonical x: the two representatives a lazy field holds of one value (empty for a
    field that is not lazy)."""
    if not f.lazy:
        return []
    rnd = random.Random(_seed(f, "alias"))
    xs = [0, 1, f.p - 1, f.one] + [rnd.randrange(f.p) for _ in range(count - 4)]
    return [(x, x + f.p) for x in xs] + [(x + f.p, x) for x in xs] + [(x + f.p, x + f.p) for x in xs[:8]]


def fp2_pair_list(f, n_random=256):
    """Fp2 operands over base field f: every (c0, c1) from the edge list (about 30^2 elements, so a0 = a1, (p - 1, 1) and
    lazy components are all in it), each paired with a fixed subset of 16 of them, plus random elements."""
    e = edge_values(f)
    elems = [(x, y) for x in e for y in e]
    rnd = random.Random(_seed(f, "fp2"))
    subset = rnd.sample(elems, 12) + [(0, 0), (f.p - 1, 1), (f.one, f.one), (f.B - 1, f.B - 1)]
    pairs = [(a, b) for a in elems for b in subset]
    for _ in range(n_random):
        pairs.append(((rnd.randrange(f.B), rnd.randrange(f.B)), (rnd.randrange(f.B), rnd.randrange(f.B))))
    return pairs


def to_limbs(x, n):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def from_limbs(v):
    return sum(int(w) << (32 * i) for i, w in enumerate(v))
