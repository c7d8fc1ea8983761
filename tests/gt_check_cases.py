"""Named Fq12 values for the tests of hk_gt_check (tests/test_gt_check_cpu.py, tests/test_gt_check_gpu.py,
tests/test_agg_verify_gt_gpu.py), per curve, as GtField tuples (12 ints, ark tower order), with the verdict each must get.
Built once per process from the oracle's pairing and GtField's integers; no GPU.

    accept   one; g = e(G1, G2); g^2; g * g' with g' = e([5] G1, [7] G2); conj(g) = g^-1
    refuse   zero; -1 (order 2); 2 in Fq; two seeded random Fq12; c = f^((q^6 - 1)(q^2 + 1)) for a seeded f - in the
             cyclotomic subgroup, of order dividing Phi_12(q) but not r; g * c
    refuse   BLS12-381 only: omega, a primitive cube root of unity in Fq.  3 | u - 1 and 3 | q - 1, so
             omega^q = omega = omega^u: the Frobenius equation x^q == x^(t - 1) HOLDS for it in exact arithmetic, and only
             the cyclotomic condition refuses it (omega^(q^4) omega = omega^2 != omega = omega^(q^2))."""
import functools
import random

from hekaton_system_amd.gt import GtField
from oracle.pyref import curve, pairing
from oracle.pyref.params import CURVES

CURVE_NAMES = ("bn254", "bls12_381")


def curve_u(cname):
    """The curve parameter u, signed."""
    T = pairing.tower(cname)
    return -T.x if T.x_is_negative else T.x


def trace_minus_one(cname):
    """t - 1, t the trace of Frobenius: 6 u^2 on BN254, u on BLS12-381."""
    u = curve_u(cname)
    return 6 * u * u if cname == "bn254" else u


def phi12(q):
    return q ** 4 - q ** 2 + 1


def embed(F, a):
    """a in Fq as an element of Fq12."""
    return tuple([a % F.q] + [0] * 11)


@functools.lru_cache(maxsize=None)
def cyclotomic_element(cname):
    """c = f^((q^6 - 1)(q^2 + 1)), f seeded: what the easy part of a final exponentiation leaves."""
    F = GtField(cname)
    rnd = random.Random(0xC1C + len(cname))
    f = tuple(rnd.randrange(F.q) for _ in range(12))
    return F.pow(f, (F.q ** 6 - 1) * (F.q ** 2 + 1))


@functools.lru_cache(maxsize=None)
def omega(cname):
    """A primitive cube root of unity in Fq (q = 1 mod 3 on both curves; the case is BLS12-381's)."""
    q = CURVES[cname].q
    return next(w for w in (pow(h, (q - 1) // 3, q) for h in range(2, 50)) if w != 1)


@functools.lru_cache(maxsize=None)
def cases(cname):
    """[(name, value, expected verdict)]."""
    cp = CURVES[cname]
    F = GtField(cname)
    T = pairing.tower(cname)
    G1, G2 = curve.G1(cp), curve.G2(cp)
    g = tuple(T.f12_flat(T.pairing(cp.g1_gen, cp.g2_gen)))
    g2 = tuple(T.f12_flat(T.pairing(G1.mul(cp.g1_gen, 5), G2.mul(cp.g2_gen, 7))))
    c = cyclotomic_element(cname)
    rnd = random.Random(0x67 + len(cname))
    out = [("one", F.one, True),
           ("g", g, True),
           ("g^2", F.mul(g, g), True),
           ("g*g'", F.mul(g, g2), True),
           ("conj(g)", F.conj(g), True),
           ("zero", tuple([0] * 12), False),
           ("-1", embed(F, -1), False),
           ("2", embed(F, 2), False),
           ("random0", tuple(rnd.randrange(F.q) for _ in range(12)), False),
           ("random1", tuple(rnd.randrange(F.q) for _ in range(12)), False),
           ("c", c, False),
           ("g*c", F.mul(g, c), False)]
    if cname == "bls12_381":
        out.append(("omega", embed(F, omega(cname)), False))
    return tuple(out)


def case(cname, name):
    return next(x for nm, x, _ in cases(cname) if nm == name)


@functools.lru_cache(maxsize=None)
def host_verdicts(cname):
    """GtField.in_gt of every case, in order: the independent reference, computed once."""
    F = GtField(cname)
    return tuple(bool(F.in_gt(x)) for _nm, x, _ in cases(cname))
