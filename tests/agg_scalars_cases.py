"""Inputs and expectations shared by test_agg_scalars_cpu.py and test_agg_scalars_gpu.py: the sizes and the scalar / challenge
families of hk_scalar_powers and hk_ipa_quotient, and what both must give - always from the Python mirror (a plain power loop,
tipa.ipa_polynomial_coeffs, tipa._divide_by_linear, FrCodec), never from the code under test.  Each expectation is computed
once per session (lru_cache) and handed out as bytes."""
import functools
import random

from hekaton_system_amd import tipa
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec

CURVES = ["bn254", "bls12_381"]

# ---- hk_scalar_powers ---------------------------------------------------------------------------------------------------
# (n, reps): a single power; below, at and above one chunk of 8; below, at and above one wavefront of 64 chunks (511 / 512 /
# 513); a second workgroup of 256 chunks (2049 = 257 chunks); reps = 5 at a length that is no multiple of the chunk
POWER_SHAPES = [(1, 1), (2, 1), (7, 1), (8, 1), (9, 1), (511, 1), (512, 1), (513, 1), (2049, 1), (9, 5)]


def power_bases(curve):
    r = CURVE_PARAMS[curve]["r"]
    return [0, 1, r - 1, 2, random.Random(41).randrange(2, r)]


@functools.lru_cache(maxsize=None)
def mirror_powers(curve, x, n, reps):
    """Montgomery bytes of x^0 .. x^(n - 1), `reps` times back to back."""
    fc = FrCodec(curve)
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * x % fc.r
    return fc.enc(out * reps).tobytes()


# ---- hk_ipa_quotient ----------------------------------------------------------------------------------------------------
# (l, shift): a single coefficient; a partial chunk; exactly one chunk; a shift of one chunk; a shift that is no multiple of
# the chunk; exactly one tile of 256 chunks (the one-workgroup kernel's largest length); a tile boundary crossed by 5
# coefficients; several tiles; 128 tiles - the first count at which a lane of the scan over the tile totals takes two tiles
QUOTIENT_SHAPES = [(0, 0), (0, 1), (1, 0), (2, 0), (3, 0), (3, 8), (4, 5), (10, 0), (11, 0), (11, 5), (11, 2048), (12, 4096),
                   (17, 131072)]


def challenge_families(curve, l):
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(1000 + l)
    base = [rnd.randrange(1, r) for _ in range(l)]

    def with_zero(pos):
        c = list(base)
        if l:
            c[pos] = 0
        return c
    return {"random": base, "ones": [1] * l, "minus_ones": [r - 1] * l, "zero_lowest": with_zero(0),
            "zero_middle": with_zero(l // 2), "zero_highest": with_zero(l - 1), "reversed": base[::-1]}


def quotient_cases(curve, l, shift):
    """[(name, challenges, rho, z)]: the full product of z in {0, 1, r - 1, random}, rho in {1, random} and the seven challenge
    families; at the two largest sizes a part of it (every third case at 8 192 coefficients, two at 262 144) so that the
    mirror's Python loops stay around a second."""
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(77 * l + shift)
    zs = [("z0", 0), ("z1", 1), ("zm1", r - 1), ("zr", rnd.randrange(2, r))]
    rhos = [("rho1", 1), ("rhor", rnd.randrange(2, r))]
    fams = list(challenge_families(curve, l).items())
    full = [("%s-%s-%s" % (zn, rn, fn), tuple(ch), rho, z) for zn, z in zs for rn, rho in rhos for fn, ch in fams]
    if (l, shift) == (12, 4096):
        return full[::3]                                       # 19 of 56: the stride is coprime to 2, 4 and 7
    if (l, shift) == (17, 131072):                             # 0.8 s of Python each: all random, and r - 1 / 1 / a zero
        return [full[3 * 14 + 7], full[2 * 14 + 4]]
    return full


def f_coeffs(curve, challenges, rho, shift):
    """Canonical coefficients of f(X) = X^shift prod_k (1 + c_k (rho X)^(2^k))."""
    return [0] * shift + tipa.ipa_polynomial_coeffs(list(challenges), rho, CURVE_PARAMS[curve]["r"])


@functools.lru_cache(maxsize=None)
def mirror_quotient(curve, challenges, rho, z, shift):
    """Montgomery bytes of f / (X - z), remainder dropped, one zero appended: Tipp.prove's own host path."""
    fc = FrCodec(curve)
    f = [0] * shift + tipa.ipa_polynomial_coeffs(list(challenges), rho, fc.r, fc.R)
    return fc.enc_canon(tipa._divide_by_linear(f, z, fc.r)).tobytes()
