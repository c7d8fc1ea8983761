"""Inputs and expectations shared by test_agg_verify_cpu.py (the host shim) and test_class_sums_gpu.py: the sizes, class counts,
class maps and bases of hk_class_power_sums, and what every case must give - always from the Python mirror
(agg_verify.class_power_sums_host: a plain loop), computed once per case and kept.

Sizes, by the shape built (csrc/class_sums.cuh: AQ_CHUNK = 8 exponents a lane, CS_WG = 256 lanes a workgroup, so 2 048
exponents a workgroup; at most CS_MAX_WGS = 1 024 workgroups, which then stride on):
    1, 7, 8, 9            below, at and past the chunk edge
    2 047, 2 048, 2 049   one exponent short of a full workgroup, the full workgroup, the first exponent of a second one
    4 097                 more than two workgroups with a tail of one
    65 537                33 workgroups, odd tail
    2^21 + 2 049          more than 1 024 workgroups of chunks: the first workgroups stride to a second round of chunks, the
                          others do not (one case: the mirror is a loop of n products)
Class counts: 1, 2, 5 (the jobs that exist), 8 | 9 and 17 (the class-group boundary on both sides, three groups), 1 024 (the cap)."""
import functools
import random

import numpy as np

from hekaton_system_amd.agg_verify import class_power_sums_host
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec

CURVES = ["bn254", "bls12_381"]
SIZES = [1, 7, 8, 9, 2047, 2048, 2049, 4097, 65537]
STRIDE_SIZE = (1 << 21) + 2049
CLASS_COUNTS = [1, 2, 5, 8, 9, 17, 1024]
MAPS = ["constant", "mod", "runs", "edges", "random", "empty", "last_only"]
BASES = ["zero", "one", "two", "minus_one", "random"]


def class_map(kind, n, C, seed):
    """n class ids below C as np.uint32.  `empty` and `last_only` need two classes: with one they are the constant map."""
    rnd = np.random.RandomState(seed)
    i = np.arange(n, dtype=np.int64)
    if kind == "constant" or (C == 1 and kind in ("empty", "last_only")):
        m = np.full(n, C // 2)
    elif kind == "mod":
        m = i % C
    elif kind == "runs":                               # C equal contiguous runs
        m = i * C // n
    elif kind == "edges":                              # run boundaries at 8 k - 1, 8 k, 8 k + 1: 7, 16, 25, then every 24 on
        bounds = np.array([b for k in range(0, n // 8 + 2, 3) for b in (8 * k + 7, 8 * k + 16, 8 * k + 25)])
        m = np.searchsorted(bounds, i, side="right") % C
    elif kind == "random":
        m = rnd.randint(0, C, n)
    elif kind == "empty":                              # class C // 3 has no member
        m = rnd.randint(0, C - 1, n)
        m = m + (m >= C // 3)
    elif kind == "last_only":                          # class C - 1 holds the last index alone
        m = rnd.randint(0, C - 1, n)
        m[n - 1] = C - 1
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(m, dtype=np.uint32)


def base(curve, kind, seed):
    r = CURVE_PARAMS[curve]["r"]
    return {"zero": 0, "one": 1, "two": 2, "minus_one": r - 1}.get(kind, random.Random(seed).randrange(3, r - 1))


def case_list(n):
    """(class count, map, base) of the cases at size n: every combination at the chunk edge; every class count with every map
    at the workgroup edge (the bases in turn) and every base once; at 65 537 every map and every class count below the cap once."""
    if n <= 9:
        return [(C, m, b) for C in CLASS_COUNTS for m in MAPS for b in BASES]
    if n <= 4097:
        out = [(C, m, BASES[(ci + mi) % len(BASES)]) for ci, C in enumerate(CLASS_COUNTS) for mi, m in enumerate(MAPS)]
        return out + [(5, "random", b) for b in BASES] + [(9, "edges", b) for b in BASES]
    if n == STRIDE_SIZE:
        return [(5, "random", "random")]
    below_cap = CLASS_COUNTS[:-1]                      # the cap's 128 passes are covered up to 4 097
    return ([(below_cap[mi % len(below_cap)], m, BASES[mi % len(BASES)]) for mi, m in enumerate(MAPS)] +
            [(C, MAPS[(ci + 3) % len(MAPS)], "random") for ci, C in enumerate(below_cap)])


@functools.lru_cache(maxsize=None)
def case(curve, n, C, kind, base_kind):
    """(x, class_of, the mirror's Montgomery bytes) of one case; computed once, never changed."""
    seed = (n * 1031 + C * 17 + MAPS.index(kind)) & 0x7fffffff
    x = base(curve, base_kind, seed)
    cls = class_map(kind, n, C, seed)
    cls.setflags(write=False)
    want = FrCodec(curve).enc(class_power_sums_host(x, cls.tolist(), C, CURVE_PARAMS[curve]["r"])).tobytes()
    return x, cls, want
