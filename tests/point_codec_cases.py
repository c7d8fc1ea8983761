"""Directed inputs of the compressed-point tests (hk_field_sqrt, hk_points_decompress_*, hk_points_compress_*), shared by
tests/test_point_codec_cpu.py (their premises, the host shim, the codec over a stub context) and tests/test_point_codec_gpu.py.
Expected values are pure Python: `pow` on integers, `ArkCodec(curve)` without a context (the mirror), oracle.pyref for points.
Everything is built once per curve and never changed."""
import functools
import json
import os
import random

import numpy as np

from hekaton_system_amd.ark_serialize import ArkCodec, SerializationError
from oracle.pyref import curve as oc
from oracle.pyref.params import CURVES

CURVE_NAMES = ("bn254", "bls12_381")
SIZES = (1, 63, 64, 65, 130)
BATCH = 130
INF_LANES = (0, 63, 64)
FLAG_INF, FLAG_LARGER = 1, 2
GUARD = 64                                       # bytes behind every output that must keep their pattern
GUARD_BYTE = 0xA5

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_codec.json")) as _f:
    FIXTURE = json.load(_f)

# published zcash encodings of the BLS12-381 generators (the constants of tests/test_ark_serialize.py, restated)
BLS_G1_COMPRESSED = ("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac58"
                     "6c55e83ff97a1aeffb3af00adb22c6bb")
BLS_G1_UNCOMPRESSED = ("17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
                       "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1")
BLS_G2_COMPRESSED = ("93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
                     "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")
BLS_G2_UNCOMPRESSED = ("13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
                       "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8"
                       "0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be"
                       "0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801")


def codec(curve):
    return _codec(curve)


@functools.lru_cache(maxsize=None)
def _codec(curve):
    return ArkCodec(curve)


def fqb(curve):
    return codec(curve).fqb


def le(curve, v):
    return int(v).to_bytes(fqb(curve), "little")


def mont(curve, v):
    """Montgomery bytes of one Fq value."""
    cd = codec(curve)
    return le(curve, v * cd.Rq % cd.q)


def mont_arr(curve, vals):
    """Packed Montgomery array of Fq values (an Fq2 element is two of them, c0 first)."""
    return np.frombuffer(b"".join(mont(curve, v) for v in vals), dtype=np.uint8).copy()


def from_mont_arr(curve, arr):
    cd = codec(curve)
    b = np.asarray(arr, dtype=np.uint8).tobytes()
    ri = pow(cd.Rq, -1, cd.q)
    return [int.from_bytes(b[i:i + cd.fqb], "little") * ri % cd.q for i in range(0, len(b), cd.fqb)]


# ---- square roots, as integers --------------------------------------------------------------------------------------------
def fq_sqrt_smaller(curve, a):
    """The root of a that is not larger than its negative, or None."""
    q = codec(curve).q
    s = pow(a, (q + 1) // 4, q)
    if s * s % q != a:
        return None
    return min(s, q - s) if s else 0


def fq2_larger(curve, y):
    half = (codec(curve).q - 1) // 2
    return y[1] > half if y[1] else y[0] > half


def fq2_sqrt_smaller(curve, a):
    cd = codec(curve)
    r = cd._fq2_sqrt(a[0] % cd.q, a[1] % cd.q)
    if r is None:
        return None
    return ((-r[0]) % cd.q, (-r[1]) % cd.q) if fq2_larger(curve, r) else r


def fq2_mul(q, a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % q, (a[0] * b[1] + a[1] * b[0]) % q)


def _is_qr(q, a):
    return a == 0 or pow(a, (q - 1) // 2, q) == 1


@functools.lru_cache(maxsize=None)
def fq_family(curve):
    """[(a, is_square)]: 0, 1, 4, q - 1 (no square: q = 3 mod 4), the squares of 1, q - 1, (q - 1) / 2, (q + 1) / 2, 32 random
    squares, 32 random non-squares."""
    q = codec(curve).q
    rnd = random.Random("fq " + curve)
    out = [(0, True), (1, True), (4, True), (q - 1, False)]
    out += [(v * v % q, True) for v in (1, q - 1, (q - 1) // 2, (q + 1) // 2)]
    out += [(pow(rnd.randrange(1, q), 2, q), True) for _ in range(32)]
    while len(out) < 8 + 32 + 32:
        v = rnd.randrange(1, q)
        if not _is_qr(q, v):
            out.append((v, False))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fq2_family(curve):
    """[((a0, a1), is_square)]: (a0, 0) with a0 a square and a non-square (root (0, s)), -1 (root (0, 1)), (0, a1) twice,
    128 random squares, 64 random non-squares (the norm is no square in Fq)."""
    q = codec(curve).q
    rnd = random.Random("fq2 " + curve)
    sq = pow(rnd.randrange(2, q), 2, q)
    out = [((0, 0), True), ((sq, 0), True), ((q - sq, 0), True), ((q - 1, 0), True), ((0, sq), True), ((0, q - sq), True)]
    for _ in range(128):
        v = (rnd.randrange(q), rnd.randrange(1, q))
        out.append((fq2_mul(q, v, v), True))
    while len(out) < 6 + 128 + 64:
        v = (rnd.randrange(q), rnd.randrange(q))
        if not _is_qr(q, (v[0] * v[0] + v[1] * v[1]) % q):
            out.append((v, False))
    return tuple(out)


def fq2_delta_branch(curve, a):
    """Which delta of the complex method the mirror's Fq2 root of a square a (a1 != 0) takes: 0 = (a0 + alpha) / 2, 1 = the
    other."""
    cd = codec(curve)
    q = cd.q
    alpha = cd._fq_sqrt((a[0] * a[0] + a[1] * a[1]) % q)
    return 0 if cd._fq_sqrt((a[0] + alpha) * pow(2, -1, q) % q) is not None else 1


# ---- points ---------------------------------------------------------------------------------------------------------------
def group_of(curve, group):
    cp = CURVES[curve]
    return oc.G1(cp) if group == 1 else oc.G2(cp)


def _coords(group, v):
    return (v,) if group == 1 else tuple(v)


def x_bytes(curve, group, x):
    """canonical little-endian x as the kernels take it (G2: c0 || c1)"""
    return b"".join(le(curve, c) for c in _coords(group, x))


def larger(curve, group, y):
    return y > (codec(curve).q - 1) // 2 if group == 1 else fq2_larger(curve, y)


def abi_point(curve, group, P):
    """packed affine Montgomery bytes of an oracle point (None: infinity)"""
    n = 2 * fqb(curve) * group
    if P is None:
        return bytes(n)
    return b"".join(mont(curve, c) for c in _coords(group, P[0]) + _coords(group, P[1]))


def _curve_y(curve, group, x):
    """some y with (x, y) on the curve, through the mirror's roots, or None"""
    cd = codec(curve)
    G = group_of(curve, group)
    F = G.F
    rhs = F.add(F.mul(F.mul(x, x), x), G.b)
    return cd._fq_sqrt(rhs) if group == 1 else cd._fq2_sqrt(*rhs)


def _rand_x(rnd, q, group):
    return rnd.randrange(q) if group == 1 else (rnd.randrange(q), rnd.randrange(q))


@functools.lru_cache(maxsize=None)
def point_family(curve, group):
    """The batch of 130 compressed points, as a tuple of (x_bytes, flag, kind, point):
      kind "sub"     k G (the generator, small and random k, P and -P): in the prime-order subgroup
           "curve"   a random x with a root, both flags: on the curve, in the subgroup only where the cofactor is 1
           "base_y"  G2, the fixture's x with y = (y0, 0) and (q - y0, 0)
           "no_root" x^3 + b is no square        "range" x = q, x = 2^(8 fq_bytes) - 1 (G2: in either coordinate)
           "inf"     at lanes 0, 63 and 64, with a non-zero x that must be ignored
    point: the oracle's affine point, None where there is none."""
    cp = CURVES[curve]
    q = cp.q
    G = group_of(curve, group)
    rnd = random.Random("points %s %d" % (curve, group))
    rows = []

    def add(P, kind):
        rows.append((x_bytes(curve, group, P[0]), FLAG_LARGER if larger(curve, group, P[1]) else 0, kind, P))

    ks = [1, 2, 3, 5, cp.r - 1] + [rnd.randrange(1, cp.r) for _ in range(12)]
    for k in ks:
        P = G.mul(G.gen, k)
        add(P, "sub")
        add(G.neg(P), "sub")
    n_curve = n_bad = 0
    while n_curve < 8 or n_bad < 4:
        x = _rand_x(rnd, q, group)
        y = _curve_y(curve, group, x)
        if y is None and n_bad < 4:
            rows.append((x_bytes(curve, group, x), rnd.choice((0, FLAG_LARGER)), "no_root", None))
            n_bad += 1
        elif y is not None and n_curve < 8:
            add((x, y), "curve")
            add(G.neg((x, y)), "curve")
            n_curve += 1
    top = (1 << (8 * fqb(curve))) - 1
    if group == 1:
        ranges = [q, top]
    else:
        ranges = [(q, 0), (0, q), (top, top)]
    rows += [(x_bytes(curve, group, x), 0, "range", None) for x in ranges]
    if group == 2:
        for e in FIXTURE[curve]["g2_y_in_base_field"]:
            x = (int(e["x"][0], 16), int(e["x"][1], 16))
            add((x, (e["y0"], 0)), "base_y")
            add((x, (q - e["y0"], 0)), "base_y")
    while len(rows) < BATCH - len(INF_LANES):
        add(G.mul(G.gen, rnd.randrange(1, cp.r)), "sub")
    rnd.shuffle(rows)
    for lane in INF_LANES:
        rows.insert(lane, (x_bytes(curve, group, _rand_x(rnd, q, group)), FLAG_INF, "inf", None))
    # lane 1 is what the batch of one decompresses: the generator
    g = next(i for i, r in enumerate(rows) if r[3] == G.gen)
    rows[1], rows[g] = rows[g], rows[1]
    assert len(rows) == BATCH
    return tuple(rows)


def batch_slice(n):
    """Which lanes of the batch a test of n points takes: the generator alone, else the first n (infinity at 0, 63, 64)."""
    return slice(1, 2) if n == 1 else slice(0, n)


def wire_of(curve, group, xb, flag):
    """The ark-serialize compressed encoding of one (x, flag) of the batch - what the mirror reads."""
    cd = codec(curve)
    nb = cd.fqb
    if flag & FLAG_INF:
        xb = bytes(len(xb))
    if not cd.zcash:
        b = bytearray(xb)
        b[-1] |= 0x40 if flag & FLAG_INF else (0x80 if flag & FLAG_LARGER else 0)
        return bytes(b)
    cs = [xb[i:i + nb][::-1] for i in range(0, len(xb), nb)]
    b = bytearray(b"".join(reversed(cs)))
    b[0] |= 0x80 | (0x40 if flag & FLAG_INF else (0x20 if flag & FLAG_LARGER else 0))
    return bytes(b)


@functools.lru_cache(maxsize=None)
def mirror_decompress(curve, group):
    """(status, points) of the whole batch through the mirror, one point at a time: status 1 and what
    `ArkCodec(curve).points_from_wire(compress=True)` returns, or 0 and zeros where it raises `x is not on the curve` - and,
    by definition of the format, where x is not below q (such an x has no encoding: its top bits are the flags')."""
    cd = codec(curve)
    pb = 2 * cd.fqb * group
    status, pts = [], []
    for xb, flag, kind, _ in point_family(curve, group):
        if kind == "range":
            status.append(0)
            pts.append(bytes(pb))
            continue
        try:
            pts.append(cd.points_from_wire(group, wire_of(curve, group, xb, flag), 1, compress=True).tobytes())
            status.append(1)
        except SerializationError as e:
            assert "x is not on the curve" in str(e)
            status.append(0)
            pts.append(bytes(pb))
    return np.array(status, dtype=np.uint8), np.frombuffer(b"".join(pts), dtype=np.uint8).reshape(BATCH, pb).copy()


def off_subgroup_lanes(curve, group):
    """Lanes whose point is on the curve but outside the prime-order subgroup - by construction; test_point_codec_cpu.py
    confirms [r] P != O for each.  BN254 G1 has cofactor 1: none."""
    if curve == "bn254" and group == 1:
        return []
    return [i for i, r in enumerate(point_family(curve, group)) if r[2] in ("curve", "base_y")]


def batch_arrays(curve, group):
    """(x_canon, flags) of the batch as the ABI takes them"""
    rows = point_family(curve, group)
    x = np.frombuffer(b"".join(r[0] for r in rows), dtype=np.uint8).reshape(BATCH, -1).copy()
    return x, np.array([r[1] for r in rows], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def compress_family(curve, group):
    """Points for compression alone (no curve check applies, so coordinates are free), as (abi bytes, x_bytes, flag): y - in
    G2 the deciding coordinate, c1, and c0 under c1 == 0 - over 1, (q - 1) / 2, (q + 1) / 2, q - 1; infinity; and every
    decompressed point of the batch."""
    q = codec(curve).q
    rnd = random.Random("compress %s %d" % (curve, group))
    edge = (1, (q - 1) // 2, (q + 1) // 2, q - 1)
    rows = []

    def add(x, y):
        rows.append((abi_point(curve, group, (x, y)), x_bytes(curve, group, x), FLAG_LARGER if larger(curve, group, y) else 0))

    for v in edge:
        if group == 1:
            add(rnd.randrange(q), v)
        else:
            add(_rand_x(rnd, q, 2), (v, 0))
            for c0 in (0,) + edge:
                add(_rand_x(rnd, q, 2), (c0, v))
    rows.append((abi_point(curve, group, None), bytes(fqb(curve) * group), FLAG_INF))
    for xb, flag, kind, P in point_family(curve, group):
        if P is not None:
            rows.append((abi_point(curve, group, P), xb, flag))
    return tuple(rows)
