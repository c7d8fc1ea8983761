"""CPU: compressed points without a device - the five symbols are declared, listed and exported; the premises of the directed
families of tests/point_codec_cases.py hold; the HK_HD bodies of csrc/point_codec.cuh, compiled for the host
(tests/host_shim/point_codec_shim.cpp), give the Python mirror's bytes over every family, and the same source as a stand-alone
program runs clean under -fsanitize=address,undefined with the digests of the plain build; the codec over a stub context
whose two calls are the mirror gives the bytes and exceptions it gives without one; ProvingKeys round-trips compressed."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.ark_serialize import ArkCodec, ProvingKeys, SerializationError
from hekaton_system_amd.cp_groth16 import CommitterKey, ProvingKey, VerifyingKey
from oracle.pyref.params import CURVES
from tests import host_build
from tests import point_codec_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_SRC = "point_codec_shim.cpp"  # under tests/host_shim
SYMBOLS = ("hk_field_sqrt", "hk_points_decompress_g1", "hk_points_decompress_g2", "hk_points_compress_g1",
           "hk_points_compress_g2")
CURVE_ID = {"bn254": 0, "bls12_381": 1}


def test_symbols_declared_listed_exported():
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    declared = set(re.findall(r"\b(hk_[a-z0-9_]+)\s*\(", hdr))
    for sym in SYMBOLS:
        assert sym in declared and sym in capi.EXPORTS
        if os.path.exists(capi.LIB_PATH):
            getattr(capi.load(), sym)


# ---- premises of the families --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", pc.CURVE_NAMES)
def test_field_families_are_what_they_say(curve):
    q = CURVES[curve].q
    assert q % 4 == 3 and q % 3 == 1
    fam = pc.fq_family(curve)
    assert collections.Counter(s for _, s in fam) == {True: 7 + 32, False: 1 + 32}
    for a, is_sq in fam:
        r = pc.fq_sqrt_smaller(curve, a)
        assert (r is not None) == is_sq
        if is_sq:
            assert r * r % q == a and r <= (q - r) % q
    fam2 = pc.fq2_family(curve)
    assert collections.Counter(s for _, s in fam2) == {True: 6 + 128, False: 64}
    for a, is_sq in fam2:
        r = pc.fq2_sqrt_smaller(curve, a)
        assert (r is not None) == is_sq, a
        if is_sq:
            assert pc.fq2_mul(q, r, r) == a and not (pc.fq2_larger(curve, r) and r != (0, 0))
    # the directed ones: a non-square a0 has the root (0, s); -1 has (0, 1), the smaller of (0, +-1)
    (_, _), (sq, _), (nsq, _), (m1, _) = [a for a, _ in fam2[:4]]
    assert pc.fq_sqrt_smaller(curve, sq) is not None and pc.fq_sqrt_smaller(curve, nsq) is None
    assert pc.fq2_sqrt_smaller(curve, (sq, 0))[1] == 0 and pc.fq2_sqrt_smaller(curve, (nsq, 0))[0] == 0
    assert m1 == q - 1 and pc.fq2_sqrt_smaller(curve, (m1, 0)) == (0, 1)
    # the random squares take both deltas of the complex method
    branches = collections.Counter(pc.fq2_delta_branch(curve, a) for a, _ in fam2[6:6 + 128])
    assert branches[0] >= 16 and branches[1] >= 16


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", pc.CURVE_NAMES)
def test_point_families_are_what_they_say(curve, group):
    cp = CURVES[curve]
    G = pc.group_of(curve, group)
    rows = pc.point_family(curve, group)
    status, pts = pc.mirror_decompress(curve, group)
    assert [i for i, r in enumerate(rows) if r[2] == "inf"] == list(pc.INF_LANES)
    assert rows[1][3] == G.gen
    for i, (xb, flag, kind, P) in enumerate(rows):
        if kind in ("no_root", "range"):
            assert status[i] == 0 and not pts[i].any()
            if kind == "range":
                nb = pc.fqb(curve)
                assert any(int.from_bytes(xb[k:k + nb], "little") >= cp.q for k in range(0, len(xb), nb))
        elif kind == "inf":
            assert status[i] == 1 and not pts[i].any() and any(xb)
        else:
            assert status[i] == 1 and G.on_curve(P) and pts[i].tobytes() == pc.abi_point(curve, group, P)
            assert (G.mul(P, cp.r) is None) == (kind == "sub" or (curve == "bn254" and group == 1)), (i, kind)
        if kind == "base_y":
            assert P[1][1] == 0
    # the stored x reach the sign rule's second arm, with either flag
    if group == 2:
        assert collections.Counter(r[1] for r in rows if r[2] == "base_y") == {0: 2, pc.FLAG_LARGER: 2}
    off = pc.off_subgroup_lanes(curve, group)
    assert (len(off) == 0) == (curve == "bn254" and group == 1)
    # P and -P: the same x under the two flags
    by_x = collections.defaultdict(set)
    for xb, flag, kind, P in rows:
        if P is not None:
            by_x[xb].add(flag)
    assert sum(1 for f in by_x.values() if f == {0, pc.FLAG_LARGER}) >= 16 + 8          # G and (r - 1) G are one pair


# ---- the HK_HD bodies on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """csrc/point_codec.cuh compiled for the host (g++) - the source the kernels run."""
    out = str(tmp_path_factory.mktemp("shim") / "point_codec_shim.so")
    host_build.build(SHIM_SRC, out, "-O2", *host_build.SHARED)
    lib = host_build.load(out)
    sz, vp, i = C.c_size_t, C.c_void_p, C.c_int
    lib.shim_field_sqrt.argtypes = [i, i, vp, sz, vp, vp]
    lib.shim_points_decompress.argtypes = [i, i, vp, vp, sz, vp, vp]
    lib.shim_points_compress.argtypes = [i, i, vp, sz, vp, vp]
    for f in (lib.shim_field_sqrt, lib.shim_points_decompress, lib.shim_points_compress):
        f.restype = None
    return lib


def expected_roots(curve, which):
    """(values, packed Montgomery roots, ok) of a field family through pow"""
    if which == 1:
        fam = pc.fq_family(curve)
        roots = [pc.fq_sqrt_smaller(curve, a) for a, _ in fam]
        flat_in = [a for a, _ in fam]
        flat_out = [r or 0 for r in roots]
    else:
        fam = pc.fq2_family(curve)
        roots = [pc.fq2_sqrt_smaller(curve, a) for a, _ in fam]
        flat_in = [c for a, _ in fam for c in a]
        flat_out = [c for r in roots for c in (r or (0, 0))]
    ok = np.array([r is not None for r in roots], dtype=np.uint8)
    return pc.mont_arr(curve, flat_in), pc.mont_arr(curve, flat_out), ok


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("curve", pc.CURVE_NAMES)
def test_shim_field_sqrt_matches_pow(shim, curve, which):
    data, want, want_ok = expected_roots(curve, which)
    n = want_ok.size
    out, ok = np.full(data.size + pc.GUARD, pc.GUARD_BYTE, np.uint8), np.full(n + pc.GUARD, pc.GUARD_BYTE, np.uint8)
    shim.shim_field_sqrt(CURVE_ID[curve], which, data.ctypes.data, n, out.ctypes.data, ok.ctypes.data)
    assert ok[:n].tobytes() == want_ok.tobytes()
    assert out[:data.size].tobytes() == want.tobytes()
    assert (out[data.size:] == pc.GUARD_BYTE).all() and (ok[n:] == pc.GUARD_BYTE).all()


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", pc.CURVE_NAMES)
def test_shim_decompress_and_compress_match_the_mirror(shim, curve, group):
    x, flags = pc.batch_arrays(curve, group)
    want_status, want_pts = pc.mirror_decompress(curve, group)
    pts, status = np.zeros_like(want_pts), np.full(pc.BATCH, 9, np.uint8)
    shim.shim_points_decompress(CURVE_ID[curve], group, x.ctypes.data, flags.ctypes.data, pc.BATCH, pts.ctypes.data,
                                status.ctypes.data)
    assert status.tobytes() == want_status.tobytes()
    assert pts.tobytes() == want_pts.tobytes()
    fam = pc.compress_family(curve, group)
    abi = np.frombuffer(b"".join(r[0] for r in fam), dtype=np.uint8).copy()
    xo, fo = np.zeros(len(fam) * x.shape[1], np.uint8), np.full(len(fam), 9, np.uint8)
    shim.shim_points_compress(CURVE_ID[curve], group, abi.ctypes.data, len(fam), xo.ctypes.data, fo.ctypes.data)
    assert xo.tobytes() == b"".join(r[1] for r in fam)
    assert fo.tolist() == [r[2] for r in fam]


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """The shim's own main: built plain and with -fsanitize=address,undefined, both exit 0, the sanitized run reports nothing
    and prints the digests of the plain one."""
    outs = []
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("point_codec_" + tag))
        host_build.build(SHIM_SRC, exe, "-DPOINT_CODEC_MAIN", *flags)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (tag, r.stderr[-2000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].splitlines()
    assert len(lines) == 4 * 3 and lines[-1].startswith("bls12_381 fq2 n=65 roots=")
    # half the inputs are squares by construction, and about half of the rest: roots and on-curve x both occur
    for l in lines:
        m = re.search(r"n=(\d+) roots=(\d+) points=(\d+)", l)
        n, roots, points = (int(v) for v in m.groups())
        assert (n + 1) // 2 <= roots <= n and (n == 1 or 0 < points < n)


# ---- the codec over a stub context -----------------------------------------------------------------------------------------
class MirrorContext:
    """Stands in for capi.Context under ArkCodec: the two point calls are the mirror's, field_convert is the host path's.
    `off_subgroup`: x (canonical bytes) of the points that a check reports with status 2."""

    def __init__(self, curve, off_subgroup=()):
        self.cd = ArkCodec(curve)
        self.off = set(off_subgroup)
        self.calls = []

    def field_convert(self, which, data, to_mont):
        return self.cd._convert(which, data, to_mont)

    def points_decompress(self, group, x_canon, flags, check=False, out=None):
        cd = self.cd
        n = flags.size
        self.calls.append(("decompress", group, n, bool(check)))
        xs = np.asarray(x_canon, dtype=np.uint8).reshape(n, group, cd.fqb)
        pts = np.zeros((n, 2 * group * cd.fqb), dtype=np.uint8)
        status = np.ones(n, dtype=np.uint8)
        for i in range(n):
            if flags[i] & 1:
                continue
            try:
                canon = cd._decompress(group, xs[i:i + 1], np.array([False]), np.array([bool(flags[i] & 2)]))
                pts[i] = cd._convert(1, canon, True)
                if check and xs[i].tobytes() in self.off:
                    status[i] = 2
            except SerializationError:
                status[i] = 0
        return pts.reshape(-1), status

    def points_compress(self, group, pts):
        cd = self.cd
        coords = 2 * group
        abi = np.asarray(pts, dtype=np.uint8).reshape(-1, coords * cd.fqb)
        self.calls.append(("compress", group, abi.shape[0]))
        inf = ~abi.any(axis=1)
        canon = cd._convert(1, abi, False).reshape(-1, coords, cd.fqb)
        neg = cd._y_negative(canon, group) & ~inf
        return canon[:, :group].reshape(-1).copy(), (inf.astype(np.uint8) | (neg.astype(np.uint8) << 1))


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", pc.CURVE_NAMES)
def test_codec_over_a_context_gives_the_hosts_bytes_and_exceptions(curve, group):
    rows = pc.point_family(curve, group)
    _, want_pts = pc.mirror_decompress(curve, group)
    good = [i for i, r in enumerate(rows) if r[2] in ("sub", "curve", "base_y", "inf")]
    off = [rows[i][0] for i in pc.off_subgroup_lanes(curve, group)]
    plain, ctx = ArkCodec(curve), MirrorContext(curve, off)
    dev = ArkCodec(curve, ctx)
    wire = b"".join(pc.wire_of(curve, group, rows[i][0], rows[i][1]) for i in good)
    abi = want_pts[good].reshape(-1)
    # reading and writing: the same bytes, through the context's calls
    got = dev.points_from_wire(group, wire, len(good), compress=True)
    assert got.tobytes() == abi.tobytes() == plain.points_from_wire(group, wire, len(good), compress=True).tobytes()
    assert dev.points_to_wire(group, abi, compress=True) == wire == plain.points_to_wire(group, abi, compress=True)
    assert [c[0] for c in ctx.calls] == ["decompress", "compress"] and ctx.calls[0][3] is False
    # uncompressed data does not go near them
    full = plain.points_to_wire(group, abi)
    assert dev.points_to_wire(group, abi) == full and dev.points_from_wire(group, full, len(good)).tobytes() == abi.tobytes()
    assert len(ctx.calls) == 2
    # the exceptions: no root, a coordinate that is not reduced, flags
    bad = next(i for i, r in enumerate(rows) if r[2] == "no_root")
    for cd in (plain, dev):
        with pytest.raises(SerializationError, match="x is not on the curve"):
            cd.points_from_wire(group, pc.wire_of(curve, group, rows[bad][0], rows[bad][1]), 1, compress=True)
        with pytest.raises(SerializationError, match="wrong length"):
            cd.points_from_wire(group, wire[:-1], len(good), compress=True)
        q_wire = pc.wire_of(curve, group, pc.x_bytes(curve, group, CURVES[curve].q if group == 1 else (CURVES[curve].q, 0)), 0)
        with pytest.raises(SerializationError, match="not reduced"):
            cd.points_from_wire(group, q_wire, 1, compress=True)
    # validate: ark's checked deserialize_compressed
    ok_lanes = [i for i in good if rows[i][2] in ("sub", "inf")]
    ok_wire = b"".join(pc.wire_of(curve, group, rows[i][0], rows[i][1]) for i in ok_lanes)
    assert dev.points_from_wire(group, ok_wire, len(ok_lanes), compress=True, validate=True).tobytes() == want_pts[ok_lanes].tobytes()
    assert ctx.calls[-1][3] is True
    if off:
        with pytest.raises(SerializationError, match="InvalidData.*subgroup"):
            dev.points_from_wire(group, wire, len(good), compress=True, validate=True)
    with pytest.raises(ValueError):
        plain.points_from_wire(group, wire, len(good), compress=True, validate=True)
    with pytest.raises(ValueError):
        dev.points_from_wire(group, full, len(good), validate=True)


# ---- the key file ------------------------------------------------------------------------------------------------------------
def _small_keys(curve):
    _, g1 = pc.mirror_decompress(curve, 1)
    _, g2 = pc.mirror_decompress(curve, 2)
    g1 = g1[[i for i, r in enumerate(pc.point_family(curve, 1)) if r[2] in ("sub", "inf")][:14]]
    g2 = g2[[i for i, r in enumerate(pc.point_family(curve, 2)) if r[2] in ("sub", "inf")][:6]]
    P1 = lambda a, b=None: g1[a:(a + 1 if b is None else b)].reshape(-1).copy()
    P2 = lambda a, b=None: g2[a:(a + 1 if b is None else b)].reshape(-1).copy()

    def mk(k):
        vk = VerifyingKey(P1(1), P2(1), P2(2), P2(3), P1(1, 3), P2(3, 5))
        ck = CommitterKey(P1(3), [P1(4, 6), P1(6, 9 + k)])
        return ProvingKey(vk, P1(9), P1(0, 5), P1(5, 10), P2(0, 5), P1(2, 13), ck, P1(10, 12))
    return ProvingKeys("BigMerkle circuit", b"\x01\x02\x03", {0: mk(0), 5: mk(1)}, {0: 0, 1: 0, 2: 5, 3: 5})


def _pk_points(cd, pk):
    """(group, array) of every point field of a ProvingKey, in wire order"""
    vk = pk.vk
    out = [(1, vk.alpha_g), (2, vk.beta_h), (2, vk.gamma_h), (2, vk.last_delta_h), (1, vk.gamma_abc_g), (2, vk.deltas_h),
           (1, pk.beta_g), (1, pk.a_g), (1, pk.b_g), (2, pk.b_h), (1, pk.h_g), (1, pk.ck.last_delta_g)]
    out += [(1, v) for v in pk.ck.deltas_abc_g] + [(1, pk.deltas_g)]
    return out


@pytest.mark.parametrize("curve", pc.CURVE_NAMES)
def test_proving_keys_round_trip_compressed_on_the_host(curve):
    cd = ArkCodec(curve)
    pks = _small_keys(curve)
    plain = pks.serialize(cd)
    assert plain == pks.serialize(cd, True, False) and ProvingKeys.deserialize(cd, plain).serialize(cd) == plain
    blob = pks.serialize(cd, compress=True)
    # framing as before; every point at point_size(group, True)
    n_points = n_vecs = 0
    want = 8 + len("BigMerkle circuit") + 8 + 3 + 8 + 8 + 4 * 16
    for k, pk in pks.minimal_proving_keys.items():
        want += 8 + 8                                                   # the map's key, the committer key's stage count
        for group, arr in _pk_points(cd, pk):
            n = arr.size // (cd.g1b if group == 1 else cd.g2b)
            want += n * cd.point_size(group, True)
            n_points += n
        want += 8 * (2 + 4 + len(pk.ck.deltas_abc_g) + 1)               # Vec length prefixes
    assert len(blob) == want and len(blob) < len(plain)
    back = ProvingKeys.deserialize(cd, blob, compress=True)
    assert back.serialize(cd) == plain and back.serialize(cd, compress=True) == blob
    for k, pk in pks.minimal_proving_keys.items():
        for (g, a), (_, b) in zip(_pk_points(cd, pk), _pk_points(cd, back.minimal_proving_keys[k])):
            assert a.tobytes() == b.tobytes()
    # and over a context whose calls are the mirror's: the same file, the same key
    dev = ArkCodec(curve, MirrorContext(curve))
    assert pks.serialize(dev, compress=True) == blob
    assert ProvingKeys.deserialize(dev, blob, compress=True, validate=True).serialize(cd) == plain
    with pytest.raises(SerializationError):
        ProvingKeys.deserialize(cd, blob[:-3], compress=True)
