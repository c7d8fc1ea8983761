"""GPU: the group sweeps through the entry points callers use - hk_msm_g1 / _g2 and hk_bases_upload + hk_msm_bases on the
SMALL path (n element-wise products + one workgroup's sum), hk_fixed_base_g1 across the size at which
MsmRun::batch_affine goes from one point per lane to two, hk_points_lincomb_*'s refusals, hk_points_fold_many_* with mixed
host and device outputs, and the fold's contract for magnitudes longer than the K-lane form reads.

Points are k G with known k (tests/msm_edges.py, tests/sweep_edges.py), every expected value is one oracle multiplication,
every comparison is exact.
"""
import ctypes

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.capi import DeviceBuffer
from tests import msm_edges as me
from tests import sweep_edges as se

pytestmark = pytest.mark.gpu


def _ctx(gid, ctx_bn254, ctx_bls):
    return ctx_bn254 if se.cname(gid) == "bn254" else ctx_bls


Io = se.Io


# ---- short MSMs on the small path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", range(4))
def test_msm_families_on_the_small_path(gid, ctx_bn254, ctx_bls, monkeypatch):
    """the families of test_plain_msm_families_through_the_bucket_pass at n = 300, without HK_MSM_NO_SMALL: k_points_mul_split
    and k_points_sum_seg see every digit extreme, one base under many scalars, bases that cancel pairwise or are at infinity and
    all-zero scalars; "one base, one scalar" at n = T and 2 T makes every add of the LDS tree a doubling.  Through hk_msm_g*
    and through a resident set (short: no tables, the same path), in both scalar forms."""
    monkeypatch.delenv("HK_MSM_NO_SMALL", raising=False)
    monkeypatch.delenv("HK_BASES_TABLES", raising=False)
    io = Io(gid)
    ctx = _ctx(gid, ctx_bn254, ctx_bls)
    cname, r = se.cname(gid), io.r
    fn = ctx.msm_g1 if io.group == 1 else ctx.msm_g2
    n, c, T = 300, 6, se.SUM_THREADS[gid]
    ks = me.pool_ks(gid, n)
    k1 = [ks[0]] * n
    pm = [ks[1] if j % 2 == 0 else r - ks[1] for j in range(n)]
    uni = me.uniform(gid, n, "one_base300")["scalars"]
    vecs = [
        ("all_equal_r_minus_1", ks, [r - 1] * n),
        ("all_equal_all_min", ks, [me.all_min(cname, c)] * n),
        ("all_equal_all_max", ks, [me.all_max(cname, c)] * n),
        ("one_base", k1, uni),
        ("one_base_one_bucket", k1, [me.one_bucket(cname, c, 1)] * n),
        ("plus_minus_even", pm, [me.alternating(cname, c, 1)] * n),
        ("plus_minus_odd", pm[:n - 1], [me.all_min(cname, c)] * (n - 1)),
        ("zeros", ks, [0] * n),
        ("inf_bases_half", [0] * (n // 2) + ks[n // 2:], me.uniform(gid, n, "inf300")["scalars"]),
        ("inf_bases_all", [0] * n, me.uniform(gid, n, "inf300")["scalars"]),
        ("one_base_one_scalar_T", [ks[0]] * T, [uni[0]] * T),
        ("one_base_one_scalar_2T", [ks[0]] * (2 * T), [uni[1]] * (2 * T)),
        ("one_base_scalar_one_2T", [ks[0]] * (2 * T), [1] * (2 * T)),
    ]
    for name, kk, scalars in vecs:
        want = me.reference(gid, kk, scalars)
        if name in ("plus_minus_even", "zeros", "inf_bases_all"):
            assert want is None
        bases = io.pts(kk)
        res = ctx.bases_upload(io.group, bases, len(kk))
        try:
            for mont in (True, False):
                sc = io.fr(scalars, mont)
                assert io.dec(fn(bases, sc, montgomery=mont)) == want, "g%d hk_msm %s mont=%d" % (gid, name, mont)
                assert io.dec(res.msm(sc, montgomery=mont)) == want, "g%d hk_msm_bases %s mont=%d" % (gid, name, mont)
        finally:
            res.free()


def _device_bases(io, ctx, ks, tag):
    """k_i G from hk_fixed_base, eight of them compared with the oracle first: the reference does not rest on the code
    under test"""
    n = len(ks)
    G = me.group(io.gid)
    bases = ctx.fixed_base(io.group, io.pts([1]), io.fr(ks, False), montgomery=False)
    rn = se.rnd(io.gid, "pick/%s/%d" % (tag, n))
    for i in [0, 1, n // 2, n - 1] + [rn.randrange(n) for _ in range(4)]:
        assert io.dec(bases[i * io.pb:(i + 1) * io.pb]) == G.mul(G.gen, ks[i]), "base %d" % i
    return bases


@pytest.mark.parametrize("gid,n", [(0, 32768), (0, 32769), (1, 16384), (1, 16385)])
def test_msm_on_both_sides_of_the_small_path_boundary(gid, n, ctx_bn254, monkeypatch):
    """n K = 65 536 is the last size hk_msm_g* runs as element-wise products + k_points_sum_seg; one base more takes the bucket
    pass.  Both give ((sum s_i k_i) mod r) G."""
    monkeypatch.delenv("HK_MSM_NO_SMALL", raising=False)
    io = Io(gid)
    assert (n * se.SPLIT_K[gid] <= se.SPLIT_MAX_LANES) == (n in (32768, 16384))
    ks = se.progression(gid, n, "boundary")
    bases = _device_bases(io, ctx_bn254, ks, "boundary")
    rn = se.rnd(gid, "boundary/scalars/%d" % n)
    scalars = me.sprinkle([rn.randrange(io.r) for _ in range(n)], [0, 1, io.r - 1, se.lam(gid), io.r - se.lam(gid)], "boundary")
    scalars[n - 1] = rn.randrange(1, io.r)                  # the last element counts
    want = me.reference(gid, ks, scalars)
    fn = ctx_bn254.msm_g1 if io.group == 1 else ctx_bn254.msm_g2
    for mont in (True, False):
        assert io.dec(fn(bases, io.fr(scalars, mont), montgomery=mont)) == want, "g%d n=%d mont=%d" % (gid, n, mont)


# ---- hk_fixed_base across the chunk switch of batch_affine ---------------------------------------------------------------------
FB_VALUES = (0, 1, 2, 3, 255, 256, 65537)


@pytest.mark.parametrize("n", [65536, 65537])
def test_fixed_base_across_the_normalisation_chunk_switch(n, ctx_bn254):
    """MsmRun::batch_affine normalises one point per lane up to 65 536 points and two from 65 537 on.  Scalars cycle through
    seven small values (0 among them, and at index 65 536, the one lane of the longer vector that holds a single point): every
    output is one of seven oracle points; a device-resident base gives the same bytes."""
    io = Io(0)
    k = me.pool_ks(0)[3]
    idx = (np.arange(n) - 2) % 7
    assert n <= 65536 or FB_VALUES[idx[65536]] == 0
    scalars = np.ascontiguousarray(np.stack([np.frombuffer(io.cd.fr_canon(v), np.uint8) for v in FB_VALUES])[idx]).reshape(-1)
    want = io.tiled([v * k for v in FB_VALUES], idx)
    base = io.pts([k])
    got = ctx_bn254.fixed_base(1, base, scalars, montgomery=False)
    bad = np.nonzero((got.reshape(n, io.pb) != want.reshape(n, io.pb)).any(axis=1))[0]
    assert bad.size == 0, "n=%d: %d outputs differ, first %r" % (n, bad.size, bad[:8])
    dbase = DeviceBuffer.from_host(ctx_bn254, base)
    try:
        again = np.zeros_like(got)
        capi.check(ctx_bn254.lib.hk_fixed_base_g1(ctx_bn254.handle, ctypes.c_void_p(dbase.ptr), scalars.ctypes.data, n, 0,
                                                  again.ctypes.data), "hk_fixed_base_g1")
        assert np.array_equal(again, got)
    finally:
        dbase.free()


# ---- hk_points_lincomb_*: refusals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", range(4))
def test_lincomb_refuses_bad_vector_counts_and_null_vectors(gid, ctx_bn254, ctx_bls):
    io = Io(gid)
    ctx = _ctx(gid, ctx_bn254, ctx_bls)
    fn = ctx.lib.hk_points_lincomb_g1 if io.group == 1 else ctx.lib.hk_points_lincomb_g2
    n = 3
    vec = io.pts(me.pool_ks(gid)[:n])
    coeffs = io.fr([1] * 9)
    out = np.full(n * io.pb, 0x5A, np.uint8)
    ptrs = lambda k, null_at=None: (ctypes.c_void_p * max(k, 1))(*[None if j == null_at else vec.ctypes.data for j in range(max(k, 1))])
    assert fn(ctx.handle, ptrs(0), coeffs.ctypes.data, 0, n, out.ctypes.data) == capi.HK_ERR_ARG
    assert fn(ctx.handle, ptrs(9), coeffs.ctypes.data, 9, n, out.ctypes.data) == capi.HK_ERR_ARG
    for k, null_at in ((1, 0), (3, 1), (8, 7)):
        assert fn(ctx.handle, ptrs(k, null_at), coeffs.ctypes.data, k, n, out.ctypes.data) == capi.HK_ERR_ARG
    assert (out == 0x5A).all()                                # a refused call writes nothing
    assert fn(ctx.handle, ptrs(8), coeffs.ctypes.data, 8, n, out.ctypes.data) == capi.HK_OK
    assert [io.dec(out[i * io.pb:(i + 1) * io.pb]) for i in range(n)] == [me.point(gid, 8 * k) for k in me.pool_ks(gid)[:n]]


# ---- hk_points_fold_many_*: mixed outputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", range(4))
def test_fold_many_into_mixed_host_and_device_outputs(gid, ctx_bn254, ctx_bls):
    """host, device, host: the per-vector copy path; the same bytes as three host outputs, and the oracle's points"""
    io = Io(gid)
    ctx = _ctx(gid, ctx_bn254, ctx_bls)
    n = 37
    c = se.rnd(gid, "fold_many").randrange(io.r)
    pairs = [se.fold_vectors(gid, c, n, tag=y) for y in range(3)]
    los, his = [io.pts(l) for l, _ in pairs], [io.pts(h) for _, h in pairs]
    host = [np.zeros(n * io.pb, np.uint8) for _ in range(3)]
    ctx.points_fold_many(io.group, los, his, c, n, host)
    for y, (l, h) in enumerate(pairs):
        assert bytes(host[y]) == bytes(io.pts(se.fold_expected(gid, c, l, h))), (gid, y)
    dev = DeviceBuffer(ctx, n * io.pb)
    try:
        mixed = [np.zeros(n * io.pb, np.uint8), dev, np.zeros(n * io.pb, np.uint8)]
        ctx.points_fold_many(io.group, los, his, c, n, mixed)
        got = [mixed[0], dev.to_host(), mixed[2]]
        for y in range(3):
            assert np.array_equal(got[y], host[y]), (gid, y)
    finally:
        dev.free()


# ---- the fold's magnitude contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", range(4))
def test_fold_is_right_for_any_host_magnitude(gid, ctx_bn254, ctx_bls):
    """The K-lane form of short vectors reads a magnitude up to 0x77..7 (ND nibbles) only.  hk_points_fold_g1 / _g2 with raw
    host coefficients: at 0x77..7, at 0x77..7 + 1 and at 2^190 the call returns HK_OK and the RIGHT vector (longer
    magnitudes go to the one-lane kernel), for n on both sides of n K = 65 536 and for a short vector."""
    io = Io(gid)
    ctx = _ctx(gid, ctx_bn254, ctx_bls)
    K = se.SPLIT_K[gid]
    fn = ctx.lib.hk_points_fold_g1 if io.group == 1 else ctx.lib.hk_points_fold_g2
    lim = se.mag_limit(gid)
    n_edge = se.SPLIT_MAX_LANES // K
    pool = me.pool_ks(gid)
    lo7, hi7 = pool[50:57], pool[60:67]
    hi7[3] = 0
    for mi, big in enumerate((lim, lim + 1, 1 << 190)):
        j = mi % K                                            # the part that holds the long magnitude
        mags = [big if t == j else 5 + t for t in range(K)]
        mask = (1 << j) | (1 if mi == 2 else 0)
        c = se.fold_scalar(gid, mags, mask)
        lo_logs = list(lo7)
        lo_logs[1] = c * hi7[1] % io.r                        # the trailing add doubles
        lo_logs[2] = (io.r - c * hi7[2]) % io.r               # ... and cancels
        want7 = se.fold_expected(gid, c, lo_logs, hi7)
        assert want7[2] == 0 and want7[3] == lo_logs[3]
        coeffs = io.fr(mags)
        for n in (33, n_edge, n_edge + 1):
            idx = np.arange(n) % 7
            lo, hi, want = io.tiled(lo_logs, idx), io.tiled(hi7, idx), io.tiled(want7, idx)
            out = np.full(n * io.pb, 0x5A, np.uint8)
            st = fn(ctx.handle, lo.ctypes.data, hi.ctypes.data, coeffs.ctypes.data, mask, n, out.ctypes.data)
            assert st == capi.HK_OK, (gid, hex(big), n, st)
            bad = np.nonzero((out.reshape(n, io.pb) != want.reshape(n, io.pb)).any(axis=1))[0]
            assert bad.size == 0, "g%d magnitude %s n=%d: %d elements differ, first %r" % (gid, hex(big), n, bad.size, bad[:8])
