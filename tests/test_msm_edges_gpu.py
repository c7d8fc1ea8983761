"""GPU: the directed scalars and vectors of tests/msm_edges.py through the entry points callers use - hk_msm_g1 / hk_msm_g2,
hk_bases_upload + hk_msm_bases, hk_commit / hk_prove - so the plans the product really picks are shown to behave like the
forced ones of tests/test_msm_plan_device_gpu.py.  Every MSM is compared exactly with
reference(ks, scalars) = ((sum s_i k_i) mod r) G, the prove path bit for bit with the Python oracle.
"""
import random

import numpy as np
import pytest

from oracle.pyref import groth16
from oracle.pyref.codec import Codec
from oracle.pyref.params import CURVES
from tests import msm_edges as me
from tests.util import pk_upload_from_oracle

pytestmark = pytest.mark.gpu


def pick_c_plain(n, bits):
    """Python copy of msm_pick_c_plain (csrc/curve_ops_impl.cuh): a retuned picker must fail these tests, not silently
    move them to another window size"""
    best, best_cost = 4, 1e300
    for c in range(3, 13):
        W = (bits + 2 + c - 1) // c
        if W << (c - 1) > me.MSM_LDS_COUNTERS:
            continue
        cost = n * W + 4.0 * (W << (c - 1))
        if cost < best_cost:
            best, best_cost = c, cost
    return best


def pick_c_tables(n, bits):
    """Python copy of msm_pick_c_tables"""
    best, best_cost = 6, 1e300
    for c in range(5, 17):
        W = (bits + 2 + c - 1) // c
        cost = n * W + 6.0 * (1 << (c - 1))
        if cost < best_cost:
            best, best_cost = c, cost
    return best


def _ctx(gid, ctx_bn254, ctx_bls):
    return ctx_bn254 if me.GROUPS[gid][0] == "bn254" else ctx_bls


def _io(gid, cd):
    g1 = me.GROUPS[gid][1] == "g1"
    return (cd.g1_vec, cd.g1_from) if g1 else (cd.g2_vec, cd.g2_from)


# ---- hk_msm_g1 / hk_msm_g2 by the bucket method ---------------------------------------------------------------------------
@pytest.mark.parametrize("gid", range(4))
def test_plain_msm_families_through_the_bucket_pass(gid, ctx_bn254, ctx_bls, monkeypatch):
    """n = 300 with HK_MSM_NO_SMALL: the plain plan (c = 6, WP = W) on vectors whose every digit is extreme, whose bases
    are all one point, cancel pairwise, are at infinity, or whose scalars are all zero (the bucket pass with E = 0)"""
    monkeypatch.setenv("HK_MSM_NO_SMALL", "1")
    n = 300
    cname, grp = me.GROUPS[gid]
    cp = CURVES[cname]
    ctx = _ctx(gid, ctx_bn254, ctx_bls)
    cd = Codec(cp)
    enc, dec = _io(gid, cd)
    fn = ctx.msm_g1 if grp == "g1" else ctx.msm_g2
    c = pick_c_plain(n, cp.r.bit_length())
    assert c == 6
    ks = me.pool_ks(gid, n)
    k1 = [ks[0]] * n
    vecs = [
        ("all_equal_r_minus_1", ks, [cp.r - 1] * n),
        ("all_equal_all_min", ks, [me.all_min(cname, c)] * n),
        ("all_equal_all_max", ks, [me.all_max(cname, c)] * n),
        ("one_base", k1, me.uniform(gid, n, "one_base300")["scalars"]),
        ("one_base_one_bucket", k1, [me.one_bucket(cname, c, 1)] * n),
        ("plus_minus_even", [ks[1] if j % 2 == 0 else cp.r - ks[1] for j in range(n)], [me.alternating(cname, c, 1)] * n),
        ("plus_minus_odd", [ks[1] if j % 2 == 0 else cp.r - ks[1] for j in range(n - 1)], [me.all_min(cname, c)] * (n - 1)),
        ("zeros", ks, [0] * n),
        ("inf_bases_half", [0] * (n // 2) + ks[n // 2:], me.uniform(gid, n, "inf300")["scalars"]),
        ("inf_bases_all", [0] * n, me.uniform(gid, n, "inf300")["scalars"]),
    ]
    for j, (name, kk, scalars) in enumerate(vecs):
        want = me.reference(gid, kk, scalars)
        if name in ("plus_minus_even", "zeros", "inf_bases_all"):
            assert want is None
        mont = j % 2 == 0
        sc = cd.fr_vec_mont(scalars) if mont else cd.fr_vec_canon(scalars)
        got = dec(fn(enc(me.points(gid, kk)), sc, montgomery=mont))
        assert got == want, "g%d %s: got %r, want %r" % (gid, name, got, want)


# ---- resident bases with shift tables ---------------------------------------------------------------------------------------
def _resident_case(gid, n, want_c, ctx, families):
    cname, grp = me.GROUPS[gid]
    cp = CURVES[cname]
    cd = Codec(cp)
    enc, dec = _io(gid, cd)
    group = 1 if grp == "g1" else 2
    pb = cd.g1_bytes if group == 1 else cd.g2_bytes
    r = cp.r
    assert pick_c_tables(n, r.bit_length()) == want_c
    c = want_c
    # bases k_i G from the device's fixed-base path; 8 of them compared with Python first, so that the reference does not
    # rest on the code under test
    rnd = random.Random("resident/%d/%d" % (gid, n))
    k0, d = rnd.randrange(1, r), rnd.randrange(1, r)
    ks = [(k0 + i * d) % r for i in range(n)]
    G = me.group(gid)
    bases = ctx.fixed_base(group, enc([G.gen]), cd.fr_vec_canon(ks), montgomery=False)
    for i in [0, 1, n // 2, n - 1] + [rnd.randrange(n) for _ in range(4)]:
        assert dec(bases[i * pb:(i + 1) * pb]) == G.mul(G.gen, ks[i]), "base %d" % i
    named = me.named_scalars(cname, c) + [me.all_min(cname, c), me.all_max(cname, c), me.alternating(cname, c, 1)]
    uni = me.sprinkle([rnd.randrange(r) for _ in range(n)], named, "resident%d" % gid)
    assert set(named) <= set(uni)
    all_vecs = {
        "all_equal_all_min": [me.all_min(cname, c)] * n,          # c = 16: every digit -2^15, one bucket holds everything
        "all_equal_all_max": [me.all_max(cname, c)] * n,
        "all_equal_r_minus_1": [r - 1] * n,
        "uniform_named": uni,
    }
    res = ctx.bases_upload(group, bases, n)
    try:
        for j, name in enumerate(f for f in families if f != "one_base"):
            scalars = all_vecs[name]
            mont = j % 2 == 1
            one = (cd.fr_mont if mont else cd.fr_canon)(scalars[0])
            sc = (np.frombuffer(one * n, dtype=np.uint8).copy() if name.startswith("all_equal")
                  else (cd.fr_vec_mont if mont else cd.fr_vec_canon)(scalars))
            got = dec(res.msm(sc, montgomery=mont))
            assert got == me.reference(gid, ks, scalars), "g%d n=%d %s" % (gid, n, name)
    finally:
        res.free()
    if "one_base" in families:
        # every base the same point: whatever order the scatter leaves a bucket in, consecutive entries are equal
        P = bases[:pb]
        res = ctx.bases_upload(group, np.tile(P, n), n)
        try:
            got = dec(res.msm(cd.fr_vec_canon(uni), montgomery=False))
            assert got == me.reference(gid, [ks[0]] * n, uni), "g%d n=%d one_base" % (gid, n)
        finally:
            res.free()


ALL_FAMILIES = ("all_equal_all_min", "all_equal_all_max", "all_equal_r_minus_1", "one_base", "uniform_named")


@pytest.mark.parametrize("gid,n,c", [(0, 8193, 13), (2, 8193, 13), (1, 2049, 11), (3, 2049, 11)])
def test_resident_bases_just_above_the_table_threshold(gid, n, c, ctx_bn254, ctx_bls):
    _resident_case(gid, n, c, _ctx(gid, ctx_bn254, ctx_bls), ALL_FAMILIES)


@pytest.mark.parametrize("gid,n", [(0, 65536), (2, 131072)])
def test_resident_bases_at_window_size_16(gid, n, ctx_bn254, ctx_bls):
    """the smallest sizes at which msm_pick_c_tables takes c = 16: digits fill the whole int16 range"""
    _resident_case(gid, n, 16, _ctx(gid, ctx_bn254, ctx_bls), ALL_FAMILIES)


# ---- prove path ----------------------------------------------------------------------------------------------------------
_keys = {}


def _uniform_circuit(cp, v, n0=20, n1=20):
    """two stages of witnesses chained by w_i * 1 = w_(i+1): every witness equals v"""
    cs = groth16.R1CS(cp.r)
    cs.begin_stage()
    ws = [cs.alloc_witness(v) for _ in range(n0)]
    cs.end_stage()
    cs.begin_stage()
    x = cs.alloc_instance(v)
    ws += [cs.alloc_witness(v) for _ in range(n1)]
    for a, b in zip(ws, ws[1:]):
        cs.enforce([(1, a)], [(1, "one")], [(1, b)])
    cs.enforce([(1, ws[-1])], [(1, "one")], [(1, x)])
    cs.end_stage()
    assert cs.is_satisfied()
    return cs


@pytest.mark.parametrize("which", ["one", "r_minus_1", "all_min"])
@pytest.mark.parametrize("compact", ["compacted", "dense"])
def test_prove_with_a_uniform_assignment(which, compact, ctx_bn254, monkeypatch):
    """the same scalar in every position of the A, B1, B2, L (idx_off) and H MSMs' inputs, with the B query compacted
    (default: its density is 1 / n) and dense (HK_B_COMPACT_BELOW=0, read per upload)"""
    cp = CURVES["bn254"]
    cd = Codec(cp)
    n_vars, n_stages = 42, 2
    # the key plans its A / B / L queries for n_ext = (n_v - 1) + r, s, r s + one kappa per committed stage (hk_pk_upload)
    n_ext = (n_vars - 1) + 3 + (n_stages - 1)
    c = pick_c_tables(n_ext, cp.r.bit_length())
    assert (n_ext, c) == (45, 7)
    v = {"one": 1, "r_minus_1": cp.r - 1, "all_min": me.all_min("bn254", c)}[which]
    cs = _uniform_circuit(cp, v)
    assert cs.num_instance + cs.num_witness == n_vars
    if "pk" not in _keys:
        _keys["pk"] = groth16.generate_parameters(cp, cs, 3, 5, 7, [11, 13], 17, 2, 3)[0]     # depends on the matrices only
    pk = _keys["pk"]
    if compact == "dense":
        monkeypatch.setenv("HK_B_COMPACT_BELOW", "0")
    else:
        monkeypatch.delenv("HK_B_COMPACT_BELOW", raising=False)
    dpk = pk_upload_from_oracle(ctx_bn254, cd, pk, cs)
    try:
        kappa, r_, s_ = 31, 32, 33
        com = cd.g1_from(dpk.commit(0, cd.fr_vec_mont(cs.stage_witness(0)), cd.fr_vec_mont([kappa])))
        assert com == groth16.commit(cp, cs, pk, 0, kappa)
        a, b, cc = dpk.prove(cd.fr_vec_mont(cs.full_assignment()), cd.fr_vec_mont([r_]), cd.fr_vec_mont([s_]),
                             cd.fr_vec_mont([kappa]))
        key = (which, "proof")
        if key not in _keys:
            _keys[key] = groth16.prove(cp, cs, pk, [com], [kappa], r_, s_)
        want = _keys[key]
        assert (cd.g1_from(a), cd.g2_from(b), cd.g1_from(cc)) == (want.a, want.b, want.c)
    finally:
        dpk.free()
