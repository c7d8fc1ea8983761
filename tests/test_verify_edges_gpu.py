"""GPU: hk_vk_prepare / hk_verify_batch / hk_points_check_* on the forged cases of tests/verify_edges.py, both curves.

Every case goes through prepare_verifying_key and DeviceVk.verify in per-proof mode, with the point check and - where
every point is valid - without it, and in batch mode under the case's own r_i or seeded nonzero 128-bit draws.  The verdicts
are compared exactly with the congruence of the forge (tests/test_verify_edges_cpu.py ties it to the oracle's pairing); in
batch mode with verify_edges.batch_model, which is that congruence for every case but the `contract` ones.  No device call
goes into an expected value.

The contract cases, as they come out on the device: two wrong proofs whose defects cancel under the r_i given
(`rand_complementary_equal`: C_0 + G and C_1 - G under equal r_i; `rand_*_cancelling`: the same idea under r - 1, 2^128 and
full-width r_i) are accepted, [1, 1], because their batch equation holds.  That is the caller's side of the documented
contract (the r_i are random and drawn after the proofs are fixed), not a fault of the entry; the assertion that two
complementary tampers are rejected is `rand_complementary_distinct`.  The cancelling pairs are kept because they are the
only inputs that show the batch pipeline from outside: a wrong r_i A_i, column sum or exponent makes their equation fail.

A case that fails is reported by name with the mode it failed in; each test collects all of its failures first.
"""
import time

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import VerifyingKey, prepare_verifying_key
from oracle.pyref import pairing
from oracle.pyref.codec import Codec
from oracle.pyref.params import CURVES
from tests import verify_edges as ve
from tests.test_pairing_cpu import Enc

pytestmark = pytest.mark.gpu
CURVE_NAMES = list(ve.CURVE_NAMES)


def _ctx(cname, ctx_bn254, ctx_bls):
    return ctx_bn254 if cname == "bn254" else ctx_bls


def _prepare(ctx, key):
    b = key.vk_bytes()
    nd = key.nd
    g2 = ctx.g2_bytes
    vk = VerifyingKey(alpha_g=b["alpha_g"], beta_h=b["beta_h"], gamma_h=b["gamma_h"], last_delta_h=b["deltas_h"][(nd - 1) * g2:],
                      gamma_abc_g=b["gamma_abc_g"], deltas_h=b["deltas_h"])
    pvk = prepare_verifying_key(ctx, vk)
    assert (pvk.device.n_deltas, pvk.device.n_abc) == (key.nd, key.n_abc)
    return pvk


def _verify_entry(dvk, ops, rand):
    """hk_verify_batch itself in batch mode, past DeviceVk.check_args: the wrapper refuses a zero r_i before the C entry sees
    it, and the entry's own answer to one is what the zero cases are about"""
    ctx = dvk.ctx
    arrs = [capi._hd(ops[k]) for k in ("a", "b", "c", "ds", "x")]
    rr = capi._hd(rand)
    out = np.zeros(ops["n"], dtype=np.uint8)
    capi.check(ctx.lib.hk_verify_batch(ctx.handle, dvk.handle, *[capi._nullable(x) for x in arrs], ops["n"],
                                       capi.HK_VERIFY_CHECK_POINTS, capi.ptr(rr), capi.ptr(out)), "hk_verify_batch")
    return out


def _run_cases(ctx, cname, cases):
    """every case in every mode it names; returns the failures as (case, mode, got, want) with long lists cut to where they
    differ"""
    cd = Codec(CURVES[cname])
    failed = []

    def compare(c, mode, got, want):
        got = [int(v) for v in got]
        if got != want:
            rows = [i for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]
            failed.append((c["name"], mode, [(i, got[i], want[i]) for i in rows]))

    by_key = {}
    for c in cases:
        by_key.setdefault(c["key"].name, []).append(c)
    for group in by_key.values():
        key = group[0]["key"]
        assert all(c["key"] is key for c in group)
        pvk = _prepare(ctx, key)                                        # one prepared key for all of its cases
        dvk = pvk.device
        for c in group:
            ops = ve.pack(c)
            assert (ops["x"] is None) == (key.nk == 0) and (ops["ds"] is None) == (key.nd == 1)
            args = (ops["a"], ops["b"], ops["c"], ops["ds"], ops["x"])
            compare(c, "proof", dvk.verify(*args, n=ops["n"], check_points=True), c["want"])
            if all(p.valid_points() for p in c["proofs"]):
                compare(c, "proof_unchecked", dvk.verify(*args, n=ops["n"], check_points=False), c["want"])
            if "batch" in c["modes"]:
                rand = c["rand"] if c["rand"] is not None else ve.seeded_rand(c)
                want = ve.batch_model(c, rand)
                assert c["contract"] or want == c["want"]
                rr = cd.fr_vec_mont(rand)
                if any(v % key.mod == 0 for v in rand):
                    compare(c, "batch", _verify_entry(dvk, ops, rr), want)
                else:
                    compare(c, "batch", dvk.verify(*args, n=ops["n"], check_points=True, rand=rr), want)
        pvk.free()
    return failed


@pytest.mark.parametrize("group", [1, 2, 3, 5, 6, 7, 8])
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_verdicts_of_forged_cases(cname, group, ctx_bn254, ctx_bls):
    """1 public inputs, 2 members at infinity, 3 commitment counts, 5 batch product bounds, 6 explicit batching scalars,
    7 a zero r_i, 8 small-order points inside proofs"""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    cases = [c for c in ve.cases(cname) if c["group"] == group]
    assert cases
    failed = _run_cases(ctx, cname, cases)
    assert not failed, "%d of %d cases: %r" % (len({f[0] for f in failed}), len(cases), failed)


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_split_launches_with_two_groups(cname, ctx_bn254, ctx_bls):
    """group 4: n = 1000 proofs of 17 members, count * S rows across the 65535-row launch bound, per-proof mode only.
    Measured on one MI355X, key preparation and both passes (checked and unchecked) included: 0.10 s on BN254, 0.14 s on
    BLS12-381 (the time is printed)."""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    cases = [c for c in ve.cases(cname) if c["group"] == 4]
    assert len(cases) == 1 and "batch" not in cases[0]["modes"]
    t0 = time.perf_counter()
    failed = _run_cases(ctx, cname, cases)
    print("split_nd15_n1000 %s: %.2f s" % (cname, time.perf_counter() - t0))
    assert not failed, failed


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_points_check_on_cofactor_points(cname, group, ctx_bn254, ctx_bls):
    """hk_points_check_g1 / _g2 against the oracle's on-curve and [r] P == O: U = [r] T, every V_l of small prime order l,
    -V_l, S + V_l, the order-3 points of BLS12-381 G1, beside subgroup points, infinity and raw curve points"""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    cd = Codec(CURVES[cname])
    pts = ve.check_points(cname, group)
    if (cname, group) == ("bn254", 1):
        assert ve.cofactor_points(cname, group) is None                  # cofactor 1: only the on-curve test is left
    want = [int(ve.in_subgroup(cname, group, P)) for _nm, P in pts]
    enc = cd.g1 if group == 1 else cd.g2
    got = ctx.points_check(group, np.frombuffer(b"".join(enc(P) for _nm, P in pts), np.uint8).copy())
    wrong = [(nm, int(g), w) for (nm, _P), g, w in zip(pts, got, want) if int(g) != w]
    assert not wrong, wrong


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_alpha_beta_of_a_forged_key(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    key = ve.case(cname, "nd3")["key"]
    T = pairing.tower(cname)
    pvk = _prepare(ctx, key)
    want = T.f12_flat(T.pairing(ve.point(cname, 1, key.alpha), ve.point(cname, 2, key.beta)))
    assert Enc(CURVES[cname]).f12_dec(pvk.alpha_beta_gt().tobytes()) == want
    pvk.free()
