"""GPU: where an entry's operands live does not change what it computes - the entries outside the jobs, which stage their
host-or-device operands through csrc/hk_internal.h `Staged` like the job entries of test_job_residency_gpu: the MSMs, the
fixed-base and element-wise sweeps, the folds, the GT powers, hk_points_check_*, hk_vk_prepare, hk_verify_batch,
hk_witness_map, hk_assignment_from_bits, hk_scalar_powers and hk_ipa_quotient.  Every one runs with all inputs on the host,
all on the device and alternating, and every host-or-device output both as a host array and as a prefilled (0xA5) device
buffer: all the results are byte-identical and not the prefill.  What the bytes ARE is the business of the entries' own test
files (test_sweep_entries_gpu, test_msm_edges_gpu, test_edge_gpu, test_verify_gpu, test_pairing_edges_gpu, test_agg_scalars).

BN254.  Points are made on the device, by hk_fixed_base from random scalars under a fixed seed.  Shapes: one element and 65
(one wave plus a lane); the MSMs at n = 3 and at the first n past the short path; hk_msm_bases with one scalar fewer than
bases (the zero tail) over a set with tables and a short one without; hk_verify_batch at one proof and at VERIFY_CHUNK + 1,
where the second chunk reads every operand at an offset and holds the one tampered proof.  Where a wrapper of capi takes host
arrays only, the C entry is called."""
import ctypes as C
import random

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.endo import phi2, psi4
from oracle.pyref import curve
from oracle.pyref.codec import Codec
from oracle.pyref.params import BN254
from tests import golden_util as gu
from tests.residency import PATTERN, PLACEMENTS, _Placed, _filled, _prefilled, _same_everywhere
from tests.util import csr_from_rows, synthetic_r1cs

pytestmark = pytest.mark.gpu
CNAME = "bn254"
R = CURVE_PARAMS[CNAME]["r"]
SPLIT_MAX_LANES, SPLIT_K = 65536, {1: 2, 2: 4}            # csrc/endo.cuh: SPLIT_MAX_LANES, EndoOf<F>::K
VERIFY_CHUNK = 1024                                       # csrc/verify.cuh
GROUPS = [1, 2]
_p = capi.ptr
_CACHE = {}


def _call(ctx, name, *args):
    capi.check(getattr(ctx.lib, name)(ctx.handle, *args), name)


def _scalars(n, tag):
    rnd = random.Random("entry_residency/%s/%d" % (tag, n))
    return FrCodec(CNAME).enc([rnd.randrange(R) for _ in range(n)])


def _generator(group):
    cd = Codec(BN254)
    gen = cd.g1(curve.G1(BN254).gen) if group == 1 else cd.g2(curve.G2(BN254).gen)
    return np.frombuffer(bytes(gen), np.uint8).copy()


def _points(ctx, group, n, tag=0):
    """n points of the group, host bytes; made once per (group, n, tag) and never written to"""
    key = ("points", group, n, tag)
    if key not in _CACHE:
        _CACHE[key] = ctx.fixed_base(group, _generator(group), _scalars(n, "points/%d/%d" % (group, tag)))
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def _gts(ctx, n):
    """n elements of GT: powers of one pairing value"""
    key = ("gts", n)
    if key not in _CACHE:
        g = ctx.multi_pairing(_points(ctx, 1, 1), _points(ctx, 2, 1))
        _CACHE[key] = ctx.gt_pow(np.tile(g, n), _scalars(n, "gts")).reshape(-1)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def _pb(ctx, group):
    return ctx.g1_bytes if group == 1 else ctx.g2_bytes


def _both_outputs(ctx, nbytes, run):
    """run(put, out) fills `out`: a host array, then a prefilled device buffer, each under every placement of the inputs"""
    def host(put):
        out = np.full(nbytes, PATTERN, np.uint8)
        run(put, out)
        return out

    def device(put):
        return _filled(ctx, nbytes, lambda z: run(put, z))[:nbytes]
    got = _same_everywhere(ctx, host)
    assert (_same_everywhere(ctx, device) == got).all()
    return got


# ---- the element-wise sweeps -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("group", GROUPS)
def test_scalar_pairing(group, n, ctx_bn254):
    ctx = ctx_bn254
    pts, sc = _points(ctx, group, n), _scalars(n, "scalar_pairing")
    _both_outputs(ctx, n * _pb(ctx, group), lambda put, out: ctx.scalar_pairing(group, put(pts), put(sc), n=n, out=out))


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("group", GROUPS)
def test_fixed_base(group, n, ctx_bn254):
    ctx = ctx_bn254
    base, sc = _points(ctx, group, 1, tag=1), _scalars(n, "fixed_base")
    _both_outputs(ctx, n * _pb(ctx, group), lambda put, out: ctx.fixed_base(group, put(base), put(sc), n=n, out=out))


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("group", GROUPS)
def test_points_check(group, n, ctx_bn254):
    ctx = ctx_bn254
    pts = _points(ctx, group, n).copy()
    pts[-_pb(ctx, group) // 2] ^= 1                                 # the last point's y: it leaves its curve
    got = _both_outputs(ctx, n, lambda put, out: _call(ctx, "hk_points_check_g%d" % group, _p(put(pts)), n, _p(out)))
    assert got.tolist() == [1] * (n - 1) + [0]


@pytest.mark.parametrize("n", [1, 65])
def test_gt_pow(n, ctx_bn254):
    ctx = ctx_bn254
    gts, sc = _gts(ctx, n), _scalars(n, "gt_pow")
    _both_outputs(ctx, n * ctx.gt_bytes, lambda put, out: _call(ctx, "hk_gt_pow", _p(put(gts)), _p(put(sc)), n, _p(out)))


def test_gt_pow_prod(ctx_bn254):
    ctx, n, group_len = ctx_bn254, 6, 3
    gts, sc = _gts(ctx, n), _scalars(n, "gt_pow_prod")
    _both_outputs(ctx, n // group_len * ctx.gt_bytes,
                  lambda put, out: _call(ctx, "hk_gt_pow_prod", _p(put(gts)), _p(put(sc)), n, group_len, 1, _p(out)))


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("group", GROUPS)
def test_points_lincomb(group, k, ctx_bn254):
    ctx, n = ctx_bn254, 65
    vecs, coeffs = [_points(ctx, group, n, tag=j) for j in range(k)], _scalars(k, "lincomb")

    def run(put, out):
        vs = [put(v) for v in vecs]
        _call(ctx, "hk_points_lincomb_g%d" % group, capi._ptr_array(vs), _p(put(coeffs)), k, n, _p(out))
    _both_outputs(ctx, n * _pb(ctx, group), run)


def _fold_scalar(group):
    """a challenge split along the group's endomorphism: the magnitudes' Montgomery bytes and the sign mask"""
    c = random.Random("entry_residency/fold/%d" % group).randrange(R)
    parts = (phi2 if group == 1 else psi4)(CNAME).decompose(c)
    assert len(parts) == SPLIT_K[group]
    return FrCodec(CNAME).enc([abs(v) for v in parts]), sum(1 << j for j, v in enumerate(parts) if v < 0)


def _fold_many(ctx, group, put, los, his, outs, n):
    """the magnitudes are the call's last input: on the host under "host", resident under "device" """
    mags, neg = _fold_scalar(group)
    lo, hi = [put(v) for v in los], [put(v) for v in his]
    _call(ctx, "hk_points_fold_many_g%d" % group, len(outs), capi._ptr_array(lo), capi._ptr_array(hi), _p(put(mags)), neg, n,
          capi._ptr_array(outs))


# k = 1 into a device buffer (normalised in place), k = 1 into a host array, k = 3 with the outputs mixed
@pytest.mark.parametrize("kinds", [(True,), (False,), (True, False, True)], ids=["k1_device", "k1_host", "k3_mixed"])
@pytest.mark.parametrize("group", GROUPS)
def test_points_fold_many(group, kinds, ctx_bn254):
    ctx, n, k = ctx_bn254, 65, len(kinds)
    nb = n * _pb(ctx, group)
    los, his = ([_points(ctx, group, n, tag=t + 2 * y) for y in range(k)] for t in (10, 11))

    def run(put):
        outs = [_prefilled(ctx, nb) if dev else np.full(nb, PATTERN, np.uint8) for dev in kinds]
        try:
            _fold_many(ctx, group, put, los, his, outs, n)
            got = [x.to_host()[:nb] if dev else x for x, dev in zip(outs, kinds)]
            assert not any((g == PATTERN).all() for g in got)
            return np.concatenate(got)
        finally:
            for x, dev in zip(outs, kinds):
                if dev:
                    x.free()
    got = _same_everywhere(ctx, run)
    if k == 1:                                                      # the in-place form and the handed-out one agree
        key = ("fold", group)
        assert (_CACHE.setdefault(key, got) == got).all()


# ---- the MSMs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,n", [(g, n) for g in GROUPS for n in (3, SPLIT_MAX_LANES // SPLIT_K[g] + 1)])
def test_msm(group, n, ctx_bn254):
    ctx = ctx_bn254
    assert (n - 1) * SPLIT_K[group] <= SPLIT_MAX_LANES < n * SPLIT_K[group] or n == 3
    bases, sc = _points(ctx, group, n), _scalars(n, "msm")
    msm = ctx.msm_g1 if group == 1 else ctx.msm_g2
    _same_everywhere(ctx, lambda put: msm(put(bases), put(sc), n_bases=n, n_scalars=n))


# a G1 set long enough for shift tables (the bucket pass over n_bases scalars) and a short G2 set without them
@pytest.mark.parametrize("group,n", [(1, 8193), (2, 5)])
def test_msm_bases_zero_tail(group, n, ctx_bn254):
    ctx = ctx_bn254
    sc = _scalars(n - 1, "msm_bases")
    rb = ctx.bases_upload(group, _points(ctx, group, n))
    try:
        _both_outputs(ctx, _pb(ctx, group), lambda put, out: capi.check(ctx.lib.hk_msm_bases(
            ctx.handle, rb.handle, _p(put(sc)), n - 1, 1, 0, _p(out)), "hk_msm_bases"))
    finally:
        rb.free()


# ---- assignments and the witness map ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_full", [0, 2])
def test_assignment_from_bits(n_full, ctx_bn254):
    ctx, n_v = ctx_bn254, 65
    rnd = random.Random("entry_residency/bits")
    bits = np.array([rnd.randrange(2) for _ in range(n_v)], np.uint8)
    cols, vals = np.array([64, 3], np.uint32)[:n_full], _scalars(n_full, "bits")

    def run(put):
        b, c, v = (put(bits), put(cols), put(vals)) if n_full else (put(bits), None, None)
        return _filled(ctx, n_v * ctx.fr_bytes, lambda z: _call(ctx, "hk_assignment_from_bits", _p(b), n_v, _p(c), _p(v), n_full,
                                                                z.ptr))[:n_v * ctx.fr_bytes]
    got = _same_everywhere(ctx, run).reshape(n_v, ctx.fr_bytes)
    for j in range(n_full):
        assert (got[cols[j]] == vals.reshape(n_full, -1)[j]).all()


def test_witness_map(ctx_bn254):
    """the R1CS of test_edge_gpu._tiny_key"""
    ctx, cd = ctx_bn254, Codec(BN254)
    cs = synthetic_r1cs(BN254, random.Random(5), n_inst=2, n_free=6, n_c=12, two_stage_split=2)
    A, B, C = (csr_from_rows(cd, M) for M in cs.matrices())
    z = np.frombuffer(bytes(cd.fr_vec_mont(cs.full_assignment())), np.uint8).copy()
    n_v = len(cs.full_assignment())
    _same_everywhere(ctx, lambda put: ctx.witness_map(A, B, C, cs.num_instance, cs.num_constraints, put(z), n_v=n_v)[0])


# ---- the aggregator's scalars: no host-or-device input, one such output ---------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
def test_scalar_powers(n, ctx_bn254):
    ctx, reps = ctx_bn254, 2
    x = random.Random("entry_residency/powers").randrange(2, R)
    _both_outputs(ctx, reps * n * ctx.fr_bytes, lambda put, out: ctx.scalar_powers(x, n, reps=reps, out=out))


@pytest.mark.parametrize("l,shift", [(1, 0), (3, 5)])
def test_ipa_quotient(l, shift, ctx_bn254):
    ctx = ctx_bn254
    rnd = random.Random("entry_residency/quotient")
    ch, rho, z = [rnd.randrange(1, R) for _ in range(l)], rnd.randrange(1, R), rnd.randrange(1, R)
    _both_outputs(ctx, (shift + (1 << l)) * ctx.fr_bytes, lambda put, out: ctx.ipa_quotient(ch, rho, z, shift=shift, out=out))


# ---- the verifier -------------------------------------------------------------------------------------------------------------
def _golden_case():
    """the first BN254 case of tests/golden/groth16.json (test_verify_gpu): two deltas and two public inputs, so that every
    operand of hk_verify_batch is present"""
    case = gu.load("groth16.json")[CNAME][0]
    pk, proof = case["pk"], case["proof"]
    key = {k: gu.hb(pk[k]) for k in ("alpha_g", "beta_h", "gamma_h", "deltas_h", "gamma_abc_g")}
    a, b, c = gu.hb(proof["a"]), gu.hb(proof["b"]), gu.hb(proof["c"])
    ds = np.concatenate([gu.hb(d) for d in case["comms"]])
    x = np.frombuffer(bytes(FrCodec(CNAME).enc(list(case["public_inputs"]))), np.uint8).copy()
    return key, (a, b, c, ds, x)


def _vk_prepare(ctx, key, put):
    alpha, beta = put(key["alpha_g"]), put(key["beta_h"])
    addr = capi._nullable
    d = capi.hk_vk_desc(addr(alpha), addr(beta), addr(key["gamma_h"]), addr(key["deltas_h"]), len(key["deltas_h"]) // ctx.g2_bytes,
                        addr(key["gamma_abc_g"]), len(key["gamma_abc_g"]) // ctx.g1_bytes)
    h = C.c_void_p()
    _call(ctx, "hk_vk_prepare", C.byref(d), C.byref(h))
    return capi.DeviceVk(ctx, h, d.n_deltas, d.n_abc)


def test_vk_prepare(ctx_bn254):
    ctx = ctx_bn254
    key, _proof = _golden_case()

    def run(put):
        dvk = _vk_prepare(ctx, key, put)
        try:
            return dvk.alpha_beta()
        finally:
            dvk.free()
    _same_everywhere(ctx, run)


@pytest.mark.parametrize("with_rand", [False, True], ids=["per_proof", "rand"])
@pytest.mark.parametrize("n", [1, VERIFY_CHUNK + 1])
def test_verify_batch(n, with_rand, ctx_bn254):
    ctx = ctx_bn254
    key, (a, b, c, ds, x) = _golden_case()
    a, b, c, ds, x = (np.tile(t, n) for t in (a, b, c, ds, x))
    want = [1] * n
    if n > 1:                                                       # the last proof, alone in the second chunk: C := A
        c[-ctx.g1_bytes:] = a[-ctx.g1_bytes:]
        want[-1] = 0
    rand = FrCodec(CNAME).enc([random.Random(7 + i).getrandbits(128) | 1 for i in range(n)]) if with_rand else None
    dvk = _vk_prepare(ctx, key, lambda t: t)
    try:
        def run(put, out):
            ops = [put(t) for t in (a, b, c, ds, x)] + [put(rand) if with_rand else None]
            _call(ctx, "hk_verify_batch", dvk.handle, *[_p(t) for t in ops[:5]], n, capi.HK_VERIFY_CHECK_POINTS, _p(ops[5]), _p(out))
        assert _both_outputs(ctx, n, run).tolist() == want
    finally:
        dvk.free()


# ---- a lane's scratch shrinks with resident operands and grows again ----------------------------------------------------------------
def test_fold_then_pair_on_one_context(ctx_bn254):
    """hk_points_fold_many then hk_pairing_pairs on a context of their own, resident operands first: that fold carves no
    input slices, so the lane's arena is at its smallest when the pairing, and then the host form of the fold, ask for more"""
    n = 65
    g1, lo, hi = _points(ctx_bn254, 1, n), _points(ctx_bn254, 2, n, tag=10), _points(ctx_bn254, 2, n, tag=11)
    with capi.Context(CNAME, 0) as ctx:
        nb = n * ctx.g2_bytes
        got = {}
        for name in ("device", "host", "alternating", "device"):
            assert name in PLACEMENTS
            put = _Placed(ctx, name)
            out = _prefilled(ctx, nb) if name == "device" else np.full(nb, PATTERN, np.uint8)
            try:
                _fold_many(ctx, 2, put, [lo], [hi], [out], n)
                gt = ctx.pairing_pairs([put(g1)], [out], [(0, 0)], n=n).reshape(-1)
            finally:
                put.free()
                if name == "device":
                    out.free()
            assert gt.any() and (got.setdefault("first", gt) == gt).all(), name
