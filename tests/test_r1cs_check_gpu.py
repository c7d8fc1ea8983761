"""GPU: hk_r1cs_check / hk_pk_r1cs_check (csrc/r1cs_check.cuh) against the host mirror cp_groth16.r1cs_bad_rows on both curves;
no expectation comes from the device.  Systems are tests/util.synthetic_r1cs; a row is made to fail by adding the term
(1, column 0) to its C row (r1cs_fixtures.with_failing_rows), or - where the matrices are shared by a batch - by shifting its
own witness and resolving the rows behind it again.

Shapes are the smallest that reach each boundary of the kernels:
  n_c 1, 63, 64, 65            one ballot word less one, exactly, plus one
  n_c 256, 257                 one workgroup of k_r1cs_rows exactly, plus one lane in a second
  n_c 1021                     the size test_witness_map_vs_oracle uses: 16 words, the last one partly filled
  failing rows 0, 63, 64, 256  first / last bit of a word, the only row of the last workgroup; cap 0, 1, 4, 300 (> n_c)
  batch 3                      another z row, another bitmap row and another output row per assignment
  n_c 32 833                   k_r1cs_compact walks its bitmap in tiles of 512 words = 32 768 rows: a second tile of two words,
                               failing rows on both sides of the tile edge (the ranks of the second tile start at the first
                               tile's count) and in the second tile alone (the first failing row is found there)
Each system is built once per session (functools.lru_cache) and never modified."""
import ctypes as C
import random
from functools import lru_cache

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import r1cs_bad_rows
from oracle.pyref import curve as ocurve, groth16
from oracle.pyref.codec import Codec
from oracle.pyref.params import CURVES
from tests.r1cs_fixtures import directed_system, resolve_from, with_failing_rows
from tests.util import csr_from_rows, pk_upload_from_oracle, running_bases, synthetic_r1cs

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "bls12_381"]
NONE = 0xFFFFFFFF
N_INST, N_FREE = 3, 6


def _ctx(curve, ctx_bn254, ctx_bls):
    return ctx_bn254 if curve == "bn254" else ctx_bls


@lru_cache(maxsize=None)
def _system(curve, n_c):
    """(A, B, C rows, z ints) of a satisfied synthetic system"""
    cp = CURVES[curve]
    cs = synthetic_r1cs(cp, random.Random(1000 + n_c), N_INST, N_FREE, n_c)
    A, B, Cm = cs.matrices()
    z = cs.full_assignment()
    assert r1cs_bad_rows(A, B, Cm, z, cp.r) == [] and z[0] == 1 and len(z) == N_INST + N_FREE + n_c
    return cs, A, B, Cm, z


def _csr3(cd, A, B, Cm):
    return csr_from_rows(cd, A), csr_from_rows(cd, B), csr_from_rows(cd, Cm)


def _sides(A, B, Cm, z, r, rows):
    ev = lambda lc: sum(c * z[j] for c, j in lc) % r
    return [x for i in rows for x in (ev(A[i]), ev(B[i]), ev(Cm[i]))]


def _expect(cd, A, B, Cm, zs, r, cap):
    """verdicts, bad_rows (batch, cap) and bad_vals (batch, cap, 96) as the header defines them, from the host mirror"""
    verdicts, rows, vals = [], np.full((len(zs), cap), NONE, np.uint32), np.zeros((len(zs), cap, 96), np.uint8)
    for b, z in enumerate(zs):
        bad = r1cs_bad_rows(A, B, Cm, z, r)
        verdicts.append((len(bad), bad[0] if bad else None))
        k = min(len(bad), cap)
        rows[b, :k] = bad[:k]
        if k:
            vals[b, :k] = np.asarray(cd.fr_vec_mont(_sides(A, B, Cm, z, r, bad[:k])), np.uint8).reshape(k, 96)
    return verdicts, rows, vals


def _check(ctx, cd, A, B, Cm, zs, r, cap, z_dev=False, pk=None):
    """one call over the assignments zs against the mirror; returns the raw outputs"""
    want_v, want_rows, want_vals = _expect(cd, A, B, Cm, zs, r, cap)
    zb = np.asarray(cd.fr_vec_mont([x for z in zs for x in z]), np.uint8)
    zarg = capi.DeviceBuffer.from_host(ctx, zb) if z_dev else zb
    try:
        if pk is not None:
            got = pk.r1cs_check(zarg, batch=len(zs), cap=cap, want_vals=True)
        else:
            got = ctx.r1cs_check(*_csr3(cd, A, B, Cm), zarg, batch=len(zs), cap=cap, want_vals=True)
    finally:
        if z_dev:
            zarg.free()
    if cap == 0:
        assert got == want_v
        return got
    verdicts, rows, vals = got
    assert verdicts == want_v
    assert rows.shape == want_rows.shape and (rows == want_rows).all(), (rows, want_rows)
    assert vals.shape == want_vals.shape and (vals == want_vals).all()
    return got


# ---- 1. row-count boundaries -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("n_c", [1, 63, 64, 65, 256, 257, 1021])
def test_satisfied_at_every_row_count_boundary(curve, n_c, ctx_bn254, ctx_bls):
    cp, cd = CURVES[curve], Codec(CURVES[curve])
    _cs, A, B, Cm, z = _system(curve, n_c)
    verdicts, rows, vals = _check(_ctx(curve, ctx_bn254, ctx_bls), cd, A, B, Cm, [z], cp.r, 4)
    assert verdicts == [(0, None)] and (rows == NONE).all() and not vals.any()
    # and the last row alone: the top bit that is in use, nothing behind it
    _check(_ctx(curve, ctx_bn254, ctx_bls), cd, A, B, with_failing_rows(Cm, [n_c - 1]), [z], cp.r, 4)


# ---- 2. failing-row positions, truncation and padding ---------------------------------------------------------------------
FAILING = [(0,), (63,), (64,), (256,), (0, 63, 64, 255, 256), tuple(range(257))]


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("failing", FAILING, ids=lambda f: "rows%d_%d" % (len(f), f[0] if len(f) == 1 else len(f)))
def test_failing_rows_caps_and_values(curve, failing, ctx_bn254, ctx_bls):
    cp, cd = CURVES[curve], Codec(CURVES[curve])
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    _cs, A, B, Cm, z = _system(curve, 257)
    Cf = with_failing_rows(Cm, failing)
    assert r1cs_bad_rows(A, B, Cf, z, cp.r) == list(failing)       # exactly those rows, on the host
    for cap in (0, 1, 4, 300):
        got = _check(ctx, cd, A, B, Cf, [z], cp.r, cap)
        if cap:
            k = min(cap, len(failing))
            assert got[0] == [(len(failing), failing[0])] and got[1][0, :k].tolist() == list(failing[:k])
            assert (got[1][0, k:] == NONE).all() and not got[2][0, k:].any()
    # verdicts only, the other way to ask for it: a cap without bad_rows is spelled cap=0 by the wrapper; want_vals=False
    assert ctx.r1cs_check(*_csr3(cd, A, B, Cf), np.asarray(cd.fr_vec_mont(z), np.uint8)) == [(len(failing), failing[0])]


# ---- 2b. a bitmap of more than one compaction tile -------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _two_tile_system(curve, n_c=32768 + 65):
    """n_c rows c_i z_j * 1 = w_i over 8 free values: what the compaction walks is the bitmap, so the rows are the cheapest
    that give one (synthetic_r1cs takes 1.5 s at this size)"""
    r = CURVES[curve].r
    rnd = random.Random(n_c)
    z = [1] + [rnd.randrange(r) for _ in range(8)]
    A, B, Cm = [], [], []
    for i in range(n_c):
        c, j = rnd.choice((1, 2, r - 1, 1 << 31)), rnd.randrange(9)
        A.append([(c, j)]); B.append([(1, 0)]); Cm.append([(1, 9 + i)])
        z.append(c * z[j] % r)
    return A, B, Cm, z


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_second_compaction_tile(curve, ctx_bn254, ctx_bls):
    cp, cd = CURVES[curve], Codec(CURVES[curve])
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    A, B, Cm, z = _two_tile_system(curve)
    ma, mb = csr_from_rows(cd, A), csr_from_rows(cd, B)
    zb = np.asarray(cd.fr_vec_mont(z), np.uint8)
    for failing in ((0, 32767, 32768, 32831, 32832), (32768, 32832)):
        Cf = with_failing_rows(Cm, failing)
        assert r1cs_bad_rows(A, B, Cf, z, cp.r) == list(failing)
        verdicts, rows = ctx.r1cs_check(ma, mb, csr_from_rows(cd, Cf), zb, cap=8)
        assert verdicts == [(len(failing), failing[0])]
        assert rows[0].tolist() == list(failing) + [NONE] * (8 - len(failing))


# ---- 3. a batch of three in one call ---------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _batch3(curve):
    """three assignments of one 201-row system: satisfied / row 5 fails / rows 5 and 200 fail.  Rows 1 and 2 differ from row 0
    in their free witnesses too, so every row's sides differ between the three."""
    cp = CURVES[curve]
    cs, A, B, Cm, z0 = _system(curve, 201)
    r, rnd = cp.r, random.Random(7)
    zs = [z0]
    for failing in ((5,), (5, 200)):
        z = list(z0)
        for j in range(N_INST, N_INST + N_FREE):
            z[j] = rnd.randrange(r)
        z = resolve_from(A, B, Cm, z, r)
        for i in failing:
            z[Cm[i][0][1]] = (z[Cm[i][0][1]] + 1) % r              # row i's own witness, then every row behind it again
            z = resolve_from(A, B, Cm, z, r, first=i + 1)
        assert r1cs_bad_rows(A, B, Cm, z, r) == list(failing)
        zs.append(z)
    assert all(zs[1][j] != zs[0][j] and zs[2][j] != zs[1][j] for j in range(N_INST, N_INST + N_FREE))
    return cs, A, B, Cm, zs


def _placeholder_key(cp, cs):
    """An oracle ProvingKey of the right lengths for `cs` whose queries are running multiples of the generators: the check
    reads a key's matrices and n_v, never its points, and a trusted setup of 201 rows in Python takes 6 - 8 s."""
    G1, G2 = ocurve.G1(cp), ocurve.G2(cp)
    n_v, n_c = len(cs.full_assignment()), cs.num_constraints
    m = 1
    while m < n_c + cs.num_instance:
        m *= 2
    p1 = running_bases(G1, max(n_v, m))
    p2 = running_bases(G2, n_v)
    vk = groth16.VerifyingKey(alpha_g=p1[1], beta_h=p2[1], gamma_h=p2[2], last_delta_h=p2[3], gamma_abc_g=p1[:cs.num_instance],
                              deltas_h=[p2[3]] * len(cs.stage_ranges))
    return groth16.ProvingKey(vk=vk, beta_g=p1[2], a_g=p1[:n_v], b_g=p1[:n_v], b_h=p2[:n_v], h_g=p1[:m - 1],
                              ck=groth16.CommitterKey(last_delta_g=p1[3], deltas_abc_g=[p1[:e - s] for s, e in cs.stage_ranges]),
                              deltas_g=[p1[3]] * len(cs.stage_ranges))


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_batch_of_three_host_device_and_key(curve, ctx_bn254, ctx_bls):
    cp, cd = CURVES[curve], Codec(CURVES[curve])
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    cs, A, B, Cm, zs = _batch3(curve)
    host = _check(ctx, cd, A, B, Cm, zs, cp.r, 4)
    assert host[0] == [(0, None), (1, 5), (2, 5)] and host[1].tolist() == [[NONE] * 4, [5] + [NONE] * 3, [5, 200, NONE, NONE]]
    dev = _check(ctx, cd, A, B, Cm, zs, cp.r, 4, z_dev=True)
    dpk = pk_upload_from_oracle(ctx, cd, _placeholder_key(cp, cs), cs)
    try:
        key_h = _check(ctx, cd, A, B, Cm, zs, cp.r, 4, pk=dpk)
        key_d = _check(ctx, cd, A, B, Cm, zs, cp.r, 4, z_dev=True, pk=dpk)
        one = _check(ctx, cd, A, B, Cm, zs[2:], cp.r, 1, pk=dpk)   # a batch of one of the key form, truncated
    finally:
        dpk.free()
    for other in (dev, key_h, key_d):
        assert other[0] == host[0] and (other[1] == host[1]).all() and (other[2] == host[2]).all()
    assert one[0] == [(2, 5)] and one[1].tolist() == [[5]]


# ---- 4. directed rows for the comparison itself ----------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_directed_rows(curve, ctx_bn254, ctx_bls):
    cp, cd = CURVES[curve], Codec(CURVES[curve])
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    A, B, Cm, z, bad, sides = directed_system(cp.r)
    n_c = len(A)
    verdicts, rows, vals = _check(ctx, cd, A, B, Cm, [z], cp.r, n_c)
    assert verdicts == [(2, 5)] and rows[0, :2].tolist() == bad == [5, 7]
    assert cd.fr_vec_from_mont(vals[0, 0].tobytes()) == [0, 0, 1]
    assert cd.fr_vec_from_mont(vals[0, 1].tobytes()) == list(sides[7])
    # every row listed - each C row shifted by one once more, so 5 and 7 fail by two - gives every row's three sides: the
    # wrapped zero of row 0 comes back as the bytes of zero, the wrapped sum of row 1 as 35
    Call = [row + [(1, 0)] for row in Cm]
    verdicts, rows, vals = _check(ctx, cd, A, B, Call, [z], cp.r, n_c)
    assert verdicts == [(n_c, 0)] and rows[0].tolist() == list(range(n_c))
    got = [tuple(cd.fr_vec_from_mont(vals[0, i].tobytes())) for i in range(n_c)]
    assert got == [(sides[i][0], sides[i][1], (sides[i][2] + 1) % cp.r) for i in range(n_c)]
    assert not vals[0, 0, :32].any() and got[1][2] == 36


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ctx_bn254):
    ctx, curve = ctx_bn254, "bn254"
    cp, cd = CURVES[curve], Codec(CURVES[curve])
    cs, A, B, Cm, zs = _batch3(curve)
    n_v, fr, cap = len(zs[0]), ctx.fr_bytes, 4
    zb = np.asarray(cd.fr_vec_mont([x for z in zs for x in z]), np.uint8)
    pre = [np.full(2 * 3, 0x5a5a5a5a, np.uint32), np.full(3 * cap, 0x6b6b6b6b, np.uint32), np.full(3 * cap * 3 * fr, 0x7c, np.uint8)]
    outs = [x.copy() for x in pre]
    keep = []
    full = ctx._csrs(_csr3(cd, A, B, Cm), keep)
    short = ctx._csrs(_csr3(cd, A, B, Cm[:-1]), keep)
    wide = [row + [(1, n_v)] if i == 77 else row for i, row in enumerate(B)]      # one column == n_v
    badcol = ctx._csrs(_csr3(cd, A, wide, Cm), keep)

    def csr_call(ms, z=zb, n_v_=n_v, batch=3, verdicts=outs[0], rows=outs[1], vals=outs[2], cap_=cap):
        p = lambda x: None if x is None else x.ctypes.data
        return ctx.lib.hk_r1cs_check(ctx.handle, C.byref(ms[0]), C.byref(ms[1]), C.byref(ms[2]), p(z), n_v_, batch, p(verdicts), p(rows),
                                     p(vals), cap_)

    def pk_call(pk, n_v_=n_v, batch=3):
        return ctx.lib.hk_pk_r1cs_check(ctx.handle, pk.handle, zb.ctypes.data, n_v_, batch, outs[0].ctypes.data, outs[1].ctypes.data,
                                        outs[2].ctypes.data, cap)

    refused = {
        "unequal n_rows": csr_call([full[0], full[1], short[2]]),
        "unequal n_rows (A)": csr_call([short[2], full[1], full[2]]),
        "a column == n_v": csr_call(badcol),
        "n_v one short of a column": csr_call(full, n_v_=n_v - 1, batch=1),
        "bad_vals without bad_rows": csr_call(full, rows=None),
        "NULL z": csr_call(full, z=None),
        "NULL verdicts": csr_call(full, verdicts=None),
        "n_v 2^32": csr_call(full, n_v_=1 << 32),
    }
    assert refused == {name: capi.HK_ERR_ARG for name in refused}
    assert ctx.lib.hk_r1cs_check(ctx.handle, None, C.byref(full[1]), C.byref(full[2]), zb.ctypes.data, n_v, 3, outs[0].ctypes.data,
                                 None, None, 0) == capi.HK_ERR_ARG
    assert ctx.lib.hk_r1cs_check(None, C.byref(full[0]), C.byref(full[1]), C.byref(full[2]), zb.ctypes.data, n_v, 3,
                                 outs[0].ctypes.data, None, None, 0) == capi.HK_ERR_ARG
    key = _placeholder_key(cp, cs)
    with_m = pk_upload_from_oracle(ctx, cd, key, cs)
    bare = ctx.pk_upload(a_g=cd.g1_vec(key.a_g), b_g=cd.g1_vec(key.b_g), b_h=cd.g2_vec(key.b_h), h_g=cd.g1_vec(key.h_g),
                         ck_stages=[cd.g1_vec(v) for v in key.ck.deltas_abc_g], deltas_g=cd.g1_vec(key.deltas_g),
                         last_delta_h=cd.g2_vec([key.last_delta_h()]), alpha_g=cd.g1_vec([key.vk.alpha_g]),
                         beta_g=cd.g1_vec([key.beta_g]), beta_h=cd.g2_vec([key.vk.beta_h]), n_inst=cs.num_instance,
                         n_constraints=cs.num_constraints)
    try:
        assert pk_call(bare) == capi.HK_ERR_ARG                    # a key without matrices
        # the wrong n_v for a key: the status hk_prove gives for the same mistake
        one, g1, g2 = np.asarray(cd.fr_vec_mont([1]), np.uint8), np.zeros(ctx.g1_bytes, np.uint8), np.zeros(ctx.g2_bytes, np.uint8)
        prove_status = ctx.lib.hk_prove(ctx.handle, with_m.handle, zb.ctypes.data, n_v + 1, one.ctypes.data, one.ctypes.data, None, 0,
                                        g1.ctypes.data, g2.ctypes.data, g1.copy().ctypes.data)
        assert prove_status == capi.HK_ERR_LEN and pk_call(with_m, n_v_=n_v + 1, batch=1) == prove_status
        assert ctx.lib.hk_pk_r1cs_check(ctx.handle, None, zb.ctypes.data, n_v, 3, outs[0].ctypes.data, None, None, 0) == capi.HK_ERR_ARG
        # nothing to do is not a refusal, and touches nothing either
        assert csr_call(full, batch=0) == capi.HK_OK and pk_call(with_m, batch=0) == capi.HK_OK
        assert csr_call(full, batch=0, z=None, verdicts=None, rows=None, vals=None) == capi.HK_OK
        for got, want in zip(outs, pre):
            assert (got == want).all()
        # the same context and key still work: the valid call fills every byte of all three
        assert pk_call(with_m) == capi.HK_OK
        want_v, want_rows, want_vals = _expect(cd, A, B, Cm, zs, cp.r, cap)
        assert outs[0].reshape(3, 2).tolist() == [[n, NONE if f is None else f] for n, f in want_v]
        assert (outs[1].reshape(3, cap) == want_rows).all() and (outs[2].reshape(3, cap, 96) == want_vals).all()
        for x, v in zip(outs, pre):
            x[:] = v
        assert csr_call(full) == capi.HK_OK
        assert (outs[1].reshape(3, cap) == want_rows).all() and (outs[2].reshape(3, cap, 96) == want_vals).all()
    finally:
        with_m.free()
        bare.free()


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_three_runs_are_byte_identical(curve, ctx_bn254, ctx_bls):
    cp, cd = CURVES[curve], Codec(CURVES[curve])
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    _cs, A, B, Cm, z = _system(curve, 257)
    Cf = with_failing_rows(Cm, (0, 63, 64, 255, 256))
    ms = _csr3(cd, A, B, Cf)
    zb = np.asarray(cd.fr_vec_mont(z), np.uint8)
    runs = []
    for _ in range(3):
        verdicts, rows, vals = ctx.r1cs_check(*ms, zb, cap=8, want_vals=True)
        runs.append((repr(verdicts).encode(), rows.tobytes(), vals.tobytes()))
    assert runs[0] == runs[1] == runs[2]
    assert runs[0][1] == np.array([0, 63, 64, 255, 256, NONE, NONE, NONE], np.uint32).tobytes()
