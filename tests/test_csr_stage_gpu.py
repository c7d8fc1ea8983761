"""GPU: every entry that stages the three matrices of an R1CS (csrc/csr.cuh: csr_host_ok, R1csStage, r1cs_validate) refuses the
same malformed matrices the same way, writes nothing when it does, and goes on working; device-resident and mixed matrix
arrays give the bytes of the all-host call.  The entries are hk_witness_map, hk_qap_eval, hk_keygen, hk_r1cs_check and
hk_pk_upload, on both curves.

The system is test_edge_gpu's _tiny_key shape (n_inst 2, 12 constraints, 20 variables, two stages).  No expectation comes from
the device: the oracle's witness map, its trapdoor's QAP evaluations at t and its proving key, and the host mirror
cp_groth16.r1cs_bad_rows.  Each system is built once per session and never modified."""
import ctypes as C
import random
from functools import lru_cache

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import r1cs_bad_rows
from oracle.pyref import groth16
from oracle.pyref.codec import Codec
from oracle.pyref.params import CURVES
from tests.util import csr_from_rows, synthetic_r1cs

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "bls12_381"]
TRAPDOOR = dict(alpha=3, beta=5, gamma=7, deltas=[11, 13], t=17, g1_scalar=2, g2_scalar=3)
SENTINEL = 0x5A
CAP = 4


def _ctx(curve, ctx_bn254, ctx_bls):
    return ctx_bn254 if curve == "bn254" else ctx_bls


@lru_cache(maxsize=None)
def _system(curve):
    cp = CURVES[curve]
    cs = synthetic_r1cs(cp, random.Random(5), n_inst=2, n_free=6, n_c=12, two_stage_split=2)
    td = TRAPDOOR
    pk, trap = groth16.generate_parameters(cp, cs, td["alpha"], td["beta"], td["gamma"], td["deltas"], td["t"], td["g1_scalar"],
                                           td["g2_scalar"])
    A, B, Cm = cs.matrices()
    z = cs.full_assignment()
    z_bad = list(z)
    z_bad[-1] = (z_bad[-1] + 1) % cp.r                              # the last row's own witness: that row alone fails
    assert r1cs_bad_rows(A, B, Cm, z, cp.r) == [] and r1cs_bad_rows(A, B, Cm, z_bad, cp.r) == [len(A) - 1]
    return cp, cs, pk, trap, (A, B, Cm), [z, z_bad]


def _malformed(ms, n_v):
    """the four defects, one matrix each; every other array is the sound one"""
    A, B, Cm = ms
    col = A[1].copy(); col[0] = n_v                                  # a column one past the assignment, in A
    rp_b = B[0].copy(); rp_b[1], rp_b[2] = rp_b[2] + 1, rp_b[1]      # not monotone, in B
    rp_c = Cm[0].copy(); rp_c[-1] += 1                               # ends at nnz + 1, in C
    rp_a = A[0].copy(); rp_a[0] = 1                                  # does not start at 0
    return {"column == n_v in A": ((A[0], col, A[2]), B, Cm), "row_ptr not monotone in B": (A, (rp_b, B[1], B[2]), Cm),
            "row_ptr ends at nnz + 1 in C": (A, B, (rp_c, Cm[1], Cm[2])), "row_ptr[0] == 1": ((rp_a, A[1], A[2]), B, Cm)}


class _Entries:
    """The four entries with output buffers, called through the raw C ABI on sentinel-filled buffers.  Each returns
    (status, {name: buffer})."""

    def __init__(self, ctx, curve):
        cp, cs, pk, trap, rows, zs = _system(curve)
        self.ctx, self.cd, self.fr = ctx, Codec(cp), ctx.fr_bytes
        self.n_inst, self.n_c, self.n_v = cs.num_instance, cs.num_constraints, len(zs[0])
        self.m = 1
        while self.m < self.n_c + self.n_inst:
            self.m *= 2
        self.stage_ranges = [tuple(x) for x in cs.stage_ranges]
        self.z = np.asarray(self.cd.fr_vec_mont(zs[0]), np.uint8)
        self.zs = np.asarray(self.cd.fr_vec_mont([x for z in zs for x in z]), np.uint8)
        self.keep = []

    def _csrs(self, ms):
        return [C.byref(x) for x in self.ctx._csrs(ms, self.keep)]

    def _buf(self, nbytes):
        return np.full(nbytes, SENTINEL, np.uint8)

    def _enc(self, x):
        return np.asarray(self.cd.fr_vec_mont([x]), np.uint8)

    def witness_map(self, ms):
        out = {"h": self._buf(self.m * self.fr)}
        m_out = C.c_size_t()
        st = self.ctx.lib.hk_witness_map(self.ctx.handle, *self._csrs(ms), self.n_inst, self.n_c, self.z.ctypes.data, self.n_v,
                                         out["h"].ctypes.data, self.m, C.byref(m_out))
        return st, out

    def qap_eval(self, ms):
        out = {k: self._buf(self.n_v * self.fr) for k in "abc"}
        out["zt"] = self._buf(self.fr)
        t, m_out = self._enc(TRAPDOOR["t"]), C.c_size_t()
        st = self.ctx.lib.hk_qap_eval(self.ctx.handle, *self._csrs(ms), self.n_inst, self.n_c, self.n_v, t.ctypes.data,
                                      out["a"].ctypes.data, out["b"].ctypes.data, out["c"].ctypes.data, out["zt"].ctypes.data,
                                      C.byref(m_out))
        return st, out

    def keygen(self, ms):
        g1, g2, n_st = self.ctx.g1_bytes, self.ctx.g2_bytes, len(self.stage_ranges)
        sizes = dict(a_g=self.n_v * g1, b_g=self.n_v * g1, b_h=self.n_v * g2, h_g=(self.m - 1) * g1, deltas_g=n_st * g1, alpha_g=g1,
                     beta_g=g1, gamma_abc_g=self.n_inst * g1, beta_h=g2, gamma_h=g2, deltas_h=n_st * g2,
                     qap_abc=3 * self.n_v * self.fr)
        out = {k: self._buf(n) for k, n in sizes.items()}
        for k, (b, e) in enumerate(self.stage_ranges):
            out["ck%d" % k] = self._buf((e - b) * g1)
        sc = [self._enc(TRAPDOOR[k]) for k in ("alpha", "beta", "gamma", "t", "g1_scalar", "g2_scalar")]
        dl = np.concatenate([self._enc(x) for x in TRAPDOOR["deltas"]])
        sr = np.array([v for be in self.stage_ranges for v in be], dtype=np.uint64)
        A, B, Cm = self.ctx._csrs(ms, self.keep)
        d = capi.hk_keygen_desc(C.pointer(A), C.pointer(B), C.pointer(Cm), self.n_inst, self.n_c, self.n_v, sr.ctypes.data, n_st,
                                *[x.ctypes.data for x in sc], dl.ctypes.data)
        ck = (C.c_void_p * n_st)(*[out["ck%d" % k].ctypes.data for k in range(n_st)])
        o = capi.hk_keygen_out(*[out[k].ctypes.data for k in ("a_g", "b_g", "b_h", "h_g")], ck,
                               *[out[k].ctypes.data for k in ("deltas_g", "alpha_g", "beta_g", "gamma_abc_g", "beta_h", "gamma_h",
                                                              "deltas_h", "qap_abc")])
        return self.ctx.lib.hk_keygen(self.ctx.handle, C.byref(d), C.byref(o), None), out

    def r1cs_check(self, ms):
        out = {"verdicts": self._buf(2 * 8), "rows": self._buf(2 * CAP * 4), "vals": self._buf(2 * CAP * 3 * self.fr)}
        st = self.ctx.lib.hk_r1cs_check(self.ctx.handle, *self._csrs(ms), self.zs.ctypes.data, self.n_v, 2, out["verdicts"].ctypes.data,
                                        out["rows"].ctypes.data, out["vals"].ctypes.data, CAP)
        return st, out

    NAMES = ("witness_map", "qap_eval", "keygen", "r1cs_check")


def _upload(ctx, cd, pk, cs, ms):
    return ctx.pk_upload(a_g=cd.g1_vec(pk.a_g), b_g=cd.g1_vec(pk.b_g), b_h=cd.g2_vec(pk.b_h), h_g=cd.g1_vec(pk.h_g),
                         ck_stages=[cd.g1_vec(v) for v in pk.ck.deltas_abc_g], deltas_g=cd.g1_vec(pk.deltas_g),
                         last_delta_h=cd.g2_vec([pk.last_delta_h()]), alpha_g=cd.g1_vec([pk.vk.alpha_g]),
                         beta_g=cd.g1_vec([pk.beta_g]), beta_h=cd.g2_vec([pk.vk.beta_h]), matrices=ms, n_inst=cs.num_instance,
                         n_constraints=cs.num_constraints)


def _want(curve):
    """the good call's bytes per entry and output, from the oracle and the host mirror"""
    cp, cs, pk, trap, (A, B, Cm), zs = _system(curve)
    cd = Codec(cp)
    fr = lambda xs: np.asarray(cd.fr_vec_mont([int(x) for x in xs]), np.uint8).tobytes()
    g1, g2 = (lambda ps: np.asarray(cd.g1_vec(ps), np.uint8).tobytes()), (lambda ps: np.asarray(cd.g2_vec(ps), np.uint8).tobytes())
    a, b, c = list(trap.a), list(trap.b), list(trap.c)
    keygen = dict(a_g=g1(pk.a_g), b_g=g1(pk.b_g), b_h=g2(pk.b_h), h_g=g1(pk.h_g), deltas_g=g1(pk.deltas_g), alpha_g=g1([pk.vk.alpha_g]),
                  beta_g=g1([pk.beta_g]), gamma_abc_g=g1(pk.vk.gamma_abc_g), beta_h=g2([pk.vk.beta_h]), gamma_h=g2([pk.vk.gamma_h]),
                  deltas_h=g2(pk.vk.deltas_h), qap_abc=fr(a + b + c))
    for k, v in enumerate(pk.ck.deltas_abc_g):
        keygen["ck%d" % k] = g1(v)
    last = len(A) - 1
    ev = lambda row: sum(co * zs[1][j] for co, j in row) % cp.r
    none = [0xFFFFFFFF] * CAP
    rows = np.array(none + [last] + none[1:], np.uint32).tobytes()
    vals = bytes(CAP * 3 * 32) + fr([ev(A[last]), ev(B[last]), ev(Cm[last])]) + bytes((CAP - 1) * 3 * 32)
    return dict(witness_map=dict(h=fr(groth16.witness_map_from_matrices(cp, A, B, Cm, cs.num_instance, len(A), zs[0]))),
                qap_eval=dict(a=fr(a), b=fr(b), c=fr(c), zt=fr([trap.zt])), keygen=keygen,
                r1cs_check=dict(verdicts=np.array([0, 0xFFFFFFFF, 1, last], np.uint32).tobytes(), rows=rows, vals=vals))


def _assert_good(name, got, want):
    st, out = got
    assert st == capi.HK_OK, name
    assert sorted(out) == sorted(want), name
    for k in out:
        assert out[k].tobytes() == want[k], (name, k)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_malformed_matrices_through_every_entry(curve, ctx_bn254, ctx_bls):
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    cp, cs, pk, trap, rows, zs = _system(curve)
    cd = Codec(cp)
    e = _Entries(ctx, curve)
    good = tuple(csr_from_rows(cd, M) for M in rows)
    want = _want(curve)
    for defect, ms in _malformed(good, e.n_v).items():
        for name in e.NAMES:
            st, out = getattr(e, name)(ms)
            assert st == capi.HK_ERR_ARG, (defect, name)
            assert all((b == SENTINEL).all() for b in out.values()), (defect, name)
            _assert_good(name, getattr(e, name)(good), want[name])            # the context's next good call
        with pytest.raises(capi.HekatonError) as err:
            _upload(ctx, cd, pk, cs, ms)
        assert err.value.status == capi.HK_ERR_ARG, defect
    # the key form after the refusals: the resident matrices are the good ones
    dpk = _upload(ctx, cd, pk, cs, good)
    try:
        verdicts, bad_rows = dpk.r1cs_check(e.zs, batch=2, cap=CAP)
        assert verdicts == [(0, None), (1, e.n_c - 1)]
        assert bad_rows.tobytes() == want["r1cs_check"]["rows"]
    finally:
        dpk.free()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_pk_upload_null_row_ptr_is_an_argument_error(curve, ctx_bn254, ctx_bls, monkeypatch):
    """A NULL row_ptr is refused before the first byte of a matrix is read.  The wrapper passes no None through, so the
    descriptor is edited on its way into hk_pk_upload."""
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    cp, cs, pk, trap, rows, zs = _system(curve)
    cd = Codec(cp)
    good = tuple(csr_from_rows(cd, M) for M in rows)
    real = ctx.lib.hk_pk_upload

    def null_row_ptr_in_b(handle, desc, out):
        desc._obj.B.contents.row_ptr = None
        return real(handle, desc, out)
    monkeypatch.setattr(ctx.lib, "hk_pk_upload", null_row_ptr_in_b)
    with pytest.raises(capi.HekatonError) as err:
        _upload(ctx, cd, pk, cs, good)
    assert err.value.status == capi.HK_ERR_ARG
    monkeypatch.undo()
    _upload(ctx, cd, pk, cs, good).free()


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("where", ["device", "mixed"])
def test_device_resident_matrix_arrays(curve, where, ctx_bn254, ctx_bls):
    """every array on the device, or row_ptr on the device and col / val on the host: the entries whose wrappers take device
    arrays (hk_qap_eval, hk_keygen, hk_r1cs_check) return the bytes of the all-host call, which are the oracle's"""
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    cp, cs, pk, trap, rows, zs = _system(curve)
    cd = Codec(cp)
    e = _Entries(ctx, curve)
    good = tuple(csr_from_rows(cd, M) for M in rows)
    want = _want(curve)
    bufs = []

    def dev(x):
        bufs.append(capi.DeviceBuffer.from_host(ctx, np.asarray(x)))
        return bufs[-1]
    try:
        ms = tuple((dev(rp), dev(col) if where == "device" else col, dev(val) if where == "device" else val)
                   for rp, col, val in good)
        for name in ("qap_eval", "keygen", "r1cs_check"):
            _assert_good(name, getattr(e, name)(ms), want[name])
            _assert_good(name, getattr(e, name)(good), want[name])
    finally:
        for b in bufs:
            b.free()
