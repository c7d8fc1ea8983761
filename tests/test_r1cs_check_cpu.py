"""CPU: the ABI surface of hk_r1cs_check / hk_pk_r1cs_check and their host side, without a device - the symbols are declared,
listed and exported; Context.r1cs_check and DevicePk.r1cs_check hand the library what include/hekaton.h says (a stub library
records it); the host mirror cp_groth16.r1cs_bad_rows and MultiStageConstraintSystem.which_is_unsatisfied on directed rows and
on a synthetic_r1cs fixture; Stage1Device.check over a stub key."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from hekaton_system_amd import capi, sha_circuit
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec, MultiStageConstraintSystem, r1cs_bad_rows
from oracle.pyref.params import CURVES
from tests.r1cs_fixtures import directed_system
from tests.util import synthetic_r1cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hk_r1cs_check", "hk_pk_r1cs_check")
NONE = 0xFFFFFFFF


def test_symbols_declared_listed_exported():
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    declared = set(re.findall(r"\b(hk_[a-z0-9_]+)\s*\(", hdr))
    for sym in NEW:
        assert sym in declared and sym in capi.EXPORTS
    assert re.search(r"uint32_t\s+n_bad;.*\n\s*uint32_t\s+first_bad;.*\n\}\s*hk_r1cs_verdict;", hdr)
    assert [f[0] for f in capi.hk_r1cs_verdict._fields_] == ["n_bad", "first_bad"] and C.sizeof(capi.hk_r1cs_verdict) == 8
    if os.path.exists(capi.LIB_PATH):
        lib = capi.load()
        for sym in NEW:
            getattr(lib, sym)


def _val(p):
    return p.value if isinstance(p, C.c_void_p) else p


def _u32(addr, n):
    return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint32)), (n,))


class _StubLib:
    """Stands in for libhekaton.so: records what the two calls are handed, writes `verdicts` ((n_bad, first_bad) per
    assignment), a pattern to bad_rows and to bad_vals, and returns `status`."""

    def __init__(self, status=capi.HK_OK, verdicts=()):
        self.status, self.verdicts, self.seen = status, verdicts, None

    def _tail(self, seen, z, n_v, batch, verdicts, rows, vals, cap):
        z, verdicts, rows, vals = _val(z), _val(verdicts), _val(rows), _val(vals)
        seen.update(z=z, n_v=n_v, batch=batch, verdicts=verdicts, rows=rows, vals=vals, cap=cap)
        self.seen = seen
        if self.status == capi.HK_OK:
            for b, (n, f) in enumerate(self.verdicts[:batch]):
                _u32(verdicts, 2 * batch)[2 * b:2 * b + 2] = (n, f)
            if rows:
                C.memset(rows, 0x31, 4 * batch * cap)
            if vals:
                C.memset(vals, 0x32, 96 * batch * cap)
        return self.status

    def hk_r1cs_check(self, handle, A, B, Cm, z, n_v, batch, verdicts, rows, vals, cap):
        ms = []
        for m in (A, B, Cm):
            m = m._obj
            ms.append((m.n_rows, m.nnz, list(np.ctypeslib.as_array(C.cast(m.row_ptr, C.POINTER(C.c_uint64)), (m.n_rows + 1,))),
                       list(_u32(m.col, m.nnz)) if m.nnz else [], bytes(C.string_at(m.val_mont, 32 * m.nnz)) if m.nnz else b""))
        return self._tail(dict(handle=handle, matrices=ms), z, n_v, batch, verdicts, rows, vals, cap)

    def hk_pk_r1cs_check(self, handle, pk, z, n_v, batch, verdicts, rows, vals, cap):
        return self._tail(dict(handle=handle, pk=pk), z, n_v, batch, verdicts, rows, vals, cap)


def _stub_context(curve, lib):
    ctx = capi.Context.__new__(capi.Context)
    ctx.lib, ctx.curve, ctx.handle, ctx.fr_bytes = lib, curve, "the-handle", 32
    return ctx


def _triples(rnd):
    """three 4-row matrices of different fill, the third one empty"""
    out = []
    for nnz_rows in ([2, 0, 1, 3], [1, 1, 1, 1], [0, 0, 0, 0]):
        rp = np.concatenate([[0], np.cumsum(nnz_rows)]).astype(np.uint64)
        nnz = int(rp[-1])
        out.append((rp, np.array([rnd.randrange(5) for _ in range(nnz)], np.uint32),
                    np.frombuffer(bytes(rnd.randrange(256) for _ in range(32 * nnz)), np.uint8)))
    return out


def test_context_r1cs_check_marshals_its_arguments():
    rnd = random.Random(3)
    A, B, Cm = _triples(rnd)
    z = np.frombuffer(bytes(rnd.randrange(256) for _ in range(3 * 5 * 32)), np.uint8)
    # verdicts only: NULL bad_rows and bad_vals, cap 0, n_v from the buffer's size and the batch
    lib = _StubLib(verdicts=[(0, NONE), (2, 1), (1, 3)])
    res = _stub_context("bn254", lib).r1cs_check(A, B, Cm, z, batch=3)
    s = lib.seen
    assert res == [(0, None), (2, 1), (1, 3)]
    assert (s["handle"], s["n_v"], s["batch"], s["cap"], s["rows"], s["vals"]) == ("the-handle", 5, 3, 0, None, None)
    assert s["z"] == z.ctypes.data and s["verdicts"]
    for got, (rp, col, val) in zip(s["matrices"], (A, B, Cm)):
        assert got == (4, col.size, list(rp), list(col), val.tobytes())
    # with cap: the rows array the library wrote to; values only when asked for
    lib = _StubLib(verdicts=[(5, 0)])
    res, rows = _stub_context("bn254", lib).r1cs_check(A, B, Cm, z, n_v=5, cap=4)
    s = lib.seen
    assert res == [(5, 0)] and (s["n_v"], s["batch"], s["cap"], s["vals"]) == (5, 1, 4, None)
    assert rows.dtype == np.uint32 and rows.shape == (1, 4) and s["rows"] == rows.ctypes.data and (rows == 0x31313131).all()
    lib = _StubLib(verdicts=[(1, 2), (0, NONE), (0, NONE)])
    res, rows, vals = _stub_context("bls12_381", lib).r1cs_check(A, B, Cm, z, batch=3, cap=2, want_vals=True)
    s = lib.seen
    assert res == [(1, 2), (0, None), (0, None)] and rows.shape == (3, 2)
    assert vals.dtype == np.uint8 and vals.shape == (3, 2, 96) and s["vals"] == vals.ctypes.data and (vals == 0x32).all()
    # want_vals without cap asks for nothing: there is no row to give the sides of
    lib = _StubLib(verdicts=[(0, NONE)])
    assert _stub_context("bn254", lib).r1cs_check(A, B, Cm, z[:160], want_vals=True) == [(0, None)]
    assert (lib.seen["rows"], lib.seen["vals"], lib.seen["cap"]) == (None, None, 0)
    # an empty batch: NULL z and verdicts, an empty list
    lib = _StubLib()
    assert _stub_context("bn254", lib).r1cs_check(A, B, Cm, np.zeros(0, np.uint8), n_v=5, batch=0) == []
    assert (lib.seen["z"], lib.seen["verdicts"], lib.seen["batch"], lib.seen["n_v"]) == (None, None, 0, 5)
    # a refusal surfaces as HekatonError with the library's status
    with pytest.raises(capi.HekatonError) as e:
        _stub_context("bn254", _StubLib(capi.HK_ERR_ARG)).r1cs_check(A, B, Cm, z, batch=3)
    assert e.value.status == capi.HK_ERR_ARG


class _FakeBuffer(capi.DeviceBuffer):
    def __init__(self, ptr_, nbytes):                              # noqa: no allocation
        self.ptr, self.nbytes = ptr_, nbytes


def test_device_pk_r1cs_check_marshals_its_arguments():
    lib = _StubLib(verdicts=[(0, NONE), (3, 7)])
    ctx = _stub_context("bn254", lib)
    pk = capi.DevicePk(ctx, "the-key")
    z = _FakeBuffer(0x7000, 2 * 11 * 32)                           # a device-resident z: its address goes through as it is
    res, rows, vals = pk.r1cs_check(z, batch=2, cap=3, want_vals=True)
    s = lib.seen
    assert res == [(0, None), (3, 7)]
    assert (s["handle"], s["pk"], s["z"], s["n_v"], s["batch"], s["cap"]) == ("the-handle", "the-key", 0x7000, 11, 2, 3)
    assert s["rows"] == rows.ctypes.data and s["vals"] == vals.ctypes.data and rows.shape == (2, 3) and vals.shape == (2, 3, 96)
    assert pk.r1cs_check(z, n_v=22) == [(0, None)]                 # the defaults: one assignment, verdicts only
    assert (lib.seen["n_v"], lib.seen["batch"], lib.seen["cap"], lib.seen["rows"], lib.seen["vals"]) == (22, 1, 0, None, None)
    with pytest.raises(capi.HekatonError) as e:
        capi.DevicePk(_stub_context("bn254", _StubLib(capi.HK_ERR_LEN)), "k").r1cs_check(z, batch=2)
    assert e.value.status == capi.HK_ERR_LEN


# ---- the host mirror ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_r1cs_bad_rows_on_the_directed_rows(curve):
    r = CURVE_PARAMS[curve]["r"]
    A, B, C, z, bad, sides = directed_system(r)
    assert len(A) == 13 and len(z) == 10 and bad == [5, 7]
    assert r1cs_bad_rows(A, B, C, z, r) == bad
    assert sides[0][0] == 0 and sides[5] == (0, 0, 1) and sides[1] == (5, 7, 35)
    assert sides[7] == (sides[6][0], sides[6][1], sides[6][2] + 1)
    assert max(len(a) for a in A) == 40 and sorted(len(a) for a in A)[-2] == 2
    # a wrong witness is reported where it is used, every row of it, in ascending order
    z2 = list(z)
    z2[3] += 1
    assert r1cs_bad_rows(A, B, C, z2, r) == [1, 5, 7, 10]          # rows 0 and 6 hold for every z3
    assert r1cs_bad_rows([], [], [], z, r) == []


def _ms_system(cs, r):
    """tests/util.synthetic_r1cs as a MultiStageConstraintSystem (same variables, rows and values)"""
    ms = MultiStageConstraintSystem(r)
    ms.instance_assignment = list(cs.instance)
    ms.witness_assignment = list(cs.witness)
    for a, b, c in zip(cs.A, cs.B, cs.C):
        ms.enforce_constraint(a, b, c)
    return ms


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_which_is_unsatisfied_agrees_with_is_satisfied(curve):
    cp = CURVES[curve]
    cs = synthetic_r1cs(cp, random.Random(5), 3, 6, 70)
    ms = _ms_system(cs, cp.r)
    assert ms.to_matrices() == cs.matrices() and ms.full_assignment() == cs.full_assignment()
    assert ms.is_satisfied() and ms.which_is_unsatisfied() is None
    # row i's own witness is column n_inst + 6 + i and occurs in no earlier row: perturbing it fails row i first
    for i in (0, 41, 69):
        bad = _ms_system(cs, cp.r)
        bad.witness_assignment[6 + i] = (bad.witness_assignment[6 + i] + 1) % cp.r
        assert not bad.is_satisfied() and bad.which_is_unsatisfied() == i
        rows = r1cs_bad_rows(*bad.to_matrices(), bad.full_assignment(), cp.r)
        assert rows[0] == i and rows == sorted(rows)
    # the term (1, column 0) added to a C row: exactly that row fails
    for i in (0, 63, 64):
        bad = _ms_system(cs, cp.r)
        bad.C[i] = bad.C[i] + [(1, "one")]
        assert bad.which_is_unsatisfied() == i and not bad.is_satisfied()
        assert r1cs_bad_rows(*bad.to_matrices(), bad.full_assignment(), cp.r) == [i]


# ---- Stage1Device.check ------------------------------------------------------------------------------------------------
class _StubKey:
    def __init__(self, verdicts, rows):
        self.verdicts, self.rows, self.calls = verdicts, rows, []

    def r1cs_check(self, z, n_v=None, batch=1, cap=0, want_vals=False):
        self.calls.append((z, n_v, batch, cap, want_vals))
        return (self.verdicts, np.array(self.rows, np.uint32)) if cap else self.verdicts


def test_stage1_device_check_names_subcircuit_and_row():
    dev = sha_circuit.Stage1Device.__new__(sha_circuit.Stage1Device)
    ok = _StubKey([(0, None)] * 3, [[NONE] * 8] * 3)
    assert dev.check(ok, "z", [4, 5, 6]) is None
    assert ok.calls == [("z", None, 3, 8, False)]
    bad = _StubKey([(0, None), (2, 17), (1, 3)], [[NONE] * 2, [17, 40], [3, NONE]])
    with pytest.raises(sha_circuit.R1csUnsatisfied) as e:
        dev.check(bad, "z", [4, 5, 6], cap=2)
    assert (e.value.subcircuit, e.value.row, e.value.n_bad) == (5, 17, 2)
    assert e.value.failures == [(5, 2, 17, [17, 40]), (6, 1, 3, [3])]
    assert "subcircuit 5" in str(e.value) and "constraint 17" in str(e.value)
    none = _StubKey([], [])
    dev.check(none, "z", [])
    assert none.calls == []                                        # nothing to check: no call
