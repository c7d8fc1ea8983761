"""CPU: the proof-verification surface (hk_vk_prepare / hk_verify_batch / hk_points_check_*) is exported, refuses NULL
contexts and arrays with a status instead of a crash, and the Python layer checks lengths and batching scalars before
any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import FrCodec, Proof, PreparedVerifyingKey, verify_proofs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hk_vk_prepare", "hk_vk_free", "hk_vk_alpha_beta", "hk_verify_batch", "hk_points_check_g1", "hk_points_check_g2"]


def test_new_symbols_declared_and_exported():
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in capi.EXPORTS
        assert getattr(lib, sym) is not None
    assert re.search(r"#define\s+HK_VERIFY_CHECK_POINTS\s+1u", hdr)


def test_null_context_and_arrays_return_a_status():
    lib = capi.load()
    ok = np.zeros(4, np.uint8)
    pts = np.zeros(4 * 128, np.uint8)
    out = C.c_void_p()
    d = capi.hk_vk_desc()
    assert lib.hk_vk_prepare(None, C.byref(d), C.byref(out)) == capi.HK_ERR_ARG
    assert lib.hk_vk_prepare(None, None, None) == capi.HK_ERR_ARG
    assert lib.hk_verify_batch(None, None, None, None, None, None, None, 4, 1, None, None) == capi.HK_ERR_ARG
    assert lib.hk_verify_batch(None, None, pts.ctypes.data, pts.ctypes.data, pts.ctypes.data, None, None, 4, 0, None,
                               ok.ctypes.data) == capi.HK_ERR_ARG
    for fn in (lib.hk_points_check_g1, lib.hk_points_check_g2):
        assert fn(None, pts.ctypes.data, 4, ok.ctypes.data) == capi.HK_ERR_ARG
        assert fn(None, None, 4, None) == capi.HK_ERR_ARG
    assert lib.hk_vk_alpha_beta(None, ok.ctypes.data) == capi.HK_ERR_ARG
    lib.hk_vk_free(None)


class _FakeCtx:
    """Sizes of a BN254 context; any call into the library through it would fail on the None handle."""
    curve = "bn254"
    fr_bytes, fq_bytes, g1_bytes, g2_bytes = 32, 32, 64, 128
    handle = None
    lib = None


def _pvk(n_deltas=2, n_abc=4):
    return PreparedVerifyingKey(None, "bn254", capi.DeviceVk(_FakeCtx(), None, n_deltas, n_abc))


def _proofs(n, nd=1):
    return [Proof(np.zeros(64, np.uint8), np.zeros(128, np.uint8), np.zeros(64, np.uint8), [np.zeros(64, np.uint8)] * nd)
            for _ in range(n)]


def test_python_length_checks_run_before_the_device():
    pvk = _pvk()
    with pytest.raises(capi.HekatonError) as ei:               # verifier.rs:53-55: len(x) + 1 != len(gamma_abc)
        verify_proofs(pvk, _proofs(2), [[1, 2, 3], [1, 2]])
    assert ei.value.status == capi.HK_ERR_LEN
    with pytest.raises(capi.HekatonError) as ei:               # one D per stage delta
        verify_proofs(pvk, _proofs(1, nd=2), [[1, 2, 3]])
    assert ei.value.status == capi.HK_ERR_LEN
    with pytest.raises(ValueError):
        verify_proofs(pvk, _proofs(2), [[1, 2, 3]])
    assert verify_proofs(pvk, [], []) == []
    dvk = pvk.device
    a, b, c, ds, x = (np.zeros(k, np.uint8) for k in (2 * 64, 2 * 128, 2 * 64, 2 * 64, 2 * 3 * 32))
    with pytest.raises(capi.HekatonError) as ei:
        dvk.verify(a, b, c, ds, x[:-32], n=2)
    assert ei.value.status == capi.HK_ERR_LEN
    with pytest.raises(capi.HekatonError) as ei:
        dvk.verify(a, b[:-1], c, ds, x, n=2)
    assert ei.value.status == capi.HK_ERR_LEN


def test_batch_scalars_must_be_nonzero():
    dvk = _pvk().device
    fc = FrCodec("bn254")
    a, b, c, ds, x = (np.zeros(k, np.uint8) for k in (2 * 64, 2 * 128, 2 * 64, 2 * 64, 2 * 3 * 32))
    with pytest.raises(ValueError):
        dvk.verify(a, b, c, ds, x, n=2, rand=fc.enc([5, 0]))
    with pytest.raises(capi.HekatonError) as ei:
        dvk.verify(a, b, c, ds, x, n=2, rand=fc.enc([5]))
    assert ei.value.status == capi.HK_ERR_LEN


def test_vk_prepare_checks_point_sizes():
    ctx = _FakeCtx()
    with pytest.raises(capi.HekatonError) as ei:
        capi.Context.vk_prepare(ctx, alpha_g=np.zeros(63, np.uint8), beta_h=np.zeros(128, np.uint8),
                                gamma_h=np.zeros(128, np.uint8), deltas_h=np.zeros(256, np.uint8),
                                gamma_abc_g=np.zeros(256, np.uint8))
    assert ei.value.status == capi.HK_ERR_LEN
