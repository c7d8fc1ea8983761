"""GPU: hk_scalar_powers and hk_ipa_quotient against the Python mirror, byte for byte (tests/agg_scalars_cases.py: a plain
power loop, tipa.ipa_polynomial_coeffs, tipa._divide_by_linear, FrCodec) - every chunk / workgroup / tile boundary of the
kernels of csrc/agg_scalars.cuh, host and device outputs with a guard behind them, the refusals; then through the callers:
tipa.setup, Tipp.prove and aggregation.twist_powers give the same bytes on the device path as under HK_AGG_HOST_SCALARS,
and the proofs verify."""
import random

import numpy as np
import pytest

from hekaton_system_amd import aggregation, capi, tipa
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from tests import agg_scalars_cases as cases

pytestmark = pytest.mark.gpu

GUARD = 64                   # bytes behind every output that must keep their pattern
PATTERN = 0xEE


@pytest.fixture
def ctx_of(ctx_bn254, ctx_bls):
    return {"bn254": ctx_bn254, "bls12_381": ctx_bls}


class _Outputs:
    """A host and a device output of `nbytes` + GUARD, patterned before every call."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.pattern = np.full(nbytes + GUARD, PATTERN, np.uint8)
        self.dev = capi.DeviceBuffer.from_host(ctx, self.pattern)

    def host(self):
        return self.pattern.copy()

    def device(self):
        capi.check(capi.load().hk_dev_upload(self.ctx.handle, self.dev.ptr, self.pattern.ctypes.data, self.pattern.nbytes), "hk_dev_upload")
        return self.dev

    def check(self, got, want, what):
        got = got.to_host() if isinstance(got, capi.DeviceBuffer) else got
        assert got[:self.nbytes].tobytes() == want, what
        assert (got[self.nbytes:] == PATTERN).all(), ("wrote past the end", what)


@pytest.mark.parametrize("n,reps", cases.POWER_SHAPES)
@pytest.mark.parametrize("curve", cases.CURVES)
def test_scalar_powers_match_the_mirror(curve, n, reps, ctx_of):
    ctx = ctx_of[curve]
    outs = _Outputs(ctx, reps * n * 32)
    try:
        for x in cases.power_bases(curve):
            want = cases.mirror_powers(curve, x, n, reps)
            outs.check(ctx.scalar_powers(x, n, reps, out=outs.host()), want, ("host", x))
            outs.check(ctx.scalar_powers(x, n, reps, out=outs.device()), want, ("device", x))
        fresh = ctx.scalar_powers(2, n, reps)                              # the wrapper's own buffer
        assert fresh.tobytes() == cases.mirror_powers(curve, 2, n, reps)
    finally:
        outs.dev.free()


@pytest.mark.parametrize("curve", cases.CURVES)
def test_scalar_powers_of_zero_are_one_then_zeros(curve, ctx_of):
    fc = FrCodec(curve)
    assert fc.dec(ctx_of[curve].scalar_powers(0, 9)) == [1] + [0] * 8


@pytest.mark.parametrize("curve", cases.CURVES)
def test_no_powers_is_ok_and_writes_nothing(curve, ctx_of):
    ctx = ctx_of[curve]
    outs = _Outputs(ctx, 0)
    try:
        outs.check(ctx.scalar_powers(5, 0, 1, out=outs.host()), b"", "host")
        outs.check(ctx.scalar_powers(5, 0, 3, out=outs.device()), b"", "device")
        outs.check(ctx.scalar_powers(5, 4, 0, out=outs.host()), b"", "no repetitions")
    finally:
        outs.dev.free()


@pytest.mark.parametrize("l,shift", cases.QUOTIENT_SHAPES)
@pytest.mark.parametrize("curve", cases.CURVES)
def test_ipa_quotient_matches_the_mirror(curve, l, shift, ctx_of):
    ctx = ctx_of[curve]
    fc = FrCodec(curve)
    r = fc.r
    n = shift + (1 << l)
    outs = _Outputs(ctx, n * 32)
    alpha = random.Random(5 * l + shift).randrange(2, r)
    try:
        for name, ch, rho, z in cases.quotient_cases(curve, l, shift):
            want = cases.mirror_quotient(curve, ch, rho, z, shift)
            assert want[-32:] == bytes(32), name                           # the appended zero
            if l <= 4:
                # the mirror itself, pinned independently: q(alpha) (alpha - z) + f(z) = f(alpha) at a random alpha
                f = cases.f_coeffs(curve, ch, rho, shift)
                ev = lambda p, x: sum(c * pow(x, i, r) for i, c in enumerate(p)) % r
                assert (ev(fc.dec(want), alpha) * (alpha - z) + ev(f, z)) % r == ev(f, alpha), name
            outs.check(ctx.ipa_quotient(ch, rho, z, shift, out=outs.host()), want, ("host", name))
            outs.check(ctx.ipa_quotient(ch, rho, z, shift, out=outs.device()), want, ("device", name))
    finally:
        outs.dev.free()


@pytest.mark.parametrize("curve", cases.CURVES)
def test_refusals_leave_the_output_untouched(curve, ctx_of):
    ctx = ctx_of[curve]
    lib = capi.load()
    fc = FrCodec(curve)
    ch = fc.enc([3] * 27)
    one = fc.enc1(1)
    p = lambda a: a.ctypes.data
    outs = _Outputs(ctx, 1024)
    try:
        for dev in (False, True):
            def refused(call, what):
                out = outs.device() if dev else outs.host()
                status = call(outs.dev.ptr if dev else out.ctypes.data)
                assert status == capi.HK_ERR_ARG, (what, status)
                outs.check(out, bytes([PATTERN]) * 1024, what)
            refused(lambda o: lib.hk_ipa_quotient(ctx.handle, p(ch), 27, p(one), p(one), 0, o), "l = 27")
            refused(lambda o: lib.hk_ipa_quotient(ctx.handle, p(ch), 26, p(one), p(one), (1 << 26) + 1, o), "shift + 2^l > 2^27")
            refused(lambda o: lib.hk_ipa_quotient(ctx.handle, p(ch), 2, p(one), p(one), (1 << 27) - 3, o), "shift + 2^l > 2^27")
            refused(lambda o: lib.hk_ipa_quotient(ctx.handle, None, 2, p(one), p(one), 0, o), "null challenges")
            refused(lambda o: lib.hk_ipa_quotient(ctx.handle, p(ch), 2, None, p(one), 0, o), "null rho")
            refused(lambda o: lib.hk_ipa_quotient(ctx.handle, p(ch), 2, p(one), None, 0, o), "null z")
            refused(lambda o: lib.hk_scalar_powers(ctx.handle, None, 4, 1, o), "null x")
            refused(lambda o: lib.hk_scalar_powers(ctx.handle, p(one), (1 << 27) + 1, 1, o), "n > 2^27")
            refused(lambda o: lib.hk_scalar_powers(ctx.handle, p(one), 1 << 26, 3, o), "reps n > 2^27")
        assert lib.hk_ipa_quotient(ctx.handle, p(ch), 2, p(one), p(one), 0, None) == capi.HK_ERR_ARG
        assert lib.hk_scalar_powers(ctx.handle, p(one), 4, 1, None) == capi.HK_ERR_ARG
    finally:
        outs.dev.free()


# ---- through the callers -----------------------------------------------------------------------------------------------
def _both_paths(monkeypatch, fn):
    monkeypatch.delenv("HK_AGG_HOST_SCALARS", raising=False)
    dev = fn()
    monkeypatch.setenv("HK_AGG_HOST_SCALARS", "1")
    try:
        return dev, fn()
    finally:
        monkeypatch.delenv("HK_AGG_HOST_SCALARS")


def _free_srs(srs):
    for b in srs.resident.values():
        b.free()


@pytest.mark.parametrize("curve", cases.CURVES)
def test_setup_gives_the_same_key_on_both_paths(curve, ctx_of, monkeypatch):
    ctx = ctx_of[curve]
    rnd = random.Random(61)
    r = CURVE_PARAMS[curve]["r"]
    alpha, beta = rnd.randrange(2, r), rnd.randrange(2, r)
    dev, host = _both_paths(monkeypatch, lambda: tipa.setup(ctx, curve, 8, alpha, beta))
    try:
        for k in ("g_alpha", "g_beta", "h_alpha", "h_beta"):
            assert np.array_equal(np.asarray(getattr(dev, k)), np.asarray(getattr(host, k))), k
        for k in ("v1", "v2", "w1", "w2"):
            assert np.array_equal(np.asarray(getattr(dev.ck, k)), np.asarray(getattr(host.ck, k))), k
        assert dev.g_alpha.size == 16 * ctx.g1_bytes and dev.h_beta.size == 8 * ctx.g2_bytes and dev.ck.n == host.ck.n == 8
    finally:
        _free_srs(dev)
        _free_srs(host)


@pytest.mark.parametrize("n", [2, 8, 32])
@pytest.mark.parametrize("curve", cases.CURVES)
def test_prove_sends_the_same_proof_on_both_paths(curve, n, ctx_of, monkeypatch):
    """A and B are random curve points (fixed-base multiples of the generators): `prove` needs no Groth16 instance, only the
    commitment and the twisted inner product of what it is given."""
    ctx = ctx_of[curve]
    fc = FrCodec(curve)
    p = CURVE_PARAMS[curve]
    r = p["r"]
    rnd = random.Random(100 + n)
    alpha, beta, twist = (rnd.randrange(2, r) for _ in range(3))
    srs = tipa.setup(ctx, curve, n, alpha, beta)
    try:
        A = np.asarray(ctx.fixed_base(1, fc.g1(p["g1"]), fc.enc([rnd.randrange(1, r) for _ in range(n)])))
        B = np.asarray(ctx.fixed_base(2, fc.g2(p["g2"]), fc.enc([rnd.randrange(1, r) for _ in range(n)])))
        T = tipa.Tipp(ctx, curve)
        com = T.com.commit_with_ip(srs.ck, A, B)
        b_twisted = ctx.scalar_pairing(2, B, fc.enc([pow(twist, i, r) for i in range(n)]), n)
        z_ab = T.F.decode(ctx.multi_pairing(A, b_twisted, n))
        dev, host = _both_paths(monkeypatch, lambda: T.prove(srs, A, B, twist, com, z_ab))
        assert dev["rounds"] == host["rounds"] and len(dev["rounds"]) == n.bit_length() - 1
        for key in ("final_a", "final_b", "final_v", "final_w", "open_v", "open_w"):
            assert np.array_equal(np.asarray(dev[key]), np.asarray(host[key])), key
        assert T.verify(tipa.verifier_key(ctx, curve, srs), com, z_ab, twist, dev)
        T.pool.shutdown()
    finally:
        _free_srs(srs)


@pytest.mark.parametrize("n", [8, 33])
@pytest.mark.parametrize("curve", cases.CURVES)
def test_twist_powers_are_equal_on_both_paths(curve, n, ctx_of, monkeypatch):
    ctx = ctx_of[curve]
    fc = FrCodec(curve)
    twist = random.Random(n).randrange(2, fc.r)
    dev, host = _both_paths(monkeypatch, lambda: aggregation.twist_powers(ctx, fc, twist, n, 5))
    try:
        assert isinstance(dev, capi.DeviceBuffer) and isinstance(host, np.ndarray)
        assert dev.to_host().tobytes() == host.tobytes() == cases.mirror_powers(curve, twist, n, 5)
    finally:
        dev.free()
