"""CPU: hk_scalar_powers and hk_ipa_quotient without a device - the symbols are declared, listed and exported; the two Context
wrappers hand the library what include/hekaton.h says (a stub library records it); tipa's and aggregation's helpers issue
the two calls by default and neither under HK_AGG_HOST_SCALARS (a stub context records them); the HK_HD chunk bodies of
csrc/agg_scalars.cuh, compiled for the host and run chunk by chunk with serial scans (tests/host_shim/agg_scalars_shim.cpp),
give the Python mirror's bytes for every size / shift / z / challenge family of the GPU test; and the same source as a
stand-alone program runs clean under -fsanitize=address,undefined with the digests of the plain build."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

from hekaton_system_amd import aggregation, capi, tipa
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from tests import agg_scalars_cases as cases
from tests import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_SRC = "agg_scalars_shim.cpp"  # under tests/host_shim


def test_symbols_declared_listed_exported():
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    declared = set(re.findall(r"\b(hk_[a-z0-9_]+)\s*\(", hdr))
    for sym in ("hk_scalar_powers", "hk_ipa_quotient"):
        assert sym in declared and sym in capi.EXPORTS
        if os.path.exists(capi.LIB_PATH):
            getattr(capi.load(), sym)


# ---- the Context wrappers over a stub library ---------------------------------------------------------------------------
def _addr(p):
    if p is None:
        return 0
    return p if isinstance(p, int) else (p.value or 0)


class _StubLib:
    """Stands in for libhekaton.so under a capi.Context: copies what the two entries are handed, writes a pattern to a host
    output and returns `status`."""

    def __init__(self, status=capi.HK_OK, host_out=True):
        self.status, self.host_out, self.seen = status, host_out, []

    def hk_scalar_powers(self, handle, x, n, reps, out):
        self.seen.append(dict(fn="powers", handle=handle, x=bytes(C.string_at(_addr(x), 32)), n=n, reps=reps, out=_addr(out)))
        if self.host_out:
            C.memset(_addr(out), 0x5a, reps * n * 32)
        return self.status

    def hk_ipa_quotient(self, handle, ch, l, rho, z, shift, out):
        self.seen.append(dict(fn="quotient", handle=handle, ch=bytes(C.string_at(_addr(ch), l * 32)) if l else None,
                              ch_null=_addr(ch) == 0, l=l, rho=bytes(C.string_at(_addr(rho), 32)),
                              z=bytes(C.string_at(_addr(z), 32)), shift=shift, out=_addr(out)))
        if self.host_out:
            C.memset(_addr(out), 0x6b, (shift + (1 << l)) * 32)
        return self.status


def _stub_context(curve, lib):
    ctx = capi.Context.__new__(capi.Context)
    ctx.lib, ctx.curve, ctx.handle, ctx.fr_bytes = lib, curve, "the-handle", 32
    return ctx


@pytest.mark.parametrize("curve", cases.CURVES)
def test_context_wrappers_marshal_their_arguments(curve):
    fc = FrCodec(curve)
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(7)
    x, rho, z = (rnd.randrange(r) for _ in range(3))
    ch = [rnd.randrange(r) for _ in range(3)]
    lib = _StubLib()
    ctx = _stub_context(curve, lib)
    out = ctx.scalar_powers(x, 9, reps=5)
    s = lib.seen[-1]
    assert (s["handle"], s["x"], s["n"], s["reps"]) == ("the-handle", fc.enc1(x).tobytes(), 9, 5)
    assert out.dtype == np.uint8 and out.size == 5 * 9 * 32 and (out == 0x5a).all() and s["out"] == out.ctypes.data
    assert ctx.scalar_powers(x, 4).size == 4 * 32 and lib.seen[-1]["reps"] == 1
    out = ctx.ipa_quotient(ch, rho, z, shift=5)
    s = lib.seen[-1]
    assert (s["handle"], s["l"], s["shift"]) == ("the-handle", 3, 5)
    assert (s["ch"], s["rho"], s["z"]) == (fc.enc(ch).tobytes(), fc.enc1(rho).tobytes(), fc.enc1(z).tobytes())
    assert out.size == (5 + 8) * 32 and (out == 0x6b).all() and s["out"] == out.ctypes.data
    # no challenges: a null pointer and l = 0, one coefficient, shift 0 by default
    out = ctx.ipa_quotient([], 1, z)
    s = lib.seen[-1]
    assert s["ch_null"] and (s["l"], s["shift"]) == (0, 0) and out.size == 32 and s["rho"] == fc.enc1(1).tobytes()
    # a device output is handed over by its address and returned as it is
    dev_lib = _StubLib(host_out=False)
    dctx = _stub_context(curve, dev_lib)
    view = capi.DeviceView(dctx, 0x7f0000001000, 13 * 32)
    assert dctx.scalar_powers(x, 13, out=view) is view and dev_lib.seen[-1]["out"] == 0x7f0000001000
    assert dctx.ipa_quotient(ch, rho, z, 5, out=view) is view and dev_lib.seen[-1]["out"] == 0x7f0000001000
    # a refusal surfaces as HekatonError with the library's status
    for call in (lambda c: c.scalar_powers(x, 4), lambda c: c.ipa_quotient(ch, rho, z)):
        with pytest.raises(capi.HekatonError) as e:
            call(_stub_context(curve, _StubLib(capi.HK_ERR_ARG)))
        assert e.value.status == capi.HK_ERR_ARG


# ---- the callers over a stub context --------------------------------------------------------------------------------------
class _Recorded(Exception):
    pass


class _FakeBuffer:
    """Stands in for capi.DeviceBuffer: an address range nobody touches."""
    live = 0

    def __init__(self, ctx, nbytes, ptr_=0x10000, owner=True):
        self.ctx, self.nbytes, self.ptr, self.owner = ctx, int(nbytes), ptr_, owner
        if owner:
            _FakeBuffer.live += 1

    def view(self, offset, nbytes):
        assert 0 <= offset and offset + nbytes <= self.nbytes
        return _FakeBuffer(self.ctx, nbytes, self.ptr + offset, owner=False)

    def free(self):
        if self.owner and self.ptr:
            _FakeBuffer.live -= 1
            self.ptr = None


class _StubCtx:
    """Stands in for capi.Context: records the two new calls; the first call after them that would need a device stops the
    caller."""
    fr_bytes, g1_bytes, g2_bytes = 32, 64, 128

    def __init__(self, curve):
        self.curve, self.calls, self.stopped_at = curve, [], None

    def scalar_powers(self, x, n, reps=1, out=None):
        self.calls.append(("powers", x, n, reps, None if out is None else (out.ptr, out.nbytes)))
        return out

    def ipa_quotient(self, challenges, rho, z, shift=0, out=None):
        self.calls.append(("quotient", tuple(challenges), rho, z, shift, None if out is None else (out.ptr, out.nbytes)))
        return out

    def fixed_base(self, group, base, scalars, n=None, montgomery=True, out=None):
        self.stopped_at = ("fixed_base", group, scalars, n)
        raise _Recorded()

    def scalar_pairing(self, group, points, scalars, n=None, out=None):
        self.stopped_at = ("scalar_pairing", group, scalars, n)
        raise _Recorded()


@pytest.fixture
def fake_buffers(monkeypatch):
    monkeypatch.setattr(capi, "DeviceBuffer", _FakeBuffer)
    _FakeBuffer.live = 0
    yield _FakeBuffer
    assert _FakeBuffer.live == 0, "a caller left a device buffer behind"


@pytest.mark.parametrize("curve", cases.CURVES)
def test_twist_powers_device_by_default_host_under_the_switch(curve, fake_buffers, monkeypatch):
    fc = FrCodec(curve)
    tw = random.Random(11).randrange(2, fc.r)
    monkeypatch.delenv("HK_AGG_HOST_SCALARS", raising=False)
    ctx = _StubCtx(curve)
    buf = aggregation.twist_powers(ctx, fc, tw, 33, 5)
    assert isinstance(buf, _FakeBuffer) and buf.nbytes == 5 * 33 * 32
    assert ctx.calls == [("powers", tw, 33, 5, (buf.ptr, buf.nbytes))]
    buf.free()
    monkeypatch.setenv("HK_AGG_HOST_SCALARS", "1")
    ctx = _StubCtx(curve)
    host = aggregation.twist_powers(ctx, fc, tw, 33, 5)
    assert ctx.calls == [] and isinstance(host, np.ndarray) and host.tobytes() == cases.mirror_powers(curve, tw, 33, 5)


@pytest.mark.parametrize("curve", cases.CURVES)
def test_setup_device_by_default_host_under_the_switch(curve, fake_buffers, monkeypatch):
    fc = FrCodec(curve)
    rnd = random.Random(12)
    alpha, beta = rnd.randrange(2, fc.r), rnd.randrange(2, fc.r)
    n = 8
    monkeypatch.delenv("HK_AGG_HOST_SCALARS", raising=False)
    ctx = _StubCtx(curve)
    with pytest.raises(_Recorded):
        tipa.setup(ctx, curve, n, alpha, beta)
    base = 0x10000
    assert sorted(ctx.calls) == sorted([("powers", alpha, 2 * n, 1, (base, 2 * n * 32)), ("powers", beta, 2 * n, 1, (base + 2 * n * 32, 2 * n * 32)),
                                        ("powers", alpha, n, 1, (base + 4 * n * 32, n * 32)), ("powers", beta, n, 1, (base + 5 * n * 32, n * 32))])
    kind, group, scalars, count = ctx.stopped_at                           # the sweeps read the powers where they were written
    assert kind == "fixed_base" and (scalars.ptr, count) == ((base, 4 * n) if group == 1 else (base + 4 * n * 32, 2 * n))
    monkeypatch.setenv("HK_AGG_HOST_SCALARS", "1")
    ctx = _StubCtx(curve)
    with pytest.raises(_Recorded):
        tipa.setup(ctx, curve, n, alpha, beta)
    assert ctx.calls == []
    kind, group, scalars, count = ctx.stopped_at
    pa, pb = cases.mirror_powers(curve, alpha, 2 * n, 1), cases.mirror_powers(curve, beta, 2 * n, 1)
    want = pa + pb if group == 1 else pa[:n * 32] + pb[:n * 32]
    assert isinstance(scalars, np.ndarray) and scalars.tobytes() == want


@pytest.mark.parametrize("curve", cases.CURVES)
def test_prove_helpers_device_by_default_host_under_the_switch(curve, fake_buffers, monkeypatch):
    fc = FrCodec(curve)
    r = fc.r
    rnd = random.Random(13)
    n = 8
    twist, z = rnd.randrange(2, r), rnd.randrange(2, r)
    t_inv = pow(twist, -1, r)
    chal = [rnd.randrange(1, r) for _ in range(3)]
    ch_rev = tuple(chal[::-1])
    chi_rev = tuple(pow(c, -1, r) for c in ch_rev)
    arena = _FakeBuffer(None, 5 * n * 32)
    wins = [arena.view(0, n * 32), arena.view(n * 32, n * 32), arena.view(2 * n * 32, n * 32), arena.view(3 * n * 32, 2 * n * 32)]
    monkeypatch.delenv("HK_AGG_HOST_SCALARS", raising=False)
    ctx = _StubCtx(curve)
    assert tipa.twist_vectors(ctx, fc, twist, t_inv, n, out=wins[:2]) == tuple(wins[:2])
    assert tipa.opening_quotients(ctx, fc, chal, t_inv, z, n, out=wins[2:]) == tuple(wins[2:])
    w = [(x.ptr, x.nbytes) for x in wins]
    assert ctx.calls == [("powers", twist, n, 1, w[0]), ("powers", t_inv, n, 1, w[1]),
                         ("quotient", chi_rev, 1, z, 0, w[2]), ("quotient", ch_rev, t_inv, z, n, w[3])]
    monkeypatch.setenv("HK_AGG_HOST_SCALARS", "1")
    ctx = _StubCtx(curve)
    twb, twib = tipa.twist_vectors(ctx, fc, twist, t_inv, n)
    qv, qw = tipa.opening_quotients(ctx, fc, chal, t_inv, z, n)
    assert ctx.calls == []
    assert (twb.tobytes(), twib.tobytes()) == (cases.mirror_powers(curve, twist, n, 1), cases.mirror_powers(curve, t_inv, n, 1))
    assert qv.tobytes() == cases.mirror_quotient(curve, chi_rev, 1, z, 0)
    assert qw.tobytes() == cases.mirror_quotient(curve, ch_rev, t_inv, z, n)
    arena.free()


# ---- the chunk bodies on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """csrc/agg_scalars.cuh compiled for the host (g++) - the source the kernels run."""
    out = str(tmp_path_factory.mktemp("shim") / "agg_scalars_shim.so")
    host_build.build(SHIM_SRC, out, "-O2", *host_build.SHARED)
    lib = host_build.load(out)
    sz, vp, i = C.c_size_t, C.c_void_p, C.c_int
    lib.shim_scalar_powers.argtypes = [i, vp, sz, sz, vp]
    lib.shim_ipa_quotient.argtypes = [i, vp, sz, vp, vp, sz, vp]
    lib.shim_ipa_coeff.argtypes = [i, vp, sz, vp, sz, sz, vp]
    return lib


@pytest.mark.parametrize("curve", cases.CURVES)
def test_host_power_chunks_match_the_mirror(shim, curve):
    fc = FrCodec(curve)
    for n, reps in cases.POWER_SHAPES:
        for x in cases.power_bases(curve):
            out = np.full(reps * n * 32, 0xee, np.uint8)
            shim.shim_scalar_powers(cases.CURVES.index(curve), fc.enc1(x).ctypes.data, n, reps, out.ctypes.data)
            assert out.tobytes() == cases.mirror_powers(curve, x, n, reps), (n, reps, x)


@pytest.mark.parametrize("curve", cases.CURVES)
def test_host_coefficients_match_the_mirror(shim, curve):
    fc = FrCodec(curve)
    rnd = random.Random(31)
    for l, shift in [(0, 0), (0, 1), (2, 0), (3, 8), (4, 5), (6, 13)]:
        ch = [rnd.randrange(fc.r) for _ in range(l)]
        rho = rnd.randrange(1, fc.r)
        want = cases.f_coeffs(curve, ch, rho, shift)
        chb, rb = fc.enc(ch), fc.enc1(rho)
        got = []
        for i in range(len(want) + 9):                                     # past the end: zero
            out = np.zeros(32, np.uint8)
            shim.shim_ipa_coeff(cases.CURVES.index(curve), chb.ctypes.data if l else None, l, rb.ctypes.data, shift, i, out.ctypes.data)
            got.append(out)
        assert fc.dec(np.concatenate(got)) == want + [0] * 9, (l, shift)


@pytest.mark.parametrize("l,shift", cases.QUOTIENT_SHAPES)
@pytest.mark.parametrize("curve", cases.CURVES)
def test_host_quotient_chunks_match_the_mirror(shim, curve, l, shift):
    fc = FrCodec(curve)
    for name, ch, rho, z in cases.quotient_cases(curve, l, shift):
        chb, rb, zb = fc.enc(list(ch)), fc.enc1(rho), fc.enc1(z)
        out = np.full((shift + (1 << l)) * 32, 0xee, np.uint8)
        shim.shim_ipa_quotient(cases.CURVES.index(curve), chb.ctypes.data if l else None, l, rb.ctypes.data, zb.ctypes.data, shift,
                               out.ctypes.data)
        assert out.tobytes() == cases.mirror_quotient(curve, ch, rho, z, shift), name
        assert not out[-32:].any(), name


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """The shim's own main over a handful of the sizes: built plain and with -fsanitize=address,undefined, both exit 0, the
    sanitized run reports nothing and prints the digests of the plain one."""
    outs = []
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("agg_scalars_" + tag))
        host_build.build(SHIM_SRC, exe, "-DAGG_SCALARS_MAIN", *flags)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (tag, r.stderr[-2000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    assert len(outs[0].splitlines()) == 2 * (6 + 9) and "quotient l=17 shift=131072" in outs[0]
