"""GPU: hk_gt_check (k_gt_check, one wavefront per Fq12 value) on the cases of tests/gt_check_cases.py, both curves.  Every
verdict is GtField.in_gt's - the plain x != 0 and x^r == 1 in Python integers - and the table's: the whole table in one call
with accepts and refusals interleaved (no wavefront's verdict leaks into its neighbour's), single elements, the table tiled
to 67 elements, n = 0 over a poisoned output, the three pointer placements, NULL pointers, a coefficient that is no canonical
Fq, and - on the accepting side - what hk_multi_pairing and hk_gt_pow themselves produce."""
import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import FrCodec
from hekaton_system_amd.gt import GtField
from oracle.pyref import curve
from oracle.pyref.params import CURVES
from tests import gt_check_cases as gc
from tests.test_pairing_cpu import Enc

pytestmark = pytest.mark.gpu


def _ctx(cname, ctx_bn254, ctx_bls):
    return ctx_bn254 if cname == "bn254" else ctx_bls


def _interleaved(cname):
    """The cases with accepts and refusals alternating as far as they go, and GtField.in_gt of each."""
    cs, host = gc.cases(cname), gc.host_verdicts(cname)
    acc = [k for k, c in enumerate(cs) if c[2]]
    ref = [k for k, c in enumerate(cs) if not c[2]]
    order = []
    while acc or ref:
        if ref:
            order.append(ref.pop(0))
        if acc:
            order.append(acc.pop(0))
    assert sorted(order) == list(range(len(cs)))
    return [cs[k] for k in order], [host[k] for k in order]


def _enc(F, xs):
    return np.frombuffer(b"".join(F.encode(x) for x in xs), np.uint8).copy()


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_whole_table_in_one_call(cname, ctx_bn254, ctx_bls):
    ctx, F = _ctx(cname, ctx_bn254, ctx_bls), GtField(cname)
    cs, host = _interleaved(cname)
    got = ctx.gt_check(_enc(F, [x for _nm, x, _w in cs]))
    assert got.dtype == np.uint8 and got.shape == (len(cs),)
    print(cname, [(nm, int(v)) for (nm, _x, _w), v in zip(cs, got)])
    assert got.tolist() == [int(h) for h in host], [nm for (nm, _x, _w), v, h in zip(cs, got, host) if int(v) != int(h)]
    assert got.tolist() == [int(w) for _nm, _x, w in cs]


@pytest.mark.parametrize("name", ["one", "zero", "c"])
@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_single_element(cname, name, ctx_bn254, ctx_bls):
    ctx, F = _ctx(cname, ctx_bn254, ctx_bls), GtField(cname)
    x = gc.case(cname, name)
    got = ctx.gt_check(_enc(F, [x]))
    assert got.tolist() == [int(F.in_gt(x))] == [int(name == "one")]


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_table_tiled_to_67(cname, ctx_bn254, ctx_bls):
    ctx, F = _ctx(cname, ctx_bn254, ctx_bls), GtField(cname)
    cs, host = _interleaved(cname)
    idx = [k % len(cs) for k in range(67)]
    got = ctx.gt_check(_enc(F, [cs[k][1] for k in idx]))
    assert got.tolist() == [int(host[k]) for k in idx]


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_n_zero_writes_nothing(cname, ctx_bn254, ctx_bls):
    ctx, F = _ctx(cname, ctx_bn254, ctx_bls), GtField(cname)
    gts = _enc(F, [gc.case(cname, "g"), gc.case(cname, "zero")])
    ok = np.full(8, 0xA5, np.uint8)
    assert ctx.lib.hk_gt_check(ctx.handle, gts.ctypes.data, 0, ok.ctypes.data) == capi.HK_OK
    assert ctx.lib.hk_gt_check(ctx.handle, None, 0, None) == capi.HK_OK
    assert (ok == 0xA5).all()
    dev_ok = capi.DeviceBuffer.from_host(ctx, ok)
    try:
        assert ctx.lib.hk_gt_check(ctx.handle, gts.ctypes.data, 0, dev_ok.ptr) == capi.HK_OK
        assert (dev_ok.to_host() == 0xA5).all()
    finally:
        dev_ok.free()
    assert ctx.gt_check(np.zeros(0, np.uint8)).shape == (0,)


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_pointer_placements(cname, ctx_bn254, ctx_bls):
    ctx, F = _ctx(cname, ctx_bn254, ctx_bls), GtField(cname)
    cs, host = _interleaved(cname)
    want = [int(h) for h in host]
    gts = _enc(F, [x for _nm, x, _w in cs])
    n = len(cs)
    assert ctx.gt_check(gts).tolist() == want                                   # host in, host out
    dev_in = capi.DeviceBuffer.from_host(ctx, gts)
    dev_ok = capi.DeviceBuffer.from_host(ctx, np.full(n + 3, 0xA5, np.uint8))
    try:
        assert ctx.gt_check(dev_in).tolist() == want                            # device in, host out
        assert ctx.gt_check(dev_in, n=3).tolist() == want[:3]
        assert ctx.lib.hk_gt_check(ctx.handle, dev_in.ptr, n, dev_ok.ptr) == capi.HK_OK      # device in, device out
        back = dev_ok.to_host()
        assert back[:n].tolist() == want and (back[n:] == 0xA5).all()           # n bytes and no more
        assert dev_in.to_host().tobytes() == gts.tobytes()                      # the input is read only
    finally:
        dev_in.free()
        dev_ok.free()


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_null_pointers_are_refused(cname, ctx_bn254, ctx_bls):
    ctx, F = _ctx(cname, ctx_bn254, ctx_bls), GtField(cname)
    gts = _enc(F, [gc.case(cname, "g")])
    ok = np.full(1, 0xA5, np.uint8)
    assert ctx.lib.hk_gt_check(ctx.handle, None, 1, ok.ctypes.data) == capi.HK_ERR_ARG
    assert ctx.lib.hk_gt_check(ctx.handle, gts.ctypes.data, 1, None) == capi.HK_ERR_ARG
    assert ctx.lib.hk_gt_check(None, gts.ctypes.data, 1, ok.ctypes.data) == capi.HK_ERR_ARG
    assert ok[0] == 0xA5
    with pytest.raises(capi.HekatonError, match="hk_gt_check"):
        ctx.gt_check(None, n=1)


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_a_coefficient_that_is_no_canonical_fq_is_refused(cname, ctx_bn254, ctx_bls):
    """The bytes of g with q added to one coefficient's Montgomery limbs: the same residue, not a field element's encoding."""
    ctx, F = _ctx(cname, ctx_bn254, ctx_bls), GtField(cname)
    g = gc.case(cname, "g")
    raw = bytearray(F.encode(g))
    for k in (0, 11):
        bad = bytearray(raw)
        v = int.from_bytes(raw[k * F.nb:(k + 1) * F.nb], "little") + F.q
        assert v < 1 << (8 * F.nb)
        bad[k * F.nb:(k + 1) * F.nb] = v.to_bytes(F.nb, "little")
        got = ctx.gt_check(np.frombuffer(bytes(raw) + bytes(bad) + bytes(raw), np.uint8))
        assert got.tolist() == [1, 0, 1], k


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_what_the_library_produces_is_accepted(cname, ctx_bn254, ctx_bls):
    """hk_multi_pairing's outputs, and hk_gt_pow's (both chains) on accepted inputs, are members."""
    ctx, F, cp = _ctx(cname, ctx_bn254, ctx_bls), GtField(cname), CURVES[cname]
    E, fc = Enc(cp), FrCodec(cname)
    G1, G2 = curve.G1(cp), curve.G2(cp)
    ps = [G1.mul(cp.g1_gen, k) for k in (1, 2, 3)]
    qs = [G2.mul(cp.g2_gen, k) for k in (1, 5, cp.r - 1)]
    g1 = np.frombuffer(b"".join(E.g1(p) for p in ps), np.uint8)
    g2 = np.frombuffer(b"".join(E.g2(q) for q in qs), np.uint8)
    outs = [ctx.multi_pairing(g1[:ctx.g1_bytes * n].copy(), g2[:ctx.g2_bytes * n].copy(), n=n) for n in (0, 1, 3)]
    accepted = [x for _nm, x, w in gc.cases(cname) if w]
    exps = [0, 1, cp.r - 1, 0x1234567890ABCDEF, cp.r // 3][:len(accepted)]
    bases = _enc(F, accepted[:len(exps)])
    outs.append(ctx.gt_pow(bases, fc.enc(exps)).reshape(-1))
    outs.append(ctx.gt_pow(bases, fc.enc(exps), in_gt=False).reshape(-1))
    allv = np.concatenate([np.asarray(o, np.uint8).reshape(-1) for o in outs])
    got = ctx.gt_check(allv)
    assert got.shape == (3 + 2 * len(exps),) and got.all(), got.tolist()
    assert F.decode(np.asarray(outs[0], np.uint8).reshape(-1)) == F.one       # the empty product
