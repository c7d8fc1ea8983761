"""GPU: hk_field_sqrt, hk_points_decompress_* and hk_points_compress_* against pure Python (pow, the codec without a context,
oracle.pyref - tests/point_codec_cases.py), byte for byte, both curves: sizes 1 / 63 / 64 / 65 / 130, host, device and mixed
pointers, 64 guard bytes behind every output; the refusals; and through the layers - a compressed key file read back on the
device, uploaded from HBM and proved with."""
import ctypes as C

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.ark_serialize import ArkCodec, ProvingKeys, SerializationError
from hekaton_system_amd.cp_groth16 import CommitterKey, ProvingKey, VerifyingKey
from tests import golden_util as gu
from tests import point_codec_cases as pc

pytestmark = pytest.mark.gpu

MODES = {"host": (False, False, False, False), "device": (True, True, True, True), "mixed": (True, False, False, True),
         "mixed2": (False, True, True, False)}


@pytest.fixture(params=pc.CURVE_NAMES)
def cc(request, ctx_bn254, ctx_bls):
    return request.param, (ctx_bn254 if request.param == "bn254" else ctx_bls)


def call(ctx, fn, head, ins, out_sizes, n, tail=(), mode=(False,) * 4):
    """fn(ctx, *head, ins.., [n], *tail.., outs..) in the order of include/hekaton.h, every buffer on the host or the device
    as `mode` says (inputs first).  Returns (status, outputs without their guards); the guards must have kept their pattern."""
    bufs, keep = [], []
    for k, a in enumerate(ins):
        a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
        b = capi.DeviceBuffer.from_host(ctx, a) if mode[k] and a.size else a
        keep.append(b)
        bufs.append(capi.ptr(b) if a.size else None)
    outs = []
    for k, size in enumerate(out_sizes):
        a = np.full(size + pc.GUARD, pc.GUARD_BYTE, dtype=np.uint8)
        b = capi.DeviceBuffer.from_host(ctx, a) if mode[len(ins) + k] else a
        outs.append(b)
    args = [ctx.handle] + list(head) + bufs + [n] + list(tail) + [capi.ptr(o) for o in outs]
    st = fn(*args)
    res = []
    for o, size in zip(outs, out_sizes):
        h = o.to_host() if isinstance(o, capi.DeviceBuffer) else o
        assert (h[size:] == pc.GUARD_BYTE).all(), "guard bytes behind an output changed"
        res.append(h[:size].copy())
    for b in keep + outs:
        if isinstance(b, capi.DeviceBuffer):
            b.free()
    return st, res


def field_sqrt(ctx, which, data, n, mode):
    eb = ctx.fq_bytes * which
    # hk_field_sqrt(ctx, which, in, n, out, ok)
    return call(ctx, ctx.lib.hk_field_sqrt, [which], [data], [n * eb, n], n, mode=(mode[0], mode[2], mode[3]))


def decompress(ctx, group, x, flags, n, check, mode):
    fn = ctx.lib.hk_points_decompress_g1 if group == 1 else ctx.lib.hk_points_decompress_g2
    return call(ctx, fn, [], [x, flags], [2 * n * ctx.fq_bytes * group, n], n, tail=[check], mode=mode)


def compress(ctx, group, pts, n, mode):
    fn = ctx.lib.hk_points_compress_g1 if group == 1 else ctx.lib.hk_points_compress_g2
    return call(ctx, fn, [], [pts], [n * ctx.fq_bytes * group, n], n, mode=(mode[0], mode[2], mode[3]))


def _roots(curve, which):
    if which == 1:
        fam = pc.fq_family(curve)
        roots = [pc.fq_sqrt_smaller(curve, a) for a, _ in fam]
        return (pc.mont_arr(curve, [a for a, _ in fam]), pc.mont_arr(curve, [r or 0 for r in roots]),
                np.array([r is not None for r in roots], dtype=np.uint8))
    fam = pc.fq2_family(curve)
    roots = [pc.fq2_sqrt_smaller(curve, a) for a, _ in fam]
    return (pc.mont_arr(curve, [c for a, _ in fam for c in a]), pc.mont_arr(curve, [c for r in roots for c in (r or (0, 0))]),
            np.array([r is not None for r in roots], dtype=np.uint8))


@pytest.mark.parametrize("which", [1, 2])
def test_field_sqrt(cc, which):
    """ok as pow says; the root is the canonical smaller one (the expected bytes are min(s, q - s) under ark's order);
    out^2 == in in integers; zeros where there is no root."""
    curve, ctx = cc
    data, want, want_ok = _roots(curve, which)
    eb = ctx.fq_bytes * which
    total = want_ok.size
    q = pc.codec(curve).q
    for n in [k for k in pc.SIZES if k <= total] + [total]:
        lo = total - n if n in (63, 65) else 0              # the tail holds the non-squares, the head the directed values
        for name, mode in MODES.items():
            st, (out, ok) = field_sqrt(ctx, which, data[lo * eb:(lo + n) * eb], n, mode)
            assert st == capi.HK_OK
            assert ok.tobytes() == want_ok[lo:lo + n].tobytes(), (n, name)
            assert out.tobytes() == want[lo * eb:(lo + n) * eb].tobytes(), (n, name)
    # the properties, on the whole family, from the device's own bytes
    st, (out, ok) = field_sqrt(ctx, which, data, total, MODES["host"])
    vals, roots = pc.from_mont_arr(curve, data), pc.from_mont_arr(curve, out)
    for i in range(total):
        a, r = vals[which * i:which * (i + 1)], roots[which * i:which * (i + 1)]
        if not ok[i]:
            assert not any(r)
        elif which == 1:
            assert r[0] * r[0] % q == a[0] and r[0] <= (q - 1) // 2
        else:
            assert pc.fq2_mul(q, tuple(r), tuple(r)) == tuple(a) and not pc.fq2_larger(curve, tuple(r))
    assert 0 < ok.sum() < total
    # what the wrapper returns
    r2, ok2 = ctx.field_sqrt(which, data)
    assert r2.tobytes() == want.tobytes() and ok2.tobytes() == want_ok.tobytes()


@pytest.mark.parametrize("group", [1, 2])
def test_points_decompress(cc, group):
    """Byte for byte what the mirror gives where it accepts, status 0 and zeros where it raises; check = 1 marks exactly the
    off-subgroup lanes with 2 - the verdicts of hk_points_check_* on the decompressed output - and changes nothing else."""
    curve, ctx = cc
    x, flags = pc.batch_arrays(curve, group)
    want_status, want_pts = pc.mirror_decompress(curve, group)
    off = np.zeros(pc.BATCH, dtype=bool)
    off[pc.off_subgroup_lanes(curve, group)] = True
    want_checked = np.where(off, 2, want_status).astype(np.uint8)
    assert (want_status[off] == 1).all() and off.any() == (not (curve == "bn254" and group == 1))
    for n in pc.SIZES:
        sl = pc.batch_slice(n)
        for name, mode in MODES.items():
            for check, ws in ((0, want_status), (1, want_checked)):
                st, (pts, status) = decompress(ctx, group, x[sl], flags[sl], n, check, mode)
                assert st == capi.HK_OK
                assert status.tobytes() == ws[sl].tobytes(), (n, name, check)
                assert pts.tobytes() == want_pts[sl].tobytes(), (n, name, check)
    valid = ctx.points_check(group, want_pts.reshape(-1))
    assert ((valid == 0) == off).all()
    # the wrapper: host arrays, and a device output that stays where it is
    pts, status = ctx.points_decompress(group, x, flags, check=True)
    assert pts.tobytes() == want_pts.tobytes() and status.tobytes() == want_checked.tobytes()
    buf = capi.DeviceBuffer(ctx, want_pts.size)
    got, status = ctx.points_decompress(group, x, flags, out=buf)
    assert got is buf and buf.to_host().tobytes() == want_pts.tobytes() and status.tobytes() == want_status.tobytes()
    buf.free()


def test_bls12_381_generators_known_answer(ctx_bls):
    """The published zcash encodings: decompressing the compressed form on the device gives the uncompressed one."""
    dev, plain = ArkCodec("bls12_381", ctx_bls), ArkCodec("bls12_381")
    for group, comp, full in ((1, pc.BLS_G1_COMPRESSED, pc.BLS_G1_UNCOMPRESSED), (2, pc.BLS_G2_COMPRESSED, pc.BLS_G2_UNCOMPRESSED)):
        pts = dev.points_from_wire(group, bytes.fromhex(comp), 1, compress=True, validate=True)
        assert plain.points_to_wire(group, pts).hex() == full
        assert dev.points_to_wire(group, pts, compress=True).hex() == comp


@pytest.mark.parametrize("group", [1, 2])
def test_points_compress(cc, group):
    """x and flag of every point and boundary y as the sign rule says; decompress(compress(P)) == P; the codec writes the same
    wire bytes with and without a context."""
    curve, ctx = cc
    fam = pc.compress_family(curve, group)
    abi = np.frombuffer(b"".join(r[0] for r in fam), dtype=np.uint8).copy()
    want_x, want_f = b"".join(r[1] for r in fam), bytes(r[2] for r in fam)
    pb, xb = 2 * ctx.fq_bytes * group, ctx.fq_bytes * group
    total = len(fam)
    for n in [k for k in pc.SIZES if k <= total] + [total]:
        lo = total - n if n in (64, 130) else 0            # the head holds the boundary values, the tail the batch's points
        for name, mode in MODES.items():
            st, (x, f) = compress(ctx, group, abi[lo * pb:(lo + n) * pb], n, mode)
            assert st == capi.HK_OK
            assert f.tobytes() == want_f[lo:lo + n], (n, name)
            assert x.tobytes() == want_x[lo * xb:(lo + n) * xb], (n, name)
    # the inverse, over infinity and the points of the batch (the tail: they are on the curve)
    first = next(i for i, r in enumerate(fam) if r[2] == pc.FLAG_INF)
    on = range(first, total)
    sel = abi[first * pb:]
    x, f = ctx.points_compress(group, sel)
    back, status = ctx.points_decompress(group, x, f)
    assert len(on) > 100 and (status == 1).all() and back.tobytes() == sel.tobytes()
    # the wire: same bytes with and without a context
    plain, dev = ArkCodec(curve), ArkCodec(curve, ctx)
    wire = plain.points_to_wire(group, abi, compress=True)
    assert dev.points_to_wire(group, abi, compress=True) == wire
    assert dev.points_from_wire(group, plain.points_to_wire(group, sel, compress=True), len(on), compress=True).tobytes() == sel.tobytes()


def test_codec_exceptions_with_a_context(cc):
    curve, ctx = cc
    dev = ArkCodec(curve, ctx)
    for group in (1, 2):
        rows = pc.point_family(curve, group)
        bad = next(r for r in rows if r[2] == "no_root")
        with pytest.raises(SerializationError, match="x is not on the curve"):
            dev.points_from_wire(group, pc.wire_of(curve, group, bad[0], bad[1]), 1, compress=True)
        off = pc.off_subgroup_lanes(curve, group)
        if off:
            w = pc.wire_of(curve, group, rows[off[0]][0], rows[off[0]][1])
            assert dev.points_from_wire(group, w, 1, compress=True).tobytes() == pc.mirror_decompress(curve, group)[1][off[0]].tobytes()
            with pytest.raises(SerializationError, match="InvalidData.*subgroup"):
                dev.points_from_wire(group, w, 1, compress=True, validate=True)


def test_refusals_leave_the_outputs_untouched(cc):
    """HK_ERR_ARG: a NULL pointer with n > 0, `which` outside {1, 2}, n >= 2^31, an input that overlaps an output.  n = 0 is
    HK_OK.  Nothing is written in either case."""
    curve, ctx = cc
    lib, h = ctx.lib, ctx.handle
    fq = ctx.fq_bytes
    n = 5
    x, flags = pc.batch_arrays(curve, 1)
    x, flags = x[1:1 + n].reshape(-1).copy(), flags[1:1 + n].copy()
    pts = pc.mirror_decompress(curve, 1)[1][1:1 + n].reshape(-1).copy()
    big = np.full(4 * n * fq, pc.GUARD_BYTE, dtype=np.uint8)
    small = np.full(n, pc.GUARD_BYTE, dtype=np.uint8)
    p = lambda a: a.ctypes.data

    def refused(st):
        assert st == capi.HK_ERR_ARG
        assert (big == pc.GUARD_BYTE).all() and (small == pc.GUARD_BYTE).all()

    # hk_field_sqrt
    for which in (0, 3, -1):
        refused(lib.hk_field_sqrt(h, which, p(pts), n, p(big), p(small)))
    refused(lib.hk_field_sqrt(h, 1, None, n, p(big), p(small)))
    refused(lib.hk_field_sqrt(h, 1, p(pts), n, None, p(small)))
    refused(lib.hk_field_sqrt(h, 1, p(pts), n, p(big), None))
    refused(lib.hk_field_sqrt(h, 1, p(pts), 1 << 31, p(big), p(small)))
    refused(lib.hk_field_sqrt(h, 1, p(big), n, p(big), p(small)))                      # in place
    refused(lib.hk_field_sqrt(h, 1, p(big), n, p(big) + n * fq - 1, p(small)))         # one shared byte
    refused(lib.hk_field_sqrt(h, 1, p(big), n, p(big) + 2 * n * fq, p(big) + n * fq - 1))
    assert lib.hk_field_sqrt(h, 1, None, 0, None, None) == capi.HK_OK
    assert lib.hk_field_sqrt(h, 2, p(pts), 0, p(big), p(small)) == capi.HK_OK
    for dec, comp in ((lib.hk_points_decompress_g1, lib.hk_points_compress_g1), (lib.hk_points_decompress_g2, lib.hk_points_compress_g2)):
        # the G2 entries read these buffers as fewer points: the rules are the same
        m = n if dec is lib.hk_points_decompress_g1 else n // 2
        refused(dec(h, None, p(flags), m, 0, p(big), p(small)))
        refused(dec(h, p(x), None, m, 0, p(big), p(small)))
        refused(dec(h, p(x), p(flags), m, 0, None, p(small)))
        refused(dec(h, p(x), p(flags), m, 1, p(big), None))
        refused(dec(h, p(x), p(flags), 1 << 31, 0, p(big), p(small)))
        refused(dec(h, p(big), p(flags), m, 0, p(big), p(small)))                      # x overlaps the points
        refused(dec(h, p(x), p(small), m, 0, p(big), p(small)))                        # the flags are the status
        refused(dec(h, p(x), p(flags), m, 0, p(big), p(big) + 1))                      # status inside the points
        assert dec(h, None, None, 0, 1, None, None) == capi.HK_OK
        assert dec(h, p(x), p(flags), 0, 1, p(big), p(small)) == capi.HK_OK
        refused(comp(h, None, m, p(big), p(small)))
        refused(comp(h, p(pts), m, None, p(small)))
        refused(comp(h, p(pts), m, p(big), None))
        refused(comp(h, p(pts), 1 << 31, p(big), p(small)))
        refused(comp(h, p(big), m, p(big), p(small)))
        refused(comp(h, p(pts), m, p(big), p(big)))
        assert comp(h, None, 0, None, None) == capi.HK_OK
        assert comp(h, p(pts), 0, p(big), p(small)) == capi.HK_OK
    assert (big == pc.GUARD_BYTE).all() and (small == pc.GUARD_BYTE).all()
    # a device range against itself
    d = capi.DeviceBuffer.from_host(ctx, big)
    refused(lib.hk_field_sqrt(h, 1, C.c_void_p(d.ptr), n, C.c_void_p(d.ptr), p(small)))
    assert d.to_host().tobytes() == big.tobytes()
    d.free()


# ---- through the layers ------------------------------------------------------------------------------------------------------
def _golden_keys(case):
    pk = case["pk"]
    g1 = len(gu.hb(pk["alpha_g"]))
    vk = VerifyingKey(gu.hb(pk["alpha_g"]), gu.hb(pk["beta_h"]), gu.hb(pk["gamma_h"]), gu.hb(pk["last_delta_h"]),
                      gu.hb(pk["gamma_abc_g"]), gu.hb(pk["deltas_h"]))
    deltas_g = gu.hb(pk["deltas_g"])
    ck = CommitterKey(deltas_g[-g1:].copy(), [gu.hb(c) for c in pk["ck"]])
    key = ProvingKey(vk, gu.hb(pk["beta_g"]), gu.hb(pk["a_g"]), gu.hb(pk["b_g"]), gu.hb(pk["b_h"]), gu.hb(pk["h_g"]), ck, deltas_g)
    return ProvingKeys("golden", b"", {0: key}, {0: 0})


def _arrays(pk):
    vk = pk.vk
    return [vk.alpha_g, vk.beta_h, vk.gamma_h, vk.last_delta_h, vk.gamma_abc_g, vk.deltas_h, pk.beta_g, pk.a_g, pk.b_g, pk.b_h,
            pk.h_g, pk.ck.last_delta_g] + list(pk.ck.deltas_abc_g) + [pk.deltas_g]


def _host(a):
    return a.to_host() if isinstance(a, capi.DeviceBuffer) else np.asarray(a, dtype=np.uint8)


def test_compressed_key_file_to_proof(cc):
    """The golden Groth16 key: serialize(compress=True), deserialize with a context - every array as it was; then again with
    the queries left on the device, hk_pk_upload from those device arrays, hk_prove: the golden proof bytes."""
    curve, ctx = cc
    case = gu.load("groth16.json")[curve][0]
    keys = _golden_keys(case)
    plain, dev = ArkCodec(curve), ArkCodec(curve, ctx)
    blob = keys.serialize(dev, compress=True)
    assert len(blob) < len(keys.serialize(plain)) * 0.55
    back = ProvingKeys.deserialize(dev, blob, compress=True, validate=True)
    want = _arrays(keys.get_pk(0))
    assert [a.tobytes() for a in _arrays(back.get_pk(0))] == [a.tobytes() for a in want]
    # a slice of the file through the mirror: the host writes what the device wrote
    assert plain.points_to_wire(1, want[4], compress=True) == dev.points_to_wire(1, want[4], compress=True)
    on_dev = ProvingKeys.deserialize(dev, blob, compress=True, device=True)
    pk = on_dev.get_pk(0)
    queries = [pk.a_g, pk.b_g, pk.b_h, pk.h_g, pk.deltas_g] + list(pk.ck.deltas_abc_g)
    assert all(isinstance(a, capi.DeviceBuffer) for a in queries)
    assert [_host(a).tobytes() for a in _arrays(pk)] == [a.tobytes() for a in want]
    dpk = ctx.pk_upload(a_g=pk.a_g, b_g=pk.b_g, b_h=pk.b_h, h_g=pk.h_g, ck_stages=pk.ck.deltas_abc_g, deltas_g=pk.deltas_g,
                        last_delta_h=pk.vk.last_delta_h, alpha_g=pk.vk.alpha_g, beta_g=pk.beta_g, beta_h=pk.vk.beta_h,
                        matrices=(gu.csr(case["A"]), gu.csr(case["B"]), gu.csr(case["C"])), n_inst=case["n_inst"],
                        n_constraints=case["n_constraints"])
    a, b, c = dpk.prove(gu.hb(case["z_mont"]), gu.hb(case["r_mont"]), gu.hb(case["s_mont"]), gu.hb(case["kappas_mont"]))
    assert (a.tobytes().hex(), b.tobytes().hex(), c.tobytes().hex()) == (case["proof"]["a"], case["proof"]["b"], case["proof"]["c"])
    dpk.free()
    for q in queries:
        q.free()
