"""CPU, no built library: the wrappers of capi that test_job_marshal_cpu.py, test_agg_scalars_cpu.py and
test_agg_verify_cpu.py do not cover, over a stub library that records what each entry is handed (the style of
test_job_marshal_cpu.py): every scalar and descriptor field arrives as given, every pointer is the operand's address or NULL,
a failing status frees exactly the DeviceBuffers the wrapper allocated - each once - and never a caller's.  Every expectation
is written from the call's own arguments.

Where a wrapper hands over the address of an EMPTY operand as it is (`_raw`) and where it hands over NULL (`_where`) is
pinned here wrapper by wrapper.  The last section holds the cases with no counterpart before the signature table and
DeviceBuffer.upload existed; everything above it holds for the wrappers as they were before."""
import ctypes as C
import random

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.endo import phi2, psi4

FR, FQ, G1, G2, GT = 32, 32, 64, 128, 384
HANDLE = "the-handle"
R = CURVE_PARAMS["bn254"]["r"]
PARAMS_DESCS = ((4, 5, 8, 56, 0), (3, 17, 8, 33, 272))


# ---- the stub library and the fake buffers -------------------------------------------------------------------------------
def _struct(s):
    """The fields of a structure: pointers as addresses (0 = NULL), nested descriptors as tuples / dicts, pointer arrays
    as they are (index them)."""
    out = {}
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is C.POINTER(capi.hk_poseidon_desc):
            v = tuple(getattr(v.contents, f) for f, _ in capi.hk_poseidon_desc._fields_) if v else None
        elif typ is C.POINTER(capi.hk_csr):
            v = _struct(v.contents) if v else None
        elif typ is C.c_void_p:
            v = v or 0
        out[name] = v
    return out


def _norm(a):
    """One argument of an entry as the tests compare it: NULL and None as 0, a c_void_p as its address, a ctypes array as a
    list, a byref() of a structure as the dict of its fields, a byref() of a plain value as the value's object."""
    if a is None:
        return 0
    if isinstance(a, (int, str)):
        return a
    if isinstance(a, C.c_void_p):
        return a.value or 0
    if isinstance(a, C.Array):
        return [v or 0 for v in a]
    obj = a._obj
    return _struct(obj) if isinstance(obj, C.Structure) else obj


class _StubLib:
    """Stands in for libhekaton.so under a capi.Context: records (entry, arguments, what `grab` read through them while the
    call was live) and returns `status`; `ref`: the value every size_t* / handle* output is given."""

    def __init__(self, status=capi.HK_OK, grab=None, ref=None):
        self.status, self.grab, self.ref, self.seen = status, grab, ref, []

    def __getattr__(self, name):
        if not name.startswith("hk_"):
            raise AttributeError(name)

        def fn(*args):
            a = [_norm(x) for x in args]
            for x in a:
                if isinstance(x, (C.c_size_t, C.c_void_p)) and self.ref is not None:
                    x.value = self.ref
            self.seen.append((name, a, self.grab(a) if self.grab else None))
            return self.status
        fn.__name__ = name
        return fn

    def hk_status_str(self, s):
        return b"HK_ERR_%d" % s


class _FakeBuffer:
    """Stands in for capi.DeviceBuffer: an address range nobody touches; every allocation and free is counted."""
    made = []

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes, self.ptr, self.frees = ctx, int(nbytes), 0x7f0000000000 + 0x100000 * (len(_FakeBuffer.made) + 1), 0
        _FakeBuffer.made.append(self)

    def free(self):
        self.frees += 1


@pytest.fixture
def fake_buffers(monkeypatch):
    monkeypatch.setattr(capi, "DeviceBuffer", _FakeBuffer)
    monkeypatch.setattr(capi, "_lib", _StubLib())                  # HekatonError's text, without a built library
    _FakeBuffer.made = []
    return _FakeBuffer


def _ctx(lib, curve="bn254"):
    ctx = capi.Context.__new__(capi.Context)
    ctx.lib, ctx.curve, ctx.handle = lib, curve, HANDLE
    ctx.fr_bytes, ctx.fq_bytes, ctx.g1_bytes, ctx.g2_bytes, ctx.gt_bytes = FR, FQ, G1, G2, GT
    return ctx


def _bytes(rnd, n):
    return np.frombuffer(bytes(rnd.getrandbits(8) for _ in range(n)), dtype=np.uint8).copy()


def _mk(rnd, ctx, resident):
    """n -> an operand of n bytes: host bytes, or a resident buffer."""
    return (lambda n: _FakeBuffer(ctx, n)) if resident else (lambda n: _bytes(rnd, n))


def _raw(x):
    """The address of input x as it is, an empty one's too; NULL for an absent one."""
    if x is None:
        return 0
    return x if isinstance(x, int) else x.ptr if isinstance(x, _FakeBuffer) else x.ctypes.data


def _where(x):
    """The address the library must be handed for input x where an empty one goes over as NULL."""
    if x is None:
        return 0
    if isinstance(x, _FakeBuffer):
        return x.ptr if x.nbytes else 0
    return x.ctypes.data if x.size else 0


def _mem(addr, n):
    return bytes(C.string_at(addr, n)) if n else b""


def _words(addr, n, dtype=np.uint32):
    return list(np.frombuffer(_mem(addr, n * np.dtype(dtype).itemsize), dtype=dtype))


def _refused(call, what):
    """`call(ctx)` over a library that answers HK_ERR_ARG: the error surfaces under the entry's name; returns the library."""
    lib = _StubLib(capi.HK_ERR_ARG)
    with pytest.raises(capi.HekatonError) as e:
        call(_ctx(lib))
    assert e.value.status == capi.HK_ERR_ARG and str(e.value).startswith(what + " failed")
    return lib


def _frees(fake_buffers):
    return [b.frees for b in fake_buffers.made]


def _is_host(x, size, dtype=np.uint8):
    return isinstance(x, np.ndarray) and x.dtype == dtype and x.size == size


# ---- MSM and sweeps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("resident", [False, True])
def test_msm(fake_buffers, group, resident):
    rnd = random.Random(21)
    lib = _StubLib()
    ctx = _ctx(lib)
    mk, pb, name = _mk(rnd, ctx, resident), (G1, G2)[group - 1], "hk_msm_g%d" % group
    for n in (0, 2):
        bases, scalars = mk(n * pb), mk(n * FR)
        fn = getattr(ctx, "msm_g%d" % group)
        if resident:
            out, flags = fn(bases, scalars, n_bases=n, n_scalars=n + 1, montgomery=False, checked=False), (n + 1, 0, 0)
        else:
            out, flags = fn(bases, scalars), (n, 1, 1)
        assert lib.seen[-1][:2] == (name, [HANDLE, _raw(bases), n, _raw(scalars), flags[0], flags[1], flags[2], out.ctypes.data])
        assert _is_host(out, pb)
    made = len(fake_buffers.made)
    _refused(lambda c: getattr(c, "msm_g%d" % group)(bases, scalars, 2, 2), name)
    assert len(fake_buffers.made) == made and not any(_frees(fake_buffers))


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("resident", [False, True])
def test_fixed_base_and_scalar_pairing(fake_buffers, group, resident):
    rnd = random.Random(22)
    lib = _StubLib()
    ctx = _ctx(lib)
    mk, pb = _mk(rnd, ctx, resident), (G1, G2)[group - 1]
    for n in (0, 2):
        base, points, scalars = mk(pb), mk(n * pb), mk(n * FR)
        res = ctx.fixed_base(group, base, scalars, n=n, montgomery=False) if resident else ctx.fixed_base(group, base, scalars)
        assert lib.seen[-1][:2] == ("hk_fixed_base_g%d" % group, [HANDLE, _raw(base), _raw(scalars), n, int(not resident), res.ctypes.data])
        assert _is_host(res, n * pb)
        res = ctx.scalar_pairing(group, points, scalars, n=n) if resident else ctx.scalar_pairing(group, points, scalars)
        assert lib.seen[-1][:2] == ("hk_scalar_pairing_g%d" % group, [HANDLE, _raw(points), _raw(scalars), n, res.ctypes.data])
        assert _is_host(res, n * pb)
        # out= given: filled and returned, whatever it is
        for out in (_FakeBuffer(ctx, n * pb), np.zeros(n * pb, np.uint8)):
            assert ctx.fixed_base(group, base, scalars, n=n, out=out) is out and lib.seen[-1][1][-1] == _raw(out)
            assert ctx.scalar_pairing(group, points, scalars, n=n, out=out) is out and lib.seen[-1][1][-1] == _raw(out)
    # a base given as a list of bytes is made an array
    lib.grab = lambda a: _mem(a[1], pb)
    ctx.fixed_base(group, list(range(pb)), scalars, n=2)
    assert lib.seen[-1][2] == bytes(range(pb))
    mine = _FakeBuffer(ctx, 2 * pb)
    made = len(fake_buffers.made)
    _refused(lambda c: c.fixed_base(group, base, scalars, n=2, out=mine), "hk_fixed_base_g%d" % group)
    _refused(lambda c: c.scalar_pairing(group, points, scalars, n=2, out=mine), "hk_scalar_pairing_g%d" % group)
    assert len(fake_buffers.made) == made and not any(_frees(fake_buffers))


# ---- GT and pairings --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_gt", [True, False])
@pytest.mark.parametrize("resident", [False, True])
def test_gt_pow_and_prod(fake_buffers, in_gt, resident):
    rnd = random.Random(23)
    lib = _StubLib()
    ctx = _ctx(lib)
    mk, name = _mk(rnd, ctx, resident), "hk_gt_pow" if in_gt else "hk_fq12_pow"
    for n in (0, 2, 4):
        gts, scalars = mk(n * GT), mk(n * FR)
        out = ctx.gt_pow(gts, scalars, in_gt=in_gt)
        assert lib.seen[-1][:2] == (name, [HANDLE, _raw(gts), _raw(scalars), n, out.ctypes.data])
        assert out.shape == (n, GT) and out.dtype == np.uint8
        out = ctx.gt_pow_prod(gts, scalars, 2, in_gt=in_gt)
        assert lib.seen[-1][:2] == ("hk_gt_pow_prod", [HANDLE, _raw(gts), _raw(scalars), n, 2, int(in_gt), out.ctypes.data])
        assert out.shape == (n // 2, GT) and out.dtype == np.uint8
    if not resident:                                                   # a (n, gt_bytes) array goes over as it lies
        g2d = gts.reshape(4, GT)
        ctx.gt_pow(g2d, scalars, in_gt=in_gt)
        assert lib.seen[-1][1][1:4] == [gts.ctypes.data, scalars.ctypes.data, 4]
    _refused(lambda c: c.gt_pow(gts, scalars, in_gt=in_gt), name)
    _refused(lambda c: c.gt_pow_prod(gts, scalars, 2, in_gt=in_gt), "hk_gt_pow_prod")
    assert not any(_frees(fake_buffers))


@pytest.mark.parametrize("resident", [False, True])
def test_multi_pairing_products_pairs(fake_buffers, resident):
    rnd = random.Random(24)
    lib = _StubLib()
    ctx = _ctx(lib)
    mk = _mk(rnd, ctx, resident)
    for n in (0, 2):
        g1, g2 = mk(n * G1), mk(n * G2)
        out = ctx.multi_pairing(g1, g2, n) if resident else ctx.multi_pairing(g1, g2)
        assert lib.seen[-1][:2] == ("hk_multi_pairing", [HANDLE, _raw(g1) if n else 0, _raw(g2) if n else 0, n, out.ctypes.data])
        assert _is_host(out, GT)
        lhs, rhs = [mk(n * G1), _bytes(rnd, n * G1)], [mk(n * G2), mk(n * G2), _bytes(rnd, n * G2)]
        out = ctx.pairing_products(lhs, rhs, n) if resident else ctx.pairing_products(lhs, rhs)
        assert lib.seen[-1][:2] == ("hk_pairing_products", [HANDLE, [_where(x) for x in lhs], 2, [_where(x) for x in rhs], 3, n,
                                                            out.ctypes.data])
        assert out.shape == (2, 3, GT) and out.dtype == np.uint8
        pairs = [(0, 1), (1, 0), (1, 2)]
        out = ctx.pairing_pairs(lhs, rhs, pairs, n) if resident else ctx.pairing_pairs(lhs, rhs, pairs)
        assert lib.seen[-1][:2] == ("hk_pairing_pairs", [HANDLE, [_where(x) for x in lhs], 2, [_where(x) for x in rhs], 3, [0, 1, 1],
                                                         [1, 0, 2], 3, n, out.ctypes.data])
        assert out.shape == (3, GT) and out.dtype == np.uint8
    # no vectors, no pairs: pointer arrays of one NULL, index arrays of nothing
    out = ctx.pairing_products([], [], 0)
    assert lib.seen[-1][1][1:6] == [[0], 0, [0], 0, 0] and out.shape == (0, 0, GT)
    out = ctx.pairing_pairs(lhs, rhs, [], 2)
    assert lib.seen[-1][1][5:9] == [[], [], 0, 2] and out.shape == (0, GT)
    _refused(lambda c: c.multi_pairing(g1, g2, 2), "hk_multi_pairing")
    _refused(lambda c: c.pairing_products(lhs, rhs, 2), "hk_pairing_products")
    _refused(lambda c: c.pairing_pairs(lhs, rhs, pairs, 2), "hk_pairing_pairs")
    assert not any(_frees(fake_buffers))


# ---- point operations -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("resident", [False, True])
def test_points_lincomb(fake_buffers, group, resident):
    rnd = random.Random(25)
    lib = _StubLib()
    ctx = _ctx(lib)
    mk, pb = _mk(rnd, ctx, resident), (G1, G2)[group - 1]
    for n in (0, 2):
        vecs, coeffs = [mk(n * pb), _bytes(rnd, n * pb), mk(n * pb)], mk(3 * FR)
        out = ctx.points_lincomb(group, vecs, coeffs, n) if resident else ctx.points_lincomb(group, vecs, coeffs)
        assert lib.seen[-1][:2] == ("hk_points_lincomb_g%d" % group, [HANDLE, [_where(x) for x in vecs], _raw(coeffs), 3, n,
                                                                       out.ctypes.data])
        assert _is_host(out, n * pb)
    _refused(lambda c: c.points_lincomb(group, vecs, coeffs, 2), "hk_points_lincomb_g%d" % group)
    assert not any(_frees(fake_buffers))


def _fold_parts(group, c):
    """The scalar c as the fold entries take it: the parts' magnitudes (Montgomery bytes) and the mask of the negative ones."""
    k = (phi2 if group == 1 else psi4)("bn254").decompose(c)
    return FrCodec("bn254").enc([abs(v) for v in k]).tobytes(), sum(1 << j for j, v in enumerate(k) if v < 0)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("resident", [False, True])
def test_points_fold_and_fold_many(fake_buffers, group, resident):
    rnd = random.Random(26)
    ctx = _ctx(None)
    mk, pb, parts = _mk(rnd, ctx, resident), (G1, G2)[group - 1], (2, 4)[group - 1]
    fold = getattr(ctx, "points_fold_g%d" % group)
    for n in (0, 2):
        c = rnd.randrange(R)
        mags, neg = _fold_parts(group, c)
        assert len(mags) == parts * FR
        lo, hi = mk(n * pb), mk(n * pb)
        lib = ctx.lib = _StubLib(grab=lambda a: _mem(a[3], parts * FR))
        res = fold(lo, hi, c, n) if resident else fold(lo, hi, c)
        name, a, seen_mags = lib.seen[-1]
        assert (name, a[:3], a[4:]) == ("hk_points_fold_g%d" % group, [HANDLE, _raw(lo), _raw(hi)], [neg, n, res.ctypes.data])
        assert seen_mags == mags and _is_host(res, n * pb)
        for out in (_FakeBuffer(ctx, n * pb), np.zeros(n * pb, np.uint8)):
            assert fold(lo, hi, c, n, out=out) is out and lib.seen[-1][1][-1] == _raw(out)
        # fold_many: up to four pairs, one scalar; the outputs are the caller's
        lib.grab = lambda a: _mem(a[4], parts * FR)
        los, his, outs = [mk(n * pb), _bytes(rnd, n * pb)], [_bytes(rnd, n * pb), mk(n * pb)], [mk(n * pb), _FakeBuffer(ctx, n * pb)]
        assert ctx.points_fold_many(group, los, his, c, n, outs) is outs
        name, a, seen_mags = lib.seen[-1]
        assert (name, a[:4], a[5:]) == ("hk_points_fold_many_g%d" % group, [HANDLE, 2, [_where(x) for x in los], [_where(x) for x in his]],
                                        [neg, n, [_where(x) for x in outs]])
        assert seen_mags == mags
    made = len(fake_buffers.made)
    _refused(lambda c_: getattr(c_, "points_fold_g%d" % group)(lo, hi, c, 2), "hk_points_fold_g%d" % group)
    _refused(lambda c_: c_.points_fold_many(group, los, his, c, 2, outs), "hk_points_fold_many_g%d" % group)
    assert len(fake_buffers.made) == made and not any(_frees(fake_buffers))


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("resident", [False, True])
def test_points_check_decompress_compress(fake_buffers, group, resident):
    rnd = random.Random(27)
    lib = _StubLib()
    ctx = _ctx(lib)
    mk, pb, xb = _mk(rnd, ctx, resident), (G1, G2)[group - 1], FQ * group
    for n in (0, 2):
        pts = mk(n * pb)
        ok = ctx.points_check(group, pts, n) if resident else ctx.points_check(group, pts)
        assert lib.seen[-1][:2] == ("hk_points_check_g%d" % group, [HANDLE, _raw(pts) if n else 0, n, ok.ctypes.data])
        assert _is_host(ok, n)
        x, flags = ctx.points_compress(group, pts)
        assert lib.seen[-1][:2] == ("hk_points_compress_g%d" % group, [HANDLE, _raw(pts) if n else 0, n, x.ctypes.data, flags.ctypes.data])
        assert _is_host(x, n * xb) and _is_host(flags, n)
        xc, fl = mk(n * xb), mk(n)
        for chk in (False, True):
            got, status = ctx.points_decompress(group, xc, fl, check=chk)
            assert lib.seen[-1][:2] == ("hk_points_decompress_g%d" % group, [HANDLE, _raw(xc) if n else 0, _raw(fl) if n else 0, n, int(chk),
                                                                             got.ctypes.data if n else 0, status.ctypes.data])
            assert _is_host(got, n * pb) and _is_host(status, n)
        for out in (_FakeBuffer(ctx, n * pb), np.zeros(n * pb, np.uint8)):
            got, status = ctx.points_decompress(group, xc, fl, out=out)
            assert got is out and lib.seen[-1][1][4:6] == [0, _raw(out) if n else 0]
    mine = _FakeBuffer(ctx, 2 * pb)
    made = len(fake_buffers.made)
    _refused(lambda c: c.points_check(group, pts, 2), "hk_points_check_g%d" % group)
    _refused(lambda c: c.points_compress(group, pts), "hk_points_compress_g%d" % group)
    _refused(lambda c: c.points_decompress(group, xc, fl, True, mine), "hk_points_decompress_g%d" % group)
    assert len(fake_buffers.made) == made and not any(_frees(fake_buffers))


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("resident", [False, True])
def test_field_sqrt(fake_buffers, which, resident):
    rnd = random.Random(28)
    lib = _StubLib()
    ctx = _ctx(lib)
    for n in (0, 2):
        data = _mk(rnd, ctx, resident)(n * FQ * which)
        out, ok = ctx.field_sqrt(which, data)
        assert lib.seen[-1][:2] == ("hk_field_sqrt", [HANDLE, which, _raw(data) if n else 0, n, out.ctypes.data, ok.ctypes.data])
        assert _is_host(out, n * FQ * which) and _is_host(ok, n)
    _refused(lambda c: c.field_sqrt(which, data), "hk_field_sqrt")
    assert not any(_frees(fake_buffers))


# ---- witness and assignment -------------------------------------------------------------------------------------------------
def test_assignment_from_bits(fake_buffers):
    rnd = random.Random(29)
    lib = _StubLib(grab=lambda a: (_mem(a[1], a[2]), _words(a[3], a[5]), _mem(a[4], a[5] * FR)))
    ctx = _ctx(lib)
    vals = _bytes(rnd, 2 * FR)
    buf = ctx.assignment_from_bits([1, 0, 1, 1, 0], [3, 1], vals)
    name, a, (bits, cols, seen_vals) = lib.seen[-1]
    assert [buf] == fake_buffers.made and buf.nbytes == 5 * FR
    assert (name, a[0], a[2], a[4:]) == ("hk_assignment_from_bits", HANDLE, 5, [vals.ctypes.data, 2, buf.ptr])
    assert (bits, cols, seen_vals) == (bytes([1, 0, 1, 1, 0]), [3, 1], vals.tobytes())
    # arrays of the entry's types go over as they lie; no full-width columns: both pointers NULL; out= is filled and returned
    bits, cols, mine = np.array([1, 1, 0], np.uint8), np.array([2], np.uint32), _FakeBuffer(ctx, 3 * FR)
    made = len(fake_buffers.made)
    assert ctx.assignment_from_bits(bits, cols, vals[:FR], out=mine) is mine
    assert lib.seen[-1][1] == [HANDLE, bits.ctypes.data, 3, cols.ctypes.data, vals.ctypes.data, 1, mine.ptr]
    assert ctx.assignment_from_bits(bits, [], np.zeros(0, np.uint8), out=mine) is mine
    assert lib.seen[-1][1] == [HANDLE, bits.ctypes.data, 3, 0, 0, 0, mine.ptr]
    ctx.assignment_from_bits(np.zeros(0, np.uint8), [], [], out=mine)
    assert lib.seen[-1][1][2:] == [0, 0, 0, 0, mine.ptr]
    _refused(lambda c: c.assignment_from_bits(bits, cols, vals[:FR], out=mine), "hk_assignment_from_bits")
    assert len(fake_buffers.made) == made and mine.frees == 0


@pytest.mark.parametrize("resident", [False, True])
def test_poseidon_path(fake_buffers, resident):
    rnd = random.Random(30)
    lib = _StubLib(grab=lambda a: _words(a[7], a[9]))
    ctx = _ctx(lib)
    mk = _mk(rnd, ctx, resident)
    batch, depth, index = 2, 3, [5, 1]
    consts, z = mk(404 * FR), _FakeBuffer(ctx, 1 << 16)
    leaf, sibs = mk(batch * 4 * FR), mk(batch * depth * FR)
    if not resident:
        leaf, sibs = leaf.reshape(batch, 4 * FR), sibs.reshape(batch, depth * FR)
    ctx.poseidon_path((consts, 404, *PARAMS_DESCS), leaf, sibs, index, 4096, 17, z)
    name, a, idx = lib.seen[-1]
    assert (name, a[:3], a[5:7], a[8:]) == ("hk_poseidon_path", [HANDLE, _raw(consts), 404], [_raw(leaf), _raw(sibs)],
                                            [depth, batch, 4096, 17, z.ptr])
    assert (tuple(a[3].values()), tuple(a[4].values()), idx) == (*PARAMS_DESCS, index)
    # a tree of one leaf has no siblings: NULL; a raw address for z_out
    sibs0 = mk(0) if resident else np.zeros((batch, 0), np.uint8)
    ctx.poseidon_path((consts, 404, *PARAMS_DESCS), leaf, sibs0, np.array(index, np.uint32), 4096, 17, 0x7e0000003000)
    a = lib.seen[-1][1]
    assert (a[5:7], a[8:]) == ([_raw(leaf), 0], [0, batch, 4096, 17, 0x7e0000003000])
    made = len(fake_buffers.made)
    _refused(lambda c: c.poseidon_path((consts, 404, *PARAMS_DESCS), leaf, sibs, index, 4096, 17, z), "hk_poseidon_path")
    assert len(fake_buffers.made) == made and not any(_frees(fake_buffers))


def test_wprog_upload_run_scatter(fake_buffers):
    rnd = random.Random(31)
    grab = lambda a: (_words(a[1], 8 * a[2]), _words(a[3], a[4]), _words(a[5], a[6]))
    lib = _StubLib(grab=grab, ref=0x77)
    ctx = _ctx(lib)
    ops, refs, vmap = [[0, 0, 0, 0, k, 0, 0, 0] for k in range(3)], [2, 0, 1, 1], [0, 33, 0xffffffff, 64, 1]
    wp = ctx.wprog_upload(ops, refs, vmap, 9, 3)
    name, a, (seen_ops, seen_refs, seen_map) = lib.seen[-1]
    assert (name, a[0], a[2], a[4], a[6:9]) == ("hk_wprog_upload", HANDLE, 3, 4, [5, 9, 3])
    assert (seen_ops, seen_refs, seen_map) == ([w for op in ops for w in op], refs, vmap)
    assert isinstance(wp, capi.WordProgram) and (wp.ctx, wp.handle.value, wp.n_v, wp.n_inputs) == (ctx, 0x77, 5, 3)
    ops, vmap = np.array(ops, np.uint32), np.array(vmap, np.uint32)                  # arrays of the entry's type; no refs: NULL
    ctx.wprog_upload(ops, [], vmap, 9, 3)
    assert lib.seen[-1][1][1:6] == [ops.ctypes.data, 3, 0, 0, vmap.ctypes.data]
    _refused(lambda c: c.wprog_upload(ops, refs, vmap, 9, 3), "hk_wprog_upload")

    # run: host inputs give the batch; a resident buffer of inputs needs batch=
    lib.grab, lib.ref = None, None
    wp = capi.WordProgram(ctx, "the-program", 5, 3)
    cols, vals = np.array([1, 4], np.uint32), _bytes(rnd, 2 * 2 * FR).reshape(2, 2 * FR)
    for inputs, batch in ((np.arange(6, dtype=np.uint32).reshape(2, 3), None), (_FakeBuffer(ctx, 4 * 2 * 3), 2),
                          (np.zeros((0, 3), np.uint32), None)):
        n = inputs.shape[0] if batch is None else batch
        made = len(fake_buffers.made)
        buf = wp.run(inputs, cols, vals, batch=batch)
        assert [buf] == fake_buffers.made[made:] and buf.nbytes == n * 5 * FR
        assert lib.seen[-1][:2] == ("hk_wprog_run", [HANDLE, "the-program", _raw(inputs), n, cols.ctypes.data, vals.ctypes.data, 2, buf.ptr])
    mine = _FakeBuffer(ctx, 2 * 5 * FR)
    made = len(fake_buffers.made)
    assert wp.run(inputs, [], [], out=mine) is mine and lib.seen[-1][1][4:] == [0, 0, 0, mine.ptr]
    lib.grab = lambda a: (_words(a[2], 6), _words(a[4], a[6]))
    wp.run([[1, 2, 3], [4, 5, 6]], [7], vals[:, :FR].copy(), out=mine)
    assert lib.seen[-1][2] == ([1, 2, 3, 4, 5, 6], [7]) and lib.seen[-1][1][3] == 2
    with pytest.raises(AssertionError):
        wp.run(_FakeBuffer(ctx, 24), cols, vals)
    with pytest.raises(AssertionError):
        wp.run(_FakeBuffer(ctx, 23), cols, vals, batch=2)
    made = len(fake_buffers.made)
    _refused(lambda c: capi.WordProgram(c, "the-program", 5, 3).run(inputs, cols, vals, out=mine), "hk_wprog_run")
    assert len(fake_buffers.made) == made and mine.frees == 0

    # scatter: the batch follows from the values; both addresses as they are, those of nothing too
    lib.grab = None
    assert wp.scatter(cols, vals, mine) is mine
    assert lib.seen[-1][:2] == ("hk_assignment_scatter", [HANDLE, cols.ctypes.data, vals.ctypes.data, 2, 2, 5, mine.ptr])
    c0, v0 = np.zeros(0, np.uint32), np.zeros(0, np.uint8)
    wp.scatter(c0, v0, mine)
    assert lib.seen[-1][1] == [HANDLE, c0.ctypes.data, v0.ctypes.data, 0, 0, 5, mine.ptr]
    _refused(lambda c: capi.WordProgram(c, "the-program", 5, 3).scatter(cols, vals, mine), "hk_assignment_scatter")
    assert mine.frees == 0


# ---- bases, field and NTT ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("resident", [False, True])
def test_bases_upload_and_msm(fake_buffers, group, resident):
    rnd = random.Random(32)
    lib = _StubLib(ref=0x99)
    ctx = _ctx(lib)
    mk, pb = _mk(rnd, ctx, resident), (G1, G2)[group - 1]
    for n in (0, 2):
        bases = mk(n * pb)
        rb = ctx.bases_upload(group, bases, n) if resident else ctx.bases_upload(group, bases)
        name, a, _ = lib.seen[-1]
        assert (name, a[:4]) == ("hk_bases_upload", [HANDLE, group, _raw(bases), n])
        assert isinstance(rb, capi.ResidentBases) and (rb.ctx, rb.handle.value, rb.group, rb.n) == (ctx, 0x99, group, n)
    _refused(lambda c: c.bases_upload(group, bases, 2), "hk_bases_upload")
    lib.ref = None
    rb = capi.ResidentBases(ctx, "the-bases", group, 2)
    for n in (0, 2):
        scalars = mk(n * FR)
        out = rb.msm(scalars, n + 1, montgomery=False, checked=False) if resident else rb.msm(scalars)
        want = [n + 1, 0, 0] if resident else [n, 1, 1]
        assert lib.seen[-1][:2] == ("hk_msm_bases", [HANDLE, "the-bases", _raw(scalars), *want, out.ctypes.data])
        assert _is_host(out, pb)
    _refused(lambda c: capi.ResidentBases(c, "the-bases", group, 2).msm(scalars, 2), "hk_msm_bases")
    assert not any(_frees(fake_buffers))


def test_field_convert_and_ntt(fake_buffers):
    rnd = random.Random(33)
    lib = _StubLib(grab=lambda a: _mem(a[2], a[4] * FR))
    ctx = _ctx(lib)
    for which in (0, 1):
        for n in (0, 2):
            data = _bytes(rnd, n * FR)
            for to_mont in (True, False):
                out = ctx.field_convert(which, data.reshape(n, FR), to_mont)
                assert lib.seen[-1][:2] == ("hk_field_convert", [HANDLE, which, data.ctypes.data, out.ctypes.data, n, int(to_mont)])
                assert _is_host(out, n * FR)
    ctx.field_convert(0, list(range(FR)), True)                        # anything array-like is made bytes
    assert lib.seen[-1][2] == bytes(range(FR)) and lib.seen[-1][1][4] == 1
    _refused(lambda c: c.field_convert(0, data, True), "hk_field_convert")
    lib.grab = None
    for data in (_bytes(rnd, 8 * FR), _FakeBuffer(ctx, 8 * FR)):
        assert ctx.ntt(data, 3) is data and lib.seen[-1][:2] == ("hk_ntt", [HANDLE, _raw(data), 3, 0, 0])
        assert ctx.ntt(data, 3, inverse=True, coset=True) is data and lib.seen[-1][1] == [HANDLE, _raw(data), 3, 1, 1]
    _refused(lambda c: c.ntt(data, 3), "hk_ntt")
    assert not any(_frees(fake_buffers))


# ---- QAP and keys -----------------------------------------------------------------------------------------------------------
def _matrices(rnd, n_rows, nnz, mk=None):
    """Three CSR triples of n_rows rows and nnz[k] entries in the entries' own types; `mk`: the values through it."""
    out = []
    for k in nnz:
        rp = np.array([0] * n_rows + [k], np.uint64)
        col = np.array([rnd.randrange(4) for _ in range(k)], np.uint32)
        out.append((rp, col, mk(k * FR) if mk else _bytes(rnd, k * FR)))
    return out


def _csr_fields(m, addr=_where):
    return dict(row_ptr=m[0].ctypes.data, col=addr(m[1]), val_mont=addr(m[2]), n_rows=len(m[0]) - 1, nnz=len(m[1]))


@pytest.mark.parametrize("resident", [False, True])
def test_witness_map(fake_buffers, resident):
    rnd = random.Random(34)
    lib = _StubLib(ref=8)
    ctx = _ctx(lib)
    ms = _matrices(rnd, 5, (3, 1, 2))
    z = _mk(rnd, ctx, resident)(4 * FR)
    out, m = ctx.witness_map(*ms, 2, 5, z, 4) if resident else ctx.witness_map(*ms, 2, 5, z)
    name, a, _ = lib.seen[-1]
    assert (name, a[0], a[4:10]) == ("hk_witness_map", HANDLE, [2, 5, _raw(z), 4, out.ctypes.data, 8])
    assert a[1:4] == [_csr_fields(x) for x in ms]
    assert _is_host(out, 8 * FR) and m == 8                             # the domain: 5 + 2 rounded up; m: what the entry wrote
    # matrices as plain lists are made arrays of the entry's types
    lib.grab = lambda a: [(_words(d["row_ptr"], d["n_rows"] + 1, np.uint64), _words(d["col"], d["nnz"]), _mem(d["val_mont"], d["nnz"] * FR))
                          for d in a[1:4]]
    ctx.witness_map(*[(list(rp), list(col), list(val)) for rp, col, val in ms], 2, 5, z, 4)
    assert lib.seen[-1][2] == [(list(rp), list(col), val.tobytes()) for rp, col, val in ms]
    assert [(d["n_rows"], d["nnz"]) for d in lib.seen[-1][1][1:4]] == [(5, 3), (5, 1), (5, 2)]
    _refused(lambda c: c.witness_map(*ms, 2, 5, z, 4), "hk_witness_map")
    assert not any(_frees(fake_buffers))


@pytest.mark.parametrize("resident", [False, True])
def test_qap_eval(fake_buffers, resident):
    rnd = random.Random(35)
    lib = _StubLib(grab=lambda a: _mem(a[7], FR), ref=8)
    ctx = _ctx(lib)
    mk = _mk(rnd, ctx, resident)
    ms = _matrices(rnd, 5, (3, 0, 2), mk)
    t = rnd.randrange(R)
    a_, b_, c_, zt, m = ctx.qap_eval(*ms, 2, 5, 4, t)
    name, a, seen_t = lib.seen[-1]
    assert (name, a[0], a[4:7], a[8:12]) == ("hk_qap_eval", HANDLE, [2, 5, 4], [a_.ctypes.data, b_.ctypes.data, c_.ctypes.data, zt.ctypes.data])
    assert a[1:4] == [_csr_fields(x) for x in ms] and seen_t == FrCodec("bn254").enc1(t).tobytes()
    assert all(_is_host(x, 4 * FR) for x in (a_, b_, c_)) and _is_host(zt, FR) and m == 8
    # t as its Montgomery bytes goes over as it is; out=: the caller's three buffers
    tb, mine = _bytes(rnd, FR), [_FakeBuffer(ctx, 4 * FR) for _ in range(3)]
    made = len(fake_buffers.made)
    got = ctx.qap_eval(*ms, 2, 5, 4, tb, out=mine)
    assert list(got[:3]) == mine and lib.seen[-1][1][7:11] == [tb.ctypes.data] + [x.ptr for x in mine]
    _refused(lambda c: c.qap_eval(*ms, 2, 5, 4, tb, out=mine), "hk_qap_eval")
    assert len(fake_buffers.made) == made and not any(_frees(fake_buffers))


KEYGEN_POINTS = ("a_g", "b_g", "b_h", "h_g", "deltas_g", "alpha_g", "beta_g", "gamma_abc_g", "beta_h", "gamma_h", "deltas_h")


def _keygen_grab(a):
    d = a[1]
    return (_words(d["stage_ranges"], 2 * d["n_stages"], np.uint64),
            [_mem(d[k], FR) for k in ("alpha", "beta", "gamma", "t", "g1_scalar", "g2_scalar")], _mem(d["deltas"], d["n_stages"] * FR))


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("with_qap", [False, True])
def test_keygen(fake_buffers, on_device, with_qap):
    rnd = random.Random(36)
    lib = _StubLib(grab=_keygen_grab, ref=4)
    ctx = _ctx(lib)
    enc = FrCodec("bn254")
    ms = _matrices(rnd, 2, (3, 0, 2))
    ranges = [(0, 1), (1, 3)]
    sc = {k: rnd.randrange(1, R) for k in ("alpha", "beta", "gamma", "t", "g1_scalar")}
    g2s = _bytes(rnd, FR)                                              # one scalar given as its Montgomery bytes
    deltas = [rnd.randrange(1, R), rnd.randrange(1, R)]
    kw = dict(matrices=ms, n_inst=1, n_constraints=2, n_v=4, stage_ranges=ranges, deltas=deltas, g2_scalar=g2s, **sc)
    res = ctx.keygen(on_device=on_device, with_qap=with_qap, **kw)
    name, a, (seen_ranges, seen_sc, seen_deltas) = lib.seen[-1]
    d, o = a[1], a[2]
    assert (name, a[0]) == ("hk_keygen", HANDLE)
    assert [d["A"], d["B"], d["C"]] == [_csr_fields(x) for x in ms]
    assert (d["n_inst"], d["n_constraints"], d["n_v"], d["n_stages"]) == (1, 2, 4, 2)
    assert seen_ranges == [0, 1, 1, 3] and seen_deltas == enc.enc(deltas).tobytes()
    assert seen_sc == [enc.enc1(sc[k]).tobytes() for k in ("alpha", "beta", "gamma", "t", "g1_scalar")] + [g2s.tobytes()]
    assert d["g2_scalar"] == g2s.ctypes.data
    # the outputs: m = 4 (2 + 1 rounded up), so 3 points of h_g; the four long ones on the device when asked
    sizes = dict(a_g=4 * G1, b_g=4 * G1, b_h=4 * G2, h_g=3 * G1, deltas_g=2 * G1, alpha_g=G1, beta_g=G1, gamma_abc_g=G1, beta_h=G2,
                 gamma_h=G2, deltas_h=2 * G2)
    for k in KEYGEN_POINTS:
        if on_device and k in KEYGEN_POINTS[:4]:
            assert isinstance(res[k], _FakeBuffer) and res[k].nbytes == sizes[k]
        else:
            assert _is_host(res[k], sizes[k])
        assert o[k] == _raw(res[k])
    assert [x.nbytes for x in fake_buffers.made] == ([sizes[k] for k in KEYGEN_POINTS[:4]] if on_device else [])
    assert [_is_host(x, n * G1) for x, n in zip(res["ck"], (1, 2))] == [True, True]
    assert [o["ck_stage"][k] for k in range(2)] == [x.ctypes.data for x in res["ck"]]
    if with_qap:
        assert _is_host(res["qap_abc"], 3 * 4 * FR) and o["qap_abc"] == res["qap_abc"].ctypes.data
    else:
        assert "qap_abc" not in res and o["qap_abc"] == 0
    assert res["m"] == 4 and set(res) == set(KEYGEN_POINTS) | {"ck", "m"} | ({"qap_abc"} if with_qap else set())
    assert not any(_frees(fake_buffers))
    # a failing status frees the device outputs of this call, each once - there are none on the host path
    made = len(fake_buffers.made)
    _refused(lambda c: c.keygen(on_device=on_device, with_qap=with_qap, **kw), "hk_keygen")
    assert _frees(fake_buffers) == [0] * made + [1] * (4 if on_device else 0)


def test_keygen_without_stages(fake_buffers):
    rnd = random.Random(37)
    lib = _StubLib(ref=1)
    ctx = _ctx(lib)
    ms = _matrices(rnd, 0, (0, 0, 0))
    res = ctx.keygen(matrices=ms, n_inst=1, n_constraints=0, n_v=1, stage_ranges=[], alpha=1, beta=2, gamma=3, deltas=[], t=4,
                     g1_scalar=5, g2_scalar=6)
    d, o = lib.seen[-1][1][1:3]
    assert (d["stage_ranges"], d["n_stages"], d["deltas"]) == (0, 0, 0)
    assert res["ck"] == [] and o["ck_stage"][0] is None                # a pointer array is never of length 0
    assert (o["h_g"], o["deltas_g"], o["deltas_h"]) == (0, 0, 0) and o["a_g"] == res["a_g"].ctypes.data      # m = 1: no h_g


def test_vk_prepare(fake_buffers):
    rnd = random.Random(38)
    lib = _StubLib(ref=0x55)
    ctx = _ctx(lib)
    arrs = [_bytes(rnd, n) for n in (G1, G2, G2, 3 * G2, 2 * G1)]
    names = ("alpha_g", "beta_h", "gamma_h", "deltas_h", "gamma_abc_g")
    vk = ctx.vk_prepare(**dict(zip(names, arrs)))
    name, a, _ = lib.seen[-1]
    assert (name, a[0]) == ("hk_vk_prepare", HANDLE)
    assert a[1] == dict(zip(names, [x.ctypes.data for x in arrs]), n_deltas=3, n_abc=2)
    assert isinstance(vk, capi.DeviceVk) and (vk.ctx, vk.handle.value, vk.n_deltas, vk.n_abc) == (ctx, 0x55, 3, 2)
    # a (n, bytes) array goes over flat; a length that is no whole number of points is refused before the library is asked
    ctx.vk_prepare(**dict(zip(names, arrs[:3] + [arrs[3].reshape(3, G2), arrs[4].reshape(2, G1)])))
    assert lib.seen[-1][1][1] == a[1]
    n_calls = len(lib.seen)
    for bad in ((0, G1 + 1), (1, G2 - 1), (2, 2 * G2), (3, 3 * G2 + 1), (4, G1 // 2)):
        broken = list(arrs)
        broken[bad[0]] = _bytes(rnd, bad[1])
        with pytest.raises(capi.HekatonError) as e:
            ctx.vk_prepare(**dict(zip(names, broken)))
        assert e.value.status == capi.HK_ERR_LEN and str(e.value).startswith("hk_vk_prepare failed")
    assert len(lib.seen) == n_calls
    _refused(lambda c: c.vk_prepare(**dict(zip(names, arrs))), "hk_vk_prepare")


PK_POINTS = ("a_g", "b_g", "b_h", "h_g")
PK_SMALL = ("deltas_g", "last_delta_h", "alpha_g", "beta_g", "beta_h")


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("with_matrices", [False, True])
def test_pk_upload(fake_buffers, resident, with_matrices):
    rnd = random.Random(39)
    lib = _StubLib(ref=0x66)
    ctx = _ctx(lib)
    mk = _mk(rnd, ctx, resident)
    big = dict(a_g=mk(4 * G1), b_g=mk(4 * G1), b_h=mk(4 * G2), h_g=mk(7 * G1))
    cks = [mk(1 * G1), _bytes(rnd, 2 * G1)]
    small = dict(zip(PK_SMALL, [mk(2 * G1), mk(G2), mk(G1), _bytes(rnd, G1), mk(G2)]))
    ms = _matrices(rnd, 5, (3, 1, 2))                                  # a key's matrices come from the host
    kw = dict(matrices=ms, n_inst=3, n_constraints=5) if with_matrices else {}
    made = len(fake_buffers.made)
    dpk = ctx.pk_upload(ck_stages=cks, **big, **small, **kw)
    name, a, _ = lib.seen[-1]
    d = a[1]
    assert (name, a[0]) == ("hk_pk_upload", HANDLE)
    assert [d[k] for k in PK_POINTS] == [_raw(big[k]) for k in PK_POINTS]
    assert (d["a_len"], d["b_g_len"], d["b_h_len"], d["h_len"]) == (4, 4, 4, 7)
    assert d["n_stages"] == 2 and [d["ck_stage"][k] for k in range(2)] == [_raw(x) for x in cks] and list(d["ck_len"][:2]) == [1, 2]
    assert [d[k] for k in PK_SMALL] == [_raw(small[k]) for k in PK_SMALL]
    if with_matrices:
        assert [d["A"], d["B"], d["C"]] == [_csr_fields(x, _raw) for x in ms] and (d["n_inst"], d["n_constraints"]) == (3, 5)
    else:
        assert [d["A"], d["B"], d["C"]] == [None] * 3 and (d["n_inst"], d["n_constraints"]) == (0, 0)
    assert isinstance(dpk, capi.DevicePk) and (dpk.ctx, dpk.handle.value) == (ctx, 0x66)
    # an empty query or stage goes over by its address, not as NULL
    h0, ck0 = mk(0), mk(0)
    ctx.pk_upload(ck_stages=[ck0], **dict(big, h_g=h0), **small)
    d = lib.seen[-1][1][1]
    assert (d["h_g"] or 0, d["h_len"], d["ck_stage"][0] or 0, d["ck_len"][0], d["n_stages"]) == (_raw(h0), 0, _raw(ck0), 0, 1)
    made = len(fake_buffers.made)
    _refused(lambda c: c.pk_upload(ck_stages=cks, **big, **small, **kw), "hk_pk_upload")
    assert len(fake_buffers.made) == made and not any(_frees(fake_buffers))


# ---- SHA, R1CS and VKD ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True])
def test_sha_tree(fake_buffers, resident):
    rnd = random.Random(40)
    lib = _StubLib()
    ctx = _ctx(lib)
    n, ns, k = 4, 2, 3
    leaves = _mk(rnd, ctx, resident)(n // 2 * 64)
    sizes = [32 * n, 2 * n * k * FR, FR]
    outs = ctx.sha_tree(leaves, n, ns, k)
    name, a, _ = lib.seen[-1]
    assert (name, a[:5]) == ("hk_sha_tree", [HANDLE, _raw(leaves), n, ns, k])
    assert list(a[5].values()) == [x.ctypes.data for x in outs] and [_is_host(x, s) for x, s in zip(outs, sizes)] == [True] * 3
    lib.grab = lambda a: _mem(a[1], 128)                                # leaves as a list of 64-byte blocks are joined
    blocks = [bytes(rnd.getrandbits(8) for _ in range(64)) for _ in range(2)]
    ctx.sha_tree(blocks, n, ns, k)
    assert lib.seen[-1][2] == b"".join(blocks)
    lib.grab = None
    empty = _mk(rnd, ctx, resident)(0)                                   # no subcircuits: the address of nothing, as it is
    outs = ctx.sha_tree(empty, 0, ns, k)
    assert lib.seen[-1][1][:5] == [HANDLE, _raw(empty), 0, ns, k] and [x.size for x in outs] == [0, 0, FR]
    made = len(fake_buffers.made)
    outs = ctx.sha_tree(leaves, n, ns, k, device_out=True)
    assert list(outs) == fake_buffers.made[made:] and [x.nbytes for x in outs] == sizes
    assert list(lib.seen[-1][1][5].values()) == [x.ptr for x in outs] and not any(_frees(fake_buffers))
    made = len(fake_buffers.made)
    _refused(lambda c: c.sha_tree(leaves, n, ns, k, device_out=True), "hk_sha_tree")
    assert _frees(fake_buffers) == [0] * made + [1] * 3
    _refused(lambda c: c.sha_tree(leaves, n, ns, k), "hk_sha_tree")
    assert len(fake_buffers.made) == made + 3


@pytest.mark.parametrize("resident", [False, True])
def test_sha_tree_inputs(fake_buffers, resident):
    rnd = random.Random(41)
    lib = _StubLib(grab=lambda a: _words(a[5], a[6]))
    ctx = _ctx(lib)
    mk = _mk(rnd, ctx, resident)
    leaves, digests, sub = mk(4 * 64), mk(8 * 32), [3, 0, 3]
    out = ctx.sha_tree_inputs(leaves, None, 8, 16, sub)
    name, a, seen_sub = lib.seen[-1]
    assert (name, a[:5], a[6:]) == ("hk_sha_tree_inputs", [HANDLE, _raw(leaves), 0, 8, 16], [3, out.ctypes.data])
    assert seen_sub == sub and out.shape == (3, 16) and out.dtype == np.uint32
    out = ctx.sha_tree_inputs(None, digests, 8, 54, [])
    a = lib.seen[-1][1]
    assert a == [HANDLE, 0, _raw(digests), 8, 54, 0, 0, out.ctypes.data] and out.shape == (0, 54)      # no rows: a NULL sub_index
    made = len(fake_buffers.made)
    out = ctx.sha_tree_inputs(leaves, digests, 8, 54, np.array(sub, np.uint32), device_out=True)
    assert [out] == fake_buffers.made[made:] and out.nbytes == 4 * 3 * 54 and lib.seen[-1][1][7] == out.ptr
    made = len(fake_buffers.made)
    _refused(lambda c: c.sha_tree_inputs(leaves, digests, 8, 54, sub, device_out=True), "hk_sha_tree_inputs")
    assert _frees(fake_buffers) == [0] * made + [1]
    _refused(lambda c: c.sha_tree_inputs(leaves, digests, 8, 54, sub), "hk_sha_tree_inputs")
    assert len(fake_buffers.made) == made + 1


R1CS_TABLES = dict(n_parts=2, n_txs=3, slot_offsets=[0, 2, 5], slot_rank=[0, 1, 1, 0, 2], slot_src=[4, 0xffffffff, 1, 2, 9],
                   sets_per_tx=3, tx_len=10, tx_stride=10, wit_offsets=[0, 4, 10], body_len=[2, 3])
R1CS_TABLE_LEN = dict(slot_offsets=3, slot_rank=5, slot_src=5, wit_offsets=3, body_len=2)


@pytest.mark.parametrize("resident", [False, True])
def test_r1cs_job_witness(fake_buffers, resident):
    rnd = random.Random(42)
    lib = _StubLib(grab=lambda a: ({k: _words(a[1][k], n) for k, n in R1CS_TABLE_LEN.items()}, _words(a[2], a[3])))
    ctx = _ctx(lib)
    t, sub = R1CS_TABLES, [2, 2, 0]
    wit, z = _mk(rnd, ctx, resident)(30 * FR), _FakeBuffer(ctx, 1 << 16)
    assert ctx.r1cs_job_witness(t, wit, sub, 4096, 9, z) is z
    name, a, (tables, seen_sub) = lib.seen[-1]
    d = a[1]
    assert (name, a[0], a[3:]) == ("hk_r1cs_job_witness", HANDLE, [3, 4096, 9, z.ptr]) and seen_sub == sub
    assert {k: d[k] for k in ("n_parts", "n_txs", "sets_per_tx", "tx_len", "tx_stride")} == \
        {k: t[k] for k in ("n_parts", "n_txs", "sets_per_tx", "tx_len", "tx_stride")}
    assert tables == {k: t[k] for k in R1CS_TABLE_LEN} and d["witness_mont"] == _raw(wit)
    lib.grab = None                                                    # no rows: a NULL sub_index; a raw address for z_out
    assert ctx.r1cs_job_witness(t, wit, [], 4096, 9, 0x7e0000004000) == 0x7e0000004000
    assert lib.seen[-1][1][2:] == [0, 0, 4096, 9, 0x7e0000004000]
    made = len(fake_buffers.made)
    _refused(lambda c: c.r1cs_job_witness(t, wit, sub, 4096, 9, z), "hk_r1cs_job_witness")
    assert len(fake_buffers.made) == made and not any(_frees(fake_buffers))


def _vkd_tables(rnd, mk):
    return dict(depth=16, split=2, n_updates=2, kinds=[0, 1], slot_addr=[1, 2, 3, 4, 5, 6, 7], slot_src=[0, 1, 2, 0xffffffff, 4, 5, 6],
                leaves=mk(2 * 2 * 66), siblings=mk(2 * 16 * FR), roots=_bytes(rnd, 2 * FR))


@pytest.mark.parametrize("resident", [False, True])
def test_vkd_witness(fake_buffers, resident):
    rnd = random.Random(43)
    lib = _StubLib(grab=lambda a: ({k: _words(a[1][k], n) for k, n in (("kinds", 2), ("slot_addr", 7), ("slot_src", 7))}, _words(a[2], a[3])))
    ctx = _ctx(lib)
    mk = _mk(rnd, ctx, resident)
    t, consts, values, sub = _vkd_tables(rnd, mk), mk(404 * FR), mk(19 * FR), [1, 0, 1]
    z = _FakeBuffer(ctx, 1 << 16)
    assert ctx.vkd_witness(t, (consts, 404, *PARAMS_DESCS), values, sub, 4096, (1, 40, 300, 310), z) is z
    name, a, (tables, seen_sub) = lib.seen[-1]
    d = a[1]
    assert (name, a[0], a[3:5], a[6]) == ("hk_vkd_witness", HANDLE, [3, 4096], z.ptr) and seen_sub == sub
    assert a[5] == dict(kind=1, hash_col0=40, index_col0=300, path_col0=310)
    assert (d["depth"], d["split"], d["n_updates"], d["n_slots"]) == (16, 2, 2, 7)
    assert tables == {k: t[k] for k in ("kinds", "slot_addr", "slot_src")}
    assert (d["leaves"], d["siblings_mont"], d["consts_mont"], d["roots_mont"], d["values_mont"]) == \
        (_where(t["leaves"]), _where(t["siblings"]), _where(consts), t["roots"].ctypes.data, _where(values))
    assert (d["n_consts"], d["leaf_hash"], d["node_hash"]) == (404, *PARAMS_DESCS)
    lib.grab = None                                                    # the columns as a ready hk_vkd_cols; no rows; no output
    cols = capi.hk_vkd_cols(0, 41, 301, 311)
    assert ctx.vkd_witness(t, (consts, 404, *PARAMS_DESCS), values, [], 4096, cols, None) is None
    a = lib.seen[-1][1]
    assert (a[2:5], a[5], a[6]) == ([0, 0, 4096], dict(kind=0, hash_col0=41, index_col0=301, path_col0=311), 0)
    assert ctx.vkd_witness(t, (consts, 404, *PARAMS_DESCS), values, sub, 4096, cols, 0x7e0000005000) == 0x7e0000005000
    assert lib.seen[-1][1][6] == 0x7e0000005000
    made = len(fake_buffers.made)
    _refused(lambda c: c.vkd_witness(t, (consts, 404, *PARAMS_DESCS), values, sub, 4096, cols, z), "hk_vkd_witness")
    assert len(fake_buffers.made) == made and not any(_frees(fake_buffers))


@pytest.mark.parametrize("resident", [False, True])
def test_vkd_tree(fake_buffers, resident):
    rnd = random.Random(44)
    lib = _StubLib(grab=lambda a: _words(a[1]["kinds"], a[1]["n_updates"]))
    ctx = _ctx(lib)
    mk = _mk(rnd, ctx, resident)
    leaves0, leaves, consts, kinds = mk(3 * 66), mk(2 * 2 * 66), mk(404 * FR), [0, 1]
    sizes = [2 * 16 * FR, 2 * FR, 2]
    outs = ctx.vkd_tree(16, leaves0, kinds, leaves, (consts, 404, *PARAMS_DESCS))
    name, a, seen_kinds = lib.seen[-1]
    d = a[1]
    assert (name, a[0], a[2:]) == ("hk_vkd_tree", HANDLE, [x.ctypes.data for x in outs]) and seen_kinds == kinds
    assert (d["depth"], d["n_leaves0"], d["leaves0"], d["n_updates"], d["leaves"], d["consts_mont"], d["n_consts"]) == \
        (16, 3, _raw(leaves0), 2, _raw(leaves), _raw(consts), 404)
    assert (d["leaf_hash"], d["node_hash"]) == PARAMS_DESCS
    assert isinstance(outs, tuple) and [_is_host(x, s) for x, s in zip(outs, sizes)] == [True] * 3
    # an empty directory - None, no bytes, an empty buffer - is NULL with M = 0; no updates: every table NULL
    for nothing in (None, b"", mk(0)):
        ctx.vkd_tree(16, nothing, kinds, leaves, (consts, 404, *PARAMS_DESCS))
        d = lib.seen[-1][1][1]
        assert (d["n_leaves0"], d["leaves0"]) == (0, 0)
    outs = ctx.vkd_tree(16, leaves0, [], mk(0), (consts, 404, *PARAMS_DESCS))
    d = lib.seen[-1][1][1]
    assert (d["n_updates"], d["kinds"], d["leaves"]) == (0, 0, 0) and [x.size for x in outs] == [0, 2 * FR, 0]
    if not resident:                                                   # bytes are read where they lie
        lib.grab = lambda a: (_mem(a[1]["leaves0"], 3 * 66), _mem(a[1]["leaves"], 4 * 66))
        ctx.vkd_tree(16, leaves0.tobytes(), kinds, bytearray(leaves.tobytes()), (consts, 404, *PARAMS_DESCS))
        assert lib.seen[-1][2] == (leaves0.tobytes(), leaves.tobytes()) and lib.seen[-1][1][1]["n_leaves0"] == 3
        lib.grab = None
    made = len(fake_buffers.made)
    outs = ctx.vkd_tree(16, leaves0, kinds, leaves, (consts, 404, *PARAMS_DESCS), device_out=True)
    assert list(outs) == fake_buffers.made[made:] and [x.nbytes for x in outs] == sizes
    assert lib.seen[-1][1][2:] == [x.ptr for x in outs] and not any(_frees(fake_buffers))
    made = len(fake_buffers.made)
    _refused(lambda c: c.vkd_tree(16, leaves0, kinds, leaves, (consts, 404, *PARAMS_DESCS), device_out=True), "hk_vkd_tree")
    assert _frees(fake_buffers) == [0] * made + [1] * 3
    # a caller's triple, the third None for no status: filled, returned, never freed
    mine = (_FakeBuffer(ctx, sizes[0]), np.zeros(sizes[1], np.uint8), None)
    made, frees = len(fake_buffers.made), _frees(fake_buffers)
    for dev in (False, True):
        lib2 = _refused(lambda c: c.vkd_tree(16, leaves0, kinds, leaves, (consts, 404, *PARAMS_DESCS), device_out=dev, out=mine), "hk_vkd_tree")
        assert lib2.seen[-1][1][2:] == [mine[0].ptr, mine[1].ctypes.data, 0]
    assert len(fake_buffers.made) == made and _frees(fake_buffers) == frees
    assert ctx.vkd_tree(16, leaves0, kinds, leaves, (consts, 404, *PARAMS_DESCS), out=mine) == mine


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("through_key", [False, True])
def test_r1cs_check(fake_buffers, resident, through_key):
    rnd = random.Random(45)
    lib = _StubLib()
    ctx = _ctx(lib)
    mk = _mk(rnd, ctx, resident)
    ms = _matrices(rnd, 5, (3, 0, 2), mk)
    if through_key:
        dpk = capi.DevicePk(ctx, "the-key")
        call, name, head, skip = dpk.r1cs_check, "hk_pk_r1cs_check", [HANDLE, "the-key"], 2
    else:
        call, name, head, skip = (lambda *a, **kw: ctx.r1cs_check(*ms, *a, **kw)), "hk_r1cs_check", [HANDLE] + [_csr_fields(x) for x in ms], 4
    z = mk(2 * 4 * FR)
    res = call(z, batch=2)                                             # n_v from the buffer's size; no rows asked for
    a = lib.seen[-1][1]
    assert (lib.seen[-1][0], a[:skip], a[skip:skip + 3], a[skip + 4:]) == (name, head, [_raw(z), 4, 2], [0, 0, 0]) and a[skip + 3] != 0
    assert res == [(0, None), (0, None)]
    res, rows = call(z if resident else z.reshape(2, 4 * FR), n_v=4, batch=2, cap=3)
    a = lib.seen[-1][1]
    assert a[skip:skip + 3] == [_raw(z), 4, 2] and a[skip + 4:] == [rows.ctypes.data, 0, 3]
    assert res == [(0, None)] * 2 and rows.shape == (2, 3) and rows.dtype == np.uint32
    res, rows, vals = call(z, batch=2, cap=3, want_vals=True)
    assert lib.seen[-1][1][skip + 4:] == [rows.ctypes.data, vals.ctypes.data, 3]
    assert vals.shape == (2, 3, 3 * FR) and vals.dtype == np.uint8
    assert call(z, n_v=4, batch=0) == []                               # no assignments: z and the verdicts NULL
    assert lib.seen[-1][1][skip:] == [0, 4, 0, 0, 0, 0, 0]
    assert call(z, batch=1) == [(0, None)] and lib.seen[-1][1][skip + 1] == 8
    made = len(fake_buffers.made)
    _refused(lambda c: (capi.DevicePk(c, "the-key").r1cs_check(z, batch=2) if through_key else c.r1cs_check(*ms, z, batch=2)), name)
    assert len(fake_buffers.made) == made and not any(_frees(fake_buffers))


def test_r1cs_check_reads_what_the_entry_wrote(fake_buffers):
    """The verdicts are read back from the array the entry was handed."""
    class Lib(_StubLib):
        def hk_pk_r1cs_check(self, ctx, pk, z, n_v, batch, verdicts, rows, vals, cap):
            (C.c_uint32 * 4).from_address(_norm(verdicts))[:] = [0, 0, 2, 7]
            return capi.HK_OK
    ctx = _ctx(Lib())
    assert capi.DevicePk(ctx, "the-key").r1cs_check(np.zeros(2 * 4 * FR, np.uint8), batch=2) == [(0, None), (2, 7)]


# ---- key handles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True])
def test_device_vk_verify(fake_buffers, resident):
    rnd = random.Random(46)
    lib = _StubLib()
    ctx = _ctx(lib)
    mk = _mk(rnd, ctx, resident)
    vk = capi.DeviceVk(ctx, "the-vk", 2, 3)                            # one commitment and two inputs per proof
    for n in (0, 2):
        ops = [mk(n * G1), mk(n * G2), mk(n * G1), mk(n * G1), mk(n * 2 * FR)]
        out = vk.verify(*ops)
        assert lib.seen[-1][:2] == ("hk_verify_batch", [HANDLE, "the-vk"] + [_where(x) for x in ops] +
                                    [n, capi.HK_VERIFY_CHECK_POINTS, 0, out.ctypes.data])
        assert _is_host(out, n)
    out = vk.verify(*ops, n=2, check_points=False)
    assert lib.seen[-1][1][7:] == [2, 0, 0, out.ctypes.data]
    # batch mode: the r_i go over as they lie; the verdicts may stay on the device
    rand, verdicts = np.full(2 * FR, 3, np.uint8), _FakeBuffer(ctx, 2)
    made = len(fake_buffers.made)
    assert vk.verify(*ops, rand=rand, verdicts=verdicts) is verdicts
    assert lib.seen[-1][1][7:] == [2, capi.HK_VERIFY_CHECK_POINTS, rand.ctypes.data, verdicts.ptr]
    if not resident:                                                   # rows of points as 2-d arrays
        vk.verify(ops[0].reshape(2, G1), ops[1].reshape(2, G2), ops[2], ops[3], ops[4].reshape(2, 2 * FR), rand=rand.reshape(2, FR))
        assert lib.seen[-1][1][2:10] == [_raw(x) for x in ops] + [2, capi.HK_VERIFY_CHECK_POINTS, rand.ctypes.data]
    # a key with no commitments and no inputs: ds and inputs may be None, and go over as NULL
    bare = capi.DeviceVk(ctx, "the-vk", 1, 1)
    bare.verify(ops[0], ops[1], ops[2], None, None)
    assert lib.seen[-1][1][2:8] == [_raw(ops[0]), _raw(ops[1]), _raw(ops[2]), 0, 0, 2]
    # lengths that do not match n proofs of this key, a zero r_i: refused before the library is asked
    n_calls = len(lib.seen)
    for k in range(5):
        broken = list(ops)
        broken[k] = mk(ops[k].nbytes + (G1 if k != 4 else FR))
        with pytest.raises(capi.HekatonError) as e:
            vk.verify(*broken, n=2)
        assert e.value.status == capi.HK_ERR_LEN and str(e.value).startswith("hk_verify_batch failed")
    with pytest.raises(capi.HekatonError):
        vk.verify(*ops, rand=rand[:FR])
    with pytest.raises(capi.HekatonError):
        vk.verify(ops[0], ops[1], ops[2], None, ops[4])
    with pytest.raises(ValueError):
        vk.verify(*ops, rand=np.concatenate([rand[:FR], np.zeros(FR, np.uint8)]))
    assert len(lib.seen) == n_calls
    _refused(lambda c: capi.DeviceVk(c, "the-vk", 2, 3).verify(*ops, verdicts=verdicts), "hk_verify_batch")
    assert len(fake_buffers.made) == made + 5 * resident and not any(_frees(fake_buffers))
    out = vk.alpha_beta()
    assert lib.seen[-1][:2] == ("hk_vk_alpha_beta", ["the-vk", out.ctypes.data]) and _is_host(out, GT)
    _refused(lambda c: capi.DeviceVk(c, "the-vk", 2, 3).alpha_beta(), "hk_vk_alpha_beta")


@pytest.mark.parametrize("resident", [False, True])
def test_device_pk_commit_and_prove(fake_buffers, resident):
    rnd = random.Random(47)
    lib = _StubLib()
    ctx = _ctx(lib)
    mk = _mk(rnd, ctx, resident)
    dpk = capi.DevicePk(ctx, "the-key")
    for n in (0, 2):
        w, kappa = mk(n * FR), _bytes(rnd, FR)
        out = dpk.commit(1, w, kappa, n) if resident else dpk.commit(1, w, kappa)
        assert lib.seen[-1][:2] == ("hk_commit", [HANDLE, "the-key", 1, _raw(w) if n else 0, n, kappa.ctypes.data, out.ctypes.data])
        assert _is_host(out, G1)
        rows, kappas = mk(3 * n * FR), _bytes(rnd, 3 * FR)
        out = dpk.commit_batch(0, rows, kappas, n, 3)
        assert lib.seen[-1][:2] == ("hk_commit_batch", [HANDLE, "the-key", 0, _raw(rows) if n else 0, n, kappas.ctypes.data, 3, out.ctypes.data])
        assert out.shape == (3, G1) and out.dtype == np.uint8
    _refused(lambda c: capi.DevicePk(c, "the-key").commit(1, w, kappa, 2), "hk_commit")
    _refused(lambda c: capi.DevicePk(c, "the-key").commit_batch(0, rows, kappas, 2, 3), "hk_commit_batch")

    z, r, s = mk(4 * FR), _bytes(rnd, FR), _bytes(rnd, FR)
    for nk in (0, 2):
        kap = _bytes(rnd, nk * FR)
        a_, b_, c_ = dpk.prove(z, r, s, kap, 4) if resident else dpk.prove(z, r, s, kap)
        assert lib.seen[-1][:2] == ("hk_prove", [HANDLE, "the-key", _raw(z), 4, r.ctypes.data, s.ctypes.data, _where(kap), nk,
                                                 a_.ctypes.data, b_.ctypes.data, c_.ctypes.data])
        assert _is_host(a_, G1) and _is_host(b_, G2) and _is_host(c_, G1)
    lib.grab = lambda a: (_mem(a[4], FR), _mem(a[5], FR))              # blinders given as lists of bytes are made arrays
    dpk.prove(z, list(r), list(s), kap, 4)
    assert lib.seen[-1][2] == (r.tobytes(), s.tobytes())
    lib.grab = None
    for batch in (0, 3):
        zs, rs, ss = mk(batch * 4 * FR), _bytes(rnd, batch * FR), _bytes(rnd, batch * FR)
        for nk in (0, 2):
            kap = _bytes(rnd, batch * nk * FR)
            a_, b_, c_ = dpk.prove_batch(zs, rs.reshape(batch, FR), ss, kap.reshape(batch, nk * FR), 4, batch)
            assert lib.seen[-1][:2] == ("hk_prove_batch", [HANDLE, "the-key", _raw(zs), 4, rs.ctypes.data, ss.ctypes.data, _where(kap),
                                                           nk if batch else 0, batch, a_.ctypes.data, b_.ctypes.data, c_.ctypes.data])
            assert (a_.shape, b_.shape, c_.shape) == ((batch, G1), (batch, G2), (batch, G1))
    _refused(lambda c: capi.DevicePk(c, "the-key").prove(z, r, s, kap[:2 * FR], 4), "hk_prove")
    _refused(lambda c: capi.DevicePk(c, "the-key").prove_batch(zs, rs, ss, kap, 4, 3), "hk_prove_batch")
    assert not any(_frees(fake_buffers))


# ---- what has no counterpart before the signature table and DeviceBuffer.upload --------------------------------------------
@pytest.mark.parametrize("resident", [False, True])
def test_empty_matrix_members_go_over_as_null(fake_buffers, resident):
    """witness_map and pk_upload build their hk_csr through the shared _csrs like qap_eval, keygen and r1cs_check: the col /
    val of a matrix without entries are NULL (they used to be the addresses of the empty arrays).  The entries read neither
    at nnz = 0: csr_host_ok asks for them only `if nnz`, hk_pk_upload copies them only `if nnz`, R1csStage stages 0 bytes."""
    rnd = random.Random(48)
    lib = _StubLib(ref=8)
    ctx = _ctx(lib)
    mk = _mk(rnd, ctx, resident)
    ms = _matrices(rnd, 5, (3, 0, 2))
    ctx.witness_map(*ms, 2, 5, mk(4 * FR), 4)
    assert lib.seen[-1][1][1:4] == [_csr_fields(x) for x in ms] and lib.seen[-1][1][2]["col"] == lib.seen[-1][1][2]["val_mont"] == 0
    pts = dict(a_g=mk(4 * G1), b_g=mk(4 * G1), b_h=mk(4 * G2), h_g=mk(7 * G1), ck_stages=[], deltas_g=mk(0), last_delta_h=mk(G2),
               alpha_g=mk(G1), beta_g=mk(G1), beta_h=mk(G2))
    ctx.pk_upload(matrices=ms, n_inst=3, n_constraints=5, **pts)
    d = lib.seen[-1][1][1]
    assert [d["A"], d["B"], d["C"]] == [_csr_fields(x) for x in ms] and d["B"]["col"] == d["B"]["val_mont"] == 0


def test_device_buffer_upload(monkeypatch):
    """DeviceBuffer.upload: hk_dev_upload of a contiguous array into this allocation; from_host allocates and uses it."""
    lib = _StubLib(ref=0x7d0000000000)
    monkeypatch.setattr(capi, "_lib", lib)
    ctx = _ctx(lib)
    src = np.arange(24, dtype=np.uint32)
    buf = capi.DeviceBuffer.from_host(ctx, src)
    assert [s[0] for s in lib.seen] == ["hk_dev_alloc", "hk_dev_upload"] and (buf.ptr, buf.nbytes) == (0x7d0000000000, 96)
    assert lib.seen[0][1][:2] == [HANDLE, 96] and lib.seen[1][1] == [HANDLE, buf.ptr, src.ctypes.data, 96]
    lib.grab = lambda a: _mem(a[2], a[3])
    assert buf.upload(src[::2]) is buf                                 # a strided view is made contiguous first
    assert lib.seen[-1][1][1::2] == [buf.ptr, 48] and lib.seen[-1][2] == src[::2].tobytes()
    win = buf.view(32, 64)                                             # a window uploads into its own range
    win.upload(src[:16])
    assert lib.seen[-1][1][:2] + lib.seen[-1][1][3:] == [HANDLE, buf.ptr + 32, 64]
    with pytest.raises(AssertionError):
        win.upload(src)                                                # more than the allocation holds
    lib.status = capi.HK_ERR_DEVICE
    with pytest.raises(capi.HekatonError) as e:
        buf.upload(src)
    assert str(e.value).startswith("hk_dev_upload failed")
