"""GPU: hk_class_power_sums against the Python mirror, byte for byte (tests/class_sums_cases.py: the sizes at every chunk /
workgroup / stride edge of csrc/class_sums.cuh, the class counts on both sides of a class group and at the cap, seven class
maps, five bases), with class_of and sums_out on the host, on the device and mixed and a guard behind every output; the
refusals of the header comment, each leaving a sentinel pattern untouched; n == 0."""
import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import FrCodec
from tests import class_sums_cases as cases

pytestmark = pytest.mark.gpu

GUARD = 64                   # bytes behind every output that must keep their pattern
PATTERN = 0xEE
PLACES = [("host", "host"), ("device", "device"), ("host", "device"), ("device", "host")]      # class_of, sums_out


@pytest.fixture
def ctx_of(ctx_bn254, ctx_bls):
    return {"bn254": ctx_bn254, "bls12_381": ctx_bls}


class _Out:
    """A host and a device output of `nbytes` + GUARD, patterned before every call."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.pattern = np.full(nbytes + GUARD, PATTERN, np.uint8)
        self.dev = capi.DeviceBuffer.from_host(ctx, self.pattern)

    def at(self, place):
        if place == "host":
            return self.pattern.copy()
        capi.check(capi.load().hk_dev_upload(self.ctx.handle, self.dev.ptr, self.pattern.ctypes.data, self.pattern.nbytes), "hk_dev_upload")
        return self.dev

    def check(self, got, want, what):
        got = got.to_host() if isinstance(got, capi.DeviceBuffer) else got
        assert got[:self.nbytes].tobytes() == want, what
        assert (got[self.nbytes:] == PATTERN).all(), ("wrote past the end", what)


@pytest.mark.parametrize("n", cases.SIZES + [cases.STRIDE_SIZE])
@pytest.mark.parametrize("curve", cases.CURVES)
def test_class_sums_match_the_mirror(curve, n, ctx_of):
    ctx = ctx_of[curve]
    outs = {nc: _Out(ctx, nc * 32) for nc in cases.CLASS_COUNTS}
    try:
        for k, (nc, kind, base_kind) in enumerate(cases.case_list(n)):
            x, cls, want = cases.case(curve, n, nc, kind, base_kind)
            cls_d = capi.DeviceBuffer.from_host(ctx, cls)
            try:
                # every placement of the two buffers on the first case, one in turn on the others
                for in_at, out_at in (PLACES if k == 0 else [PLACES[k % 4]]):
                    got = ctx.class_power_sums(x, cls if in_at == "host" else cls_d, nc, out=outs[nc].at(out_at))
                    outs[nc].check(got, want, (n, nc, kind, base_kind, in_at, out_at))
            finally:
                cls_d.free()
        nc, kind, base_kind = cases.case_list(n)[0]
        x, cls, want = cases.case(curve, n, nc, kind, base_kind)
        assert ctx.class_power_sums(x, cls, nc).tobytes() == want                     # the wrapper's own buffer
    finally:
        for o in outs.values():
            o.dev.free()


@pytest.mark.parametrize("curve", cases.CURVES)
def test_no_subcircuits_gives_zeros(curve, ctx_of):
    ctx = ctx_of[curve]
    out = _Out(ctx, 5 * 32)
    try:
        for place in ("host", "device"):
            out.check(ctx.class_power_sums(7, np.zeros(0, np.uint32), 5, out=out.at(place)), bytes(5 * 32), place)
    finally:
        out.dev.free()


@pytest.mark.parametrize("curve", cases.CURVES)
def test_refusals_leave_the_output_untouched(curve, ctx_of):
    ctx = ctx_of[curve]
    lib = capi.load()
    fc = FrCodec(curve)
    x = fc.enc1(3)
    n, nc = 65537, 5
    good = cases.class_map("random", n, nc, 1)
    out = _Out(ctx, 1024 * 32)
    up = lambda a: capi.DeviceBuffer.from_host(ctx, a)
    bufs = []
    try:
        def refused(cls, n_, nc_, what, x_=x):
            """On every placement: HK_ERR_ARG and the sentinel as it was.  cls: a uint32 array, or None for a null pointer."""
            cls_d = None
            if cls is not None:
                cls_d = up(cls)
                bufs.append(cls_d)
            for in_at, out_at in PLACES:
                o = out.at(out_at)
                cp = None if cls is None else (cls.ctypes.data if in_at == "host" else cls_d.ptr)
                op = o.ctypes.data if out_at == "host" else o.ptr
                status = lib.hk_class_power_sums(ctx.handle, None if x_ is None else x_.ctypes.data, cp, n_, nc_, op)
                assert status == capi.HK_ERR_ARG, (what, in_at, out_at, status)
                out.check(o, bytes([PATTERN]) * (1024 * 32), (what, in_at, out_at))
        refused(good, n, nc, "null x", x_=None)
        refused(None, n, nc, "null class_of")
        refused(good, (1 << 27) + 1, nc, "n > 2^27")                                  # refused before class_of is read
        refused(good, n, 0, "no classes")
        refused(good, n, 1025, "n_classes > 1024")
        # an id out of range: at index 0, at n - 1, in the middle of a late workgroup (the 30th of 33), equal to n_classes and
        # far above it
        for at, bad in ((0, nc), (n - 1, nc), (29 * 2048 + 1000, nc), (29 * 2048 + 1001, 0xFFFFFFFF)):
            cls = good.copy()
            cls[at] = bad
            refused(cls, n, nc, ("class id", at, bad))
        cls = np.array([0, 1, 9, 3], np.uint32)                                       # 9 is in the second class group's range
        refused(cls, 4, 9, "class id == n_classes past the first group")
        assert lib.hk_class_power_sums(ctx.handle, x.ctypes.data, good.ctypes.data, n, nc, None) == capi.HK_ERR_ARG
        assert lib.hk_class_power_sums(None, x.ctypes.data, good.ctypes.data, n, nc, out.at("host").ctypes.data) == capi.HK_ERR_ARG
        # and the same arguments with every id in range are taken
        got = ctx.class_power_sums(3, good, nc)
        assert got.tobytes() == fc.enc(cases.class_power_sums_host(3, good.tolist(), nc, fc.r)).tobytes()
    finally:
        for b in bufs:
            b.free()
        out.dev.free()


@pytest.mark.parametrize("curve", cases.CURVES)
def test_sums_feed_gt_pow_prod_where_they_lie(curve, ctx_of):
    """What verify_aggregate does with them: the Montgomery bytes are hk_gt_pow_prod's exponents as they are."""
    from hekaton_system_amd.cp_groth16 import CURVE_PARAMS
    from hekaton_system_amd.gt import GtField
    ctx, F, fc = ctx_of[curve], GtField(curve), FrCodec(curve)
    p = CURVE_PARAMS[curve]
    e = ctx.multi_pairing(fc.g1(p["g1"]), fc.g2(p["g2"]), 1)                          # a GT element
    cls = np.array([0, 1, 1, 0, 2], np.uint32)
    x = 5
    sums = ctx.class_power_sums(x, cls, 3)
    assert fc.dec(sums) == [1 + 125, 5 + 25, 625]
    got = ctx.gt_pow_prod(np.concatenate([e, e, e]), sums, 3)
    want = ctx.gt_pow(e.reshape(1, -1), fc.enc1(1 + 5 + 25 + 125 + 625))
    assert F.decode(got[0]) == F.decode(want[0])
