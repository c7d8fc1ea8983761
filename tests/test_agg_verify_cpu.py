"""CPU: the aggregate verifier's pieces without a device - hk_class_power_sums is declared, listed and exported, and
Context.class_power_sums hands the library what include/hekaton.h says (a stub library records it); the HK_HD chunk body of
csrc/class_sums.cuh, compiled for the host and run chunk by chunk in the kernels' shape (tests/host_shim/class_sums_shim.cpp),
gives the Python mirror's bytes on every case of the GPU test; the same source as a stand-alone program runs clean under
-fsanitize=address,undefined with the digests of the plain build; AggProof and AggVerifyingKey round-trip through their wire
forms and refuse what they must; the mirror satisfies the identities of a geometric sum."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

from hekaton_system_amd import agg_verify as av, capi
from hekaton_system_amd.aggregation import IppCom
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.gt import GtField
from oracle.pyref import curve as pycurve
from oracle.pyref.codec import Codec
from oracle.pyref.params import CURVES as PARAMS
from tests import class_sums_cases as cases
from tests import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_SRC = "class_sums_shim.cpp"  # under tests/host_shim


def test_symbol_declared_listed_exported():
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    declared = set(re.findall(r"\b(hk_[a-z0-9_]+)\s*\(", hdr))
    assert "hk_class_power_sums" in declared and "hk_class_power_sums" in capi.EXPORTS
    if os.path.exists(capi.LIB_PATH):
        getattr(capi.load(), "hk_class_power_sums")


# ---- the Context wrapper over a stub library ----------------------------------------------------------------------------
def _addr(p):
    if p is None:
        return 0
    return p if isinstance(p, int) else (p.value or 0)


class _StubLib:
    """Stands in for libhekaton.so under a capi.Context: copies what the entry is handed, writes a pattern to a host output
    and returns `status`."""

    def __init__(self, status=capi.HK_OK, host_in=True, host_out=True):
        self.status, self.host_in, self.host_out, self.seen = status, host_in, host_out, []

    def hk_class_power_sums(self, handle, x, class_of, n, n_classes, out):
        self.seen.append(dict(handle=handle, x=bytes(C.string_at(_addr(x), 32)), class_of=_addr(class_of), n=n, n_classes=n_classes,
                              ids=bytes(C.string_at(_addr(class_of), 4 * n)) if self.host_in else None, out=_addr(out)))
        if self.host_out:
            C.memset(_addr(out), 0x5a, n_classes * 32)
        return self.status


def _stub_context(curve, lib):
    ctx = capi.Context.__new__(capi.Context)
    ctx.lib, ctx.curve, ctx.handle, ctx.fr_bytes = lib, curve, "the-handle", 32
    return ctx


@pytest.mark.parametrize("curve", cases.CURVES)
def test_context_wrapper_marshals_its_arguments(curve):
    fc = FrCodec(curve)
    x = random.Random(7).randrange(CURVE_PARAMS[curve]["r"])
    ids = [0, 4, 4, 1, 3, 2, 0, 0, 4]
    lib = _StubLib()
    ctx = _stub_context(curve, lib)
    for given in (ids, np.array(ids, np.uint32), np.array(ids, np.int64)):            # anything array-like becomes uint32
        out = ctx.class_power_sums(x, given, 5)
        s = lib.seen[-1]
        assert (s["handle"], s["x"], s["n"], s["n_classes"]) == ("the-handle", fc.enc1(x).tobytes(), 9, 5)
        assert s["ids"] == np.array(ids, "<u4").tobytes() and s["class_of"] != 0
        assert out.dtype == np.uint8 and out.size == 5 * 32 and (out == 0x5a).all() and s["out"] == out.ctypes.data
    # a caller's host output is filled and returned as it is
    mine = np.zeros(5 * 32, np.uint8)
    assert ctx.class_power_sums(x, ids, 5, out=mine) is mine and (mine == 0x5a).all()
    # no subcircuits: n = 0 and still a pointer
    out = ctx.class_power_sums(x, np.zeros(0, np.uint32), 3)
    assert (lib.seen[-1]["n"], lib.seen[-1]["n_classes"]) == (0, 3) and lib.seen[-1]["class_of"] != 0 and out.size == 3 * 32
    # device operands are handed over by their addresses, the output left in place and returned as it is
    dev_lib = _StubLib(host_in=False, host_out=False)
    dctx = _stub_context(curve, dev_lib)
    cls_d, out_d = capi.DeviceView(dctx, 0x7f0000001000, 13 * 4), capi.DeviceView(dctx, 0x7f0000002000, 5 * 32)
    assert dctx.class_power_sums(x, cls_d, 5, out=out_d) is out_d
    s = dev_lib.seen[-1]
    assert (s["class_of"], s["n"], s["n_classes"], s["out"]) == (0x7f0000001000, 13, 5, 0x7f0000002000)
    # mixed: host ids, device output
    mix = _StubLib(host_out=False)
    assert _stub_context(curve, mix).class_power_sums(x, ids, 5, out=out_d) is out_d and mix.seen[-1]["ids"] is not None
    # a refusal surfaces as HekatonError with the library's status
    with pytest.raises(capi.HekatonError) as e:
        _stub_context(curve, _StubLib(capi.HK_ERR_ARG)).class_power_sums(x, ids, 5)
    assert e.value.status == capi.HK_ERR_ARG


# ---- the chunk body on the host -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """csrc/class_sums.cuh compiled for the host (g++) - the source the kernels run."""
    out = str(tmp_path_factory.mktemp("shim") / "class_sums_shim.so")
    host_build.build(SHIM_SRC, out, "-O2", *host_build.SHARED)
    lib = host_build.load(out)
    lib.shim_class_power_sums.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    lib.shim_class_power_sums.restype = C.c_int
    return lib


@pytest.mark.parametrize("n", cases.SIZES + [cases.STRIDE_SIZE])
@pytest.mark.parametrize("curve", cases.CURVES)
def test_host_chunks_match_the_mirror(shim, curve, n):
    fc = FrCodec(curve)
    for nc, kind, base_kind in cases.case_list(n):
        x, cls, want = cases.case(curve, n, nc, kind, base_kind)
        out = np.full(nc * 32, 0xee, np.uint8)
        rc = shim.shim_class_power_sums(cases.CURVES.index(curve), fc.enc1(x).ctypes.data, cls.ctypes.data, n, nc, out.ctypes.data)
        assert rc == 0 and out.tobytes() == want, (n, nc, kind, base_kind)


@pytest.mark.parametrize("curve", cases.CURVES)
def test_host_chunks_refuse_a_class_out_of_range(shim, curve):
    fc = FrCodec(curve)
    n, nc = 4097, 5
    for at in (0, n - 1, 2048 + 1000):
        cls = cases.class_map("random", n, nc, 3).copy()
        cls[at] = nc
        out = np.full(nc * 32, 0xee, np.uint8)
        assert shim.shim_class_power_sums(cases.CURVES.index(curve), fc.enc1(5).ctypes.data, cls.ctypes.data, n, nc, out.ctypes.data) == 1
        assert (out == 0xee).all(), at
        with pytest.raises(ValueError):
            av.class_power_sums_host(5, cls.tolist(), nc, fc.r)


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """The shim's own main over a handful of the sizes, every buffer exactly as long as the entry says: built plain and with
    -fsanitize=address,undefined, both exit 0, the sanitized run reports nothing and prints the digests of the plain one."""
    outs = []
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("class_sums_" + tag))
        host_build.build(SHIM_SRC, exe, "-DCLASS_SUMS_MAIN", *flags)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (tag, r.stderr[-2000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].splitlines()
    assert len(lines) == 2 * 2 * 8 and "bls12_381 sums n=65537 classes=5 rc=0" in outs[0]
    assert all(l.endswith("rc=1 same=1") for l in lines if " refused " in l) and sum(" refused " in l for l in lines) == 16


# ---- the mirror ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", cases.CURVES)
def test_mirror_identities(curve):
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(41)
    for n, nc in ((1, 1), (9, 2), (64, 5), (1000, 17)):
        cls = cases.class_map("random", n, nc, n).tolist()
        x = rnd.randrange(2, r)
        # all classes together: the geometric sum (x^n - 1) / (x - 1)
        assert sum(av.class_power_sums_host(x, cls, nc, r)) % r == (pow(x, n, r) - 1) * pow(x - 1, -1, r) % r
        assert av.class_power_sums_host(1, cls, nc, r) == [cls.count(c) for c in range(nc)]
        assert av.class_power_sums_host(0, cls, nc, r) == [1 if c == cls[0] else 0 for c in range(nc)]
    assert av.class_power_sums_host(3, [], 4, r) == [0, 0, 0, 0]


# ---- wire forms ---------------------------------------------------------------------------------------------------------
class _Synth:
    """Synthetic members: random Fq12 values for the GT slots, generator multiples for the points."""

    def __init__(self, curve, seed):
        self.curve, self.cp, self.F, self.rnd = curve, PARAMS[curve], GtField(curve), random.Random(seed)
        self.cd, self.G1, self.G2 = Codec(self.cp), pycurve.G1(self.cp), pycurve.G2(self.cp)

    def gt(self):
        return tuple(self.rnd.randrange(self.F.q) for _ in range(12))

    def com(self, ip=False):
        return IppCom(self.F, self.gt(), self.gt(), self.gt() if ip else None)

    def g1(self):
        return np.frombuffer(self.cd.g1(self.G1.mul(self.cp.g1_gen, self.rnd.randrange(1, 1 << 20))), np.uint8).copy()

    def g2(self):
        return np.frombuffer(self.cd.g2(self.G2.mul(self.cp.g2_gen, self.rnd.randrange(1, 1 << 20))), np.uint8).copy()

    def proof(self, n=8, rounds=None):
        rounds = n.bit_length() - 1 if rounds is None else rounds
        tipp = dict(rounds=[{k: self.gt() for k in ("TL", "UL", "ZL", "TR", "UR", "ZR")} for _ in range(rounds)],
                    final_a=self.g1(), final_b=self.g2(), final_v=(self.g2(), self.g2()), final_w=(self.g1(), self.g1()),
                    open_v=(self.g2(), self.g2()), open_w=(self.g1(), self.g1()))
        return av.AggProof(self.curve, n, self.com(ip=True), self.com(), [[self.gt() for _ in range(4)] for _ in range(4)], tipp)

    def key(self, class_of, n_s=4):
        n = len(class_of)
        vk = dict(n=n, g=self.g1(), h=self.g2(), g_alpha=self.g1(), g_beta=self.g1(), h_alpha=self.g2(), h_beta=self.g2())
        return av.AggVerifyingKey(self.curve, n, n_s, vk, [self.com() for _ in range(n_s)], self.com(), self.com(), self.com(),
                                  class_of, [self.gt() for _ in range(max(class_of) + 1)])


def _same_com(a, b):
    return (a.t, a.u, a.ip) == (b.t, b.u, b.ip)


@pytest.mark.parametrize("curve", cases.CURVES)
def test_proof_round_trips_and_refuses(curve):
    sy = _Synth(curve, 5)
    p = sy.proof()
    data = p.serialize()
    q = av.AggProof.deserialize(None, curve, data)
    assert q.n == 8 and _same_com(q.com_ab, p.com_ab) and _same_com(q.com_c, p.com_c) and q.cross_terms == p.cross_terms
    assert q.tipp["rounds"] == p.tipp["rounds"] and len(q.tipp["rounds"]) == 3
    for key in ("final_a", "final_b", "final_v", "final_w", "open_v", "open_w"):
        assert np.array_equal(np.concatenate([np.ravel(x) for x in np.atleast_2d(q.tipp[key])]),
                              np.concatenate([np.ravel(x) for x in np.atleast_2d(p.tipp[key])])), key
    assert isinstance(q.tipp["final_v"], tuple) and q.tipp["final_v"][1].size == sy.cd.g2_bytes
    assert q.serialize() == data
    # the transcript form of the cross terms is the one inside the proof
    assert av.cross_terms_bytes(sy.F, p.cross_terms) in data
    fq = sy.F.nb
    with pytest.raises(ValueError):
        av.AggProof.deserialize(None, curve, data[:-1])                               # a length that does not match
    with pytest.raises(ValueError):
        av.AggProof.deserialize(None, curve, data[:100])
    with pytest.raises(ValueError):
        av.AggProof.deserialize(None, curve, data + b"\0")                            # trailing bytes
    for off in (8, 8 + 11 * fq, 8 + 5 * 12 * fq + 16 + 3 * fq):                       # com_ab.t's first and last Fq, a cross term
        bad = bytearray(data)
        bad[off:off + fq] = sy.F.q.to_bytes(fq, "little")                            # q itself: not canonical
        with pytest.raises(ValueError):
            av.AggProof.deserialize(None, curve, bytes(bad))
    for rounds in (2, 4):                                                             # not log2 8
        with pytest.raises(ValueError, match="rounds"):
            av.AggProof.deserialize(None, curve, sy.proof(8, rounds).serialize())
    bad = bytearray(data)
    bad[0:8] = (6).to_bytes(8, "little")                                              # n not a power of two
    with pytest.raises(ValueError):
        av.AggProof.deserialize(None, curve, bytes(bad))
    bad = bytearray(data)
    bad[8 + 5 * 12 * fq:8 + 5 * 12 * fq + 8] = (5).to_bytes(8, "little")              # five rows of cross terms
    with pytest.raises(ValueError):
        av.AggProof.deserialize(None, curve, bytes(bad))
    # a point's coordinate that is not reduced (the last byte of the proof is inside open_w's last coordinate)
    bad = bytearray(data)
    if curve == "bn254":
        bad[-fq:] = sy.F.q.to_bytes(fq, "little")
    else:
        bad[-fq:] = sy.F.q.to_bytes(fq, "big")
    with pytest.raises(ValueError):
        av.AggProof.deserialize(None, curve, bytes(bad))


@pytest.mark.parametrize("class_of,runs", [
    ([0] * 8, [(0, 8)]),                                                              # one class
    ([0, 1] * 4, [(0, 1), (1, 1)] * 4),                                               # alternating
    ([0, 0, 0, 1, 1, 2, 2, 3], [(0, 3), (1, 2), (2, 2), (3, 1)]),                     # the last run has length 1
])
@pytest.mark.parametrize("curve", cases.CURVES)
def test_key_round_trips_with_its_class_runs(curve, class_of, runs):
    sy = _Synth(curve, 6)
    k = sy.key(class_of)
    assert av.class_runs(k.class_of) == runs
    data = k.serialize()
    j = av.AggVerifyingKey.deserialize(None, curve, data)
    assert (j.curve, j.n, j.n_s) == (curve, 8, 4) and j.class_of.dtype == np.uint32 and j.class_of.tolist() == class_of
    assert j.alpha_beta == k.alpha_beta and j.tipp_vk["n"] == 8
    for key in ("g", "h", "g_alpha", "g_beta", "h_alpha", "h_beta"):
        assert np.array_equal(j.tipp_vk[key], k.tipp_vk[key]), key
    for a, b in zip(j.com_s + [j.com_h, j.com_delta0, j.com_delta1], k.com_s + [k.com_h, k.com_delta0, k.com_delta1]):
        assert _same_com(a, b)
    assert j.serialize() == data
    # the run-length form is what is on the wire: (class, run length) as u64 pairs behind their count
    packed = len(runs).to_bytes(8, "little") + b"".join(c.to_bytes(8, "little") + l.to_bytes(8, "little") for c, l in runs)
    assert packed in data


@pytest.mark.parametrize("curve", cases.CURVES)
def test_key_refusals(curve):
    sy = _Synth(curve, 8)
    k = sy.key([0, 0, 0, 1, 1, 2, 2, 3])
    data = k.serialize()
    fq = sy.F.nb
    for bad in (data[:-1], data + b"\0", data[:40]):
        with pytest.raises(ValueError):
            av.AggVerifyingKey.deserialize(None, curve, bad)
    at = data.index((4).to_bytes(8, "little") + (0).to_bytes(8, "little") + (3).to_bytes(8, "little"))   # the runs
    for off, val in ((at + 16, 4),          # the first run one longer: the runs cover 9 subcircuits
                     (at + 16, 0),          # an empty run
                     (at + 8, 4),           # a class id that is not below the class count
                     (at, 3)):              # one run fewer: what follows no longer parses to the end
        bad = bytearray(data)
        bad[off:off + 8] = val.to_bytes(8, "little")
        with pytest.raises(ValueError):
            av.AggVerifyingKey.deserialize(None, curve, bytes(bad))
    bad = bytearray(data)
    bad[-fq:] = sy.F.q.to_bytes(fq, "little")                                         # the last alpha_beta's last Fq
    with pytest.raises(ValueError):
        av.AggVerifyingKey.deserialize(None, curve, bytes(bad))
    bad = bytearray(data)
    bad[8:16] = (5).to_bytes(8, "little")                                             # n_s without as many com_s
    with pytest.raises(ValueError):
        av.AggVerifyingKey.deserialize(None, curve, bytes(bad))


def test_verdict_is_truthy_when_accepted():
    assert av.AggVerdict(True, av.ACCEPTED) and not av.AggVerdict(False, av.R_PRODUCT)
    assert av.AggVerdict(False, av.R_TIPP).reason == "tipp"


def test_lincomb_takes_in_gt_and_defaults_to_the_split_chain():
    """IppCom.lincomb hands in_gt to hk_gt_pow_prod: True unless the caller says otherwise."""
    F = GtField("bn254")

    class Ctx:
        curve, gt_bytes = "bn254", 12 * 32

        def __init__(self):
            self.flags = []

        def gt_pow_prod(self, gts, scalars, group_len, in_gt=True):
            self.flags.append(in_gt)
            return np.tile(np.frombuffer(F.encode(F.one), np.uint8), (gts.size // self.gt_bytes // group_len, 1))

    ctx = Ctx()
    a, b = IppCom(F, F.one, F.one, ctx=ctx), IppCom(F, F.one, F.one, ctx=ctx)
    IppCom.lincomb([(a, None), (b, 5)])
    IppCom.lincomb([(a, None), (b, 5)], in_gt=False)
    IppCom.lincomb([(a, None), (b, 5)], in_gt=True)
    assert ctx.flags == [True, False, True]
