"""CPU: the ABI surface of hk_trace_sort / hk_stage0_witness and their host wrappers, without a device - the symbols are
declared, listed and exported; Context.trace_sort and Context.stage0_witness hand the library what include/hekaton.h says (a
stub library records it); transcript.sort_subtraces_by_addr_device over a stub context that sorts with numpy returns the
lists of the pinned host mirror; ShaMerkleJob without a context and Stage1Device without `traces=` are the code they were."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from hekaton_system_amd import capi, sha_circuit, transcript
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.poseidon import device_params
from hekaton_system_amd.sha_circuit import ShaMerkleJob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hk_trace_sort", "hk_stage0_witness")


def test_symbols_declared_listed_exported():
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    declared = set(re.findall(r"\b(hk_[a-z0-9_]+)\s*\(", hdr))
    for sym in NEW:
        assert sym in declared and sym in capi.EXPORTS
    assert "stays with the caller" not in hdr                      # the sentence under hk_exec_tree points at hk_trace_sort now
    if os.path.exists(capi.LIB_PATH):
        lib = capi.load()
        for sym in NEW:
            getattr(lib, sym)


def _val(p):
    return p.value if isinstance(p, C.c_void_p) else p


class _StubLib:
    """Stands in for libhekaton.so under a capi.Context: records what the two calls are handed, writes a pattern to every
    output and returns `status`."""

    def __init__(self, status=capi.HK_OK):
        self.status, self.seen = status, None

    def hk_trace_sort(self, handle, k, src, n, out, perm):
        src, out, perm = _val(src), _val(out), _val(perm)
        self.seen = dict(handle=handle, k=k, n=n, src=bytes(C.string_at(src, n * k * 32)) if src else None, out=out, perm=perm)
        if out:
            C.memset(out, 0x21, n * k * 32)
        if perm:
            C.memset(perm, 0x22, 4 * n)
        return self.status

    def hk_stage0_witness(self, handle, offsets, n_sub, n_portals, time_e, addr_e, sub_index, batch, w_out):
        off = list(np.ctypeslib.as_array(C.cast(offsets, C.POINTER(C.c_uint32)), (n_sub + 1,)))
        sub = list(np.ctypeslib.as_array(C.cast(sub_index, C.POINTER(C.c_uint32)), (batch,))) if sub_index else None
        self.seen = dict(handle=handle, offsets=off, n_sub=n_sub, n_portals=n_portals,
                         time=bytes(C.string_at(_val(time_e), off[-1] * 64)), addr=bytes(C.string_at(_val(addr_e), off[-1] * 64)),
                         sub_index=sub, batch=batch, w_out=_val(w_out))
        return self.status


def _stub_context(curve, lib):
    ctx = capi.Context.__new__(capi.Context)
    ctx.lib, ctx.curve, ctx.handle, ctx.fr_bytes = lib, curve, "the-handle", 32
    return ctx


@pytest.mark.parametrize("k", [2, 4])
def test_context_trace_sort_marshals_its_arguments(k):
    rnd = random.Random(k)
    n = 7
    time_b = np.frombuffer(bytes(rnd.randrange(256) for _ in range(n * k * 32)), np.uint8)
    lib = _StubLib()
    out = _stub_context("bn254", lib).trace_sort(k, time_b)
    s = lib.seen
    assert (s["handle"], s["k"], s["n"], s["src"]) == ("the-handle", k, n, time_b.tobytes())       # n from the buffer's size
    assert s["perm"] is None                                       # not wanted: a NULL perm_out
    assert isinstance(out, np.ndarray) and out.size == n * k * 32 and s["out"] == out.ctypes.data and (out == 0x21).all()
    # with the permutation: a uint32 array the library wrote to; an explicit count of fewer entries than the buffer holds
    lib = _StubLib()
    out, perm = _stub_context("bn254", lib).trace_sort(k, time_b, n_entries=5, want_perm=True)
    s = lib.seen
    assert s["n"] == 5 and s["src"] == time_b.tobytes()[:5 * k * 32]
    assert out.size == 5 * k * 32 and perm.dtype == np.uint32 and perm.size == 5 and s["perm"] == perm.ctypes.data
    assert (perm == 0x22222222).all()
    # nothing to sort: NULL pointers, empty results
    lib = _StubLib()
    out, perm = _stub_context("bn254", lib).trace_sort(k, np.zeros(0, np.uint8), want_perm=True)
    assert (lib.seen["n"], lib.seen["src"], lib.seen["out"], lib.seen["perm"]) == (0, None, None, None)
    assert out.size == 0 and perm.size == 0
    # a refusal surfaces as HekatonError with the library's status
    with pytest.raises(capi.HekatonError) as e:
        _stub_context("bn254", _StubLib(capi.HK_ERR_ARG)).trace_sort(k, time_b)
    assert e.value.status == capi.HK_ERR_ARG


def test_context_stage0_witness_marshals_its_arguments():
    rnd = random.Random(11)
    offsets = [0, 3, 6, 9, 12]
    time_b = np.frombuffer(bytes(rnd.randrange(256) for _ in range(12 * 64)), np.uint8)
    addr_b = np.frombuffer(bytes(rnd.randrange(256) for _ in range(12 * 64)), np.uint8)
    lib = _StubLib()
    ctx = _stub_context("bls12_381", lib)
    assert ctx.stage0_witness(offsets, 3, time_b, addr_b, [2, 0, 2], 0x7000) == 0x7000
    s = lib.seen
    assert (s["handle"], s["offsets"], s["n_sub"], s["n_portals"]) == ("the-handle", offsets, 4, 3)
    assert (s["time"], s["addr"]) == (time_b.tobytes(), addr_b.tobytes())
    assert (s["sub_index"], s["batch"], s["w_out"]) == ([2, 0, 2], 3, 0x7000)
    ctx.stage0_witness(offsets, 3, time_b, addr_b, [], 0x7000)
    assert (lib.seen["sub_index"], lib.seen["batch"]) == (None, 0)
    with pytest.raises(capi.HekatonError):
        _stub_context("bn254", _StubLib(capi.HK_ERR_ARG)).stage0_witness(offsets, 3, time_b, addr_b, [1], 0x7000)


class _NumpySortCtx:
    """Stands in for capi.Context: trace_sort as the header defines it, done with numpy's stable sorts on the decoded keys."""

    def __init__(self, curve):
        self.curve, self.fc, self.calls = curve, FrCodec(curve), []

    def trace_sort(self, k, time_b, n_entries=None, device_out=False, want_perm=False):
        self.calls.append((k, n_entries, device_out, want_perm))
        rows = np.asarray(time_b, np.uint8).reshape(-1, k * 32)
        vals = self.fc.dec(time_b)
        addr = np.array(vals[0::k], dtype=np.uint64)
        if k == 2:
            order = np.argsort(addr, kind="stable")
        else:
            order = np.lexsort((np.array(vals[2::k], dtype=np.uint64), addr))      # stable; the last key is the primary one
        return rows[order].reshape(-1).copy()


def _subtraces(mem, lengths, r, seed, n_addr=5, n_ts=3):
    rnd = random.Random(seed)
    if mem == transcript.ROM:
        mk = lambda: transcript.RomTranscriptEntry(rnd.randrange(n_addr), rnd.randrange(r))
    else:
        mk = lambda: transcript.RamTranscriptEntry(rnd.choice([0, 7, (1 << 64) - 1, 1 << 32, 9][:n_addr]), rnd.randrange(r),
                                                   rnd.choice([0, (1 << 32) - 1, 5][:n_ts]), bool(rnd.randrange(2)))
    return [[mk() for _ in range(ln)] for ln in lengths]


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("mem", [transcript.ROM, transcript.RAM])
@pytest.mark.parametrize("lengths", [(0, 3, 0, 2), (5, 1, 0, 0, 17, 4), (0, 0), (40,)])
def test_sort_subtraces_by_addr_device_equals_the_host_mirror(curve, mem, lengths):
    r = CURVE_PARAMS[curve]["r"]
    st = _subtraces(mem, lengths, r, seed=len(lengths))
    want = transcript.sort_subtraces_by_addr(st)
    flat = [e for s in st for e in s]
    if len(flat) > 10:                                             # ties: equal keys whose payloads differ
        keys = [e.sort_key() for e in flat]
        assert len(set(keys)) < len(keys) and len(set(flat)) > len(set(keys))
    stub = _NumpySortCtx(curve)
    got = transcript.sort_subtraces_by_addr_device(stub, st)
    assert got == want and [len(s) for s in got] == list(lengths)
    assert all(type(e) is type(flat[0]) for s in got for e in s)
    if flat:
        assert stub.calls == [(2 if mem == transcript.ROM else 4, len(flat), False, False)]
    else:
        assert stub.calls == []                                    # nothing to sort: no call


def _job(curve="bn254"):
    rnd = random.Random(21)
    return ShaMerkleJob(curve, 8, 1, 4, [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(4)])


def test_job_without_a_context_is_unchanged():
    """`time` and `addr` restated from the docstring of ShaMerkleJob and the pinned host sort."""
    job = _job()
    entries = [[transcript.RomTranscriptEntry(a, v) for a, v in ops] for ops in job.time]
    assert [len(ops) for ops in job.time] == [4] * 8
    assert job.time[0][:3] == [(0, 0)] * 3 and job.time[0][3][0] == 1          # a leaf: placeholders, then set(node 0)
    assert [a for a, _ in job.time[4][:2]] == [1, 2]                            # the first parent reads nodes 0 and 1
    want = transcript.sort_subtraces_by_addr(entries)
    assert job.addr == [[(e.addr, e.val) for e in st] for st in want]
    assert job.stage0_ints(3) == [x for e in job.time[3] for x in e] + [x for e in job.addr[3] for x in e]
    assert job.entry_chal is None and job.root is None


class _FakeBuffer:
    """Stands in for capi.DeviceBuffer: remembers the bytes it was made from (or, made as DeviceBuffer(ctx, nbytes), the size
    asked for) and whether it was freed."""
    made = []

    def __init__(self, *a):
        self.data, self.freed = a[-1], False
        self.nbytes = a[-1] if isinstance(a[-1], int) else len(a[-1])
        _FakeBuffer.made.append(self)

    @classmethod
    def from_host(cls, ctx, arr):
        return cls(np.asarray(arr).tobytes())

    def to_host(self):
        return np.frombuffer(self.data, np.uint8)

    def free(self):
        self.freed = True


class _ExecTreeCtx:
    fr_bytes = 32

    def __init__(self, curve):
        self.curve, self.calls = curve, []

    def exec_tree(self, *a, **kw):
        self.calls.append((a, kw))
        return tuple(_FakeBuffer(FrCodec(self.curve).enc([k]).tobytes()) for k in range(5))


def test_stage1_device_without_traces_makes_the_same_calls(monkeypatch):
    monkeypatch.setattr(capi, "DeviceBuffer", _FakeBuffer)
    _FakeBuffer.made = []
    job = _job()
    job.set_challenges(123, 456)
    fc = FrCodec("bn254")
    flat = lambda tr: fc.enc([x for ops in tr for e in ops for x in e]).tobytes()
    consts = device_params("bn254", fc)[0].tobytes()
    ctx = _ExecTreeCtx("bn254")
    dev = job.stage1_device(ctx)
    # three uploads in this order - time, addr, constants - then one exec_tree over them
    assert [b.data for b in _FakeBuffer.made[:3]] == [flat(job.time), flat(job.addr), consts]
    (a, kw), = ctx.calls
    assert a[1] == 2 and list(a[2]) == [4 * i for i in range(9)] and a[3] is _FakeBuffer.made[0] and a[4] is _FakeBuffer.made[1]
    assert a[0][0] is _FakeBuffer.made[2] and bytes(a[5]) == fc.enc([123, 456]).tobytes() and kw == dict(device_out=True)
    assert dev.root == 4 and dev.traces == _FakeBuffer.made[:2]
    dev.free()
    assert all(b.freed for b in _FakeBuffer.made)
    # with traces=: the two buffers are adopted, only the constants go up, and free() leaves the adopted ones alone
    _FakeBuffer.made = []
    mine = [_FakeBuffer(b"time"), _FakeBuffer(b"addr")]
    ctx2 = _ExecTreeCtx("bn254")
    dev2 = sha_circuit.Stage1Device(job, ctx2, traces=mine)
    assert [b.data for b in _FakeBuffer.made[:3]] == [b"time", b"addr", consts]
    (a, kw), = ctx2.calls
    assert a[3] is mine[0] and a[4] is mine[1] and kw == dict(device_out=True)
    dev2.free()
    assert not mine[0].freed and not mine[1].freed and all(b.freed for b in _FakeBuffer.made[2:])


class _Stage0Ctx:
    fr_bytes = 32

    def __init__(self):
        self.curve, self.sorts, self.rows = "bn254", [], []

    def trace_sort(self, k, time_b, n_entries=None, device_out=False, want_perm=False):
        self.sorts.append((k, time_b, n_entries, device_out, want_perm))
        return _FakeBuffer(b"sorted")

    def stage0_witness(self, *a):
        self.rows.append(a)


def test_stage0_device_uploads_once_and_sorts_on_the_device(monkeypatch):
    monkeypatch.setattr(capi, "DeviceBuffer", _FakeBuffer)
    _FakeBuffer.made = []
    job = _job()
    fc = FrCodec("bn254")
    ctx = _Stage0Ctx()
    dev = job.stage0_device(ctx)
    assert [b.data for b in _FakeBuffer.made[:1]] == [fc.enc([x for ops in job.time for e in ops for x in e]).tobytes()]
    (k, src, n, device_out, want_perm), = ctx.sorts
    assert (k, n, device_out, want_perm) == (2, 32, True, False) and src is dev.traces[0] and dev.traces[1].data == b"sorted"
    assert list(dev.offsets) == [4 * i for i in range(9)]
    w = dev.rows([5, 0, 5])
    (offsets, n_portals, t, a, members, w_out), = ctx.rows
    assert list(offsets) == list(dev.offsets) and n_portals == 4 and t is dev.traces[0] and a is dev.traces[1]
    assert list(members) == [5, 0, 5] and w_out is w and w.data == 3 * 16 * 32        # the row buffer's size in bytes
    dev.free()
    assert dev.traces == []
