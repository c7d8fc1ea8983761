"""CPU: the Context wrappers of the job entries - stage0_witness, ram_stage0_witness, stage1_witness, ram_stage1_witness,
exec_tree, trace_sort, r1cs_job_trace, vkd_trace - over a stub library that records what it is handed (the style of
test_agg_scalars_cpu.py): every scalar and descriptor field arrives as given, every pointer is the buffer's address or NULL
for an empty or absent one, a failing status frees exactly the DeviceBuffers the wrapper allocated, and a caller's `out`
buffers are never freed.  Every expectation is written from the call's arguments."""
import ctypes as C
import random

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec

FR = 32
HANDLE = "the-handle"


def _addr(p):
    if p is None:
        return 0
    return p if isinstance(p, int) else (p.value or 0)


def _struct(ref):
    """The fields of the structure behind a byref(): pointers as addresses (0 = NULL), nested descriptors as tuples."""
    s, out = ref._obj, {}
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is C.POINTER(capi.hk_poseidon_desc):
            v = tuple(getattr(v.contents, f) for f, _ in capi.hk_poseidon_desc._fields_) if v else None
        elif typ is C.c_void_p:
            v = v or 0
        out[name] = v
    return out


def _words(p, n):
    return list(np.frombuffer(C.string_at(_addr(p), 4 * n), dtype=np.uint32)) if n else []


class _FakeBuffer:
    """Stands in for capi.DeviceBuffer: an address range nobody touches; every allocation and free is counted."""
    made = []

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes, self.ptr, self.frees = ctx, int(nbytes), 0x7f0000000000 + 0x100000 * (len(_FakeBuffer.made) + 1), 0
        _FakeBuffer.made.append(self)

    def free(self):
        self.frees += 1


class _StubLib:
    """Stands in for libhekaton.so under a capi.Context: records what each entry is handed and returns `status`."""

    def __init__(self, status=capi.HK_OK):
        self.status, self.seen = status, []

    def _rec(self, **kw):
        self.seen.append(kw)
        return self.status

    def _s0(self, fn, handle, offsets, n_sub, n_portals, te, ae, sub, batch, w):
        return self._rec(fn=fn, handle=handle, offsets=_words(offsets, n_sub + 1), n_sub=n_sub, n_portals=n_portals, te=_addr(te),
                         ae=_addr(ae), sub=_words(sub, batch), sub_null=_addr(sub) == 0, batch=batch, w=_addr(w))

    def hk_stage0_witness(self, *a):
        return self._s0("hk_stage0_witness", *a)

    def hk_ram_stage0_witness(self, *a):
        return self._s0("hk_ram_stage0_witness", *a)

    def _s1(self, fn, n_chal, handle, d, sub, batch, n_v, z):
        f = _struct(d)
        return self._rec(fn=fn, handle=handle, d=f, offsets=_words(f["offsets"], f["n_sub"] + 1),
                         chal=bytes(C.string_at(f["challenges_mont"], n_chal * FR)), sub=_words(sub, batch),
                         sub_null=_addr(sub) == 0, batch=batch, n_v=n_v, z=_addr(z))

    def hk_stage1_witness(self, *a):
        return self._s1("hk_stage1_witness", 2, *a)

    def hk_ram_stage1_witness(self, *a):
        return self._s1("hk_ram_stage1_witness", 4, *a)

    def hk_exec_tree(self, handle, d, o):
        f = _struct(d)
        return self._rec(fn="hk_exec_tree", handle=handle, d=f, o=_struct(o), offsets=_words(f["offsets"], f["n_sub"] + 1),
                         chal=bytes(C.string_at(f["challenges_mont"], f["entry_fields"] * FR)))

    def hk_trace_sort(self, handle, k, src, n, out, perm):
        return self._rec(fn="hk_trace_sort", handle=handle, k=k, src=_addr(src), n=n, out=_addr(out), perm=_addr(perm))

    def hk_r1cs_job_trace(self, handle, d, out):
        f = _struct(d)
        return self._rec(fn="hk_r1cs_job_trace", handle=handle, d=f, out=_addr(out),
                         tables={k: _words(f[k], n) for k, n in self.table_len.items()})

    def hk_vkd_trace(self, handle, d, values, entries):
        f = _struct(d)
        return self._rec(fn="hk_vkd_trace", handle=handle, d=f, values=_addr(values), entries=_addr(entries),
                         tables={k: _words(f[k], n) for k, n in self.table_len.items()})


@pytest.fixture
def fake_buffers(monkeypatch):
    monkeypatch.setattr(capi, "DeviceBuffer", _FakeBuffer)
    _FakeBuffer.made = []
    return _FakeBuffer


def _ctx(lib, curve="bn254"):
    ctx = capi.Context.__new__(capi.Context)
    ctx.lib, ctx.curve, ctx.handle, ctx.fr_bytes = lib, curve, HANDLE, FR
    return ctx


def _bytes(rnd, n):
    return np.frombuffer(bytes(rnd.getrandbits(8) for _ in range(n)), dtype=np.uint8).copy()


def _where(x):
    """The address the library must be handed for input x: NULL for an absent or empty one."""
    if x is None:
        return 0
    if isinstance(x, _FakeBuffer):
        return x.ptr if x.nbytes else 0
    return x.ctypes.data if x.size else 0


def _refused(call, table_len=None):
    """`call(ctx)` over a library that answers HK_ERR_ARG: the error surfaces; returns what the library saw."""
    lib = _StubLib(capi.HK_ERR_ARG)
    lib.table_len = table_len
    with pytest.raises(capi.HekatonError) as e:
        call(_ctx(lib))
    assert e.value.status == capi.HK_ERR_ARG
    return lib


PARAMS_DESCS = ((4, 5, 8, 56, 0), (3, 17, 8, 33, 272))


def _params(consts):
    return consts, 404, PARAMS_DESCS[0], PARAMS_DESCS[1]


# ---- stage 0 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stage0_witness", "ram_stage0_witness"])
@pytest.mark.parametrize("resident", [False, True])
def test_stage0_wrappers(fake_buffers, name, resident):
    rnd = random.Random(11)
    lib = _StubLib()
    ctx = _ctx(lib)
    offsets, sub = [0, 3, 6, 9, 12], [2, 0, 2]
    te, ae = (_FakeBuffer(ctx, 12 * 4 * FR) for _ in range(2)) if resident else (_bytes(rnd, 12 * 4 * FR) for _ in range(2))
    w = _FakeBuffer(ctx, 1 << 16)
    made = len(fake_buffers.made)
    assert getattr(ctx, name)(offsets, 3, te, ae, sub, w) is w
    s = lib.seen[-1]
    assert (s["fn"], s["handle"], s["offsets"], s["n_sub"], s["n_portals"]) == ("hk_" + name, HANDLE, offsets, 4, 3)
    assert (s["te"], s["ae"], s["sub"], s["batch"], s["w"]) == (_where(te), _where(ae), sub, 3, w.ptr)
    # a raw device address for the output; no rows: a NULL sub_index and batch 0
    assert getattr(ctx, name)(offsets, 3, te, ae, [], 0x7e0000001000) == 0x7e0000001000
    s = lib.seen[-1]
    assert s["sub_null"] and (s["batch"], s["w"]) == (0, 0x7e0000001000)
    # a refusal frees nothing: the wrapper allocated nothing
    _refused(lambda c: getattr(c, name)(offsets, 3, te, ae, sub, w))
    assert len(fake_buffers.made) == made and all(b.frees == 0 for b in fake_buffers.made)


# ---- stage 1 ----------------------------------------------------------------------------------------------------------------
def _stage1_inputs(rnd, ctx, resident, nf, empty):
    """(time, addr, evals, leaves, siblings, root): host bytes or resident buffers; `empty` names one given with no bytes."""
    sizes = [12 * (nf - 2), 12 * (nf - 2), 4 * 2, 4 * nf, 4 * 2, 1]
    sizes = [0 if k == empty else n * FR for k, n in enumerate(sizes)]
    return [_FakeBuffer(ctx, n) if resident else _bytes(rnd, n) for n in sizes]


@pytest.mark.parametrize("ram", [False, True])
@pytest.mark.parametrize("resident,empty", [(False, None), (True, None), (False, 0), (True, 5)])
def test_stage1_wrappers(fake_buffers, ram, resident, empty):
    rnd = random.Random(12)
    r = CURVE_PARAMS["bn254"]["r"]
    lib = _StubLib()
    ctx = _ctx(lib)
    te, ae, evals, leaves, sibs, root = _stage1_inputs(rnd, ctx, resident, 6 if ram else 4, empty)
    consts = _FakeBuffer(ctx, 404 * FR) if resident else _bytes(rnd, 404 * FR)
    nodes = object()                                           # exec_tree's third output is not looked at
    offsets, sub, n_chal = [0, 3, 6, 9, 12], [1, 1, 3], 4 if ram else 2
    chal = [rnd.randrange(r) for _ in range(n_chal)]
    z = _FakeBuffer(ctx, 1 << 20)
    layout = (7, 11, 500, 900) if ram else (7, 11, 500)
    fn = ctx.ram_stage1_witness if ram else ctx.stage1_witness
    made = len(fake_buffers.made)
    assert fn(_params(consts), 3, offsets, te, ae, chal, (evals, leaves, nodes, sibs, root), sub, 4096, layout, z) is z
    s = lib.seen[-1]
    d = s["d"]
    assert (s["fn"], s["handle"]) == ("hk_ram_stage1_witness" if ram else "hk_stage1_witness", HANDLE)
    assert (d["n_sub"], d["n_portals"], d["depth"], s["offsets"]) == (4, 3, 2, offsets)
    got = [d[k] for k in ("time_entries_mont", "addr_entries_mont", "evals_mont", "leaves_mont", "siblings_mont", "root_mont")]
    assert got == [_where(x) for x in (te, ae, evals, leaves, sibs, root)]
    assert s["chal"] == FrCodec("bn254").enc(chal).tobytes()
    assert (d["consts_mont"], d["n_consts"], d["leaf_hash"], d["node_hash"]) == (consts.ptr if resident else consts.ctypes.data,
                                                                                 404, PARAMS_DESCS[0], PARAMS_DESCS[1])
    cols = ("inst_col0", "stage0_col0", "col0", "pos_col0") if ram else ("inst_col0", "col0", "pos_col0")
    assert tuple(d[k] for k in cols) == layout
    assert (s["sub"], s["batch"], s["n_v"], s["z"]) == (sub, 3, 4096, z.ptr)
    if ram:
        assert d["template_mont"] == 0                                  # no template: NULL
        tmpl = _FakeBuffer(ctx, 4096 * FR) if resident else _bytes(rnd, 4096 * FR)
        fn(_params(consts), 3, offsets, te, ae, chal, (evals, leaves, nodes, sibs, root), sub, 4096, layout, z, template=tmpl)
        assert lib.seen[-1]["d"]["template_mont"] == _where(tmpl)
        made += resident
    # challenges as their Montgomery bytes: handed over as they are; a raw address for z_out; no rows
    cb = _bytes(rnd, n_chal * FR)
    assert fn(_params(consts), 3, offsets, te, ae, cb, (evals, leaves, nodes, sibs, root), [], 4096, layout, 0x7e0000002000) \
        == 0x7e0000002000
    s = lib.seen[-1]
    assert s["chal"] == cb.tobytes() and s["d"]["challenges_mont"] == cb.ctypes.data
    assert s["sub_null"] and (s["batch"], s["z"]) == (0, 0x7e0000002000)
    _refused(lambda c: (c.ram_stage1_witness if ram else c.stage1_witness)(
        _params(consts), 3, offsets, te, ae, chal, (evals, leaves, nodes, sibs, root), sub, 4096, layout, z))
    assert len(fake_buffers.made) == made and all(b.frees == 0 for b in fake_buffers.made)


# ---- exec_tree --------------------------------------------------------------------------------------------------------------
EXEC_OUTS = ("evals_mont", "leaves_mont", "nodes_mont", "siblings_mont", "root_mont")


@pytest.mark.parametrize("entry_fields", [2, 4])
@pytest.mark.parametrize("resident", [False, True])
def test_exec_tree_wrapper(fake_buffers, entry_fields, resident):
    rnd = random.Random(13)
    r = CURVE_PARAMS["bn254"]["r"]
    lib = _StubLib()
    ctx = _ctx(lib)
    offsets, k = [0, 3, 6, 9, 12], entry_fields
    te, ae = (_FakeBuffer(ctx, 12 * k * FR) for _ in range(2)) if resident else (_bytes(rnd, 12 * k * FR) for _ in range(2))
    consts = _bytes(rnd, 404 * FR)
    chal = [rnd.randrange(r) for _ in range(k)]
    sizes = [2 * 4, (2 + k) * 4, 2 * 4 - 1, 4 * 2, 1]                      # n_sub = 4, depth = 2
    outs = ctx.exec_tree(_params(consts), k, offsets, te, ae, chal)
    s = lib.seen[-1]
    d = s["d"]
    assert (s["handle"], d["n_sub"], d["entry_fields"], s["offsets"]) == (HANDLE, 4, k, offsets)
    assert (d["time_entries_mont"], d["addr_entries_mont"]) == (_where(te), _where(ae))
    assert s["chal"] == FrCodec("bn254").enc(chal).tobytes()
    assert (d["consts_mont"], d["n_consts"], d["leaf_hash"], d["node_hash"]) == (consts.ctypes.data, 404, *PARAMS_DESCS)
    assert [x.size for x in outs] == [n * FR for n in sizes] and all(x.dtype == np.uint8 for x in outs)
    assert [s["o"][f] for f in EXEC_OUTS] == [x.ctypes.data for x in outs]
    # empty traces reach the library as NULL
    empty = np.zeros(0, np.uint8)
    ctx.exec_tree(_params(consts), k, [0, 0, 0], empty, _FakeBuffer(ctx, 0) if resident else empty, chal)
    d = lib.seen[-1]["d"]
    assert (d["n_sub"], d["time_entries_mont"], d["addr_entries_mont"]) == (2, 0, 0)
    # device outputs: five allocations of the sizes, returned as they are
    made = len(fake_buffers.made)
    outs = ctx.exec_tree(_params(consts), k, offsets, te, ae, _bytes(rnd, k * FR), device_out=True)
    assert list(outs) == fake_buffers.made[made:] and [x.nbytes for x in outs] == [n * FR for n in sizes]
    assert [lib.seen[-1]["o"][f] for f in EXEC_OUTS] == [x.ptr for x in outs] and all(x.frees == 0 for x in outs)
    # a refusal frees exactly those five, once each - and never the inputs or a caller's `out`
    made = len(fake_buffers.made)
    _refused(lambda c: c.exec_tree(_params(consts), k, offsets, te, ae, chal, device_out=True))
    assert len(fake_buffers.made) == made + 5 and [b.frees for b in fake_buffers.made[made:]] == [1] * 5
    assert all(b.frees == 0 for b in fake_buffers.made[:made])
    mine = [_FakeBuffer(ctx, n * FR) for n in sizes]
    made, frees = len(fake_buffers.made), [b.frees for b in fake_buffers.made]
    for dev in (False, True):
        lib2 = _refused(lambda c: c.exec_tree(_params(consts), k, offsets, te, ae, chal, device_out=dev, out=mine))
        assert [lib2.seen[-1]["o"][f] for f in EXEC_OUTS] == [x.ptr for x in mine]
    assert len(fake_buffers.made) == made and [b.frees for b in fake_buffers.made] == frees
    assert list(ctx.exec_tree(_params(consts), k, offsets, te, ae, chal, out=mine)) == mine


# ---- trace_sort -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry_fields", [2, 4])
@pytest.mark.parametrize("resident", [False, True])
def test_trace_sort_wrapper(fake_buffers, entry_fields, resident):
    rnd = random.Random(14)
    lib = _StubLib()
    ctx = _ctx(lib)
    k, n = entry_fields, 9
    src = _FakeBuffer(ctx, n * k * FR) if resident else _bytes(rnd, n * k * FR)
    out = ctx.trace_sort(k, src)
    s = lib.seen[-1]
    assert (s["handle"], s["k"], s["src"], s["n"], s["perm"]) == (HANDLE, k, _where(src), n, 0)
    assert out.dtype == np.uint8 and out.size == n * k * FR and s["out"] == out.ctypes.data
    out, perm = ctx.trace_sort(k, src, n_entries=5, want_perm=True)
    s = lib.seen[-1]
    assert (s["n"], s["out"], s["perm"]) == (5, out.ctypes.data, perm.ctypes.data)
    assert out.size == 5 * k * FR and perm.dtype == np.uint32 and perm.size == 5
    # nothing to sort: every pointer NULL
    ctx.trace_sort(k, np.zeros(0, np.uint8), want_perm=True)
    s = lib.seen[-1]
    assert (s["src"], s["n"], s["out"], s["perm"]) == (0, 0, 0, 0)
    # device outputs, and what a refusal frees: the one or two buffers of this call
    made = len(fake_buffers.made)
    out, perm = ctx.trace_sort(k, src, device_out=True, want_perm=True)
    assert [out, perm] == fake_buffers.made[made:] and (out.nbytes, perm.nbytes) == (n * k * FR, 4 * n)
    assert (lib.seen[-1]["out"], lib.seen[-1]["perm"]) == (out.ptr, perm.ptr) and out.frees == perm.frees == 0
    for want_perm in (False, True):
        made, frees = len(fake_buffers.made), [b.frees for b in fake_buffers.made]
        _refused(lambda c: c.trace_sort(k, src, device_out=True, want_perm=want_perm))
        assert [b.frees for b in fake_buffers.made] == frees + [1] * (1 + want_perm)
    made = len(fake_buffers.made)
    _refused(lambda c: c.trace_sort(k, src, want_perm=True))
    assert len(fake_buffers.made) == made


# ---- r1cs_job_trace ---------------------------------------------------------------------------------------------------------
R1CS_TABLES = dict(n_parts=2, n_txs=3, slot_offsets=[0, 2, 5], slot_rank=[0, 1, 1, 0, 2], slot_src=[4, 0xffffffff, 1, 2, 9],
                   sets_per_tx=3, tx_len=10, tx_stride=10, wit_offsets=[0, 4, 10], body_len=[2, 3])


@pytest.mark.parametrize("resident", [False, True])
def test_r1cs_job_trace_wrapper(fake_buffers, resident):
    rnd = random.Random(15)
    lib = _StubLib()
    lib.table_len = dict(slot_offsets=3, slot_rank=5, slot_src=5, wit_offsets=3, body_len=2)
    ctx = _ctx(lib)
    t = R1CS_TABLES
    wit = _FakeBuffer(ctx, 30 * FR) if resident else _bytes(rnd, 30 * FR)
    n = 3 * 5 * 2 * FR
    out = ctx.r1cs_job_trace(t, wit)
    s = lib.seen[-1]
    d = s["d"]
    assert s["handle"] == HANDLE and {k: d[k] for k in ("n_parts", "n_txs", "sets_per_tx", "tx_len", "tx_stride")} == \
        {k: t[k] for k in ("n_parts", "n_txs", "sets_per_tx", "tx_len", "tx_stride")}
    assert s["tables"] == {k: t[k] for k in lib.table_len} and d["witness_mont"] == _where(wit)
    assert out.dtype == np.uint8 and out.size == n and s["out"] == out.ctypes.data
    # an empty table reaches the library as NULL
    lib.table_len = dict(slot_offsets=3)
    ctx.r1cs_job_trace(dict(t, slot_rank=[], slot_src=[], wit_offsets=[], body_len=[]), wit)
    d = lib.seen[-1]["d"]
    assert [d[k] for k in ("slot_rank", "slot_src", "wit_offsets", "body_len")] == [0] * 4 and d["slot_offsets"] != 0
    # a device output is allocated, returned as it is, and freed by a refusal; a caller's `out` never is
    made = len(fake_buffers.made)
    out = ctx.r1cs_job_trace(t, wit, device_out=True)
    assert [out] == fake_buffers.made[made:] and out.nbytes == n and lib.seen[-1]["out"] == out.ptr and out.frees == 0
    made = len(fake_buffers.made)
    _refused(lambda c: c.r1cs_job_trace(t, wit, device_out=True), lib.table_len)
    assert [b.frees for b in fake_buffers.made[made:]] == [1] and all(b.frees == 0 for b in fake_buffers.made[:made])
    mine = _FakeBuffer(ctx, n)
    made, frees = len(fake_buffers.made), [b.frees for b in fake_buffers.made]
    for dev in (False, True):
        assert _refused(lambda c: c.r1cs_job_trace(t, wit, device_out=dev, out=mine), lib.table_len).seen[-1]["out"] == mine.ptr
    assert len(fake_buffers.made) == made and [b.frees for b in fake_buffers.made] == frees
    assert ctx.r1cs_job_trace(t, wit, out=mine) is mine


# ---- vkd_trace --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True])
def test_vkd_trace_wrapper(fake_buffers, resident):
    rnd = random.Random(16)
    lib = _StubLib()
    lib.table_len = dict(kinds=2, slot_addr=7, slot_src=7)
    ctx = _ctx(lib)
    mk = (lambda n: _FakeBuffer(ctx, n)) if resident else (lambda n: _bytes(rnd, n))
    t = dict(depth=16, split=2, n_updates=2, kinds=[0, 1], slot_addr=[1, 2, 3, 4, 5, 6, 7], slot_src=[0, 1, 2, 0xffffffff, 4, 5, 6],
             leaves=mk(2 * 2 * 64), siblings=mk(2 * 16 * FR), roots=_bytes(rnd, 2 * FR))
    consts = mk(404 * FR)
    sizes = [(3 + 2 * (2 + 3 * 2)) * FR, 2 * 7 * FR]
    vals, entries = ctx.vkd_trace(t, _params(consts))
    s = lib.seen[-1]
    d = s["d"]
    assert s["handle"] == HANDLE and (d["depth"], d["split"], d["n_updates"], d["n_slots"]) == (16, 2, 2, 7)
    assert s["tables"] == {k: t[k] for k in lib.table_len}
    assert (d["leaves"], d["siblings_mont"], d["consts_mont"], d["roots_mont"], d["values_mont"]) == \
        (_where(t["leaves"]), _where(t["siblings"]), _where(consts), t["roots"].ctypes.data, 0)
    assert (d["n_consts"], d["leaf_hash"], d["node_hash"]) == (404, *PARAMS_DESCS)
    assert [vals.size, entries.size] == sizes and (s["values"], s["entries"]) == (vals.ctypes.data, entries.ctypes.data)
    made = len(fake_buffers.made)
    outs = ctx.vkd_trace(t, _params(consts), device_out=True)
    assert list(outs) == fake_buffers.made[made:] and [x.nbytes for x in outs] == sizes
    assert (lib.seen[-1]["values"], lib.seen[-1]["entries"]) == (outs[0].ptr, outs[1].ptr) and all(x.frees == 0 for x in outs)
    made = len(fake_buffers.made)
    _refused(lambda c: c.vkd_trace(t, _params(consts), device_out=True), lib.table_len)
    assert [b.frees for b in fake_buffers.made[made:]] == [1, 1] and all(b.frees == 0 for b in fake_buffers.made[:made])
    mine = (_FakeBuffer(ctx, sizes[0]), _FakeBuffer(ctx, sizes[1]))
    made, frees = len(fake_buffers.made), [b.frees for b in fake_buffers.made]
    for dev in (False, True):
        s = _refused(lambda c: c.vkd_trace(t, _params(consts), device_out=dev, out=mine), lib.table_len).seen[-1]
        assert (s["values"], s["entries"]) == (mine[0].ptr, mine[1].ptr)
    assert len(fake_buffers.made) == made and [b.frees for b in fake_buffers.made] == frees
    assert ctx.vkd_trace(t, _params(consts), out=mine) is mine
