"""CPU: the ABI surface of hk_exec_tree and its host wrappers, without a device - the symbol is declared, listed and
exported; Context.exec_tree fills the two structs as include/hekaton.h lays them out (a stub library records them);
transcript.exec_tree_device and ShaMerkleJob.set_challenges hand a context the flattened traces the host mirror walks (a
stub context records them); ExecTree.from_levels serves a host tree's own levels unchanged; set_challenges without a
context is the code it was."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from hekaton_system_amd import capi, transcript
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.poseidon import ExecTree, device_params
from hekaton_system_amd.sha_circuit import ShaMerkleJob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exec_tree_symbol_declared_listed_exported():
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    declared = set(re.findall(r"\b(hk_[a-z0-9_]+)\s*\(", hdr))
    assert "hk_exec_tree" in declared and "hk_exec_tree" in capi.EXPORTS
    assert "hk_exec_tree_desc" in hdr and "hk_exec_tree_out" in hdr
    if os.path.exists(capi.LIB_PATH):
        getattr(capi.load(), "hk_exec_tree")


def test_struct_layouts_follow_the_header():
    d, o = capi.hk_exec_tree_desc, capi.hk_exec_tree_out
    assert [f[0] for f in d._fields_] == ["n_sub", "entry_fields", "offsets", "time_entries_mont", "addr_entries_mont",
                                          "challenges_mont", "consts_mont", "n_consts", "leaf_hash", "node_hash"]
    assert (d.n_sub.offset, d.entry_fields.offset, d.offsets.offset) == (0, 4, 8)
    assert C.sizeof(d) == 8 + 8 * 8
    assert [f[0] for f in o._fields_] == ["evals_mont", "leaves_mont", "nodes_mont", "siblings_mont", "root_mont"]
    assert C.sizeof(o) == 5 * 8


class _StubLib:
    """Stands in for libhekaton.so under a capi.Context: copies what hk_exec_tree is handed, writes a pattern to every
    output and returns `status`."""

    def __init__(self, status=capi.HK_OK):
        self.status, self.seen = status, None

    def hk_exec_tree(self, handle, desc, out):
        d, o = desc._obj, out._obj
        n, k = d.n_sub, d.entry_fields
        total = int(np.ctypeslib.as_array(C.cast(d.offsets, C.POINTER(C.c_uint32)), (n + 1,))[-1])
        grab = lambda p, nbytes: bytes(C.string_at(p, nbytes)) if p else None
        self.seen = dict(handle=handle, n_sub=n, entry_fields=k,
                         offsets=list(np.ctypeslib.as_array(C.cast(d.offsets, C.POINTER(C.c_uint32)), (n + 1,))),
                         time=grab(d.time_entries_mont, total * k * 32), addr=grab(d.addr_entries_mont, total * k * 32),
                         chal=grab(d.challenges_mont, k * 32), consts=grab(d.consts_mont, d.n_consts * 32),
                         n_consts=d.n_consts,
                         leaf=tuple(getattr(d.leaf_hash.contents, f[0]) for f in capi.hk_poseidon_desc._fields_),
                         node=tuple(getattr(d.node_hash.contents, f[0]) for f in capi.hk_poseidon_desc._fields_))
        depth = n.bit_length() - 1
        for tag, (p, count) in enumerate(((o.evals_mont, 2 * n), (o.leaves_mont, (2 + k) * n), (o.nodes_mont, 2 * n - 1),
                                          (o.siblings_mont, n * depth), (o.root_mont, 1))):
            C.memset(p, 0x10 + tag, count * 32)
        return self.status


def _stub_context(curve, lib):
    ctx = capi.Context.__new__(capi.Context)
    ctx.lib, ctx.curve, ctx.handle, ctx.fr_bytes = lib, curve, "the-handle", 32
    return ctx


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("k", [2, 4])
def test_context_exec_tree_marshals_its_arguments(curve, k):
    fc = FrCodec(curve)
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(5)
    params = device_params(curve, fc)
    offsets = [0, 0, 3, 3, 5, 6, 6, 9, 11]
    n = len(offsets) - 1
    time_b = fc.enc([rnd.randrange(r) for _ in range(offsets[-1] * k)])
    addr_b = fc.enc([rnd.randrange(r) for _ in range(offsets[-1] * k)])
    chal = [rnd.randrange(r) for _ in range(k)]
    lib = _StubLib()
    outs = _stub_context(curve, lib).exec_tree(params, k, offsets, time_b, addr_b, chal)
    s = lib.seen
    assert (s["handle"], s["n_sub"], s["entry_fields"], s["offsets"]) == ("the-handle", n, k, offsets)
    assert s["time"] == time_b.tobytes() and s["addr"] == addr_b.tobytes()
    assert s["chal"] == fc.enc(chal).tobytes()                             # ints are encoded, in the order given
    assert s["consts"] == params[0].tobytes() and s["n_consts"] == params[1]
    assert (s["leaf"], s["node"]) == (params[2], params[3])
    # five arrays of the documented lengths, each the buffer the library wrote to
    want = [2 * n, (2 + k) * n, 2 * n - 1, n * 3, 1]
    assert [x.size for x in outs] == [32 * w for w in want]
    for tag, x in enumerate(outs):
        assert (x == 0x10 + tag).all()
    # challenges already in Montgomery bytes pass through as they are
    lib2 = _StubLib()
    _stub_context(curve, lib2).exec_tree(params, k, np.array(offsets, np.uint32), time_b, addr_b, fc.enc(chal))
    assert lib2.seen["chal"] == s["chal"]
    # a refusal surfaces as HekatonError with the library's status
    with pytest.raises(capi.HekatonError) as e:
        _stub_context(curve, _StubLib(capi.HK_ERR_ARG)).exec_tree(params, k, offsets, time_b, addr_b, chal)
    assert e.value.status == capi.HK_ERR_ARG


def test_from_levels_serves_a_host_trees_own_levels():
    rnd = random.Random(9)
    r = CURVE_PARAMS["bn254"]["r"]
    leaves = [[rnd.randrange(r) for _ in range(4)] for _ in range(8)]
    host = ExecTree("bn254", leaves)
    tree = ExecTree.from_levels("bn254", leaves, host.levels)
    assert (tree.root, tree.depth) == (host.root, host.depth)
    for i in range(8):
        assert tree.path(i) == host.path(i)
        assert tree.verify(leaves[i], *tree.path(i))
    assert not tree.verify(leaves[0], *tree.path(1))
    with pytest.raises(AssertionError):
        ExecTree.from_levels("bn254", leaves, host.levels[:-1])


class _Recorded(Exception):
    pass


class _StubCtx:
    """Stands in for capi.Context: records what a wrapper hands to exec_tree, then stops."""
    fr_bytes = 32

    def __init__(self, curve):
        self.curve, self.args = curve, None

    def exec_tree(self, *a, **kw):
        self.args = (a, kw)
        raise _Recorded()


@pytest.mark.parametrize("mem", [transcript.ROM, transcript.RAM])
def test_exec_tree_device_hands_over_the_flattened_traces(mem):
    curve = "bn254"
    fc = FrCodec(curve)
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(3)
    if mem == transcript.ROM:
        mk = lambda: transcript.RomTranscriptEntry(rnd.randrange(50), rnd.randrange(r))
    else:
        mk = lambda: transcript.RamTranscriptEntry(rnd.randrange(50), rnd.randrange(r), rnd.randrange(1 << 32), bool(rnd.randrange(2)))
    time_st = [[mk() for _ in range(ln)] for ln in (0, 3, 0, 2)]
    addr_st = transcript.sort_subtraces_by_addr(time_st)
    com = b"super commitment bytes"
    stub = _StubCtx(curve)
    with pytest.raises(_Recorded):
        transcript.exec_tree_device(stub, mem, com, time_st, addr_st)
    (params, k, offsets, time_b, addr_b, chal), kw = stub.args
    assert k == (2 if mem == transcript.ROM else 4) and not kw
    assert list(offsets) == [0, 0, 3, 3, 5]
    assert fc.dec(time_b) == [x for st in time_st for e in st for x in e.to_field_elements()]
    assert fc.dec(addr_b) == [x for st in addr_st for e in st for x in e.to_field_elements()]
    assert tuple(chal) == transcript.RunningEvaluation.new(mem, com, r).challenges      # hashed as the host mirror does
    assert params[1:] == device_params(curve, fc)[1:]
    # explicit challenges are taken as given
    stub2 = _StubCtx(curve)
    with pytest.raises(_Recorded):
        transcript.exec_tree_device(stub2, mem, list(chal), time_st, addr_st)
    assert tuple(stub2.args[0][5]) == tuple(chal)


def _job(curve):
    rnd = random.Random(21)
    return ShaMerkleJob(curve, 8, 1, 4, [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(4)])


def test_set_challenges_with_a_context_hands_over_the_job_traces():
    job = _job("bn254")
    fc = FrCodec("bn254")
    stub = _StubCtx("bn254")
    with pytest.raises(_Recorded):
        job.set_challenges(12345, 67890, ctx=stub)
    (params, k, offsets, time_b, addr_b, chal), _ = stub.args
    assert k == 2 and list(offsets) == [4 * i for i in range(9)] and tuple(chal) == (12345, 67890)
    assert fc.dec(time_b) == [x % job.r for ops in job.time for e in ops for x in e]
    assert fc.dec(addr_b) == [x % job.r for ops in job.addr for e in ops for x in e]


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_set_challenges_without_a_context_is_unchanged(curve):
    """The values today's code gives, restated from the two pinned host mirrors: transcript.running_evaluations for the
    evaluations, poseidon.ExecTree for the tree."""
    job = _job(curve)
    r = job.r
    ech, tr = 0x1234567 % r, (r - 5)
    job.set_challenges(ech, tr)
    entries = lambda tr_: [[transcript.RomTranscriptEntry(a, v % r) for a, v in ops] for ops in tr_]
    ev = transcript.RunningEvaluation(transcript.ROM, r, (ech, tr))
    te, ae = [1], [1]
    for t_st, a_st in zip(entries(job.time), entries(job.addr)):
        for a, b in zip(t_st, a_st):
            ev.update_time_ordered(a)
            ev.update_addr_ordered(b)
        te.append(ev.time_ordered_eval)
        ae.append(ev.addr_ordered_eval)
    assert (job.time_eval0, job.addr_eval0) == (te, ae)
    leaves = [[te[i + 1], ae[i + 1], job.addr[i][-1][0] % r, job.addr[i][-1][1] % r] for i in range(8)]
    host = ExecTree(curve, leaves)
    assert job.root == host.root and job.tree.levels == host.levels
    assert [job.tree.path(i) for i in range(8)] == [host.path(i) for i in range(8)]
