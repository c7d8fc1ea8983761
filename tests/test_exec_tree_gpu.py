"""GPU: hk_exec_tree (csrc/exec_tree.cuh) against the pinned host mirror - transcript.running_evaluations for the
evaluations and the leaves, poseidon.ExecTree for every digest, path and the root - byte for byte on both curves.

Shapes are the smallest that reach each boundary of the kernels:
  n_sub 2            one active quad in a wave of the fused tree launch
  n_sub 64           the last size whose leaf level is hashed inside the fused launch (64 states = one workgroup)
  n_sub 128          the first with a leaf launch of its own (two workgroups) in front of the fused levels
  n_sub 1024         levels of 512, 256 and 128 states: one launch each before the fused ones
  long traces        [0, 1, 70 001, 70 001, 100 003]: 12 501 chunks of 8 entries = 49 scan tiles of 256 chunks, boundaries
                     inside a chunk (1, 70 001 and 100 003 leave 1, 1 and 3 entries of their chunk), an empty subtrace
                     after a long one.  With chunks of 8 none of these lies on a chunk edge, and the scan has one more
                     size boundary of its own: the scan over the tile totals gives each of its 64 lanes ceil(tiles / 64)
                     consecutive tiles, so above 64 tiles (131 072 entries) a lane walks more than one.  The second case,
                     [0, 2 048, 131 079, 131 079, 140 003], has 69 tiles, a boundary on a chunk edge that is also a tile
                     edge (2 048 = chunk 256 = the first chunk of tile 1) and one with the longest leftover (7 entries).
Each host reference is computed once per session (functools.lru_cache) and never modified."""
import ctypes as C
import random
from functools import lru_cache

import numpy as np
import pytest

from hekaton_system_amd import capi, transcript
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.poseidon import ExecTree, device_params, merkle_params
from hekaton_system_amd.sha_circuit import ShaMerkleJob, poseidon_path_trace
from hekaton_system_amd.transcript import RAM, ROM, RamTranscriptEntry, RomTranscriptEntry, RunningEvaluation

pytestmark = pytest.mark.gpu

COM = b"exec tree test: the super commitment's bytes"
ZERO_ADDR = 1 << 40                      # the address of the entry whose factor is zero: sorts behind every other


def _lengths(n_sub, rnd):
    """Subtrace lengths 0 .. 9: an empty first subtrace, an empty one in the middle, 9 at the end."""
    lens = [rnd.randrange(10) for _ in range(n_sub)]
    lens[0] = 0
    if n_sub >= 4:
        lens[n_sub // 2] = 0
        lens[1] = 5
    lens[-1] = 9
    return lens


def _rom_traces(curve, lens, seed, zero_at=None):
    """Time-ordered ROM subtraces of the given lengths and their address-ordered copy.  Values include 0 and r - 1; the
    entry at flat position zero_at (time order) has a factor of exactly zero under COM's challenges."""
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(seed)
    ech, tr = RunningEvaluation.new(ROM, COM, r).challenges
    total = sum(lens)
    flat = [RomTranscriptEntry(rnd.randrange(50), rnd.randrange(r)) for _ in range(total)]
    if total > 2:
        flat[0] = RomTranscriptEntry(7, 0)
        flat[1] = RomTranscriptEntry(3, r - 1)
    if zero_at is not None:
        flat[zero_at] = RomTranscriptEntry(ZERO_ADDR, (tr - ech * ZERO_ADDR) % r)
    time_st, at = [], 0
    for ln in lens:
        time_st.append(flat[at:at + ln])
        at += ln
    return time_st, transcript.sort_subtraces_by_addr(time_st)


def _host(curve, mem, time_st, addr_st):
    """(leaves as running_evaluations returns them, the leaf fields, the host tree)"""
    r = CURVE_PARAMS[curve]["r"]
    leaves = transcript.running_evaluations(mem, COM, r, time_st, addr_st)
    fields = [[ev.time_ordered_eval, ev.addr_ordered_eval] + last.to_field_elements() for ev, last in leaves]
    return leaves, fields, ExecTree(curve, fields)


@lru_cache(maxsize=None)
def _rom_case(curve, n_sub):
    lens = _lengths(n_sub, random.Random(100 + n_sub))
    total = sum(lens)
    time_st, addr_st = _rom_traces(curve, lens, 200 + n_sub, zero_at=(2 * total) // 3)
    return time_st, addr_st, _host(curve, ROM, time_st, addr_st)


def _check_arrays(ctx, curve, k, got, fields, tree):
    """evals, leaves, every node, every sibling row and the root of one call against the host tree"""
    fc = FrCodec(curve)
    evals, leaves, nodes, siblings, root = got
    n = len(fields)
    assert fc.dec(evals) == [x for f in fields for x in f[:2]]
    assert fc.dec(leaves) == [x for f in fields for x in f]
    assert fc.dec(nodes) == [x for lvl in tree.levels for x in lvl]
    sib = fc.dec(siblings)
    for i in range(n):
        assert sib[i * tree.depth:(i + 1) * tree.depth] == tree.path(i)[0], i
    assert fc.dec(root) == [tree.root]


def _run(ctx, curve, mem, time_st, addr_st, **kw):
    fc = FrCodec(curve)
    r = CURVE_PARAMS[curve]["r"]
    chal = RunningEvaluation.new(mem, COM, r).challenges
    offsets, time_b = transcript.flatten_subtraces(fc, time_st)
    _, addr_b = transcript.flatten_subtraces(fc, addr_st)
    return ctx.exec_tree(device_params(curve, fc), len(chal), offsets, time_b, addr_b, chal, **kw)


@pytest.mark.parametrize("n_sub", [2, 4, 64, 128])
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_rom_tree_equals_the_host_mirror(curve, n_sub, ctx_bn254, ctx_bls):
    ctx = ctx_bn254 if curve == "bn254" else ctx_bls
    time_st, addr_st, (leaves, fields, tree) = _rom_case(curve, n_sub)
    # the zero factor took effect: the last evaluations are 0, in both orders, and the first non-empty one is not
    assert fields[-1][:2] == [0, 0] and fields[0][:2] == [1, 1]
    if n_sub >= 64:                                                # it stays 0 over many subtraces; time order meets it first
        assert fields[1][0] != 0 and fields[-2][0] == 0 and fields[-2][1] != 0
    _check_arrays(ctx, curve, 2, _run(ctx, curve, ROM, time_st, addr_st), fields, tree)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_exec_tree_device_returns_the_leaves_of_running_evaluations(curve, ctx_bn254, ctx_bls):
    ctx = ctx_bn254 if curve == "bn254" else ctx_bls
    time_st, addr_st, (leaves, fields, tree) = _rom_case(curve, 4)
    got_leaves, got_tree = transcript.exec_tree_device(ctx, ROM, COM, time_st, addr_st)
    assert len(got_leaves) == len(leaves)
    for (ev, last), (hev, hlast) in zip(got_leaves, leaves):
        assert (ev.mem_type, ev.challenges, ev.time_ordered_eval, ev.addr_ordered_eval, last) == \
               (hev.mem_type, hev.challenges, hev.time_ordered_eval, hev.addr_ordered_eval, hlast)
    assert (got_tree.root, got_tree.depth, got_tree.levels, got_tree.leaves) == (tree.root, tree.depth, tree.levels, tree.leaves)
    for i in range(4):
        assert got_tree.path(i) == tree.path(i) and got_tree.verify(fields[i], *got_tree.path(i))


def test_ram_entries(ctx_bn254):
    curve, n_sub = "bn254", 8
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(31)
    lens = _lengths(n_sub, rnd)
    mk = lambda: RamTranscriptEntry(rnd.randrange(6), rnd.randrange(r), rnd.randrange(1 << 32), bool(rnd.randrange(2)))
    time_st = [[mk() for _ in range(ln)] for ln in lens]
    time_st[1][0] = RamTranscriptEntry(2, 0, 0, False)
    time_st[1][1] = RamTranscriptEntry(2, r - 1, (1 << 32) - 1, True)
    addr_st = transcript.sort_subtraces_by_addr(time_st)
    leaves, fields, tree = _host(curve, RAM, time_st, addr_st)
    assert len(fields[0]) == 6
    _check_arrays(ctx_bn254, curve, 4, _run(ctx_bn254, curve, RAM, time_st, addr_st), fields, tree)


@pytest.mark.parametrize("offsets", [(0, 1, 70001, 70001, 100003), (0, 2048, 131079, 131079, 140003)])
def test_long_trace(offsets, ctx_bn254):
    curve = "bn254"
    lens = [b - a for a, b in zip(offsets, offsets[1:])]
    time_st, addr_st = _rom_traces(curve, lens, 41)
    leaves, fields, tree = _host(curve, ROM, time_st, addr_st)
    assert fields[1][0] != fields[1][1] and fields[3][0] == fields[3][1] != 0      # orders differ midway, agree at the end
    _check_arrays(ctx_bn254, curve, 2, _run(ctx_bn254, curve, ROM, time_st, addr_st), fields, tree)


def test_tree_of_1024_leaves(ctx_bn254):
    curve, n_sub = "bn254", 1024
    time_st, addr_st = _rom_traces(curve, [1] * n_sub, 51)
    leaves, fields, tree = _host(curve, ROM, time_st, addr_st)
    _check_arrays(ctx_bn254, curve, 2, _run(ctx_bn254, curve, ROM, time_st, addr_st), fields, tree)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_device_resident_inputs_and_outputs_feed_poseidon_path(curve, ctx_bn254, ctx_bls):
    ctx = ctx_bn254 if curve == "bn254" else ctx_bls
    fc = FrCodec(curve)
    n_sub = 8
    lens = _lengths(n_sub, random.Random(61))
    time_st, addr_st = _rom_traces(curve, lens, 62)
    leaves, fields, tree = _host(curve, ROM, time_st, addr_st)
    chal = RunningEvaluation.new(ROM, COM, CURVE_PARAMS[curve]["r"]).challenges
    offsets, time_b = transcript.flatten_subtraces(fc, time_st)
    _, addr_b = transcript.flatten_subtraces(fc, addr_st)
    params = device_params(curve, fc)
    bufs = [capi.DeviceBuffer.from_host(ctx, x) for x in (time_b, addr_b)]
    outs = ctx.exec_tree(params, 2, offsets, bufs[0], bufs[1], chal, device_out=True)
    assert all(isinstance(x, capi.DeviceBuffer) for x in outs)
    _check_arrays(ctx, curve, 2, [x.to_host() for x in outs], fields, tree)
    # leaves and siblings go to hk_poseidon_path as they are
    leaf_cfg, node_cfg = merkle_params(curve)
    traces = [poseidon_path_trace(leaf_cfg, node_cfg, fields[i], *tree.path(i)) for i in range(n_sub)]
    block = len(traces[0])
    z = capi.DeviceBuffer.from_host(ctx, np.zeros(n_sub * block * ctx.fr_bytes, np.uint8))
    ctx.poseidon_path(params, outs[1], outs[3], np.arange(n_sub, dtype=np.uint32), block, 0, z)
    got = z.to_host().reshape(n_sub, block * ctx.fr_bytes)
    root = fc.dec(outs[4].to_host())[0]
    for i in range(n_sub):
        assert fc.dec(got[i]) == traces[i], i
        assert traces[i][-2] == root                               # state[1] of the last permutation
    for x in list(outs) + bufs + [z]:
        x.free()


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_sha_merkle_job_set_challenges_on_the_device(curve, ctx_bn254, ctx_bls):
    ctx = ctx_bn254 if curve == "bn254" else ctx_bls
    rnd = random.Random(71)
    data = [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(4)]
    r = CURVE_PARAMS[curve]["r"]
    ech, tr = rnd.randrange(r), rnd.randrange(r)
    host = ShaMerkleJob(curve, 8, 1, 4, data)
    host.set_challenges(ech, tr)
    dev = ShaMerkleJob(curve, 8, 1, 4, data)
    dev.set_challenges(ech, tr, ctx=ctx)
    assert (dev.time_eval0, dev.addr_eval0, dev.root) == (host.time_eval0, host.addr_eval0, host.root)
    for i in range(8):
        assert dev.tree.path(i) == host.tree.path(i)
        assert dev.inputs(i)["path"] == host.inputs(i)["path"]


def test_refusals_leave_the_outputs_untouched(ctx_bn254):
    ctx, curve = ctx_bn254, "bn254"
    fc = FrCodec(curve)
    fr = ctx.fr_bytes
    consts, n_consts, ld, nd = device_params(curve, fc)
    entries = fc.enc(list(range(1, 1 + 8 * 4)))                    # enough for 8 entries of either width
    chal = fc.enc([5, 6, 7, 8])
    outs = [np.full(64 * fr, 0xA5, np.uint8) for _ in range(5)]

    def call(n_sub, k, offsets, leaf=ld, n_c=n_consts):
        off = np.array(offsets, np.uint32)
        a, b = capi.hk_poseidon_desc(*leaf), capi.hk_poseidon_desc(*nd)
        d = capi.hk_exec_tree_desc(n_sub, k, off.ctypes.data, entries.ctypes.data, entries.ctypes.data, chal.ctypes.data,
                                   consts.ctypes.data, n_c, C.pointer(a), C.pointer(b))
        o = capi.hk_exec_tree_out(*[x.ctypes.data for x in outs])
        return ctx.lib.hk_exec_tree(ctx.handle, C.byref(d), C.byref(o))

    refused = [call(1, 2, [0, 2]),                                 # n_sub 1
               call(6, 2, [0, 1, 2, 3, 4, 5, 6]),                  # n_sub 6
               call(4, 3, [0, 1, 2, 3, 4]),                        # entry_fields 3
               call(4, 2, [1, 1, 2, 3, 4]),                        # offsets[0] != 0
               call(4, 2, [0, 3, 2, 3, 4]),                        # decreasing offsets
               call(4, 2, [0, 1, 2, 3, 4], leaf=(5,) + ld[1:]),    # a descriptor with t = 5
               call(4, 2, [0, 1, 2, 3, 4], n_c=n_consts - 4)]      # n_consts four short
    assert refused == [capi.HK_ERR_ARG] * 7
    assert all((x == 0xA5).all() for x in outs)
    # the same arguments, well-formed, are accepted and the lane is still usable
    assert call(4, 2, [0, 1, 2, 3, 4]) == capi.HK_OK
    assert not (outs[4][:fr] == 0xA5).all()
