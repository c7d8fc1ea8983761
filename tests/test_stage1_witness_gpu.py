"""GPU: hk_stage1_witness (csrc/stage1.cuh) against the host mirror, byte for byte on both curves - sha_circuit.full_values
for the three instance values and the portal block, sha_circuit.poseidon_path_trace for the membership block, both fed from
transcript.running_evaluations + poseidon.ExecTree and never from the device.  Every z_out starts as a byte pattern and every
column outside the three written ranges is asserted unchanged, column 0 included.

Shapes are the smallest that reach each boundary of the two kernels:
  8 x 4, rows [5, 0, 7, 2, 2]   unordered, a repeat, the first and the last subcircuit; the address steps hold d = 0 inside a
                                subcircuit, d = 0 across a boundary, d = 1, d > 1, values 0 and r - 1
  2 x 1                         depth 1, one entry per order: the shortest chains and path
  unsorted addresses            a step that wraps to r - delta (the witness of a false statement is still defined)
  128 x 1, 65 rows              two workgroups of quads, the second with one row and 63 quads that recompute it and store
                                nothing; 12 lanes per row of k_s1_values over four workgroups
Each host reference is computed once per session (functools.lru_cache) and never modified."""
import ctypes as C
import random
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from hekaton_system_amd import capi, transcript
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.poseidon import ExecTree, device_params, merkle_params
from hekaton_system_amd.sha_circuit import ShaMerkleJob, full_values, poseidon_inputs, poseidon_path_trace
from hekaton_system_amd.transcript import ROM, RomTranscriptEntry, RunningEvaluation

pytestmark = pytest.mark.gpu

COM = b"stage-1 witness test: the super commitment's bytes"
N_INST = 4


def _ctx(curve, ctx_bn254, ctx_bls):
    return ctx_bn254 if curve == "bn254" else ctx_bls


def _pattern(nbytes, seed=0):
    """The prefill of a z_out: no 32-byte run of it is a value the call writes."""
    return ((np.arange(nbytes, dtype=np.uint64) * 131 + 89 + seed) % 251).astype(np.uint8)


class _Case:
    """One job's two traces (lists of (addr, val) per subcircuit, k entries each) with everything the host mirror gives:
    challenges, the leaf fields after every subcircuit, the tree, and per subcircuit the expected instance values, portal
    block and membership block as Montgomery bytes."""

    def __init__(self, curve, time, addr):
        self.curve, self.time, self.addr = curve, time, addr
        self.n, self.k = len(time), len(time[0])
        self.fc = fc = FrCodec(curve)
        self.r = r = CURVE_PARAMS[curve]["r"]
        entries = lambda tr: [[RomTranscriptEntry(a % r, v % r) for a, v in st] for st in tr]
        self.chal = RunningEvaluation.new(ROM, COM, r).challenges
        leaves = transcript.running_evaluations(ROM, COM, r, entries(time), entries(addr))
        self.fields = [[ev.time_ordered_eval, ev.addr_ordered_eval] + last.to_field_elements() for ev, last in leaves]
        self.tree = ExecTree(curve, self.fields)
        self.depth = self.tree.depth
        self.offsets = np.arange(self.n + 1, dtype=np.uint32) * self.k
        flat = lambda tr: fc.enc([x % r for st in tr for e in st for x in e])
        self.time_b, self.addr_b = flat(time), flat(addr)
        self.params = device_params(curve, fc)
        # full_values' view of a class of k portals: the block starts behind the instance and the membership block follows
        self.layout = SimpleNamespace(r=r, N_INST=N_INST, pos_col0=N_INST + 10 * self.k + 4, kind="leaf", fc=fc)
        leaf_cfg, node_cfg = merkle_params(curve)
        self.block = len(poseidon_path_trace(leaf_cfg, node_cfg, self.fields[0], *self.tree.path(0)))
        self._cfgs = (leaf_cfg, node_cfg)

    def inputs(self, i):
        """The Stage1Request of subcircuit i (coordinator.rs:569-604) as full_values reads it."""
        return dict(entry_chal=self.chal[0], tr_chal=self.chal[1], root=self.tree.root, time=self.time[i], addr=self.addr[i],
                    time_eval0=self.fields[i - 1][0] if i else 1, addr_eval0=self.fields[i - 1][1] if i else 1,
                    prev=self.addr[i - 1][-1] if i else (0, 0), path=self.tree.path(i))

    @lru_cache(maxsize=None)
    def row(self, i):
        """(instance 3 Fr, portal block 10 k + 4 Fr, membership block) of subcircuit i, Montgomery bytes"""
        cols, vals = full_values(self.layout, [self.inputs(i)])
        assert cols.tolist() == [1, 2, 3] + list(range(N_INST, N_INST + 10 * self.k + 4))
        trace = poseidon_path_trace(*self._cfgs, self.fields[i], *self.tree.path(i))
        assert trace[-2] == self.tree.root                         # state[1] of the last permutation
        return vals[0][:96].copy(), vals[0][96:].copy(), self.fc.enc(trace)

    def expect(self, sub_index, n_v, cols3, prefill):
        """z_out after the call: the prefill with the three ranges of every row replaced"""
        z = prefill.copy().reshape(len(sub_index), n_v * 32)
        for b, i in enumerate(sub_index):
            for c0, part in zip(cols3, self.row(int(i))):
                z[b, c0 * 32:c0 * 32 + part.size] = part
        return z.reshape(-1)


def _exec_outs(ctx, case, **kw):
    return ctx.exec_tree(case.params, 2, case.offsets, case.time_b, case.addr_b, case.chal, **kw)


def _check(ctx, case, sub_index, cols3=None, tail=5):
    """exec_tree then stage1_witness over host arrays; the whole z_out against the mirror.  Returns (z bytes, exec outs)."""
    k = case.k
    cols3 = cols3 or (1, N_INST, N_INST + 10 * k + 4)
    n_v = max(c + ln for c, ln in zip(cols3, (3, 10 * k + 4, case.block))) + tail
    prefill = _pattern(len(sub_index) * n_v * 32)
    z = capi.DeviceBuffer.from_host(ctx, prefill)
    outs = _exec_outs(ctx, case)
    ctx.stage1_witness(case.params, k, case.offsets, case.time_b, case.addr_b, case.chal, outs, sub_index, n_v, cols3, z)
    got = z.to_host()
    z.free()
    want = case.expect(sub_index, n_v, cols3, prefill)
    if not (got == want).all():
        bad = np.flatnonzero((got != want).reshape(-1, 32).any(axis=1))
        raise AssertionError("first differing (row, column): %s of %d differing" % (divmod(int(bad[0]), n_v), bad.size))
    return got.reshape(len(sub_index), n_v, 32), outs


# ---- 1. directed traces ---------------------------------------------------------------------------------------------
DIRECTED_ROWS = [5, 0, 7, 2, 2]


@lru_cache(maxsize=None)
def _directed(curve):
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(17)
    addrs = [[0, 0, 1, 2], [3, 4, 5, 5], [5, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15], [16, 17, 40, 41], [42, 43, 44, 45],
             [46, 47, 47, 48]]
    by_addr = {}
    for a in sorted({a for st in addrs for a in st}):
        by_addr[a] = rnd.randrange(r)                              # one value per address: equal addresses, equal values
    by_addr[5], by_addr[17], by_addr[0] = r - 1, 0, 0
    addr = [[(a, by_addr[a]) for a in st] for st in addrs]
    flat = [e for st in addr for e in st]
    rnd.shuffle(flat)                                              # the time order: the same multiset
    time = [flat[4 * i:4 * i + 4] for i in range(8)]
    return _Case(curve, time, addr)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_directed_rom_traces(curve, ctx_bn254, ctx_bls):
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    case = _directed(curve)
    r, k = case.r, case.k
    # the premises, over the selected rows: the address steps and values the trace was built to hold
    inner, edge, vals = [], [], []
    for i in set(DIRECTED_ROWS):
        chain = [case.inputs(i)["prev"]] + case.addr[i]
        steps = [(b[0] - a[0]) % r for a, b in zip(chain, chain[1:])]
        edge.append((i, steps[0]))
        inner += steps[1:]
        vals += [v for _a, v in case.addr[i]]
    assert 0 in inner and 1 in inner and any(1 < d < r // 2 for d in inner)
    assert (0, 0) in edge and (2, 0) in edge and (5, 1) in edge    # d = 0 behind the padding and across the 1 | 2 boundary
    assert 0 in vals and r - 1 in vals
    assert case.fields[-1][0] == case.fields[-1][1]               # the same multiset in both orders
    got, outs = _check(ctx, case, DIRECTED_ROWS)
    # each row's two chains end on the evaluations hk_exec_tree gave for its subcircuit
    evals = np.asarray(outs[0]).reshape(case.n, 2, 32)
    t_end, a_end = N_INST + 4 * k + 2 * k, N_INST + 4 * k + (1 + 2 * k) + 2 * k
    for b, i in enumerate(DIRECTED_ROWS):
        assert (got[b, t_end] == evals[i, 0]).all() and (got[b, a_end] == evals[i, 1]).all(), (b, i)
    # the same rows under another layout: the membership block first, gaps between the three ranges
    _check(ctx, case, DIRECTED_ROWS, cols3=(case.block + 9, case.block + 20, 2), tail=1)


# ---- 2. the smallest shape ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_two_subcircuits_of_one_entry(curve, ctx_bn254, ctx_bls):
    r = CURVE_PARAMS[curve]["r"]
    case = _Case(curve, [[(1, r - 1)], [(0, 0)]], [[(0, 0)], [(1, r - 1)]])
    assert case.depth == 1
    _check(_ctx(curve, ctx_bn254, ctx_bls), case, [1, 0])
    _check(_ctx(curve, ctx_bn254, ctx_bls), case, [0])


# ---- 3. an address order that is not sorted ----------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_unsorted_address_buffer(curve, ctx_bn254, ctx_bls):
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(23)
    addr = [[(9, rnd.randrange(r)), (4, rnd.randrange(r))], [(3, rnd.randrange(r)), (3, rnd.randrange(r))],
            [(1 << 40, rnd.randrange(r)), (7, rnd.randrange(r))], [(8, 0), (2, r - 1)]]
    time = [list(reversed(st)) for st in reversed(addr)]
    case = _Case(curve, time, addr)
    steps = [(b[0] - a[0]) % r for i in range(4) for a, b in zip([case.inputs(i)["prev"]] + addr[i], addr[i])]
    assert r - 5 in steps and r - 1 in steps and (7 - (1 << 40)) % r in steps and 0 in steps     # wrapped, within and across
    _check(_ctx(curve, ctx_bn254, ctx_bls), case, [0, 1, 2, 3])


# ---- 4. a partly filled second workgroup -------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _wide(curve):
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(29)
    addr = [[(i // 2, rnd.randrange(r))] for i in range(128)]
    flat = [st[0] for st in addr]
    rnd.shuffle(flat)
    return _Case(curve, [[e] for e in flat], addr)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_sixty_five_rows_of_128_subcircuits(curve, ctx_bn254, ctx_bls):
    case = _wide(curve)
    rnd = random.Random(31)
    rows = [rnd.randrange(128) for _ in range(65)]
    rows[0], rows[63], rows[64] = 127, 0, 101                      # the last row of the batch sits alone in its workgroup
    assert case.depth == 7
    _check(_ctx(curve, ctx_bn254, ctx_bls), case, rows)


# ---- 5. the device-resident chain --------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_device_resident_chain_equals_host_inputs(curve, ctx_bn254, ctx_bls):
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    case = _directed(curve)
    k = case.k
    cols3 = (1, N_INST, N_INST + 10 * k + 4)
    n_v = cols3[2] + case.block + 3
    rows = [3, 4, 6, 1, 0]
    prefill = _pattern(len(rows) * n_v * 32, seed=5)
    # hk_exec_tree -> hk_stage1_witness with traces, constants and every intermediate in device memory, nothing read back
    bufs = [capi.DeviceBuffer.from_host(ctx, x) for x in (case.time_b, case.addr_b, case.params[0])]
    params_d = (bufs[2],) + case.params[1:]
    outs_d = ctx.exec_tree(params_d, 2, case.offsets, bufs[0], bufs[1], case.chal, device_out=True)
    assert all(isinstance(x, capi.DeviceBuffer) for x in outs_d)
    z_d = capi.DeviceBuffer.from_host(ctx, prefill)
    ctx.stage1_witness(params_d, k, case.offsets, bufs[0], bufs[1], case.chal, outs_d, rows, n_v, cols3, z_d)
    got_d = z_d.to_host()
    # all-host inputs
    outs_h = _exec_outs(ctx, case)
    z_h = capi.DeviceBuffer.from_host(ctx, prefill)
    ctx.stage1_witness(case.params, k, case.offsets, case.time_b, case.addr_b, case.chal, outs_h, rows, n_v, cols3, z_h)
    got_h = z_h.to_host()
    for x in bufs + list(outs_d) + [z_d, z_h]:
        x.free()
    assert (got_d == got_h).all()
    assert (got_d == case.expect(rows, n_v, cols3, prefill)).all()


# ---- 6. a whole job through ShaMerkleJob.stage1_device -------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_sha_merkle_job_stage1_device_fills_every_class(curve, ctx_bn254, ctx_bls):
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    rnd = random.Random(37)
    data = [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(4)]
    r = CURVE_PARAMS[curve]["r"]
    job = ShaMerkleJob(curve, 8, 1, 4, data)
    job.set_challenges(rnd.randrange(r), rnd.randrange(r))         # the host path: the reference of this test
    before = (list(job.time_eval0), list(job.addr_eval0), job.root)
    dev = job.stage1_device(ctx)
    assert dev.root == job.root and (job.time_eval0, job.addr_eval0, job.root) == before
    classes = {}
    for i in range(job.n):
        classes.setdefault(job.class_of(i), []).append(i)
    assert len(classes) == 5
    fc = FrCodec(curve)
    params = device_params(curve, fc)
    leaf_cfg, node_cfg = merkle_params(curve)
    for key, members in classes.items():
        circ = job.make_class(members[0])
        prefill = _pattern(len(members) * circ.n_v * 32, seed=len(members))
        # the parent path: full_values + poseidon_inputs on the host, then the two existing calls
        ws = [job.inputs(i) for i in members]
        cols, vals = full_values(circ, ws)
        leaves, sibs, idx = poseidon_inputs(circ, ws)
        z_ref = capi.DeviceBuffer.from_host(ctx, prefill)
        vals = np.ascontiguousarray(vals)
        capi.check(ctx.lib.hk_assignment_scatter(ctx.handle, cols.ctypes.data, vals.ctypes.data, cols.size, len(members), circ.n_v,
                                                 z_ref.ptr), "hk_assignment_scatter")
        ctx.poseidon_path(params, leaves, sibs, idx, circ.n_v, circ.pos_col0, z_ref)
        z_new = capi.DeviceBuffer.from_host(ctx, prefill)
        assert dev.fill(circ, members, z_new) is z_new
        want, got = z_ref.to_host(), z_new.to_host()
        z_ref.free()
        z_new.free()
        assert (got == want).all(), key
        assert not (got == prefill).all()
        # both sides above run one membership kernel: the block itself against the host trace
        rows = got.reshape(len(members), circ.n_v, ctx.fr_bytes)
        for m, w in enumerate(ws):
            trace = poseidon_path_trace(leaf_cfg, node_cfg, fc.dec(leaves[m]), [s % r for s in w["path"][0]], w["path"][1])
            assert fc.dec(rows[m, circ.pos_col0:circ.pos_col0 + len(trace)].reshape(-1)) == trace, (key, members[m])
    dev.free()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_z_out_untouched(ctx_bn254):
    ctx, curve = ctx_bn254, "bn254"
    case = _directed(curve)
    fr = ctx.fr_bytes
    consts, n_consts, ld, nd = case.params
    k, block = case.k, case.block
    pos0 = N_INST + 10 * k + 4
    n_v = pos0 + block + 2
    outs = _exec_outs(ctx, case)
    chal = case.fc.enc(list(case.chal))
    prefill = _pattern(3 * n_v * fr, seed=9)
    z = capi.DeviceBuffer.from_host(ctx, prefill)
    uneven = case.offsets.copy()
    uneven[3] -= 1                                                 # subcircuit 2 owns 3 entries, subcircuit 3 owns 5

    def call(n_sub=8, n_portals=k, depth=3, offsets=case.offsets, rows=(1, 6, 6), leaf=ld, n_c=n_consts, cols3=(1, N_INST, pos0),
             null=None, batch=None, n_v_=n_v):
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        sub = np.array(rows, np.uint32)
        a, b = capi.hk_poseidon_desc(*leaf), capi.hk_poseidon_desc(*nd)
        d = capi.hk_stage1_desc(n_sub, n_portals, depth, off.ctypes.data, case.time_b.ctypes.data, case.addr_b.ctypes.data,
                                chal.ctypes.data, outs[0].ctypes.data, outs[1].ctypes.data, outs[3].ctypes.data,
                                outs[4].ctypes.data, consts.ctypes.data, n_c, C.pointer(a), C.pointer(b), *cols3)
        if null and null != "sub_index":
            setattr(d, null, None)
        return ctx.lib.hk_stage1_witness(ctx.handle, C.byref(d), None if null == "sub_index" else sub.ctypes.data,
                                         len(rows) if batch is None else batch, n_v_, z.ptr)

    refused = {name: call(null=name) for name in ("offsets", "time_entries_mont", "addr_entries_mont", "challenges_mont",
                                                  "evals_mont", "leaves_mont", "siblings_mont", "root_mont", "consts_mont",
                                                  "leaf_hash", "node_hash", "sub_index")}
    refused.update({
        "n_sub 6": call(n_sub=6, offsets=case.offsets[:7]),
        "n_sub 1": call(n_sub=1, depth=0, offsets=case.offsets[:2], rows=(0,)),
        "depth 2": call(depth=2),
        "depth 4": call(depth=4),
        "n_portals 0": call(n_portals=0),
        "offsets[0] 1": call(offsets=[1] + list(case.offsets[1:])),
        "decreasing offsets": call(offsets=[0, 4, 8, 7, 16, 20, 24, 28, 32]),
        "sub_index 8": call(rows=(1, 8, 6)),
        "3 entries": call(offsets=uneven, rows=(1, 2)),
        "5 entries": call(offsets=uneven, rows=(3,)),
        "another k": call(n_portals=3),
        "t 5": call(leaf=(5,) + ld[1:]),
        "leaf alpha 17": call(leaf=ld[:1] + (17,) + ld[2:]),
        "consts four short": call(n_c=n_consts - 4),
        "instance at column 0": call(cols3=(0, N_INST, pos0)),
        "portal block at column 0": call(cols3=(10 * k + 4, 0, pos0)),
        "instance past n_v": call(cols3=(n_v - 2, N_INST, pos0)),
        "membership past n_v": call(cols3=(1, N_INST, pos0 + 3)),
        "membership short of n_v by one": call(n_v_=pos0 + block - 1),
        "portal block past n_v by one": call(cols3=(1, n_v - 10 * k - 3, N_INST)),
        "instance in the portal block": call(cols3=(N_INST + 10 * k + 3, N_INST, pos0 + 2)),
        "portal block on the membership block's last column": call(cols3=(1, N_INST + block - 1, N_INST)),
        "instance in the membership block": call(cols3=(pos0 + block - 1, N_INST, pos0)),
    })
    assert refused == {name: capi.HK_ERR_ARG for name in refused}
    # the uneven offsets themselves are fine for the subcircuits that own k entries
    assert call(batch=0) == capi.HK_OK and call(rows=(), batch=0, null="sub_index") == capi.HK_OK
    assert (z.to_host() == prefill).all()
    # the same context still works: a valid call, and one over offsets where only the selected subcircuits own k entries
    assert call() == capi.HK_OK
    got = z.to_host()
    assert (got == case.expect([1, 6, 6], n_v, (1, N_INST, pos0), prefill)).all()
    assert call(offsets=uneven, rows=(0, 7, 5)) == capi.HK_OK
    z.free()
