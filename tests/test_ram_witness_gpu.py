"""GPU: hk_ram_stage0_witness / hk_ram_stage1_witness (csrc/ram_witness.cuh) against the host mirror
(vm_circuit.RamJob.stage0_ints / assignment_bytes), byte for byte over whole rows on both curves, and the chain
hk_trace_sort -> hk_exec_tree -> hk_ram_stage1_witness -> hk_r1cs_check without a host value in between.

Shapes, the smallest that reach each boundary:
  n_sub 2 (depth 1), 4, 8; ops 1 and 2; the first, middle and last class of each job
  t0 = 0, 2^16 - 5, 2^32 - 400     timestamp bits 8, 16, 24 and 31 are set somewhere (asserted)
  n_sub 8, ops 2 (288 entries)     a row's 4 000 columns cross many waves; batches of 65 (past one wave, repeats, arbitrary
                                   order) and 130 (past one 64-row membership workgroup)
  a random program, k = 100        four chunks per running-evaluation chain, the last of 4 entries (RW_CHUNK = 32); the VM jobs
                                   above have k = 19 (one chunk), 22, 35 and 38 (two)
Each host row is computed once per session and never modified."""
import ctypes as C
import dataclasses
from functools import lru_cache

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import FrCodec, r1cs_bad_rows
from hekaton_system_amd.poseidon import device_params
from hekaton_system_amd.vm_circuit import RamStage1Device
from tests.vm_cases import CHAL, T0S, TAMPERINGS, random_ram_job, vm_job

pytestmark = pytest.mark.gpu

CURVES = ("bn254", "bls12_381")
JOBS = ((1, 1, T0S[0]), (2, 1, T0S[1]), (3, 2, T0S[2]))


def _ctx(curve, ctx_bn254, ctx_bls):
    return ctx_bn254 if curve == "bn254" else ctx_bls


def _pattern(nbytes, seed=0):
    """The prefill of an output: no 32-byte run of it is a value the calls write."""
    return ((np.arange(nbytes, dtype=np.uint64) * 131 + 89 + seed) % 251).astype(np.uint8)


@lru_cache(maxsize=None)
def _job(curve, log_n, ops, t0):
    return vm_job(curve, log_n, ops, t0=t0)


@lru_cache(maxsize=None)
def _row(curve, log_n, ops, t0, idx):
    return _job(curve, log_n, ops, t0).assignment_bytes(idx)


def _members(job, which, batch):
    """`batch` subcircuits of one class in an arbitrary order, with repeats once the class runs out."""
    pool = {"first": [0], "last": [job.n - 1], "middle": list(range(1, job.n - 1))}[which]
    return [pool[(5 * b + 3) % len(pool)] for b in range(batch)]


def _fill(ctx, job, dev, members, template, prefill=None, **kw):
    circ = job.make_class(members[0])
    if prefill is None:
        prefill = _pattern(len(members) * circ.n_v * ctx.fr_bytes)
    z = capi.DeviceBuffer.from_host(ctx, prefill)
    try:
        dev.fill(circ, members, z, template=template, **kw)
        return z.to_host().reshape(len(members), circ.n_v * ctx.fr_bytes)
    finally:
        z.free()


def _diff(got, want, n_v):
    if not (got == want).all():
        bad = np.flatnonzero((got != want).reshape(-1, 32).any(axis=1))
        raise AssertionError("first differing (row, column): %s of %d differing" % (divmod(int(bad[0]), n_v), bad.size))


CASES = [(0, "first", 1), (0, "last", 1), (1, "first", 1), (1, "middle", 3), (1, "last", 1), (2, "first", 1), (2, "middle", 65),
         (2, "middle", 130), (2, "last", 3)]


def test_the_jobs_set_the_high_timestamp_bits():
    seen = 0
    for log_n, ops, t0 in JOBS:
        for st in _job("bn254", log_n, ops, t0).time:
            for e in st:
                seen |= e.i
    assert all(seen >> b & 1 for b in (0, 8, 16, 24, 31))


@pytest.mark.parametrize("curve", CURVES)
def test_stage0_rows_equal_the_host_mirror(curve, ctx_bn254, ctx_bls):
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    fc = FrCodec(curve)
    for jn, which, batch in CASES:
        if batch == 130:
            continue
        job = _job(curve, *JOBS[jn])
        if which == "middle" and job.n < 4:
            continue
        members = _members(job, which, batch)
        dev0 = job.stage0_device(ctx)
        try:
            w = dev0.rows(members)
            got = w.to_host().reshape(len(members), -1)
            w.free()
            # the address order the device sorted is the host's
            assert (dev0.traces[1].to_host() == job.flat("addr")).all()
        finally:
            dev0.free()
        for b, i in enumerate(members):
            assert (got[b] == fc.enc(job.stage0_ints(i))).all(), (jn, which, b)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("jn,which,batch", CASES)
def test_stage1_rows_equal_the_host_mirror_byte_for_byte(curve, jn, which, batch, ctx_bn254, ctx_bls):
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    job = _job(curve, *JOBS[jn])
    members = _members(job, which, batch)
    circ = job.make_class(members[0])
    dev = job.stage1_device(ctx)
    try:
        assert dev.root == job.root
        got = _fill(ctx, job, dev, members, template=True)
    finally:
        dev.free()
    want = np.stack([_row(curve, *JOBS[jn], i) for i in members])
    _diff(got, want, circ.n_v)


@lru_cache(maxsize=None)
def _long_job(curve):
    return random_ram_job(curve, seed=33, n_sub=4, k=100)


@pytest.mark.parametrize("curve", CURVES)
def test_chains_of_four_chunks_equal_the_host_mirror(curve, ctx_bn254, ctx_bls):
    """k = 100 = 3 x 32 + 4: every chain runs through k_rw_chunk_prod / _scan / _walk with chunks 0 .. 3, in batches where the
    chain index mixes row and order."""
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    job = _long_job(curve)
    assert {len(st) for st in job.time} == {100} and len({e.addr for st in job.time for e in st}) == 5
    dev = job.stage1_device(ctx)
    try:
        for members in ([2, 1, 1, 2, 1], [0, 0], [3, 3, 3]):
            circ = job.make_class(members[0])
            got = _fill(ctx, job, dev, members, template=True)
            want = np.stack([job.assignment_bytes(i) for i in sorted(set(members))])
            _diff(got, want[[sorted(set(members)).index(i) for i in members]], circ.n_v)
            # the chain columns themselves are in the comparison: the last cur of each order is the evaluation after the row
            fr = ctx.fr_bytes
            for b, i in enumerate(members):
                for y, ev in enumerate((job.time_eval0, job.addr_eval0)):
                    c = circ.col0 + 35 + y * 401 + 400
                    assert circ.fc.dec(got[b, c * fr:(c + 1) * fr]) == [ev[i + 1]]
    finally:
        dev.free()


@pytest.mark.parametrize("curve", CURVES)
def test_set_challenges_through_the_device_equals_the_host(curve, ctx_bn254, ctx_bls):
    """`RamJob.set_challenges(chals, ctx=ctx)`: evaluations, tree and root from one hk_exec_tree call (entry_fields = 4)."""
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    host = _job(curve, *JOBS[1])
    job = vm_job(curve, *JOBS[1][:2], t0=JOBS[1][2], chal=None)
    job.set_challenges(CHAL, ctx=ctx)
    assert job.chal == host.chal and job.root == host.root
    assert job.time_eval0 == host.time_eval0 and job.addr_eval0 == host.addr_eval0
    assert job.tree.levels == host.tree.levels and job.tree.leaves == host.tree.leaves
    assert all(job.tree.path(i) == host.tree.path(i) for i in range(job.n))
    assert job.assignment_ints(2) == host.assignment_ints(2)
    # ... and from the super commitment's bytes, hashed to the four RAM challenges
    com = b"a super commitment's bytes"
    a, b = vm_job(curve, 1, 1, chal=None), vm_job(curve, 1, 1, chal=None)
    a.set_challenges(com)
    b.set_challenges(com, ctx=ctx)
    assert len(a.chal) == 4 and a.chal == b.chal and a.root == b.root and a.time_eval0 == b.time_eval0


@pytest.mark.parametrize("curve", CURVES)
def test_without_a_template_the_other_columns_keep_their_bytes(curve, ctx_bn254, ctx_bls):
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    job = _job(curve, *JOBS[1])
    members = [2, 1, 1]
    circ = job.make_class(1)
    assert circ.dummy_products and circ.dummy_col0 < circ.n_v
    fr = ctx.fr_bytes
    prefill = _pattern(3 * circ.n_v * fr, seed=4)
    dev = job.stage1_device(ctx)
    try:
        got = _fill(ctx, job, dev, members, template=False, prefill=prefill)
    finally:
        dev.free()
    want = prefill.copy().reshape(3, circ.n_v * fr)
    for b, i in enumerate(members):
        want[b, fr:circ.dummy_col0 * fr] = _row(curve, *JOBS[1], i)[fr:circ.dummy_col0 * fr]
    _diff(got, want, circ.n_v)


def test_host_device_and_mixed_inputs_and_two_runs_give_equal_bytes(ctx_bn254):
    ctx, curve = ctx_bn254, "bn254"
    job = _job(curve, *JOBS[1])
    fc = FrCodec(curve)
    members = np.array([1, 2, 2], np.uint32)
    circ = job.make_class(1)
    params = device_params(curve, fc)
    time_b, addr_b = job.flat("time"), job.flat("addr")
    outs = ctx.exec_tree(params, 4, job.offsets, time_b, addr_b, job.chal)
    tmpl = fc.enc(circ.template_ints())
    layout = (1, circ.N_INST, circ.col0, circ.pos_col0)
    up = lambda x: capi.DeviceBuffer.from_host(ctx, x)
    dev_all = [up(x) for x in (time_b, addr_b) + tuple(outs) + (tmpl,)]
    want = np.stack([_row(curve, *JOBS[1], int(i)) for i in members])
    variants = {"host": [time_b, addr_b, *outs, tmpl], "device": dev_all,
                "mixed": [dev_all[0], addr_b, outs[0], dev_all[3], outs[2], dev_all[5], outs[4], dev_all[7]],
                "device again": dev_all}
    for name, (t, a, ev, lf, nd, sb, rt, tm) in variants.items():
        z = capi.DeviceBuffer.from_host(ctx, _pattern(3 * circ.n_v * 32, seed=2))
        ctx.ram_stage1_witness(params, circ.np_, job.offsets, t, a, job.chal, (ev, lf, nd, sb, rt), members, circ.n_v, layout, z,
                               template=tm)
        got = z.to_host().reshape(3, -1)
        z.free()
        _diff(got, want, circ.n_v)
    # stage 0 from host-resident traces
    w = capi.DeviceBuffer(ctx, 3 * 70 * circ.np_ * 32)
    ctx.ram_stage0_witness(job.offsets, circ.np_, time_b, dev_all[1], members, w)
    got = w.to_host().reshape(3, -1)
    w.free()
    for b, i in enumerate(members):
        assert (got[b] == fc.enc(job.stage0_ints(int(i)))).all()
    for x in dev_all:
        x.free()


# ---- the chain end to end on the device -------------------------------------------------------------------------------
def _classes(job):
    groups = {}
    for idx in range(job.n):
        groups.setdefault(job.class_of(idx), []).append(idx)
    return list(groups.values())


@pytest.mark.parametrize("curve", CURVES)
def test_the_chain_satisfies_the_r1cs_on_the_device(curve, ctx_bn254, ctx_bls):
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    job = vm_job(curve, 2, 1, t0=T0S[2], chal=None)
    job.chal = CHAL                                        # nothing of the round is computed on the host
    dev = job.stage1_device(ctx)
    host = _job(curve, 2, 1, T0S[2])
    try:
        for members in _classes(job):
            circ = job.make_class(members[0])
            z = capi.DeviceBuffer(ctx, len(members) * circ.n_v * ctx.fr_bytes)
            dev.fill(circ, members, z)
            verdicts = ctx.r1cs_check(*circ.csr(circ.fc), z, n_v=circ.n_v, batch=len(members))
            got = z.to_host().reshape(len(members), -1)
            z.free()
            assert verdicts == [(0, None)] * len(members)
            for b, i in enumerate(members):
                assert (got[b] == host.assignment_bytes(i)).all()
    finally:
        dev.free()


def _device_verdicts(ctx, job, patch=None):
    """[(n_bad, first_bad)] per subcircuit from rows made on the device out of the job's (tampered) traces."""
    up = lambda x: capi.DeviceBuffer.from_host(ctx, x)
    traces = [up(job.flat("time")), up(job.flat("addr"))]
    dev = RamStage1Device(job, ctx, traces=traces)
    out = [None] * job.n
    try:
        for members in _classes(job):
            circ = job.make_class(members[0])
            z = capi.DeviceBuffer(ctx, len(members) * circ.n_v * ctx.fr_bytes)
            dev.fill(circ, members, z)
            if patch:
                patch(circ, members, z)
            for i, v in zip(members, ctx.r1cs_check(*circ.csr(circ.fc), z, n_v=circ.n_v, batch=len(members))):
                out[i] = v
            z.free()
    finally:
        dev.free()
        for x in traces:
            x.free()
    return out


@pytest.mark.parametrize("tamper", TAMPERINGS, ids=lambda f: f.__name__)
def test_a_tampered_trace_fails_where_the_host_mirror_says(tamper, ctx_bn254):
    ctx = ctx_bn254
    job = vm_job("bn254", 2, 1, chal=None)
    sub, _block, _pair, _rule = tamper(job)
    job.set_challenges(CHAL)
    want = []
    for idx in range(job.n):
        circ = job.make_class(idx)
        bad = r1cs_bad_rows(*circ.rows(), job.assignment_ints(idx), circ.r)
        want.append((len(bad), bad[0] if bad else None))
    assert want[sub][0] >= 1
    assert _device_verdicts(ctx, job) == want


def test_a_tampered_frame_of_subcircuit_0_fails_where_the_host_mirror_says(ctx_bn254):
    """Tampering 7: the device call always writes the padding entry and the evaluation 1 in front of entry 0, so the row is
    patched after the call (hk_assignment_scatter) and the same patched row goes through the host mirror."""
    ctx = ctx_bn254
    job = _job("bn254", 2, 1, T0S[1])
    circ0 = job.make_class(0)
    fc = circ0.fc
    for col, val in ((circ0.col0, 5), (circ0.col0 + 35, 2), (circ0.col0 + 35 + 1 + 4 * circ0.np_, 2)):
        def patch(circ, members, z):
            if members[0] == 0:
                cols, vals = np.array([col], np.uint32), fc.enc([val])
                capi.check(ctx.lib.hk_assignment_scatter(ctx.handle, cols.ctypes.data, vals.ctypes.data, 1, 1, circ.n_v, z.ptr),
                           "hk_assignment_scatter")
        z = job.assignment_ints(0)
        z[col] = val
        bad = r1cs_bad_rows(*circ0.rows(), z, circ0.r)
        assert bad and circ0.block_of(bad[0]) in ("prev", "time_chain", "addr_chain")
        got = _device_verdicts(ctx, job, patch)
        assert got[0] == (len(bad), bad[0]) and got[1:] == [(0, None)] * 3


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _with(job, sub, j, order, **changes):
    """A copy of the job's flattened traces with one entry of subcircuit `sub` replaced (Montgomery bytes)."""
    tr = {"time": [list(st) for st in job.time], "addr": [list(st) for st in job.addr]}
    tr[order][sub][j] = dataclasses.replace(tr[order][sub][j], **changes)
    fc = FrCodec(job.curve)
    return [fc.enc([x % job.r for st in tr[o] for e in st for x in e.to_field_elements()]) for o in ("time", "addr")]


def test_refusals_leave_the_outputs_untouched(ctx_bn254):
    ctx, curve = ctx_bn254, "bn254"
    job = _job(curve, *JOBS[1])
    fc = FrCodec(curve)
    fr = ctx.fr_bytes
    circ = job.make_class(1)
    k, n_v = circ.np_, circ.n_v
    consts, n_consts, ld, nd = params = device_params(curve, fc)
    time_b, addr_b = job.flat("time"), job.flat("addr")
    outs = ctx.exec_tree(params, 4, job.offsets, time_b, addr_b, job.chal)
    chal = fc.enc(list(job.chal))
    tmpl = fc.enc(circ.template_ints())
    prefill = _pattern(2 * n_v * fr, seed=9)
    z = capi.DeviceBuffer.from_host(ctx, prefill)
    w_prefill = _pattern(2 * 70 * k * fr, seed=3)
    w = capi.DeviceBuffer.from_host(ctx, w_prefill)
    host_out = np.zeros(2 * n_v * fr, np.uint8)
    cols4 = (1, circ.N_INST, circ.col0, circ.pos_col0)
    block = circ.pos_cols
    offs = [int(x) for x in job.offsets]

    def call1(n_sub=4, n_portals=k, depth=2, offsets=offs, rows=(1, 2), leaf=ld, node=nd, n_c=n_consts, cols=cols4, null=None,
              batch=None, n_v_=n_v, traces=(time_b, addr_b), out=None):
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        sub = np.array(rows, np.uint32)
        a, b = capi.hk_poseidon_desc(*leaf), capi.hk_poseidon_desc(*node)
        d = capi.hk_ram_stage1_desc(n_sub, n_portals, depth, off.ctypes.data, traces[0].ctypes.data, traces[1].ctypes.data,
                                    chal.ctypes.data, outs[0].ctypes.data, outs[1].ctypes.data, outs[3].ctypes.data,
                                    outs[4].ctypes.data, consts.ctypes.data, n_c, C.pointer(a), C.pointer(b), tmpl.ctypes.data,
                                    *cols)
        if null and null != "sub_index":
            setattr(d, null, None)
        return ctx.lib.hk_ram_stage1_witness(ctx.handle, C.byref(d), None if null == "sub_index" else sub.ctypes.data,
                                             len(rows) if batch is None else batch, n_v_, z.ptr if out is None else out)

    def call0(n_sub=4, n_portals=k, offsets=offs, rows=(1, 2), null=None, batch=None, traces=(time_b, addr_b), out=None):
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        sub = np.array(rows, np.uint32)
        args = dict(offsets=off.ctypes.data, time=traces[0].ctypes.data, addr=traces[1].ctypes.data, sub_index=sub.ctypes.data)
        if null:
            args[null] = None
        return ctx.lib.hk_ram_stage0_witness(ctx.handle, args["offsets"], n_sub, n_portals, args["time"], args["addr"],
                                             args["sub_index"], len(rows) if batch is None else batch, w.ptr if out is None else out)

    uneven = list(offs)
    uneven[2] -= 1                                                 # subcircuit 1 owns k - 1 entries, subcircuit 2 owns k + 1
    big_ts = _with(job, 1, 3, "time", i=1 << 32)
    big_ts_addr = _with(job, 2, 0, "addr", i=(1 << 32) + 7)
    read2 = _with(job, 2, 5, "addr", read=2)
    read2_time = _with(job, 1, 0, "time", read=2)
    refused = {"1: null " + name: call1(null=name) for name in
               ("offsets", "time_entries_mont", "addr_entries_mont", "challenges_mont", "evals_mont", "leaves_mont", "siblings_mont",
                "root_mont", "consts_mont", "leaf_hash", "node_hash", "sub_index")}
    refused.update({"0: null " + name: call0(null=name) for name in ("offsets", "time", "addr", "sub_index")})
    refused.update({
        "1: n_sub 3": call1(n_sub=3, offsets=offs[:4]),
        "1: n_sub 1": call1(n_sub=1, depth=0, offsets=offs[:2], rows=(0,), n_portals=offs[1]),
        "1: depth 1": call1(depth=1),
        "1: depth 3": call1(depth=3),
        "1: n_portals 0": call1(n_portals=0),
        "0: n_portals 0": call0(n_portals=0),
        "1: offsets[0] 1": call1(offsets=[1] + offs[1:]),
        "0: offsets[0] 1": call0(offsets=[1] + offs[1:]),
        "1: decreasing offsets": call1(offsets=[0, 60, 50, 89, 124]),
        "0: decreasing offsets": call0(offsets=[0, 60, 50, 89, 124]),
        "1: sub_index 4": call1(rows=(1, 4)),
        "0: sub_index 4": call0(rows=(1, 4)),
        "1: k - 1 entries": call1(offsets=uneven, rows=(1,)),
        "1: k + 1 entries": call1(offsets=uneven, rows=(2,)),
        "0: k - 1 entries": call0(offsets=uneven, rows=(1,)),
        "1: the first class's k": call1(rows=(0, 1)),
        "0: the first class's k": call0(rows=(0, 1)),
        "1: t 5": call1(leaf=(5,) + ld[1:]),
        "1: leaf alpha 17": call1(leaf=ld[:1] + (17,) + ld[2:]),
        "1: consts four short": call1(n_c=n_consts - 4),
        "1: node t 4": call1(node=(4,) + nd[1:]),
        "1: node alpha 5": call1(node=nd[:1] + (5,) + nd[2:]),
        "1: node rounds odd": call1(node=nd[:2] + (nd[2] + 1,) + nd[3:]),
        "1: z_out NULL": call1(out=0),
        "0: w_out NULL": call0(out=0),
        # lane counts (include/hekaton.h): refused before sub_index or a trace is read
        "1: k 2^16 + 1": call1(n_portals=(1 << 16) + 1),
        "0: k 2^16 + 1": call0(n_portals=(1 << 16) + 1),
        "1: batch 2^20": call1(batch=1 << 20),
        "0: batch 2^20": call0(batch=1 << 20),
        "1: batch x (40 + 105 k) >= 2^38": call1(n_portals=1 << 16, batch=1 << 16),
        "0: batch x (40 + 105 k) >= 2^38": call0(n_portals=1 << 16, batch=1 << 16),
        "1: batch x n_v >= 2^38": call1(batch=1 << 19, n_v_=1 << 19),
        "1: instance at column 0": call1(cols=(0,) + cols4[1:]),
        "1: stage 0 at column 0": call1(cols=(n_v - 5, 0, cols4[2], cols4[3])),
        "1: instance past n_v": call1(cols=(n_v - 4,) + cols4[1:]),
        "1: membership past n_v": call1(n_v_=circ.pos_col0 + block - 1),
        "1: instance in stage 0": call1(cols=(circ.N_INST + 3,) + cols4[1:]),
        "1: stage 0 over the portal block's first column": call1(cols=(1, circ.N_INST + 1, cols4[2], cols4[3])),
        "1: portal block over the membership block's first column": call1(cols=(1, circ.N_INST, cols4[2] + 1, cols4[3])),
        "1: z_out on the host": call1(out=host_out.ctypes.data),
        "0: w_out on the host": call0(out=host_out.ctypes.data),
        # found on the device
        "1: timestamp 2^32 (time order)": call1(traces=big_ts),
        "0: timestamp 2^32 (time order)": call0(traces=big_ts),
        "1: timestamp 2^32 + 7 (address order)": call1(traces=big_ts_addr),
        "0: timestamp 2^32 + 7 (address order)": call0(traces=big_ts_addr),
        "1: read 2 (address order)": call1(traces=read2),
        "0: read 2 (address order)": call0(traces=read2),
        "1: read 2 (time order)": call1(traces=read2_time),
        "0: read 2 (time order)": call0(traces=read2_time),
    })
    assert refused == {name: capi.HK_ERR_ARG for name in refused}
    assert call1(batch=0) == capi.HK_OK and call1(rows=(), batch=0, null="sub_index") == capi.HK_OK
    assert call0(batch=0) == capi.HK_OK and call0(rows=(), batch=0, null="sub_index") == capi.HK_OK
    assert (z.to_host() == prefill).all() and (w.to_host() == w_prefill).all() and not host_out.any()
    # the same bad value in a subcircuit that is NOT selected does not refuse - not even in the entry in front of the selected
    # one - and the lane still works: the rows are the honest ones wherever the bad entry is not read
    assert call1(traces=big_ts, rows=(2, 3)) == capi.HK_OK and call0(traces=big_ts, rows=(2, 3)) == capi.HK_OK
    assert call1(traces=read2, rows=(1, 3)) == capi.HK_OK and call0(traces=read2, rows=(3, 1)) == capi.HK_OK
    last_bad = _with(job, 1, k - 1, "addr", i=(1 << 32) + 7)        # the previous entry of subcircuit 2
    assert call1(traces=last_bad, rows=(2, 2)) == capi.HK_OK
    assert call1(offsets=uneven, rows=(3, 3)) == capi.HK_OK
    assert call1() == capi.HK_OK and call0() == capi.HK_OK
    want = np.stack([_row(curve, *JOBS[1], i) for i in (1, 2)])
    _diff(z.to_host().reshape(2, -1), want, n_v)
    assert (w.to_host() == fc.enc(job.stage0_ints(1) + job.stage0_ints(2))).all()
    z.free()
    w.free()
