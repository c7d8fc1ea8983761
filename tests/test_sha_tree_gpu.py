"""GPU: hk_sha_tree / hk_sha_tree_inputs (csrc/sha256.cuh, csrc/sha_tree.cuh) against the host mirror, byte for byte on both
curves.  Every expectation comes from the host: hashlib through ShaMerkleJob's constructor (digests, the time-ordered trace,
sha_root), sha_circuit.program_inputs (the word-program inputs), FrCodec (Montgomery bytes), and for the chain from the leaves
ShaMerkleSubcircuit.assignment_bytes over the host job's Stage1Requests - never from the device.

Shapes (n_sub): 4 has no parent level; 8, 16; 256 is the largest whose leaf level (n / 2 + 1 = 129 lanes) still fits the
one-workgroup tail, so the whole tree is one launch; 512 has 257 leaf-level lanes, the first level launch; 2 048 has two wide
levels.  ns = 1 has no 32-byte iteration, ns = 2 the first one; n_portals = 3 leaves a parent no placeholder.  Leaves are
random with one all-zero leaf (the padding subcircuit's input), one all-0xff leaf and two equal leaves among them."""
import ctypes as C
import random
from functools import lru_cache

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.sha_circuit import ShaMerkleJob, program_inputs

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]


def _ctx(curve, ctx_bn254, ctx_bls):
    return ctx_bn254 if curve == "bn254" else ctx_bls


@lru_cache(maxsize=None)
def _leaves(n, seed=0):
    rnd = random.Random(1000 * seed + n)
    nl = n // 2
    lv = [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(nl)]
    if nl == 2:
        return (bytes(64), b"\xff" * 64) if seed % 2 == 0 else (lv[0], lv[0])
    lv[1], lv[2], lv[-1] = bytes(64), b"\xff" * 64, lv[0]
    return tuple(lv)


@lru_cache(maxsize=None)
def _host(curve, n, ns, k, seed=0):
    """(job, digests, time-ordered trace, sha_root) of the host job, the last three as the bytes hk_sha_tree must write"""
    job = ShaMerkleJob(curve, n, ns, k, list(_leaves(n, seed)))
    fc = FrCodec(curve)
    digests = np.frombuffer(b"".join(job.digest), np.uint8)
    time_b = fc.enc([x for ops in job.time for e in ops for x in e])
    time_b.setflags(write=False)
    return job, digests, time_b, fc.enc([job.sha_root])


def _flat(leaves):
    return np.frombuffer(b"".join(leaves), np.uint8)


def _assert_tree(got, want, what):
    for name, g, w in zip(("digests", "time", "sha_root"), got, want):
        g = g.to_host() if isinstance(g, capi.DeviceBuffer) else g
        assert g.size == w.size, (what, name)
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            raise AssertionError("%s: %s differs from byte %d on" % (what, name, at))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [4, 8, 16])
def test_small_trees_equal_the_host_job(curve, n, ctx_bn254, ctx_bls):
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    for ns in (1, 2, 3):
        for k in (3, 4, 7):
            seed = ns + k                                          # n = 4: both leaf pairs come up
            _job, *want = _host(curve, n, ns, k, seed)
            _assert_tree(ctx.sha_tree(list(_leaves(n, seed)), n, ns, k), want, (curve, n, ns, k))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,ns,k", [(256, 1, 4), (256, 3, 7), (512, 2, 3), (2048, 3, 4)])
def test_wide_trees_equal_the_host_job(curve, n, ns, k, ctx_bn254, ctx_bls):
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    _job, *want = _host(curve, n, ns, k)
    _assert_tree(ctx.sha_tree(_flat(_leaves(n)), n, ns, k), want, (curve, n, ns, k))


def _raw_tree(ctx, leaves, n, ns, k, outs, handle="ctx"):
    o = capi.hk_sha_tree_out(*[capi.ptr(x) for x in outs])
    return ctx.lib.hk_sha_tree(ctx.handle if handle == "ctx" else handle, capi.ptr(leaves), n, ns, k, C.byref(o))


@pytest.mark.parametrize("curve", CURVES)
def test_residency_single_outputs_and_repeats(curve, ctx_bn254, ctx_bls):
    """Host- and device-resident leaves and outputs give the same bytes; so does each output alone and a second call."""
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    n, ns, k = 16, 2, 4
    _job, *want = _host(curve, n, ns, k)
    host_lv = _flat(_leaves(n))
    dev_lv = capi.DeviceBuffer.from_host(ctx, host_lv)
    bufs = []
    try:
        for lv in (host_lv, dev_lv):
            for device_out in (False, True):
                for rep in range(2):
                    got = ctx.sha_tree(lv, n, ns, k, device_out=device_out)
                    bufs += [x for x in got if isinstance(x, capi.DeviceBuffer)]
                    _assert_tree(got, want, (curve, type(lv).__name__, device_out, rep))
        # device-resident leaves that are not 16-byte aligned (a view into a larger buffer)
        shifted = capi.DeviceBuffer.from_host(ctx, np.concatenate([np.zeros(4, np.uint8), host_lv]))
        bufs.append(shifted)
        _assert_tree(ctx.sha_tree(shifted.view(4, host_lv.size), n, ns, k), want, (curve, "unaligned view"))
        # each output alone, into host and into device memory
        for which in range(3):
            for device_out in (False, True):
                out = capi.DeviceBuffer(ctx, want[which].size) if device_out else np.full(want[which].size, 0xA5, np.uint8)
                if device_out:
                    bufs.append(out)
                outs = [None] * 3
                outs[which] = out
                assert _raw_tree(ctx, dev_lv, n, ns, k, outs) == capi.HK_OK
                got = out.to_host() if device_out else out
                assert np.array_equal(got, want[which]), (curve, which, device_out)
    finally:
        dev_lv.free()
        for b in bufs:
            b.free()


def _program_inputs_of(job, circ, members):
    """program_inputs over what it reads of a Stage1Request: the leaf, or the first two time-ordered entries"""
    ws = [dict(leaf=(bytes(64) if job.kind[i] == "padding" else job.leaves[i]) if job.kind[i] in ("leaf", "padding") else None,
               time=job.time[i]) for i in members]
    return program_inputs(circ, ws)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [8, 64])
def test_inputs_equal_program_inputs(curve, n, ctx_bn254, ctx_bls):
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    ns, k = 2, 4
    job, digests, _time, _root = _host(curve, n, ns, k)
    host_lv = _flat(_leaves(n))
    dev_lv, dev_dg = capi.DeviceBuffer.from_host(ctx, host_lv), capi.DeviceBuffer.from_host(ctx, digests)
    classes = {}
    for i in range(n):
        classes.setdefault(job.class_of(i), []).append(i)
    assert len(classes) == 5
    rnd = random.Random(n)
    try:
        for key, members in classes.items():
            circ = job.make_class(members[0])
            n_inputs = circ.tape.n_inputs
            assert n_inputs == (16 if key[0] in ("leaf", "padding") else 54)
            order = members + members[:2]                          # any order, repeats
            rnd.shuffle(order)
            want = _program_inputs_of(job, circ, order)
            assert want.shape == (len(order), n_inputs)
            got = ctx.sha_tree_inputs(host_lv, digests, n, n_inputs, order)
            assert got.dtype == np.uint32 and np.array_equal(got, want), (curve, n, key, "host")
            # only the input the kind reads, device-resident, into device memory
            lv, dg = (dev_lv, None) if n_inputs == 16 else (None, dev_dg)
            buf = ctx.sha_tree_inputs(lv, dg, n, n_inputs, order, device_out=True)
            try:
                assert np.array_equal(buf.to_host().view(np.uint32).reshape(len(order), n_inputs), want), (curve, n, key, "device")
            finally:
                buf.free()
        # leaves and the padding subcircuit in one call: both read `leaves` with n_inputs = 16
        mixed = [n - 1, 0, n // 2 - 1, n - 1, 1]
        want = _program_inputs_of(job, job.make_class(1), mixed)
        assert not want[0].any() and np.array_equal(ctx.sha_tree_inputs(dev_lv, None, n, 16, mixed), want)
    finally:
        dev_lv.free()
        dev_dg.free()


def test_refusals_leave_the_outputs_untouched(ctx_bn254):
    """Every HK_ERR_ARG of the header, each before any launch: pattern-filled outputs keep their bytes."""
    ctx = ctx_bn254
    n, ns, k = 8, 1, 4
    lv = _flat(_leaves(n)).copy()
    PAT = 0xA5
    outs = [np.full(32 * n, PAT, np.uint8), np.full(64 * n * k, PAT, np.uint8), np.full(32, PAT, np.uint8)]
    big = np.full(64 * (1 << 10), PAT, np.uint8)                   # stands in for an output of a size never reached
    big_lv = np.zeros(64, np.uint8)                                # and for leaves never read, far from it

    def refused(leaves=lv, n=n, ns=ns, k=k, o=outs, handle="ctx", null_out=False):
        if null_out:
            st = ctx.lib.hk_sha_tree(ctx.handle, capi.ptr(leaves), n, ns, k, None)
        else:
            st = _raw_tree(ctx, leaves, n, ns, k, o, handle)
        assert st == capi.HK_ERR_ARG, st
        assert all((x == PAT).all() for x in outs) and (big == PAT).all()

    refused(handle=None)
    refused(leaves=None)
    refused(null_out=True)
    refused(o=[None, None, None])
    for bad_n in (0, 1, 2, 3, 6, 12, 24, (1 << 20) + 1, 1 << 21, 0xffffffff):
        refused(n=bad_n, leaves=big_lv, o=[big, None, None])
    for bad_ns in (0, 1 << 16, 0xffffffff):
        refused(ns=bad_ns)
    for bad_k in (0, 1, 2):
        refused(k=bad_k)
    refused(n=1 << 20, k=256, leaves=big_lv, o=[big, None, None])     # n_sub x n_portals = 2^28
    refused(n=1 << 14, k=1 << 14, leaves=big_lv, o=[big, None, None])
    # an output range that overlaps the leaves: each of the three outputs, the output starting inside or in front of them
    whole = np.full(4096, PAT, np.uint8)
    inner = whole[1024:1024 + lv.size]
    inner[:] = lv
    for which in range(3):
        for at in (1024 + 32, 1024 + lv.size - 1, 1024 - 1):
            o = [None] * 3
            o[which] = whole.ctypes.data + at
            st = _raw_tree(ctx, inner, n, ns, k, o)
            assert st == capi.HK_ERR_ARG
            assert (whole[:1024] == PAT).all() and (whole[1024 + lv.size:] == PAT).all() and np.array_equal(inner, lv)

    # hk_sha_tree_inputs
    dg = np.zeros(32 * n, np.uint8)
    out = np.full(8 * 54, PAT & 0xff, np.uint8).view(np.uint32)
    u32 = lambda xs: np.array(xs, np.uint32)

    def refused_inputs(leaves=lv, digests=dg, n=n, n_inputs=16, sub=(0,), o=out, handle="ctx", null_sub=False):
        sub = u32(sub)
        st = ctx.lib.hk_sha_tree_inputs(ctx.handle if handle == "ctx" else handle, capi.ptr(leaves), capi.ptr(digests), n, n_inputs,
                                        None if null_sub else sub.ctypes.data, sub.size, capi.ptr(o))
        assert st == capi.HK_ERR_ARG, st
        assert (out.view(np.uint8) == PAT).all()

    refused_inputs(handle=None)
    refused_inputs(null_sub=True)
    refused_inputs(o=None)
    for bad_n in (0, 2, 6, 1 << 21):
        refused_inputs(n=bad_n)
    for bad_inputs in (0, 15, 17, 27, 53, 55, 64):
        refused_inputs(n_inputs=bad_inputs, sub=(0,))
        refused_inputs(n_inputs=bad_inputs, sub=(4,))
    for i in (4, 5, 6, 8, 9, 0xffffffff):                          # 16: a leaf or the padding subcircuit only
        refused_inputs(n_inputs=16, sub=(0, i))
    for i in (0, 3, 7, 8, 0xffffffff):                             # 54: a parent or the root only
        refused_inputs(n_inputs=54, sub=(4, i))
    refused_inputs(n_inputs=16, leaves=None)                       # the input the kind needs
    refused_inputs(n_inputs=54, digests=None, sub=(4,))
    both = np.zeros(4096, np.uint8)
    for n_inputs, sub, src in ((16, (0,), "leaves"), (54, (4,), "digests")):
        kw = {src: both[1024:1024 + (lv.size if src == "leaves" else dg.size)]}
        for at in (1024 + 8, 1024 - 4):
            st = ctx.lib.hk_sha_tree_inputs(ctx.handle, capi.ptr(kw.get("leaves", lv)), capi.ptr(kw.get("digests", dg)), n, n_inputs,
                                            u32(sub).ctypes.data, 1, both.ctypes.data + at)
            assert st == capi.HK_ERR_ARG and not both.any()
    # batch == 0: HK_OK, nothing done
    assert ctx.lib.hk_sha_tree_inputs(ctx.handle, capi.ptr(lv), capi.ptr(dg), n, 16, None, 0, capi.ptr(out)) == capi.HK_OK
    assert (out.view(np.uint8) == PAT).all()


class _ClassMatrices:
    """A class's matrices resident on the device, with DevicePk's r1cs_check: what Stage1Device.check needs of a key."""

    def __init__(self, ctx, circ):
        self.ctx = ctx
        self.bufs = [tuple(capi.DeviceBuffer.from_host(ctx, x) for x in m) for m in circ.csr(circ.fc)]

    def r1cs_check(self, z, n_v=None, batch=1, cap=0, want_vals=False):
        return self.ctx.r1cs_check(*self.bufs, z, n_v=n_v, batch=batch, cap=cap, want_vals=want_vals)

    def free(self):
        for m in self.bufs:
            for x in m:
                x.free()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [8, 64])
def test_chain_from_the_leaves_equals_the_host_path(curve, n, ctx_bn254, ctx_bls):
    """ShaMerkleJob.on_device -> stage 0 rows, word-program inputs, stage 1 fill: every assignment equals the one the host
    builds from the same leaves and challenges (ShaMerkleSubcircuit.assignment_bytes over the host job's requests), and
    satisfies its class's R1CS where it lies.  Then one leaf byte is flipped on the device side only."""
    ctx = _ctx(curve, ctx_bn254, ctx_bls)
    ns, k = 1, 4
    rnd = random.Random(41 + n)
    r, fr = CURVE_PARAMS[curve]["r"], ctx.fr_bytes
    fc = FrCodec(curve)
    leaves = list(_leaves(n))
    ech, tr = rnd.randrange(r), rnd.randrange(r)
    host = ShaMerkleJob(curve, n, ns, k, leaves, ech, tr)          # the host path: hashlib, Python lists, the host exec tree
    classes = {}
    for i in range(n):
        classes.setdefault(host.class_of(i), []).append(i)

    def run(job, check):
        """{class: assignments (bytes)} of a job made by on_device; with check also the stage-0 rows and the R1CS verdicts"""
        assert not any(hasattr(job, a) for a in ("time", "addr", "digest"))
        job.set_challenges(ech, tr, ctx)
        dev0 = job.stage0_device(ctx)
        dev1 = None
        out = {}
        try:
            assert dev0.traces[0] is job.tree.time
            if check:
                members = list(range(n)) + [n - 2, 0]
                rows = dev0.rows(members)
                want = fc.enc([x for i in members for x in host.stage0_ints(i)])
                got = rows.to_host()
                rows.free()
                assert np.array_equal(got, want), (curve, n, "stage-0 rows")
            dev1 = job.stage1_device(ctx, traces=dev0.traces)
            assert not check or dev1.root == host.root
            for key, members in classes.items():
                circ = job.make_class(members[0])
                ops, refs, vmap = circ.tape.word_program(circ.n_v)
                wp = ctx.wprog_upload(ops, refs, vmap, circ.tape.n_values, circ.tape.n_inputs)
                inputs = job.tree.inputs(circ, members)
                z = wp.run(inputs, [], [], batch=len(members))
                mats = _ClassMatrices(ctx, circ) if check else None
                try:
                    dev1.fill(circ, members, z, sha_root=job.tree.sha_root)
                    out[key] = z.to_host().reshape(len(members), circ.n_v, fr)
                    if check:
                        verdicts = mats.r1cs_check(z, batch=len(members))
                        assert verdicts == [(0, None)] * len(members), (curve, n, key, verdicts)
                        assert dev1.check(mats, z, members) is None
                finally:
                    inputs.free()
                    z.free()
                    wp.free()
                    if mats:
                        mats.free()
        finally:
            if dev1 is not None:
                dev1.free()
            dev0.free()
            job.free()
        return out

    got = run(ShaMerkleJob.on_device(ctx, curve, n, ns, k, leaves), check=True)
    for key, members in classes.items():
        circ = host.make_class(members[0])
        want = circ.assignment_bytes([host.inputs(i) for i in members]).reshape(len(members), circ.n_v, fr)
        if not np.array_equal(got[key], want):
            b, col = [int(x[0]) for x in np.nonzero((got[key] != want).any(axis=2))]
            raise AssertionError("%s n=%d class %s: subcircuit %d differs from column %d on" % (curve, n, key, members[b], col))
    # one leaf byte flipped on the device side only: the assignments differ (leaf 3 is neither first nor special)
    flipped = list(leaves)
    flipped[3] = bytes([flipped[3][0] ^ 1]) + flipped[3][1:]
    other = run(ShaMerkleJob.on_device(ctx, curve, n, ns, k, flipped), check=False)
    leaf_key = ("leaf", False, False)
    b = classes[leaf_key].index(3)
    assert not np.array_equal(other[leaf_key][b], got[leaf_key][b])
    assert not np.array_equal(other[("root", False, False)], got[("root", False, False)])       # the root hash moved with it
