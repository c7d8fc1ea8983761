"""GPU: where a job entry's operands live does not change what it computes.  Each entry below stages host-resident inputs in
lane scratch and reads device-resident ones in place (csrc/hk_internal.h `Staged`); here every one of them runs with all
inputs on the host, all on the device and alternating, and the three outputs are byte-identical (and not the prefill).
hk_vkd_trace and hk_r1cs_job_trace do the same for their host-or-device outputs.  The smallest case of each entry's own test
file: the VKD job `small`, hk_exec_tree at n_sub = 2, hk_poseidon_path at batch 1 and 65 (one wave plus a lane), a three-entry
word program at batch 1 with n_full 0 and 1.  What the bytes ARE is the business of those files."""
import ctypes as C
import random

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.poseidon import device_params
from tests.r1cs_job_fixtures import JOBS, make_job
from tests.residency import PATTERN, _filled, _prefilled, _same_everywhere
from tests.vkd_fixtures import job_small

pytestmark = pytest.mark.gpu
CNAME = "bn254"


# ---- the VKD job ------------------------------------------------------------------------------------------------------------
def test_vkd_trace_inputs_and_outputs(ctx_bn254):
    ctx, job = ctx_bn254, job_small(CNAME)
    t, params = job.tables(), device_params(CNAME, FrCodec(CNAME))
    sizes = [job.values_bytes().size, job.flat("time").size]

    def outputs(kinds):                        # kinds[k]: output k is a device buffer
        def run(put):
            tt = dict(t, leaves=put(t["leaves"]), siblings=put(t["siblings"]))
            out = [_prefilled(ctx, n) if dev else np.full(n, PATTERN, np.uint8) for n, dev in zip(sizes, kinds)]
            try:
                ctx.vkd_trace(tt, (put(params[0]),) + tuple(params[1:]), out=tuple(out))
                return np.concatenate([x.to_host()[:n] if dev else x for x, n, dev in zip(out, sizes, kinds)])
            finally:
                for x, dev in zip(out, kinds):
                    if dev:
                        x.free()
        return _same_everywhere(ctx, run)

    got = [outputs(kinds) for kinds in ((False, False), (True, True), (True, False), (False, True))]
    assert all((g == got[0]).all() for g in got)


def test_vkd_witness_inputs(ctx_bn254):
    ctx, job = ctx_bn254, job_small(CNAME)
    t, params, values = job.tables(), device_params(CNAME, FrCodec(CNAME)), job.values_bytes()
    kinds = set()
    for key, members in job.classes().items():
        circ = job.make_class(members[0])
        if circ.device_cols[0] in kinds:                   # a padding class differs from the other in its first-ness alone
            continue
        kinds.add(circ.device_cols[0])
        sel = (members[::-1] + members[:1])[:3]

        def run(put):
            tt = dict(t, leaves=put(t["leaves"]), siblings=put(t["siblings"]))
            pp, vv = (put(params[0]),) + tuple(params[1:]), put(values)
            return _filled(ctx, len(sel) * circ.n_v * ctx.fr_bytes,
                           lambda z: ctx.vkd_witness(tt, pp, vv, sel, circ.n_v, circ.device_cols, z))
        _same_everywhere(ctx, run)
    assert len(kinds) == 7


# ---- the partitioned R1CS job -------------------------------------------------------------------------------------------------
def test_r1cs_job_trace_input_and_output(ctx_bn254):
    ctx = ctx_bn254
    job = make_job(CNAME, sorted(JOBS)[0], chal=None)
    t, wit, n = job.tables(), job.witness_bytes(), job.flat("time").size

    def output(dev):
        def run(put):
            out = _prefilled(ctx, n) if dev else np.full(n, PATTERN, np.uint8)
            try:
                ctx.r1cs_job_trace(t, put(wit), out=out)
                return out.to_host()[:n] if dev else out
            finally:
                if dev:
                    out.free()
        return _same_everywhere(ctx, run)

    assert (output(False) == output(True)).all()


# ---- hk_exec_tree at n_sub = 2 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry_fields", [2, 4])
def test_exec_tree_inputs(entry_fields, ctx_bn254):
    ctx, fc, r = ctx_bn254, FrCodec(CNAME), CURVE_PARAMS[CNAME]["r"]
    rnd = random.Random(21)
    k, offsets = entry_fields, [0, 3, 5]
    time_e, addr_e = (fc.enc([rnd.randrange(r) for _ in range(5 * k)]) for _ in range(2))
    chal = [rnd.randrange(r) for _ in range(k)]
    params = device_params(CNAME, fc)

    def run(put):
        te, ae = put(time_e), put(addr_e)
        outs = ctx.exec_tree((put(params[0]),) + tuple(params[1:]), k, offsets, te, ae, chal)
        return np.concatenate(outs)
    _same_everywhere(ctx, run)


# ---- hk_poseidon_path, hk_wprog_run, hk_assignment_scatter: the C entries, whose wrappers take host arrays only ------------------
def _p(x):
    return capi.ptr(x)


@pytest.mark.parametrize("batch", [1, 65])
def test_poseidon_path_inputs(batch, ctx_bn254):
    ctx, fc, r = ctx_bn254, FrCodec(CNAME), CURVE_PARAMS[CNAME]["r"]
    rnd = random.Random(22)
    consts, n_consts, ld, nd = device_params(CNAME, fc)
    depth, col0 = 3, 5

    def trace_len(t, alpha, rf, rp, _off):
        chain = 3 if alpha == 5 else 5
        return rf * (t * chain + t) + rp * (chain + t)
    n_v = col0 + 2 * trace_len(*ld) + depth * (3 + trace_len(*nd)) + 7
    leaf = fc.enc([rnd.randrange(r) for _ in range(batch * 4)])
    sibs = fc.enc([rnd.randrange(r) for _ in range(batch * depth)])
    index = np.array([rnd.randrange(1 << depth) for _ in range(batch)], np.uint32)
    a, b = capi.hk_poseidon_desc(*ld), capi.hk_poseidon_desc(*nd)

    def run(put):
        c, lf, sb, ix = put(consts), put(leaf), put(sibs), put(index)

        def fill(z):
            capi.check(ctx.lib.hk_poseidon_path(ctx.handle, _p(c), int(n_consts), C.byref(a), C.byref(b), _p(lf), _p(sb), _p(ix),
                                                depth, batch, n_v, col0, z.ptr), "hk_poseidon_path")
        return _filled(ctx, batch * n_v * ctx.fr_bytes, fill)
    got = _same_everywhere(ctx, run).reshape(batch, n_v, ctx.fr_bytes)
    assert (got[:, :col0] == PATTERN).all() and (got[:, -7:] == PATTERN).all()


@pytest.mark.parametrize("n_full", [0, 1])
def test_wprog_run_and_scatter_inputs(n_full, ctx_bn254):
    """value 0 = input 0, value 1 = input 1, value 2 = their XOR; columns 1 .. 32 are the bits of value 2, 33 .. 64 those of
    value 0, column 0 the constant, 65 .. 69 full-width columns the program leaves alone."""
    ctx, fc = ctx_bn254, FrCodec(CNAME)
    fr, n_v = ctx.fr_bytes, 70
    ops = np.zeros((3, 8), np.uint32)
    ops[1, 4] = 1                                                  # WOP_INPUT (0) with imm = the input's index
    ops[2, :3] = (2, 0, 1)                                         # WOP_XOR of values 0 and 1
    vmap = np.full(n_v, 0xffffffff, np.uint32)
    vmap[1:33] = (2 << 5) | np.arange(32)
    vmap[33:65] = (0 << 5) | np.arange(32)
    wp = ctx.wprog_upload(ops, np.zeros(0, np.uint32), vmap, 3, 2)
    inputs = np.array([[0x80C0FFEE, 0x12345678]], np.uint32)
    cols, vals = np.array([66], np.uint32)[:n_full], fc.enc([0x1D0B])[:n_full * fr]
    try:
        def run(put):
            i, c, v = (put(inputs), put(cols), put(vals)) if n_full else (put(inputs), None, None)
            return _filled(ctx, n_v * fr, lambda z: capi.check(ctx.lib.hk_wprog_run(
                ctx.handle, wp.handle, _p(i), 1, _p(c), _p(v), n_full, z.ptr), "hk_wprog_run"))
        got = _same_everywhere(ctx, run).reshape(n_v, fr)
        one, zero = fc.enc([1]), fc.enc([0])
        x = int(inputs[0, 0] ^ inputs[0, 1])
        assert (got[0] == one).all()
        for bit in range(32):
            assert (got[1 + bit] == (one if (x >> bit) & 1 else zero)).all(), bit
            assert (got[33 + bit] == (one if (int(inputs[0, 0]) >> bit) & 1 else zero)).all(), bit
        assert (got[65] == PATTERN).all() and (got[67:] == PATTERN).all()
        assert (got[66] == (vals if n_full else PATTERN)).all()
        if n_full:                                                 # the same value through hk_assignment_scatter alone
            def scatter(put):
                c, v = put(cols), put(vals)
                return _filled(ctx, n_v * fr, lambda z: capi.check(ctx.lib.hk_assignment_scatter(
                    ctx.handle, _p(c), _p(v), 1, 1, n_v, z.ptr), "hk_assignment_scatter"))
            got = _same_everywhere(ctx, scatter).reshape(n_v, fr)
            assert (got[66] == vals).all() and (got[:66] == PATTERN).all() and (got[67:] == PATTERN).all()
    finally:
        wp.free()
