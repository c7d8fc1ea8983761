"""GPU: the VKD job on the device (hk_vkd_trace / hk_vkd_witness, csrc/vkd.cuh) against its host mirror
(hekaton_system_amd/vkd_circuit.py), byte for byte: the value table and the trace of five jobs with host and device
operands, whole assignment rows of every class of jobs A and B from hk_vkd_witness + hk_stage1_witness on a prefilled
buffer (shuffled members, 130 rows), what hk_vkd_witness alone leaves alone, a whole round of job A with nothing of it
computed on the host, a wrong final root and a wrong sibling found by hk_r1cs_check in the row the mirror names, and every
refusal with its outputs untouched."""
import ctypes as C
import random

import numpy as np
import pytest

from hekaton_system_amd import aggregation as agg, capi, tipa
from hekaton_system_amd.chacha import ChaCha12Rng
from hekaton_system_amd.cp_groth16 import (CURVE_PARAMS, FrCodec, Proof, SeededRng, generate_parameters_device,
                                           prepare_verifying_key, r1cs_bad_rows, verify_proofs)
from hekaton_system_amd.merlin import Transcript as Merlin
from hekaton_system_amd.poseidon import device_params
from hekaton_system_amd.sha_circuit import R1csUnsatisfied
from hekaton_system_amd.vkd_circuit import KINDS, SRC_ZERO, Update, VkdJob
from tests.vkd_fixtures import CHAL, DEPTH, SPLIT, assignments, job_a, job_b, job_small

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
PATTERN = 0xA5
JOBS = {"a": job_a, "b": job_b}


def _ctx(cname, ctx_bn254, ctx_bls):
    return ctx_bn254 if cname == "bn254" else ctx_bls


def _prefilled(ctx, nbytes):
    return capi.DeviceBuffer.from_host(ctx, np.full(max(nbytes, 1), PATTERN, np.uint8))


def _params(cname):
    return device_params(cname, FrCodec(cname))


# ---- the trace ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("name", ["a", "b", "log4", "small"])
def test_values_and_trace_equal_the_mirror(cname, name, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    job = {"a": lambda c: job_a(c), "b": lambda c: job_b(c), "log4": lambda c: VkdJob.random(c, 4, DEPTH, SPLIT),
           "small": job_small}[name](cname)
    t, params = job.tables(), _params(cname)
    want_v, want_t = job.values_bytes(), job.flat("time")
    dev = [capi.DeviceBuffer.from_host(ctx, np.ascontiguousarray(x).reshape(-1).view(np.uint8))
           for x in (t["leaves"], t["siblings"], params[0])]
    t_d = dict(t, leaves=dev[0], siblings=dev[1])
    params_d = (dev[2],) + tuple(params[1:])
    try:
        got = [ctx.vkd_trace(t, params), ctx.vkd_trace(t_d, params_d), ctx.vkd_trace(t_d, params)]
        for tt, pp in ((t, params), (t_d, params_d)):
            v, tr = ctx.vkd_trace(tt, pp, device_out=True)
            got.append((v.to_host()[:want_v.size], tr.to_host()[:want_t.size]))
            v.free()
            tr.free()
        for v, tr in got:
            assert v.size == want_v.size and (v == want_v).all()
            assert tr.size == want_t.size and (tr == want_t).all()
    finally:
        for x in dev:
            x.free()


@pytest.mark.parametrize("cname", CURVES)
def test_trace_of_the_depth_128_job(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    job = VkdJob.random(cname, 4, 128, 4)
    assert job.L == 32 and job.n == 16
    _v, tr = ctx.vkd_trace(job.tables(), _params(cname))
    assert (tr == job.flat("time")).all()


@pytest.mark.parametrize("cname", CURVES)
def test_stage0_rows_equal_the_mirror(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    job = job_b(cname)
    dev0 = job.stage0_device(ctx)
    try:
        assert (dev0.traces[1].to_host()[:job.flat("addr").size] == job.flat("addr")).all()
        for key, members in job.classes().items():
            circ = job.make_class(members[0])
            members = members[::-1] + members[:1]
            w = dev0.rows(members)
            want = circ.stage0_witness_bytes([job.inputs(i) for i in members])
            assert (w.to_host().reshape(len(members), -1) == want).all(), key
            w.free()
    finally:
        dev0.free()


# ---- whole rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("name", ["a", "b"])
def test_filled_rows_equal_assignment_bytes(cname, name, ctx_bn254, ctx_bls):
    """hk_vkd_witness + hk_stage1_witness on a buffer prefilled with a non-zero pattern: every byte of every row is the host
    mirror's, for every class: its members shuffled, then repeated to 130 rows (two workgroups of quads and a partial one)."""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    job, want = JOBS[name](cname), assignments(cname, name)
    rnd = random.Random(7)
    dev0 = job.stage0_device(ctx)
    dev = job.stage1_device(ctx, dev0=dev0)
    try:
        assert dev.root == job.root
        for key, members in job.classes().items():
            circ = job.make_class(members[0])
            shuffled = list(members)
            rnd.shuffle(shuffled)
            for sel in (shuffled, [shuffled[b % len(shuffled)] for b in range(130)]):
                z = _prefilled(ctx, len(sel) * circ.n_v * ctx.fr_bytes)
                try:
                    dev.fill(circ, sel, z)
                    got = z.to_host().reshape(len(sel), -1)
                finally:
                    z.free()
                for b, i in enumerate(sel):
                    assert (got[b] == want[i]).all(), (key, i, len(sel), b)
    finally:
        dev.free()
        dev0.free()


@pytest.mark.parametrize("cname", CURVES)
def test_witness_call_alone_keeps_every_other_column(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    fr = ctx.fr_bytes
    job, want = job_b(cname), assignments(cname, "b")
    t, params, values = job.tables(), _params(cname), job.values_bytes()
    for key, members in job.classes().items():
        circ = job.make_class(members[0])
        members = members[::-1]
        z = _prefilled(ctx, len(members) * circ.n_v * fr)
        try:
            ctx.vkd_witness(t, params, values, members, circ.n_v, circ.device_cols, z)
            got = z.to_host().reshape(len(members), circ.n_v, fr)
        finally:
            z.free()
        lo = circ.body_col0
        assert lo + circ.body_cols == circ.n_v
        assert (got[:, 1:lo] == PATTERN).all(), key
        for b, i in enumerate(members):
            w = want[i].reshape(circ.n_v, fr)
            assert (got[b, 0] == w[0]).all() and (got[b, lo:] == w[lo:]).all(), (key, i)


# ---- a whole round -----------------------------------------------------------------------------------------------------
def _oracle_accepts(cname, vk, proof, pub):
    from oracle.pyref import groth16 as og, pairing
    from oracle.pyref.codec import Codec
    from oracle.pyref.params import CURVES as OC
    cd = Codec(OC[cname])
    g1, g2 = cd.g1_bytes, cd.g2_bytes
    ovk = og.VerifyingKey(alpha_g=cd.g1_from(vk.alpha_g), beta_h=cd.g2_from(vk.beta_h), gamma_h=cd.g2_from(vk.gamma_h),
                          last_delta_h=cd.g2_from(vk.last_delta_h),
                          gamma_abc_g=[cd.g1_from(vk.gamma_abc_g[i * g1:(i + 1) * g1]) for i in range(len(vk.gamma_abc_g) // g1)],
                          deltas_h=[cd.g2_from(vk.deltas_h[i * g2:(i + 1) * g2]) for i in range(len(vk.deltas_h) // g2)])
    op = og.Proof(cd.g1_from(proof.a), cd.g2_from(proof.b), cd.g1_from(proof.c), [cd.g1_from(d) for d in proof.ds])
    return pairing.verify_proof(cname, ovk, op, pub)


@pytest.mark.parametrize("cname", CURVES)
def test_whole_round_of_job_a_on_the_device(cname, ctx_bn254, ctx_bls):
    """hk_vkd_trace -> trace_sort -> hk_commit_batch per class; the challenges from the commitments; exec_tree -> fill ->
    r1cs_check -> hk_prove_batch; every proof verified, one per class by the oracle too; the 32 aggregated.  The job is made
    by `on_device`: no hash of it runs on the host."""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    r, fc = CURVE_PARAMS[cname]["r"], FrCodec(cname)
    host = job_a(cname)
    job = VkdJob.on_device(ctx, cname, host.initial_root, host.final_root, host.updates, DEPTH, SPLIT)
    assert job.values is None and job.time is None
    n, groups = job.n, job.classes()
    assert n == 32 and len(groups) == 8
    classes, pvks = {}, {}
    srs = None
    try:
        for key, members in groups.items():
            circ = job.make_class(members[0])
            pk, _td = generate_parameters_device(circ, cname, SeededRng(bytes([len(classes) + 1]) * 32), ctx)
            assert len(pk.vk.gamma_abc_g) == 4 * ctx.g1_bytes
            classes[key] = (circ, pk, pk.upload(ctx))
        rng = ChaCha12Rng(b"\x0c" * 32)
        srs = tipa.setup(ctx, cname, n, rng.fr(r), rng.fr(r))
        kappas = [rng.fr(r) for _ in range(n)]
        coms, proofs = [None] * n, [None] * n
        for key, members in groups.items():
            circ, _pk, dpk = classes[key]
            w = job.dev0.rows(members)
            out = dpk.commit_batch(0, w, fc.enc([kappas[i] for i in members]), circ.n0, len(members))
            w.free()
            for i, com in zip(members, out):
                coms[i] = com.copy()
        super_com = agg.TIPPCommitment(ctx, cname).commit_only_left(srs.ck, np.concatenate(coms))
        job.set_challenges(agg.rom_challenges(super_com, r), ctx=ctx)
        dev = job.dev1
        pub = list(job.chal) + [dev.root]
        for key, members in groups.items():
            circ, _pk, dpk = classes[key]
            z = capi.DeviceBuffer(ctx, len(members) * circ.n_v * ctx.fr_bytes)
            try:
                dev.fill(circ, members, z)
                assert dev.check(dpk, z, members) is None          # hk_pk_r1cs_check: all satisfied
                rs, ss = fc.enc([rng.fr(r) for _ in members]), fc.enc([rng.fr(r) for _ in members])
                a, b, c = dpk.prove_batch(z, rs, ss, fc.enc([kappas[i] for i in members]), circ.n_v, len(members))
            finally:
                z.free()
            for i, pa, pb, pc in zip(members, a, b, c):
                proofs[i] = Proof(pa.copy(), pb.copy(), pc.copy(), [coms[i]])
        for key, members in groups.items():
            pvks[key] = prepare_verifying_key(ctx, classes[key][1].vk)
            assert verify_proofs(pvks[key], [proofs[i] for i in members], [pub] * len(members)) == [1] * len(members)
            assert _oracle_accepts(cname, classes[key][1].vk, proofs[members[0]], pub)
        assert verify_proofs(pvks[job.class_of(9)], [proofs[9]], [pub[:2] + [pub[2] + 1]]) == [0]      # not under another root
        # the host mirror under the same challenges computes the same root: nothing above came from it
        mirror = VkdJob(cname, host.initial_root, host.final_root, host.updates, DEPTH, SPLIT)
        mirror.set_challenges(job.chal)
        assert mirror.root == dev.root
        apk = agg.AggProvingKey(ctx, cname, srs.ck, [classes[job.class_of(i)][1].vk for i in range(n)])
        proof, inst = apk.agg_subcircuit_proofs(Merlin(b"test-vkd-job"), super_com, proofs, pub, srs)
        assert tipa.Tipp(ctx, cname).verify(tipa.verifier_key(ctx, cname, srs), inst["commitment"], inst["output"], inst["twist"],
                                            proof)
    finally:
        job.free()
        for pvk in pvks.values():
            pvk.free()
        for _c, _pk, dpk in classes.values():
            dpk.free()
        if srs is not None:
            for rb in srs.resident.values():
                rb.free()


# ---- tampered jobs through the device path -----------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_tampered_jobs_fail_in_the_row_the_mirror_names(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    r = CURVE_PARAMS[cname]["r"]
    honest = job_a(cname)
    ups = list(honest.updates)
    u = ups[1]
    ups[1] = Update(u.username, u.counter, u.key1, u.key2, u.path[:9] + [u.path[9] ^ 1] + u.path[10:])
    cases = [(VkdJob(cname, honest.initial_root, honest.final_root ^ 2, honest.updates, DEPTH, SPLIT), [31, 30]),
             (VkdJob(cname, honest.initial_root, honest.final_root, ups, DEPTH, SPLIT), [19, 27])]
    for job, (bad_i, other) in cases:
        job.set_challenges(*CHAL)
        dev = job.stage1_device(ctx)
        try:
            assert dev.root == job.root
            for i in (bad_i, other):
                circ = job.make_class(i)
                want = r1cs_bad_rows(*circ.rows(), job.assignment_ints(i), r)
                if i == bad_i:
                    assert len(want) == 1 and circ.block_of(want[0]) == "equal"
                mats = [tuple(capi.DeviceBuffer.from_host(ctx, x) for x in m) for m in circ.csr(circ.fc)]
                z = _prefilled(ctx, circ.n_v * ctx.fr_bytes)
                try:
                    dev.fill(circ, [i], z)
                    verdicts, rows = ctx.r1cs_check(*mats, z, n_v=circ.n_v, batch=1, cap=8)
                    assert verdicts == [(len(want), want[0] if want else None)]
                    checker = type("M", (), {"r1cs_check": lambda self, z, **kw: ctx.r1cs_check(*mats, z, n_v=circ.n_v, **kw)})()
                    if want:
                        with pytest.raises(R1csUnsatisfied) as e:
                            dev.check(checker, z, [i])
                        assert (e.value.subcircuit, e.value.row) == (i, want[0])
                    else:
                        assert dev.check(checker, z, [i]) is None
                finally:
                    z.free()
                    for m in mats:
                        for x in m:
                            x.free()
        finally:
            dev.free()


# ---- refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_every_refusal_leaves_the_outputs_untouched(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    job = job_b(cname)
    fr = ctx.fr_bytes
    base, params, values = job.tables(), _params(cname), job.values_bytes()
    circ = job.make_class(9)                                        # a plain compute path
    members = np.array([9, 13, 8], np.uint32)
    assert all(job.type_of(int(i)) == "compute path" for i in members)
    n_tr, n_val = int(job.offsets[-1]) * 2 * fr, values.size
    z = _prefilled(ctx, len(members) * circ.n_v * fr)
    outs_d = (_prefilled(ctx, n_val), _prefilled(ctx, n_tr))
    outs_h = (np.full(n_val, PATTERN, np.uint8), np.full(n_tr, PATTERN, np.uint8))

    def desc(vals=values, **kw):
        t = dict(base)
        t.update(kw)
        return ctx._vkd_desc(t, params, vals)

    def untouched():
        return (z.to_host() == PATTERN).all() and all((x.to_host() == PATTERN).all() for x in outs_d) and \
            all((x == PATTERN).all() for x in outs_h)

    def trace(d, outs):
        return ctx.lib.hk_vkd_trace(ctx.handle, C.byref(d[0]), capi.ptr(outs[0]), capi.ptr(outs[1]))

    def witness(d, sub=members, n_v=circ.n_v, cols=circ.device_cols, out=z, batch=None):
        sub = np.ascontiguousarray(sub, dtype=np.uint32)
        c = capi.hk_vkd_cols(*[int(x) for x in cols])
        return ctx.lib.hk_vkd_witness(ctx.handle, C.byref(d[0]), sub.ctypes.data, sub.size if batch is None else batch, n_v,
                                      C.byref(c), capi.ptr(out))

    def null(d, field):
        setattr(d[0], field, None)
        return d

    src, kinds = base["slot_src"].copy(), base["kinds"].copy()
    src[40] = len(job.values)
    kinds[1] = 2
    bad_both = [null(desc(), f) for f in ("kinds", "leaves", "siblings_mont", "consts_mont", "roots_mont", "slot_addr", "slot_src")]
    bad_both += [desc(depth=36), desc(depth=16),                                # no multiple of 8 split; L = 4
                 desc(split=0), desc(split=1), desc(depth=0), desc(depth=512), desc(n_updates=0), desc(kinds=kinds),
                 desc(slot_src=src)]
    ARG, LEN = capi.HK_ERR_ARG, capi.HK_ERR_LEN
    try:
        for k, d in enumerate(bad_both):
            for outs in (outs_d, outs_h):
                assert trace(d, outs) == ARG, k
            assert witness(d) == ARG, k
            assert untouched(), k
        ok = desc()
        assert ctx.lib.hk_vkd_trace(ctx.handle, C.byref(ok[0]), None, capi.ptr(outs_d[1])) == ARG
        assert ctx.lib.hk_vkd_trace(ctx.handle, C.byref(ok[0]), capi.ptr(outs_d[0]), None) == ARG
        assert ctx.lib.hk_vkd_trace(ctx.handle, None, capi.ptr(outs_d[0]), capi.ptr(outs_d[1])) == ARG
        assert trace(ok, (outs_d[0], outs_d[0])) == ARG                         # the two outputs overlap
        assert witness(null(desc(), "values_mont")) == ARG
        big = desc()
        big[0].n_slots = 1 << 30                                                # 2^31 lanes of k_vkd_trace: refused before a slot is read
        assert trace(big, outs_d) == LEN and witness(big) == LEN
        assert witness(desc(slot_addr=base["slot_addr"][:-1], slot_src=base["slot_src"][:-1])) == ARG   # not the layout's slots
        k3, h0, i0, p0 = circ.device_cols
        hgc = job.make_class(7)
        calls = [(dict(sub=[9, 32, 8]), ARG),                                   # sub_index[b] >= N
                 (dict(sub=[9, 10, 8]), ARG), (dict(sub=[9, 7, 8]), ARG),       # of another class than cols states
                 (dict(cols=(7, h0, i0, p0)), ARG),                             # no class
                 (dict(cols=hgc.device_cols), LEN),                             # n_v too small for that class ...
                 (dict(cols=hgc.device_cols, n_v=hgc.n_v), ARG),                # ... and with room, not these members' class
                 (dict(n_v=circ.n_v - 1), LEN), (dict(cols=(k3, h0, i0, 0)), LEN), (dict(cols=(k3, h0, i0, p0 + 1)), LEN),
                 (dict(out=np.full(z.nbytes, PATTERN, np.uint8)), ARG),         # z_out on the host
                 (dict(out=None), ARG), (dict(batch=1 << 20), LEN), (dict(n_v=1 << 31), LEN)]
        for kw, status in calls:
            assert witness(ok, **kw) == status, kw
        assert ctx.lib.hk_vkd_witness(ctx.handle, C.byref(ok[0]), None, 3, circ.n_v, C.byref(capi.hk_vkd_cols(*circ.device_cols)),
                                      z.ptr) == ARG
        assert ctx.lib.hk_vkd_witness(ctx.handle, C.byref(ok[0]), members.ctypes.data, 3, circ.n_v, None, z.ptr) == ARG
        assert untouched()
        # nothing to do is no error, and writes nothing
        assert witness(ok, sub=np.zeros(0, np.uint32)) == capi.HK_OK
        pad = job.make_class(2)
        assert witness(ok, sub=[2, 0], n_v=pad.n_v, cols=(KINDS.index("write pp"), 0, 0, 0)) == ARG
        assert untouched()
        # a class without body columns gets its column 0 and nothing else
        zp = _prefilled(ctx, 2 * pad.n_v * fr)
        try:
            assert witness(ok, sub=[2, 1], n_v=pad.n_v, cols=pad.device_cols, out=zp) == capi.HK_OK
            got = zp.to_host().reshape(2, pad.n_v, fr)
        finally:
            zp.free()
        assert (got[:, 0] == FrCodec(cname).enc([1])).all() and (got[:, 1:] == PATTERN).all()
        # ... and the same descriptor, unharmed, still works
        assert trace(ok, outs_h) == capi.HK_OK and (outs_h[0] == values).all() and (outs_h[1] == job.flat("time")).all()
    finally:
        z.free()
        for x in outs_d:
            x.free()
    assert SRC_ZERO == 0xFFFFFFFF
