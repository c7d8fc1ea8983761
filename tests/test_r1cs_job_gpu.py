"""GPU: the partitioned R1CS job on the device (hk_r1cs_job_trace / hk_r1cs_job_witness, csrc/r1cs_job.cuh) against its host
mirror (hekaton_system_amd/r1cs_circuit.py), byte for byte, on the three fixture jobs of tests/r1cs_job_fixtures.py: the
trace, the stage-0 rows, whole assignment rows from r1cs_job_witness + hk_stage1_witness on a prefilled buffer, what
r1cs_job_witness alone leaves alone, host / device inputs, a whole round of the (4, 4) job with nothing of it computed on the
host, an owner's tampering found by hk_r1cs_check in the row the mirror names, and every refusal with its output untouched."""
import ctypes as C
import random

import numpy as np
import pytest

from hekaton_system_amd import aggregation as agg, capi, tipa
from hekaton_system_amd.chacha import ChaCha12Rng
from hekaton_system_amd.cp_groth16 import (CURVE_PARAMS, FrCodec, Proof, SeededRng, generate_parameters_device,
                                           prepare_verifying_key, r1cs_bad_rows, verify_proofs)
from hekaton_system_amd.merlin import Transcript as Merlin
from hekaton_system_amd.r1cs_circuit import PartitionedR1csJob, SRC_ZERO
from hekaton_system_amd.sha_circuit import R1csUnsatisfied
from tests.r1cs_job_fixtures import JOBS, job_parts, make_job, owner_tampering

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
PATTERN = 0xA5
_JOBS = {}


def _ctx(cname, ctx_bn254, ctx_bls):
    return ctx_bn254 if cname == "bn254" else ctx_bls


def _job(cname, name):
    """The job with its challenges set and the host assignment of every subcircuit, computed once and never changed."""
    if (cname, name) not in _JOBS:
        job = make_job(cname, name)
        _JOBS[cname, name] = (job, [job.assignment_bytes(i) for i in range(job.n)])
    return _JOBS[cname, name]


def _groups(job):
    groups = {}
    for idx in range(job.n):
        groups.setdefault(job.class_of(idx), []).append(idx)
    return groups


def _prefilled(ctx, nbytes):
    return capi.DeviceBuffer.from_host(ctx, np.full(max(nbytes, 1), PATTERN, np.uint8))


# ---- the trace ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("name", sorted(JOBS))
def test_trace_equals_the_host_trace(cname, name, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    jobs = [make_job(cname, name, chal=None)]
    if JOBS[name][2]:                                  # also with one block shared by every transaction (tx_stride 0)
        jobs.append(PartitionedR1csJob(cname, job_parts(name)[0], JOBS[name][1]))
    assert {j.tx_stride for j in jobs} == ({0, jobs[0].tx_len} if JOBS[name][2] else {0})
    for job in jobs:
        t, wit, want = job.tables(), job.witness_bytes(), job.flat("time")
        wit_d = capi.DeviceBuffer.from_host(ctx, wit)
        try:
            got = [ctx.r1cs_job_trace(t, wit), ctx.r1cs_job_trace(t, wit_d), ctx.r1cs_job_trace(t, wit)]
            for w in (wit, wit_d):
                out_d = ctx.r1cs_job_trace(t, w, device_out=True)
                got.append(out_d.to_host()[:want.size])
                out_d.free()
            for g in got:
                assert g.size == want.size and (g == want).all()
        finally:
            wit_d.free()


@pytest.mark.parametrize("cname", CURVES)
def test_stage0_rows_equal_the_mirror(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    for name in sorted(JOBS):
        job, _ = _job(cname, name)
        dev0 = job.stage0_device(ctx)
        try:
            assert (dev0.traces[0].to_host()[:job.flat("time").size] == job.flat("time")).all()
            assert (dev0.traces[1].to_host()[:job.flat("addr").size] == job.flat("addr")).all()
            for key, members in _groups(job).items():
                circ = job.make_class(members[0])
                members = members[::-1] + members[:1]
                w = dev0.rows(members)
                want = circ.stage0_witness_bytes([job.inputs(i) for i in members])
                assert (w.to_host().reshape(len(members), -1) == want).all(), (name, key)
                w.free()
        finally:
            dev0.free()


# ---- whole rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("name", sorted(JOBS))
def test_filled_rows_equal_assignment_bytes(cname, name, ctx_bn254, ctx_bls):
    """r1cs_job_witness + hk_stage1_witness on a buffer prefilled with a non-zero pattern: every byte of every row is the host
    mirror's, for the first, a middle and the last subcircuit's class, batches of 1, 3 and 65, repeats, any order."""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    job, want = _job(cname, name)
    rnd = random.Random(11)
    groups = _groups(job)
    middle = max((m for k, m in groups.items() if not k[1] and not k[2]), key=len, default=None)
    picked = [groups[job.class_of(0)], groups[job.class_of(job.n - 1)]] + ([middle] if middle else [])
    dev0 = job.stage0_device(ctx)
    dev = job.stage1_device(ctx, dev0=dev0)
    try:
        assert dev.root == job.root
        on_dev = make_job(cname, name, chal=None)                  # the host job with hk_exec_tree behind set_challenges
        on_dev.set_challenges(job.chal, ctx=ctx)
        assert (on_dev.root, on_dev.time_eval0, on_dev.addr_eval0) == (job.root, job.time_eval0, job.addr_eval0)
        assert (on_dev.assignment_bytes(job.n - 1) == want[job.n - 1]).all()
        for members in picked:
            circ = job.make_class(members[0])
            for batch in (1, 3, 65):
                sel = [rnd.choice(members) for _ in range(batch)]
                if batch >= len(members):
                    sel[:len(members)] = members[::-1]             # every member, out of order, then repeats
                z = _prefilled(ctx, batch * circ.n_v * ctx.fr_bytes)
                try:
                    dev.fill(circ, sel, z)
                    got = z.to_host().reshape(batch, -1)
                finally:
                    z.free()
                for b, i in enumerate(sel):
                    assert (got[b] == want[i]).all(), (name, i, batch, b)
    finally:
        dev.free()
        dev0.free()


@pytest.mark.parametrize("cname", CURVES)
def test_witness_call_alone_keeps_every_other_column(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    fr = ctx.fr_bytes
    for name in sorted(JOBS):
        job, want = _job(cname, name)
        t, wit = job.tables(), job.witness_bytes()
        for p in range(job.P):
            members = [i for i in range(job.n) if i % job.P == p][::-1]
            circ = job.make_class(members[0])
            # first / last classes of a partition differ in rows, not in columns: one layout per partition
            assert all(job.make_class(i).n_v == circ.n_v and job.make_class(i).body_col0 == circ.body_col0 for i in members)
            z = _prefilled(ctx, len(members) * circ.n_v * fr)
            try:
                ctx.r1cs_job_witness(t, wit, members, circ.n_v, circ.body_col0, z)
                got = z.to_host().reshape(len(members), circ.n_v, fr)
            finally:
                z.free()
            lo, hi = circ.body_col0, circ.body_col0 + circ.part.body_len
            assert hi == circ.n_v
            assert (got[:, 1:lo] == PATTERN).all() and (got[:, hi:] == PATTERN).all()
            for b, i in enumerate(members):
                w = want[i].reshape(circ.n_v, fr)
                assert (got[b, 0] == w[0]).all() and (got[b, lo:hi] == w[lo:hi]).all(), (name, i)


@pytest.mark.parametrize("cname", CURVES)
def test_host_device_and_mixed_inputs_agree(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    job, want = _job(cname, "p4t4")
    fc = FrCodec(cname)
    t, wit = job.tables(), job.witness_bytes()
    wit_d = capi.DeviceBuffer.from_host(ctx, wit)
    from hekaton_system_amd.poseidon import device_params
    params = device_params(cname, fc)
    time_h, addr_h = job.flat("time"), job.flat("addr")
    outs_h = ctx.exec_tree(params, 2, job.offsets, time_h, addr_h, fc.enc(list(job.chal)))
    time_d, addr_d = capi.DeviceBuffer.from_host(ctx, time_h), capi.DeviceBuffer.from_host(ctx, addr_h)
    members = [13, 5, 5, 1, 9]
    circ = job.make_class(5)
    rows = []
    try:
        for w, tr in ((wit, (time_h, addr_h)), (wit_d, (time_d, addr_d)), (wit_d, (time_h, addr_d)), (wit, (time_h, addr_h))):
            z = _prefilled(ctx, len(members) * circ.n_v * ctx.fr_bytes)
            try:
                ctx.r1cs_job_witness(t, w, members, circ.n_v, circ.body_col0, z)
                ctx.stage1_witness(params, circ.np_, job.offsets, tr[0], tr[1], fc.enc(list(job.chal)), outs_h, members,
                                   circ.n_v, (1, circ.N_INST, circ.pos_col0), z)
                rows.append(z.to_host().reshape(len(members), -1))
            finally:
                z.free()
    finally:
        for x in (wit_d, time_d, addr_d):
            x.free()
    for got in rows:
        for b, i in enumerate(members):
            assert (got[b] == want[i]).all()


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
def test_whole_round_of_the_4x4_job_on_the_device(cname, ctx_bn254, ctx_bls):
    """Upload the witnesses; trace -> trace_sort -> hk_commit_batch per class; the challenges from the commitments; exec_tree
    -> fill -> r1cs_check -> hk_prove_batch; every proof verified, one per class by the oracle too; the 16 aggregated."""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    r, fc = CURVE_PARAMS[cname]["r"], FrCodec(cname)
    job = make_job(cname, "p4t4", chal=None)
    n, groups = job.n, _groups(job)
    assert n == 16 and len(groups) == 6
    classes = {}
    for key, members in groups.items():
        circ = job.make_class(members[0])
        pk, _td = generate_parameters_device(circ, cname, SeededRng(bytes([len(classes) + 1]) * 32), ctx)
        assert len(pk.vk.gamma_abc_g) == 4 * ctx.g1_bytes
        classes[key] = (circ, pk, pk.upload(ctx))
    rng = ChaCha12Rng(b"\x0b" * 32)
    srs = tipa.setup(ctx, cname, n, rng.fr(r), rng.fr(r))
    kappas = [rng.fr(r) for _ in range(n)]
    coms, proofs = [None] * n, [None] * n
    dev0 = job.stage0_device(ctx)
    dev = None
    pvks = {}
    try:
        for key, members in groups.items():
            circ, _pk, dpk = classes[key]
            w = dev0.rows(members)
            out = dpk.commit_batch(0, w, fc.enc([kappas[i] for i in members]), circ.n0, len(members))
            w.free()
            for i, com in zip(members, out):
                coms[i] = com.copy()
        super_com = agg.TIPPCommitment(ctx, cname).commit_only_left(srs.ck, np.concatenate(coms))
        job.chal = agg.rom_challenges(super_com, r)
        dev = job.stage1_device(ctx, dev0=dev0)
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
        assert verify_proofs(pvks[job.class_of(5)], [proofs[5]], [pub[:2] + [pub[2] + 1]]) == [0]      # not under another root
        # the host mirror under the same challenges computes the same root: nothing above came from it
        job.set_challenges(job.chal)
        assert job.root == dev.root
        apk = agg.AggProvingKey(ctx, cname, srs.ck, [classes[job.class_of(i)][1].vk for i in range(n)])
        proof, inst = apk.agg_subcircuit_proofs(Merlin(b"test-r1cs-job"), super_com, proofs, pub, srs)
        assert tipa.Tipp(ctx, cname).verify(tipa.verifier_key(ctx, cname, srs), inst["commitment"], inst["output"], inst["twist"],
                                            proof)
    finally:
        if dev is not None:
            dev.free()
        dev0.free()
        for pvk in pvks.values():
            pvk.free()
        for _c, _pk, dpk in classes.values():
            dpk.free()
        for rb in srs.resident.values():
            rb.free()


@pytest.mark.parametrize("cname", CURVES)
def test_owner_tampering_is_found_in_the_row_the_mirror_names(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    r = CURVE_PARAMS[cname]["r"]
    job, _honest = owner_tampering(cname)
    dev = job.stage1_device(ctx)
    try:
        for members in ([5], [6, 2], [7]):             # the owner; a borrower beside the same partition of another transaction
            circ = job.make_class(members[0])
            want = [r1cs_bad_rows(*circ.rows(), job.assignment_ints(i), r) for i in members]
            assert want[0] and circ.block_of(want[0][0]) == "constraints"
            mats = [tuple(capi.DeviceBuffer.from_host(ctx, x) for x in m) for m in circ.csr(circ.fc)]
            z = _prefilled(ctx, len(members) * circ.n_v * ctx.fr_bytes)
            try:
                dev.fill(circ, members, z)
                verdicts, rows = ctx.r1cs_check(*mats, z, n_v=circ.n_v, batch=len(members), cap=8)
                assert verdicts == [(len(w), w[0] if w else None) for w in want]
                for b, w in enumerate(want):
                    assert rows[b, :len(w)].tolist() == w
                checker = type("M", (), {"r1cs_check": lambda self, z, **kw: ctx.r1cs_check(*mats, z, n_v=circ.n_v, **kw)})()
                with pytest.raises(R1csUnsatisfied) as e:
                    dev.check(checker, z, members)
                assert (e.value.subcircuit, e.value.row) == (members[0], want[0][0])
            finally:
                z.free()
                for m in mats:
                    for x in m:
                        x.free()
    finally:
        dev.free()


# ---- refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_every_refusal_leaves_the_output_untouched(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    job, _ = _job(cname, "p4t4")
    fr = ctx.fr_bytes
    base, wit = job.tables(), job.witness_bytes()
    circ = job.make_class(5)
    members = np.array([5, 9, 1], np.uint32)
    n_tr = int(job.offsets[-1]) * 2 * fr
    z = _prefilled(ctx, len(members) * circ.n_v * fr)
    out_d = _prefilled(ctx, n_tr)
    out_h = np.full(n_tr, PATTERN, np.uint8)

    def desc(witness=wit, **kw):
        t = dict(base)
        t.update(kw)
        return ctx._r1cs_job_desc(t, witness)

    def untouched():
        return (z.to_host() == PATTERN).all() and (out_d.to_host() == PATTERN).all() and (out_h == PATTERN).all()

    def trace(d, out):
        return ctx.lib.hk_r1cs_job_trace(ctx.handle, C.byref(d[0]), capi.ptr(out))

    def witness(d, sub=members, n_v=circ.n_v, col0=circ.body_col0, out=z, batch=None):
        sub = np.ascontiguousarray(sub, dtype=np.uint32)
        return ctx.lib.hk_r1cs_job_witness(ctx.handle, C.byref(d[0]), sub.ctypes.data if sub is not None else None,
                                           sub.size if batch is None else batch, n_v, col0, capi.ptr(out))

    def null(d, field):
        setattr(d[0], field, None)
        return d

    rank, src, so, wo, bl = (base[k].copy() for k in ("slot_rank", "slot_src", "slot_offsets", "wit_offsets", "body_len"))
    rank[3], src[4] = base["sets_per_tx"], base["tx_len"]
    so[2] = so[1] - 1
    bl[1] = wo[2] - wo[1]                              # the body would take every wire, the constant included
    wo[2] = wo[1]
    bad_both = [null(desc(), f) for f in ("slot_offsets", "slot_rank", "slot_src", "witness_mont")]
    bad_both += [desc(n_parts=0), desc(n_txs=0), desc(slot_offsets=so), desc(slot_rank=rank), desc(slot_src=src),
                 desc(sets_per_tx=1 << 30, slot_rank=base["slot_rank"]),               # 1 + 4 x 2^30 is not below 2^32
                 desc(tx_stride=base["tx_len"] - 1), desc(tx_len=0)]
    try:
        for k, d in enumerate(bad_both):
            for out in (out_d, out_h):
                assert trace(d, out) == capi.HK_ERR_ARG, k
            assert witness(d) == capi.HK_ERR_ARG, k
            assert untouched(), k
        assert ctx.lib.hk_r1cs_job_trace(ctx.handle, C.byref(desc()[0]), None) == capi.HK_ERR_ARG
        assert ctx.lib.hk_r1cs_job_trace(ctx.handle, None, capi.ptr(out_d)) == capi.HK_ERR_ARG
        bad_wit = [null(desc(), "wit_offsets"), null(desc(), "body_len"), desc(wit_offsets=wo), desc(body_len=bl)]
        for k, d in enumerate(bad_wit):
            assert witness(d) == capi.HK_ERR_ARG, k
        ok = desc()
        calls = [dict(sub=[5, 16, 1]),                                     # sub_index[b] >= P T
                 dict(sub=[5, 9, 2]),                                      # another partition
                 dict(col0=0), dict(col0=circ.body_col0 + 1),              # the body range not inside [1, n_v)
                 dict(n_v=circ.body_col0 + circ.part.body_len - 1),
                 dict(out=np.full(z.nbytes, PATTERN, np.uint8)),           # z_out on the host
                 dict(out=None), dict(batch=1 << 20), dict(n_v=1 << 31)]
        for kw in calls:
            assert witness(ok, **kw) == capi.HK_ERR_ARG, kw
        assert ctx.lib.hk_r1cs_job_witness(ctx.handle, C.byref(ok[0]), None, 3, circ.n_v, circ.body_col0, z.ptr) == capi.HK_ERR_ARG
        assert untouched()
        # nothing to do is no error, and writes nothing
        assert witness(ok, sub=np.zeros(0, np.uint32)) == capi.HK_OK
        empty = desc(slot_offsets=np.zeros(5, np.uint32), slot_rank=np.zeros(0, np.uint32), slot_src=np.zeros(0, np.uint32))
        empty[0].slot_rank = empty[0].slot_src = so.ctypes.data            # any non-NULL pointer: no slot is read
        assert trace(empty, out_d) == capi.HK_OK
        assert untouched()
        # ... and the same descriptor, unharmed, still works
        assert trace(ok, out_h) == capi.HK_OK and (out_h == job.flat("time")).all()
    finally:
        z.free()
        out_d.free()
    assert SRC_ZERO == 0xFFFFFFFF
