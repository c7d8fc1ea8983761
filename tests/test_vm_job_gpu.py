"""GPU: one whole VM job (hekaton_system_amd/vm_circuit.py `VmJob`; distributed-prover/src/vm/) with both witness stages on
the device: keys of its three classes (hk_keygen), stage-0 rows (hk_ram_stage0_witness) into hk_commit_batch, the super
commitment and the four RAM challenges, hk_trace_sort -> hk_exec_tree -> hk_ram_stage1_witness into hk_prove_batch, every
proof through hk_verify_batch with the five public inputs, the proofs aggregated under a six-element gamma_abc_g, and a proof
made from a tampered trace rejected."""
import numpy as np
import pytest

from hekaton_system_amd import aggregation as agg, capi, tipa
from hekaton_system_amd.chacha import ChaCha12Rng
from hekaton_system_amd.cp_groth16 import (CURVE_PARAMS, FrCodec, Proof, SeededRng, generate_parameters_device,
                                           prepare_verifying_key, verify_proofs)
from hekaton_system_amd.merlin import Transcript as Merlin
from hekaton_system_amd.transcript import RAM, RunningEvaluation
from hekaton_system_amd.vm_circuit import RamStage1Device
from tests.vm_cases import tamper_read_value, vm_job

pytestmark = pytest.mark.gpu


def _groups(job):
    groups = {}
    for idx in range(job.n):
        groups.setdefault(job.class_of(idx), []).append(idx)
    return groups


def _prove_rows(ctx, job, dev, classes, members, kappas, rng, r, fc):
    """hk_ram_stage1_witness rows of `members` (one class) into hk_prove_batch: [(a, b, c)] per member."""
    circ, _pk, dpk = classes[job.class_of(members[0])]
    z = capi.DeviceBuffer(ctx, len(members) * circ.n_v * ctx.fr_bytes)
    try:
        dev.fill(circ, members, z)
        rs, ss = fc.enc([rng.fr(r) for _ in members]), fc.enc([rng.fr(r) for _ in members])
        a, b, c = dpk.prove_batch(z, rs, ss, fc.enc([kappas[i] for i in members]), circ.n_v, len(members))
    finally:
        z.free()
    return list(zip(a, b, c))


@pytest.mark.parametrize("cname,full", [("bn254", True), ("bls12_381", False)])
def test_vm_job_commit_prove_verify_aggregate(cname, full, ctx_bn254, ctx_bls):
    ctx = ctx_bn254 if cname == "bn254" else ctx_bls
    r = CURVE_PARAMS[cname]["r"]
    fc = FrCodec(cname)
    job = vm_job(cname, 2, 1, dummy=4, chal=None)
    n = job.n
    groups = _groups(job)
    assert len(groups) == 3
    # ---- 1. keys of the three classes
    classes = {}
    for key, members in groups.items():
        circ = job.make_class(members[0])
        pk, _td = generate_parameters_device(circ, cname, SeededRng(bytes([len(classes) + 1]) * 32), ctx)
        assert len(pk.vk.gamma_abc_g) == 6 * ctx.g1_bytes
        classes[key] = (circ, pk, pk.upload(ctx))
    rng = ChaCha12Rng(b"\x09" * 32)
    srs = tipa.setup(ctx, cname, n, rng.fr(r), rng.fr(r))
    vks = [classes[job.class_of(i)][1].vk for i in range(n)]
    # ---- 2. stage-0 rows from the device into hk_commit_batch
    kappas = [rng.fr(r) for _ in range(n)]
    coms = [None] * n
    dev0 = job.stage0_device(ctx)
    for key, members in groups.items():
        circ, _pk, dpk = classes[key]
        w = dev0.rows(members)
        out = dpk.commit_batch(0, w, fc.enc([kappas[i] for i in members]), circ.n0, len(members))
        w.free()
        for i, com in zip(members, out):
            coms[i] = com.copy()
    # the commitment of the host's stage-0 witness is the same one
    circ, _pk, dpk = classes[job.class_of(1)]
    assert (dpk.commit(0, fc.enc(job.stage0_ints(1)), fc.enc1(kappas[1])) == coms[1]).all()
    # ---- 3. the super commitment, then the four RAM challenges
    com = agg.TIPPCommitment(ctx, cname)
    super_com = com.commit_only_left(srs.ck, np.concatenate(coms))
    job.chal = RunningEvaluation.new(RAM, super_com, r).challenges
    assert len(job.chal) == 4
    # ---- 4. stage 1 on the device, then hk_prove_batch
    dev = job.stage1_device(ctx, traces=dev0.traces)
    pub = list(job.chal) + [dev.root]
    proofs = [None] * n
    for key, members in groups.items():
        for i, (a, b, c) in zip(members, _prove_rows(ctx, job, dev, classes, members, kappas, rng, r, fc)):
            proofs[i] = Proof(a.copy(), b.copy(), c.copy(), [coms[i]])
    dev.free()
    dev0.free()
    # ---- 5. every proof accepted with public inputs (c1, c2, c3, tr_chal, root)
    pvks = {key: prepare_verifying_key(ctx, classes[key][1].vk) for key in groups}
    for key, members in groups.items():
        assert verify_proofs(pvks[key], [proofs[i] for i in members], [pub] * len(members)) == [1] * len(members)
    # ... and not with another root
    key = job.class_of(1)
    assert verify_proofs(pvks[key], [proofs[1]], [pub[:4] + [pub[4] + 1]]) == [0]
    if full:
        # ---- 6. the four proofs aggregated under six gamma_abc_g elements, the TIPP proof accepted
        apk = agg.AggProvingKey(ctx, cname, srs.ck, vks)
        assert apk.n_s == 6 and len(apk.com_s) == 6
        proof, inst = apk.agg_subcircuit_proofs(Merlin(b"test-vm"), super_com, proofs, pub, srs)
        T = tipa.Tipp(ctx, cname)
        assert T.verify(tipa.verifier_key(ctx, cname, srs), inst["commitment"], inst["output"], inst["twist"], proof)
        with pytest.raises(AssertionError):
            apk.agg_front(super_com, proofs, pub[:3], pt=Merlin(b"test-vm"))           # three inputs are not this key's
        # ---- 7. a proof made from a tampered trace (a read that returns another value) is rejected
        bad_job = vm_job(cname, 2, 1, dummy=4, chal=None)
        sub, _block, _pair, _rule = tamper_read_value(bad_job)
        bad_job.chal = job.chal
        up = lambda x: capi.DeviceBuffer.from_host(ctx, x)
        traces = [up(bad_job.flat("time")), up(bad_job.flat("addr"))]
        bad_dev = RamStage1Device(bad_job, ctx, traces=traces)
        a, b, c = _prove_rows(ctx, bad_job, bad_dev, classes, [sub], kappas, rng, r, fc)[0]
        # its own stage-0 commitment and its own root: the proof is wrong for no other reason than the broken rule
        circ, _pk, dpk = classes[bad_job.class_of(sub)]
        com_bad = dpk.commit(0, fc.enc(bad_job.stage0_ints(sub)), fc.enc1(kappas[sub]))
        bad_pub = list(job.chal) + [bad_dev.root]
        assert verify_proofs(pvks[bad_job.class_of(sub)], [Proof(a.copy(), b.copy(), c.copy(), [com_bad])], [bad_pub]) == [0]
        bad_dev.free()
        for x in traces:
            x.free()
    for pvk in pvks.values():
        pvk.free()
    for _c, _pk, dpk in classes.values():
        dpk.free()
    for rb in srs.resident.values():
        rb.free()
