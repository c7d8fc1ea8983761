"""GPU: agg_verify.verify_aggregate on real aggregates.  The job is the "tiny" synthetic config of tests/test_tipa_gpu.py
(8 subcircuits, 5 key classes) aggregated under Merlin(b"test-agg-verify"): the key and the proof go through their wire forms
and the verifier accepts from the bytes, the super commitment and the public inputs alone; it derives the prover's own twist,
s, t, com_lr and z_lr, and its prod_c e(alpha_c, beta_c)^(sigma_c) is the prover's multi-pairing bit for bit; every single
change is rejected with the reason of the check that must catch it; a bad subcircuit proof aggregated with
assert_products=False is caught by the product equation; a proof with a point off its curve does not deserialize; and the
smallest VM job (six gamma_abc_g elements, RAM challenges among the public inputs) is accepted with mem_type=RAM."""
import random

import numpy as np
import pytest

from hekaton_system_amd import agg_verify as av, aggregation as agg, capi, tipa
from hekaton_system_amd.chacha import ChaCha12Rng
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec, Proof, SeededRng, generate_parameters, generate_parameters_device
from hekaton_system_amd.merlin import Transcript as Merlin
from hekaton_system_amd.transcript import RAM, RunningEvaluation
from hekaton_system_amd.workload import config_classes, make_config, representative_subcircuit

pytestmark = pytest.mark.gpu

LABEL = b"test-agg-verify"


class _Job:
    pass


def _tiny_job(ctx, cname):
    """The aggregate of the tiny config, and what a test needs of the proving side to compare with or to aggregate again."""
    r = CURVE_PARAMS[cname]["r"]
    fc = FrCodec(cname)
    family, n, reps = config_classes("tiny")
    rnd = random.Random(21)
    keys = {}
    for rep in reps:
        circ = make_config(cname, "tiny", rep)
        pk, _td = generate_parameters(circ, cname, SeededRng(bytes([rep + 17]) * 32), ctx)
        keys[rep] = (circ, pk, pk.upload(ctx))
    proofs, coms, vks, pub = [], [], [], None
    for idx in range(n):
        circ, pk, dpk = keys[representative_subcircuit(family, n, idx)]
        circ.set_witness_seed(4)
        z = circ.assignment_ints()
        pub = pub or z[1:4]
        kappa = ChaCha12Rng(bytes([idx + 60]) * 32).fr(r)
        com = dpk.commit(0, circ.stage0_witness_bytes(), fc.enc1(kappa))
        a, b, c = dpk.prove(circ.full_assignment_bytes(), fc.enc1(rnd.randrange(r)), fc.enc1(rnd.randrange(r)), fc.enc([kappa]),
                            n_v=circ.n_v)
        proofs.append(Proof(a, b, c, [com])); coms.append(com); vks.append(pk.vk)
    for _c, _pk, dpk in keys.values():
        dpk.free()
    j = _Job()
    j.n, j.pub, j.proofs = n, list(pub), proofs
    j.classes = [representative_subcircuit(family, n, idx) for idx in range(n)]
    j.srs = tipa.setup(ctx, cname, n, rnd.randrange(2, r), rnd.randrange(2, r))
    j.apk = agg.AggProvingKey(ctx, cname, j.srs.ck, vks)
    j.super_com = j.apk.com.commit_only_left(j.srs.ck, np.concatenate(coms))
    tipp_proof, j.inst = j.apk.agg_subcircuit_proofs(Merlin(LABEL), j.super_com, proofs, pub, j.srs)
    avk = av.AggVerifyingKey.from_proving_key(j.apk, tipa.verifier_key(ctx, cname, j.srs))
    j.key_bytes, j.proof_bytes = avk.serialize(), av.AggProof.from_instance(tipp_proof, j.inst).serialize()
    return j


@pytest.fixture(scope="module")
def jobs(ctx_bn254, ctx_bls):
    made = {}

    def get(cname):
        if cname not in made:
            made[cname] = _tiny_job(ctx_bn254 if cname == "bn254" else ctx_bls, cname)
        return made[cname]
    yield get
    for j in made.values():
        for rb in j.srs.resident.values():
            rb.free()


def _ctx(cname, ctx_bn254, ctx_bls):
    return ctx_bn254 if cname == "bn254" else ctx_bls


def _read(ctx, cname, j):
    return av.AggVerifyingKey.deserialize(ctx, cname, j.key_bytes), av.AggProof.deserialize(ctx, cname, j.proof_bytes)


@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_accepts_from_bytes_alone(cname, jobs, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    j = jobs(cname)
    key_bytes, proof_bytes, super_com, pub = j.key_bytes, j.proof_bytes, agg.IppCom(j.apk.F, j.super_com.t, j.super_com.u), list(j.pub)
    del j                                                     # nothing of the proving side below this line
    avk = av.AggVerifyingKey.deserialize(ctx, cname, key_bytes)
    proof = av.AggProof.deserialize(ctx, cname, proof_bytes)
    assert (avk.n, avk.n_s, len(avk.alpha_beta), proof.n, len(proof.tipp["rounds"])) == (8, 4, 5, 8, 3)
    # the key's size does not depend on the proofs: seven points, 2 (n_s + 3) + 5 GT elements, the class runs
    assert not hasattr(avk, "alpha") and avk.class_of.size == 8
    verdict = av.verify_aggregate(ctx, avk, super_com, pub, proof, Merlin(LABEL))
    assert verdict and verdict.ok and verdict.reason == av.ACCEPTED
    assert avk.serialize() == key_bytes and proof.serialize() == proof_bytes


@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_derives_the_provers_values(cname, jobs, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    j = jobs(cname)
    fc = FrCodec(cname)
    avk, proof = _read(ctx, cname, j)
    assert avk.class_of.tolist() == [sorted(set(j.classes), key=j.classes.index).index(c) for c in j.classes]
    trace = {}
    assert av.verify_aggregate(ctx, avk, j.super_com, j.pub, proof, Merlin(LABEL), trace=trace)
    inst = j.inst
    assert trace["twist"] == inst["twist"] and trace["com_lr"] == inst["commitment"] and trace["z_lr"] == inst["output"]
    # s and t as agg_front drew them: a reader of the same transcript
    pt = Merlin(LABEL)
    pt.append_serializable(b"AB-commitment", inst["com_ab"].serialize_uncompressed())
    pt.append_serializable(b"C-commitment", inst["com_c"].serialize_uncompressed())
    pt.append_serializable(b"D-commitment", j.super_com.serialize_uncompressed())
    assert pt.challenge_scalar(b"r-random-fiatshamir", fc.r) == trace["twist"]
    pt.append_serializable(b"cross-terms", av.cross_terms_bytes(j.apk.F, inst["cross_terms"]))
    assert (pt.challenge_scalar(b"s-random-fiatshamir", fc.r), pt.challenge_scalar(b"t-random-fiatshamir", fc.r)) == (trace["s"], trace["t"])
    # sigma is the mirror's, and prod_c e(alpha_c, beta_c)^(sigma_c) is the prover's multi-pairing of the swept alphas
    assert fc.dec(trace["sigma"]) == av.class_power_sums_host(trace["twist"], avk.class_of.tolist(), 5, fc.r)
    tw = agg.twist_powers(ctx, fc, inst["twist"], j.n, 1)
    try:
        alpha_r = ctx.scalar_pairing(1, j.apk.alpha, tw, j.n)
    finally:
        tw.free()
    want = ctx.multi_pairing(alpha_r, j.apk.beta, j.n)
    assert trace["z_alpha_beta_bytes"].tobytes() == np.asarray(want, np.uint8).tobytes()


def _gt_sq(F, x):
    return F.mul(x, x)


def avk_F(avk):
    return avk.com_h.F


# name -> (what to change, the reason expected).  change(ctx, avk, proof, call): `call` holds super_com, pub and label
_REJECTIONS = {
    "a public input + 1": (lambda ctx, avk, proof, call: call["pub"].__setitem__(1, call["pub"][1] + 1), av.R_TIPP),
    "another super_com": (lambda ctx, avk, proof, call: call.__setitem__("super_com", agg.IppCom(
        avk_F(avk), _gt_sq(avk_F(avk), call["super_com"].t), call["super_com"].u)), av.R_PRODUCT),
    "cross[0][0] squared": (lambda ctx, avk, proof, call: proof.cross_terms[0].__setitem__(0, _gt_sq(avk_F(avk), proof.cross_terms[0][0])),
                            av.R_PRODUCT),
    "cross[1][2] replaced": (lambda ctx, avk, proof, call: proof.cross_terms[1].__setitem__(2, proof.cross_terms[2][1]), av.R_TIPP),
    "com_c altered": (lambda ctx, avk, proof, call: setattr(proof, "com_c", agg.IppCom(
        avk_F(avk), proof.com_c.u, proof.com_c.t, ctx=ctx)), av.R_PRODUCT),
    "two classes' alpha_beta exchanged": (lambda ctx, avk, proof, call: avk.alpha_beta.__setitem__(
        slice(0, 2), [avk.alpha_beta[1], avk.alpha_beta[0]]), av.R_PRODUCT),
    "two indices of different classes exchanged": (lambda ctx, avk, proof, call: _swap_classes(avk), av.R_PRODUCT),
    "another transcript label": (lambda ctx, avk, proof, call: call.__setitem__("label", b"another label"), av.R_PRODUCT),
    "a round message altered": (lambda ctx, avk, proof, call: proof.tipp["rounds"][1].__setitem__(
        "ZL", avk_F(avk).mul(proof.tipp["rounds"][1]["ZL"], proof.tipp["rounds"][1]["ZR"])), av.R_TIPP),
    "final_a doubled": (lambda ctx, avk, proof, call: proof.tipp.__setitem__(
        "final_a", ctx.points_lincomb(1, [proof.tipp["final_a"]], FrCodec(ctx.curve).enc([2]), n=1)), av.R_TIPP),
    "one public input fewer": (lambda ctx, avk, proof, call: call["pub"].pop(), av.R_INPUT_COUNT),
    "a proof of another size": (lambda ctx, avk, proof, call: setattr(proof, "n", 16), av.R_SIZE),
}


def _swap_classes(avk):
    cls = avk.class_of.copy()
    i = 0
    k = next(k for k in range(len(cls)) if cls[k] != cls[i])
    cls[i], cls[k] = cls[k], cls[i]
    avk.class_of = cls


@pytest.mark.parametrize("what", list(_REJECTIONS))
@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_rejects_one_change_with_its_reason(cname, what, jobs, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    j = jobs(cname)
    avk, proof = _read(ctx, cname, j)
    call = dict(super_com=j.super_com, pub=list(j.pub), label=LABEL)
    change, reason = _REJECTIONS[what]
    change(ctx, avk, proof, call)
    verdict = av.verify_aggregate(ctx, avk, call["super_com"], call["pub"], proof, Merlin(call["label"]))
    assert not verdict and not verdict.ok and verdict.reason == reason, (what, verdict)


@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_a_bad_subcircuit_proof_is_caught_by_the_product_equation(cname, jobs, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    j = jobs(cname)
    fc = FrCodec(cname)
    bad = list(j.proofs)
    p3 = bad[3]
    bad[3] = Proof(p3.a, p3.b, ctx.points_lincomb(1, [np.asarray(p3.c, np.uint8)], fc.enc([2]), n=1), p3.ds)
    with pytest.raises(AssertionError):                       # the aggregator's own assertion, as before
        j.apk.agg_subcircuit_proofs(Merlin(LABEL), j.super_com, bad, j.pub, j.srs)
    tipp_proof, inst = j.apk.agg_subcircuit_proofs(Merlin(LABEL), j.super_com, bad, j.pub, j.srs, assert_products=False)
    proof = av.AggProof.deserialize(ctx, cname, av.AggProof.from_instance(tipp_proof, inst).serialize())
    avk = av.AggVerifyingKey.deserialize(ctx, cname, j.key_bytes)
    verdict = av.verify_aggregate(ctx, avk, j.super_com, j.pub, proof, Merlin(LABEL))
    assert not verdict and verdict.reason == av.R_PRODUCT


@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_a_proof_with_a_point_off_its_curve_does_not_deserialize(cname, jobs, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    j = jobs(cname)
    fq, g1b, g2b = ctx.fq_bytes, ctx.g1_bytes, ctx.g2_bytes
    gt = 12 * fq
    final_b = 8 + 5 * gt + 8 + 4 * (8 + 4 * gt) + 8 + 3 * 6 * gt + g1b        # n, com_ab, com_c, cross terms, rounds, final_a
    assert len(j.proof_bytes) == final_b + g2b + 2 * g2b + 2 * g1b + 2 * g2b + 2 * g1b
    bad = bytearray(j.proof_bytes)
    # the lowest byte of y's c0: little-endian x | y on BN254, big-endian x.c1 x.c0 y.c1 y.c0 on BLS12-381
    bad[final_b + 2 * fq if cname == "bn254" else final_b + g2b - 1] ^= 1
    with pytest.raises(ValueError, match="G2 point is not on the curve"):
        av.AggProof.deserialize(ctx, cname, bytes(bad))
    av.AggProof.deserialize(None, cname, bytes(bad))           # without a context the points are not checked


# ---- six gamma_abc_g elements: the smallest VM job -----------------------------------------------------------------------
def test_vm_job_is_accepted_with_its_ram_challenges(ctx_bn254):
    from tests.vm_cases import vm_job
    cname, ctx = "bn254", ctx_bn254
    r = CURVE_PARAMS[cname]["r"]
    fc = FrCodec(cname)
    job = vm_job(cname, 2, 1, dummy=4, chal=None)
    n = job.n
    groups = {}
    for idx in range(n):
        groups.setdefault(job.class_of(idx), []).append(idx)
    assert n == 4 and len(groups) == 3
    classes = {}
    for key, members in groups.items():
        circ = job.make_class(members[0])
        pk, _td = generate_parameters_device(circ, cname, SeededRng(bytes([len(classes) + 31]) * 32), ctx)
        classes[key] = (circ, pk, pk.upload(ctx))
    rng = ChaCha12Rng(b"\x0b" * 32)
    srs = tipa.setup(ctx, cname, n, rng.fr(r), rng.fr(r))
    vks = [classes[job.class_of(i)][1].vk for i in range(n)]
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
    super_com = agg.TIPPCommitment(ctx, cname).commit_only_left(srs.ck, np.concatenate(coms))
    job.chal = RunningEvaluation.new(RAM, super_com, r).challenges
    dev = job.stage1_device(ctx, traces=dev0.traces)
    pub = list(job.chal) + [dev.root]
    proofs = [None] * n
    for key, members in groups.items():
        circ, _pk, dpk = classes[key]
        z = capi.DeviceBuffer(ctx, len(members) * circ.n_v * ctx.fr_bytes)
        try:
            dev.fill(circ, members, z)
            rs, ss = fc.enc([rng.fr(r) for _ in members]), fc.enc([rng.fr(r) for _ in members])
            a, b, c = dpk.prove_batch(z, rs, ss, fc.enc([kappas[i] for i in members]), circ.n_v, len(members))
        finally:
            z.free()
        for i, abc in zip(members, zip(a, b, c)):
            proofs[i] = Proof(abc[0].copy(), abc[1].copy(), abc[2].copy(), [coms[i]])
    dev.free()
    dev0.free()
    for _c, _pk, dpk in classes.values():
        dpk.free()
    try:
        apk = agg.AggProvingKey(ctx, cname, srs.ck, vks)
        tipp_proof, inst = apk.agg_subcircuit_proofs(Merlin(b"test-agg-verify-vm"), super_com, proofs, pub, srs)
        key_bytes = av.AggVerifyingKey.from_proving_key(apk, tipa.verifier_key(ctx, cname, srs)).serialize()
        proof_bytes = av.AggProof.from_instance(tipp_proof, inst).serialize()
    finally:
        for rb in srs.resident.values():
            rb.free()
    avk = av.AggVerifyingKey.deserialize(ctx, cname, key_bytes)
    proof = av.AggProof.deserialize(ctx, cname, proof_bytes)
    assert (avk.n, avk.n_s, len(avk.alpha_beta), len(pub)) == (4, 6, 3, 5)
    verdict = av.verify_aggregate(ctx, avk, super_com, pub, proof, Merlin(b"test-agg-verify-vm"), mem_type=RAM)
    assert verdict and verdict.reason == av.ACCEPTED
    # tr_chal is the fourth public input: another one is not what the super commitment gives
    wrong = pub[:3] + [(pub[3] + 1) % r] + pub[4:]
    verdict = av.verify_aggregate(ctx, avk, super_com, wrong, proof, Merlin(b"test-agg-verify-vm"), mem_type=RAM)
    assert not verdict and verdict.reason == av.R_INPUT_CHALLENGES
    # without mem_type the statement is whatever the caller says, and the proof is not one of it
    verdict = av.verify_aggregate(ctx, avk, super_com, wrong, proof, Merlin(b"test-agg-verify-vm"))
    assert not verdict and verdict.reason == av.R_TIPP
