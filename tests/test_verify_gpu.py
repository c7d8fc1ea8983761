"""GPU: CP-Groth16 proof verification (hk_vk_prepare / hk_verify_batch / hk_points_check_*, cp-groth16/src/verifier.rs).

Verdicts are pinned against the oracle's big-int verifier (oracle/pyref/pairing.verify_proof) and its [r] P == O
subgroup test, on both curves: the golden fixtures, proofs of the product (hk_prove_batch) with one tamper per row,
points off the curve or outside the prime-order subgroup, shapes across the chunk and grid bounds, and a whole
worker-path job through the coordinator helper."""
import random
import threading

import numpy as np
import pytest

from hekaton_system_amd import aggregation as agg, capi
from hekaton_system_amd.cp_groth16 import (FrCodec, Proof, SeededRng, VerifyingKey, generate_parameters,
                                           prepare_verifying_key, verify_proof, verify_proofs)
from hekaton_system_amd.workload import make_config
from oracle.pyref import curve, groth16 as og, pairing
from oracle.pyref.codec import Codec
from oracle.pyref.params import CURVES
from tests import golden_util as gu
from tests.test_oracle_py import _proof_from_case
from tests.test_pairing_cpu import Enc

pytestmark = pytest.mark.gpu
CURVE_NAMES = ["bn254", "bls12_381"]
N_PROOFS = 37


def _ctx(cname, ctx_bn254, ctx_bls):
    return ctx_bn254 if cname == "bn254" else ctx_bls


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


# ---- oracle helpers -----------------------------------------------------------------------------------------------
def _sqrt_fq(a, q):
    s = pow(a, (q + 1) // 4, q)                 # q = 3 mod 4 on both curves
    return s if s * s % q == a % q else None


def _sqrt_fq2(a, q):
    a0, a1 = a
    n = _sqrt_fq((a0 * a0 + a1 * a1) % q, q)
    if n is None:
        return None
    inv2 = pow(2, -1, q)
    for t in ((a0 + n) * inv2 % q, (a0 - n) * inv2 % q):
        x0 = _sqrt_fq(t, q)
        if x0:
            x1 = a1 * pow(2 * x0, -1, q) % q
            if ((x0 * x0 - x1 * x1) % q, 2 * x0 * x1 % q) == (a0 % q, a1 % q):
                return (x0, x1)
    return None


def _on_curve_g1(cp, start):
    """A point on the G1 curve found from x = start upward (not multiplied by any cofactor)."""
    G1 = curve.G1(cp)
    x = start
    while True:
        y = _sqrt_fq((x ** 3 + G1.b) % cp.q, cp.q)
        if y:
            P = (x, y)
            assert G1.on_curve(P)
            return P
        x += 1


def _on_twist_g2(cp, start):
    """A point on the twist found from x = (start, 1) upward, the cofactor NOT cleared."""
    G2 = curve.G2(cp)
    F = G2.F
    x = (start, 1)
    while True:
        rhs = F.add(F.mul(F.mul(x, x), x), G2.b)
        y = _sqrt_fq2(rhs, cp.q)
        if y:
            Q = (x, y)
            assert G2.on_curve(Q)
            return Q
        x = (x[0] + 1, 1)


def _in_subgroup(G, P, r):
    return G.mul(P, r) is None


# ---- proofs of the product ----------------------------------------------------------------------------------------
_CLASSES = {}


def _product_proofs(ctx, cname):
    """N_PROOFS stage-1 proofs of one "tiny" class (hk_prove_batch), their commitments and public inputs, plus the
    VerifyingKey of a second class of the same shape."""
    if cname in _CLASSES:
        return _CLASSES[cname]
    fc = FrCodec(cname)
    fr = ctx.fr_bytes
    circ = make_config(cname, "tiny")
    pk, _td = generate_parameters(circ, cname, SeededRng(b"VERIFY-CLASS-A-0123456789abcdef!"), ctx)
    pk2, _td2 = generate_parameters(circ, cname, SeededRng(b"VERIFY-CLASS-B-0123456789abcdef!"), ctx)
    dpk = pk.upload(ctx)
    z, coms, xs = [], [], []
    kaps = [0x3000_0005 + 1299709 * j for j in range(N_PROOFS)]
    for j in range(N_PROOFS):
        circ.set_witness_seed(900 + j)
        zj = circ.full_assignment_bytes()
        z.append(zj)
        coms.append(dpk.commit(0, circ.stage0_witness_bytes(), fc.enc1(kaps[j])))
        xs.append(fc.dec(zj[fr:circ.N_INST * fr]))
    rs = [0x1000_0001 + 7919 * j for j in range(N_PROOFS)]
    ss = [0x2000_0003 + 104729 * j for j in range(N_PROOFS)]
    a, b, c = dpk.prove_batch(np.concatenate(z), fc.enc(rs), fc.enc(ss), fc.enc(kaps), circ.n_v, N_PROOFS)
    proofs = [Proof(a[j].copy(), b[j].copy(), c[j].copy(), [coms[j]]) for j in range(N_PROOFS)]
    dpk.free()
    _CLASSES[cname] = (pk.vk, pk2.vk, proofs, xs)
    return _CLASSES[cname]


def _oracle_vk(cd, vk):
    g1, g2 = cd.g1_bytes, cd.g2_bytes
    return og.VerifyingKey(
        alpha_g=cd.g1_from(vk.alpha_g), beta_h=cd.g2_from(vk.beta_h), gamma_h=cd.g2_from(vk.gamma_h),
        last_delta_h=cd.g2_from(vk.last_delta_h),
        gamma_abc_g=[cd.g1_from(vk.gamma_abc_g[i * g1:(i + 1) * g1]) for i in range(len(vk.gamma_abc_g) // g1)],
        deltas_h=[cd.g2_from(vk.deltas_h[i * g2:(i + 1) * g2]) for i in range(len(vk.deltas_h) // g2)])


def _oracle_proof(cd, p):
    return og.Proof(cd.g1_from(p.a), cd.g2_from(p.b), cd.g1_from(p.c), [cd.g1_from(d) for d in p.ds])


def _vk_from_case(cd, case):
    pk = case["pk"]
    return VerifyingKey(alpha_g=gu.hb(pk["alpha_g"]), beta_h=gu.hb(pk["beta_h"]), gamma_h=gu.hb(pk["gamma_h"]),
                        last_delta_h=gu.hb(pk["last_delta_h"]), gamma_abc_g=gu.hb(pk["gamma_abc_g"]),
                        deltas_h=gu.hb(pk["deltas_h"]))


def _flat(ctx, proofs, xs):
    fc = FrCodec(ctx.curve)
    cat = lambda v: np.concatenate([np.asarray(t, np.uint8).reshape(-1) for t in v])
    return (cat([p.a for p in proofs]), cat([p.b for p in proofs]), cat([p.c for p in proofs]),
            cat([d for p in proofs for d in p.ds]), fc.enc([v for x in xs for v in x]))


def _rand(ctx, n, seed=5):
    rnd = random.Random(seed)
    return FrCodec(ctx.curve).enc([rnd.getrandbits(128) | 1 for _ in range(n)])


# ---- golden fixtures ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_golden_fixtures_accepted_and_alpha_beta_exact(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    cp = CURVES[cname]
    cd = Codec(cp)
    T = pairing.tower(cname)
    E = Enc(cp)
    G1 = curve.G1(cp)
    for case in gu.load("groth16.json")[cname]:
        ovk, oproof = _proof_from_case(cd, case)
        pvk = prepare_verifying_key(ctx, _vk_from_case(cd, case))
        assert E.f12_dec(pvk.alpha_beta_gt().tobytes()) == T.f12_flat(T.pairing(ovk.alpha_g, ovk.beta_h))
        proof = Proof(gu.hb(case["proof"]["a"]), gu.hb(case["proof"]["b"]), gu.hb(case["proof"]["c"]),
                      [gu.hb(c) for c in case["comms"]])
        x = case["public_inputs"]
        assert pairing.verify_proof(cname, ovk, oproof, x)
        assert verify_proof(pvk, proof, x)
        bad = Proof(proof.a, proof.b, _u8(cd.g1(G1.add(oproof.c, G1.gen))), proof.ds)
        assert not pairing.verify_proof(cname, ovk, og.Proof(oproof.a, oproof.b, G1.add(oproof.c, G1.gen), oproof.ds), x)
        assert verify_proofs(pvk, [proof, bad, proof], [x, x, x]) == [1, 0, 1]
        pvk.free()


# ---- proofs of the product ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_product_proofs_and_tampering(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    cp = CURVES[cname]
    cd = Codec(cp)
    G1, G2 = curve.G1(cp), curve.G2(cp)
    vk, vk2, proofs, xs = _product_proofs(ctx, cname)
    pvk = prepare_verifying_key(ctx, vk)
    n = len(proofs)
    assert verify_proofs(pvk, proofs, xs) == [1] * n
    assert verify_proofs(pvk, proofs, xs, batch_rng=random.Random(1)) == [1] * n
    r = cp.r

    def tampered(kind):
        ps = [Proof(p.a, p.b, p.c, list(p.ds)) for p in proofs]
        ys = [list(x) for x in xs]
        if kind == "swap_a":
            ps[3].a, ps[20].a = proofs[20].a, proofs[3].a
            return ps, ys, {3, 20}
        if kind == "input":
            ys[7][1] = (ys[7][1] + 1) % r
            return ps, ys, {7}
        if kind == "d_other":
            ps[11].ds = [proofs[12].ds[0]]
            return ps, ys, {11}
        if kind == "neg_b":
            ps[30].b = _u8(cd.g2(G2.neg(cd.g2_from(proofs[30].b))))
            return ps, ys, {30}
        if kind == "c_plus_g":
            ps[0].c = _u8(cd.g1(G1.add(cd.g1_from(proofs[0].c), G1.gen)))
            return ps, ys, {0}
        raise ValueError(kind)

    for kind in ("swap_a", "input", "d_other", "neg_b", "c_plus_g"):
        ps, ys, bad = tampered(kind)
        want = [0 if i in bad else 1 for i in range(n)]
        got = verify_proofs(pvk, ps, ys)
        assert got == want, kind
        assert verify_proofs(pvk, ps, ys, batch_rng=random.Random(2)) == want, kind
        if kind in ("input", "neg_b"):                     # spot checks against the oracle verifier
            ovk = _oracle_vk(cd, vk)
            i = min(bad)
            assert pairing.verify_proof(cname, ovk, _oracle_proof(cd, ps[i]), ys[i]) is False
            assert pairing.verify_proof(cname, ovk, _oracle_proof(cd, ps[i + 1]), ys[i + 1]) is True
    pvk2 = prepare_verifying_key(ctx, vk2)
    assert verify_proofs(pvk2, proofs, xs) == [0] * n
    pvk2.free()
    pvk.free()


# ---- point checks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_points_check_matches_oracle_subgroup_test(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    cp = CURVES[cname]
    cd = Codec(cp)
    G1, G2 = curve.G1(cp), curve.G2(cp)
    rnd = random.Random(31)
    g1 = [G1.mul(cp.g1_gen, rnd.randrange(1, cp.r)) for _ in range(5)] + [None]
    g1 += [_on_curve_g1(cp, 5 + 1000 * k) for k in range(4)]
    g1 += [(g1[0][0], (g1[0][1] + 1) % cp.q)]                                  # off the curve
    g2 = [G2.mul(cp.g2_gen, rnd.randrange(1, cp.r)) for _ in range(5)] + [None]
    g2 += [_on_twist_g2(cp, 3 + 1000 * k) for k in range(4)]
    g2 += [(g2[0][0], (g2[0][1][0], (g2[0][1][1] + 1) % cp.q))]
    want1 = [int(G1.on_curve(P) and _in_subgroup(G1, P, cp.r)) for P in g1]
    want2 = [int(G2.on_curve(Q) and _in_subgroup(G2, Q, cp.r)) for Q in g2]
    assert want1[-1] == 0 and want2[-1] == 0
    assert 0 in want2[6:10]                                                   # twist points outside the subgroup
    if cname == "bn254":
        assert want1[6:10] == [1] * 4                                         # cofactor 1: on the curve is enough
    else:
        assert 0 in want1[6:10]
    got1 = ctx.points_check(1, _u8(b"".join(cd.g1(P) for P in g1)))
    got2 = ctx.points_check(2, _u8(b"".join(cd.g2(Q) for Q in g2)))
    assert list(got1) == want1
    assert list(got2) == want2


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_invalid_points_give_verdict_2(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    cp = CURVES[cname]
    cd = Codec(cp)
    G1, G2 = curve.G1(cp), curve.G2(cp)
    vk, _vk2, proofs, xs = _product_proofs(ctx, cname)
    pvk = prepare_verifying_key(ctx, vk)
    ps = [Proof(p.a, p.b, p.c, list(p.ds)) for p in proofs[:8]]
    ys = xs[:8]
    A = cd.g1_from(ps[0].a)
    ps[0].a = _u8(cd.g1((A[0], (A[1] + 1) % cp.q)))                          # off the curve
    Q = next(q for q in (_on_twist_g2(cp, 3 + 1000 * k) for k in range(8)) if not _in_subgroup(G2, q, cp.r))
    ps[1].b = _u8(cd.g2(Q))                                                    # on the twist, outside G2
    want = [2, 2, 1, 1, 1, 1, 1, 1]
    if cname == "bls12_381":
        P = next(p for p in (_on_curve_g1(cp, 5 + 1000 * k) for k in range(8)) if not _in_subgroup(G1, p, cp.r))
        ps[2].c = _u8(cd.g1(P))                                                # on the curve, outside G1
        want[2] = 2
    else:
        P = _on_curve_g1(cp, 77)                                               # BN254 G1: every curve point is valid
        assert _in_subgroup(G1, P, cp.r)
        ps[2].ds = [_u8(cd.g1(P))]
        want[2] = 0
    inf = _u8(bytes(ctx.g1_bytes))
    ps[3].a = inf
    ps[4].c = inf
    ps[5].ds = [inf]
    ovk = _oracle_vk(cd, vk)
    for i in (3, 4, 5):                                                        # infinity is valid: the oracle's verdict
        want[i] = int(pairing.verify_proof(cname, ovk, _oracle_proof(cd, ps[i]), ys[i]))
    got = verify_proofs(pvk, ps, ys)
    assert got == want
    assert verify_proofs(pvk, ps, ys, batch_rng=random.Random(3)) == want
    # without the check flag such proofs still get a verdict (no fault); batch mode needs the flag
    a, b, c, ds, x = _flat(ctx, ps, ys)
    v = pvk.device.verify(a, b, c, ds, x, check_points=False)
    assert v.shape == (8,) and set(v.tolist()) <= {0, 1}
    assert v[6] == 1 and v[7] == 1
    with pytest.raises(capi.HekatonError) as ei:
        pvk.device.verify(a, b, c, ds, x, check_points=False, rand=_rand(ctx, 8))
    assert ei.value.status == capi.HK_ERR_ARG
    pvk.free()


# ---- shapes and errors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_shapes_chunks_and_errors(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    vk, _vk2, proofs, xs = _product_proofs(ctx, cname)
    pvk = prepare_verifying_key(ctx, vk)
    dvk = pvk.device
    assert verify_proofs(pvk, proofs[:1], xs[:1]) == [1]
    assert verify_proofs(pvk, [], []) == []
    a, b, c, ds, x = _flat(ctx, proofs[:1], xs[:1])
    assert dvk.verify(a[:0], b[:0], c[:0], ds[:0], x[:0], n=0).shape == (0,)
    # n above the 16-bit grid.y bound of count x steps (and above one chunk): repeated rows, one bad proof
    n = 1100
    idx = [i % len(proofs) for i in range(n)]
    big = [proofs[i] for i in idx]
    bx = [xs[i] for i in idx]
    bad = Proof(big[1050].a, big[1050].b, big[1049].c, big[1050].ds)
    big[1050] = bad
    want = [1] * n
    want[1050] = 0
    assert verify_proofs(pvk, big, bx) == want
    assert verify_proofs(pvk, big, bx, batch_rng=random.Random(4)) == want
    # host and device pointers
    a, b, c, ds, x = _flat(ctx, proofs, xs)
    host = dvk.verify(a, b, c, ds, x)
    bufs = [capi.DeviceBuffer.from_host(ctx, t) for t in (a, b, c, ds, x)]
    vout = capi.DeviceBuffer(ctx, len(proofs))
    dvk.verify(*bufs, n=len(proofs), verdicts=vout)
    assert vout.to_host().tolist() == host.tolist() == [1] * len(proofs)
    for t in bufs + [vout]:
        t.free()
    # wrong input length
    with pytest.raises(capi.HekatonError) as ei:
        verify_proofs(pvk, proofs[:2], [xs[0], xs[1][:-1]])
    assert ei.value.status == capi.HK_ERR_LEN
    pvk.free()


def test_two_threads_share_a_context(ctx_bn254):
    ctx = ctx_bn254
    vk, _vk2, proofs, xs = _product_proofs(ctx, "bn254")
    pvk = prepare_verifying_key(ctx, vk)
    ps = [Proof(p.a, p.b, p.c, list(p.ds)) for p in proofs]
    ps[5] = Proof(proofs[6].a, proofs[5].b, proofs[5].c, proofs[5].ds)
    ps[33] = Proof(proofs[33].a, proofs[33].b, proofs[33].c, proofs[32].ds)
    serial = [verify_proofs(pvk, ps, xs), verify_proofs(pvk, ps[::-1], xs[::-1])]
    got = [None, None]

    def run(k):
        for _ in range(3):
            got[k] = verify_proofs(pvk, ps if k == 0 else ps[::-1], xs if k == 0 else xs[::-1])

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == serial
    assert serial[0].count(0) == 2
    pvk.free()


# ---- end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_worker_job_proofs_accepted_by_coordinator_helper(cname, ctx_bn254, ctx_bls):
    from hekaton_system_amd.chacha import ChaCha12Rng
    from hekaton_system_amd.cp_groth16 import CURVE_PARAMS
    from hekaton_system_amd.sha_circuit import ShaMerkleJob
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    r = CURVE_PARAMS[cname]["r"]
    fc = FrCodec(cname)
    n, ns, n_portals = 8, 1, 4
    leaves = [bytes([(29 * i + 3 * k) & 0xff for k in range(64)]) for i in range(n // 2)]
    job = ShaMerkleJob(cname, n, ns, n_portals, leaves)
    classes = {}
    for idx in range(n):
        key = job.class_of(idx)
        if key not in classes:
            circ = job.make_class(idx)
            pk, _td = generate_parameters(circ, cname, SeededRng(bytes([len(classes) + 1]) * 32), ctx)
            classes[key] = (circ, pk, pk.upload(ctx))
    rng = ChaCha12Rng(b"\x07" * 32)
    seeds = [rng.gen_seed() for _ in range(n)]
    kappas = [ChaCha12Rng(sd).fr(r) for sd in seeds]
    coms = [classes[job.class_of(i)][2].commit(0, fc.enc(job.stage0_ints(i)), fc.enc1(kappas[i])) for i in range(n)]
    entry_chal, tr_chal = 0x1234567, 0x7654321
    job.set_challenges(entry_chal, tr_chal)
    proofs = []
    for i in range(n):
        circ, pk, dpk = classes[job.class_of(i)]
        w = job.inputs(i)
        a, b, c = dpk.prove(circ.assignment_bytes(w)[0], fc.enc1(rng.fr(r)), fc.enc1(rng.fr(r)), fc.enc([kappas[i]]), n_v=circ.n_v)
        proofs.append(Proof(a, b, c, [coms[i]]))
    pub = [entry_chal, tr_chal, job.root]
    vks = [classes[job.class_of(i)][1].vk for i in range(n)]
    assert agg.verify_subcircuit_proofs(ctx, vks, proofs, pub) == []
    assert agg.verify_subcircuit_proofs(ctx, vks, proofs, pub, batch_rng=random.Random(8)) == []
    bad = list(proofs)
    bad[5] = Proof(proofs[5].a, proofs[5].b, proofs[5].c, [coms[4]])
    assert agg.verify_subcircuit_proofs(ctx, vks, bad, pub) == [5]
    for _c, _pk, dpk in classes.values():
        dpk.free()
