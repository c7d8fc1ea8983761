"""GPU parity at realistic sizes: the HIP path against the multi-threaded C++ oracle (bit-exact) and,
at BASELINE.json's full size, against size-independent checks: every proof must satisfy the Groth16
equation in the exponent under the SRS trapdoor (the pairing-free form of verifier.rs:23-43), and
h * Z == a*b - c at a random point."""
import random
import time

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import (FrCodec, SeededRng, generate_parameters, CommitmentBuilder,
                                           CURVE_PARAMS)
from hekaton_system_amd.workload import make_config, SyntheticSubcircuit
from oracle.c_oracle import COracle
from oracle.pyref import curve as ocurve
from oracle.pyref.codec import Codec
from oracle.pyref.params import CURVES

pytestmark = pytest.mark.gpu


def _trapdoor_check(cname, circ, td, z, h, comms, kappas, r_, s_, proof):
    """Recomputes log(A), log(B), log(C), log(D_i) in Fr from the toxic waste and compares group
    elements; also checks the verifier equation in the exponent."""
    cp = CURVES[cname]
    cd = Codec(cp)
    G1, G2 = ocurve.G1(cp), ocurve.G2(cp)
    mod = cp.r
    inv = lambda x: pow(x, -1, mod)
    ni, n0 = circ.N_INST, circ.n0
    dl = td.deltas[-1]
    az = sum(x * y for x, y in zip(z, td.a)) % mod
    bz = sum(x * y for x, y in zip(z, td.b)) % mod
    abc = [(td.beta * a + td.alpha * b + c) % mod for a, b, c in zip(td.a, td.b, td.c)]
    log_a = (r_ * dl + az + td.alpha) % mod
    log_b = (s_ * dl + bz + td.beta) % mod
    l_log = sum(z[i] * abc[i] for i in range(ni + n0, len(z))) % mod * inv(dl) % mod
    hsum, tp = 0, 1
    for i in range(td.m - 1):
        hsum += h[i] * tp
        tp = tp * td.t % mod
    h_log = hsum % mod * td.zt % mod * inv(dl) % mod
    log_c = (s_ * log_a + r_ * log_b - r_ * s_ % mod * dl + l_log + h_log) % mod
    d_logs = []
    for k, kappa in enumerate(kappas):
        d = sum(z[i] * abc[i] for i in range(ni, ni + n0)) % mod * inv(td.deltas[k]) % mod
        d_logs.append((d + kappa * dl) % mod)
        log_c = (log_c - kappa * td.deltas[k]) % mod
    g = G1.mul(G1.gen, td.g1_scalar)
    hh = G2.mul(G2.gen, td.g2_scalar)
    assert cd.g1_from(proof[0]) == G1.mul(g, log_a), "A"
    assert cd.g2_from(proof[1]) == G2.mul(hh, log_b), "B"
    assert cd.g1_from(proof[2]) == G1.mul(g, log_c), "C"
    for com, d in zip(comms, d_logs):
        assert cd.g1_from(com) == G1.mul(g, d), "D"
    ic = sum(z[i] * abc[i] for i in range(ni)) % mod * inv(td.gamma) % mod
    lhs = log_a * log_b % mod
    rhs = (td.alpha * td.beta + ic * td.gamma + sum(d * dk for d, dk in zip(d_logs, td.deltas)) + log_c * dl) % mod
    assert lhs == rhs, "Groth16 equation"


def _run_config(ctx, cname, name, check_oracle_prove, check_oracle_commit=False, class_rep=None):
    fc = FrCodec(cname)
    circ = make_config(cname, name, class_rep)
    t0 = time.time()
    pk, td = generate_parameters(circ, cname, SeededRng(b"HEKATON1" * 4), ctx)
    dpk = pk.upload(ctx)
    print("setup %.1fs" % (time.time() - t0))
    circ.set_witness_seed(77)
    z_ints = circ.assignment_ints()
    zb = circ.full_assignment_bytes()
    w0 = circ.stage0_witness_bytes()
    kappa, r_, s_ = 0x1111, 0x2222_3333_4444, 0x5555_6666
    com = dpk.commit(0, w0, fc.enc1(kappa))
    zdev = capi.DeviceBuffer.from_host(ctx, zb)
    a, b, c = dpk.prove(zdev, fc.enc1(r_), fc.enc1(s_), fc.enc([kappa]), n_v=circ.n_v)
    # independent quotient polynomial from the CPU oracle, and the GPU witness map against it bit for bit
    co = COracle(cname)
    A, B, C = pk.matrices
    h_o, m = co.witness_map(A, B, C, circ.N_INST, circ.n_c, zb)
    h_g, m2 = ctx.witness_map(A, B, C, circ.N_INST, circ.n_c, zdev, n_v=circ.n_v)
    assert m == m2 and np.array_equal(h_o, h_g)
    h = fc.dec(h_o)
    assert h[-1] == 0
    _trapdoor_check(cname, circ, td, z_ints, h, [com], [kappa], r_, s_, (a, b, c))
    if check_oracle_prove or check_oracle_commit:
        view = co.pk_view(a_g=pk.a_g, b_g=pk.b_g, b_h=pk.b_h, h_g=pk.h_g, ck_stages=pk.ck.deltas_abc_g,
                          deltas_g=pk.deltas_g, last_delta_h=pk.vk.last_delta_h, alpha_g=pk.vk.alpha_g,
                          beta_g=pk.beta_g, beta_h=pk.vk.beta_h)
        assert np.array_equal(co.commit(view, 0, w0, fc.enc1(kappa)), com)
    if check_oracle_prove:
        oa, ob, oc = co.prove(view, A, B, C, circ.N_INST, circ.n_c, zb, fc.enc1(r_), fc.enc1(s_), fc.enc([kappa]))
        assert np.array_equal(oa, a) and np.array_equal(ob, b) and np.array_equal(oc, c)
    zdev.free(); dpk.free()


def test_config0_big_merkle_4x1_bit_exact_vs_cpu_oracle(ctx_bn254):
    """BASELINE configs[0] shape (m = 2^16): commit + prove bit-exact vs the C++ oracle, and valid."""
    _run_config(ctx_bn254, "bn254", "big-merkle-4x1", check_oracle_prove=True)


def test_config1_big_merkle_64x32_full_size_properties(ctx_bn254):
    """BASELINE configs[1] shape (m = 2^21, n_v ~ 1.3e6): proof valid under the trapdoor, witness map
    bit-exact vs the CPU oracle."""
    _run_config(ctx_bn254, "bn254", "big-merkle-64x32", check_oracle_prove=False)


def test_config2_big_merkle_512x64_full_size_properties(ctx_bn254):
    """BASELINE configs[2] shape (m = 2^22, n_v ~ 2.6e6; one GPU's share of the 8-GPU job proves exactly this
    subcircuit shape): witness map bit-exact vs the CPU oracle, commit + proof valid under the trapdoor."""
    _run_config(ctx_bn254, "bn254", "big-merkle-512x64", check_oracle_prove=False)


def test_config3_vkd_256_bit_exact_vs_cpu_oracle(ctx_bn254):
    """BASELINE configs[3] (vkd, 256 subcircuits, 7 proving-key classes).  The per-subcircuit size is the flagged
    placeholder of SURVEY.md §8 (m = 2^17, n0 = 8 192 portal witnesses): commit (an 8 192-term MSM) and proof
    bit-exact vs the C++ oracle and valid under the trapdoor, on the most common class ("compute path", 8)."""
    _run_config(ctx_bn254, "bn254", "vkd-256", check_oracle_prove=True, class_rep=8)


def test_config4_vm_1024x1024_commit_bit_exact_and_proof_valid(ctx_bn254):
    """BASELINE configs[4] shape (m = 2^20, n_v ~ 1.7e6, 217 280 stage-0 witnesses): the only config whose
    hk_commit is a large MSM (committer.rs:89) - bit-exact vs `COracle.commit`; witness map bit-exact; proof and
    commitment valid under the trapdoor."""
    _run_config(ctx_bn254, "bn254", "vm-1024x1024", check_oracle_prove=False, check_oracle_commit=True, class_rep=1)


@pytest.mark.parametrize("group,n,dense", [(1, 1 << 16, True), (1, 1 << 16, False), (2, 1 << 13, True),
                                           (1, 100_003, True)])
def test_msm_primitive_large_vs_cpu_oracle(group, n, dense, ctx_bn254):
    """hk_msm_g1/g2 over caller-supplied bases (no shift tables) vs the ark-style Pippenger on the CPU."""
    fc = FrCodec("bn254")
    p = CURVE_PARAMS["bn254"]
    rnd = random.Random(n + group)
    base = fc.g1(p["g1"]) if group == 1 else fc.g2(p["g2"])
    ks = [rnd.randrange(1, p["r"]) for _ in range(n)]
    bases = ctx_bn254.fixed_base(group, base, fc.enc(ks))
    scal = [rnd.randrange(p["r"]) if (dense or rnd.random() < 0.15) else rnd.randrange(2) for _ in range(n)]
    sb = fc.enc(scal)
    got = (ctx_bn254.msm_g1 if group == 1 else ctx_bn254.msm_g2)(bases, sb)
    want = COracle("bn254").msm(group, bases, sb)
    assert np.array_equal(got, want)
    # linearity: every base is k_i * G, so the sum must be (sum s_i k_i) * G
    tot = sum(s * k for s, k in zip(scal, ks)) % p["r"]
    chk = ctx_bn254.fixed_base(group, base, fc.enc([tot]))
    assert np.array_equal(got, chk)


@pytest.mark.parametrize("log_m", [16, 20])
def test_ntt_large_roundtrip_and_oracle(log_m, ctx_bn254):
    fc = FrCodec("bn254")
    rng = np.random.default_rng(log_m)
    m = 1 << log_m
    raw = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
    raw[:, 31] &= 0x0f                                  # < r
    x = raw.ravel().copy()
    dev = capi.DeviceBuffer.from_host(ctx_bn254, x)
    ctx_bn254.ntt(dev, log_m, inverse=False, coset=True)
    fwd = dev.to_host()
    want = COracle("bn254").ntt(x.copy(), log_m, inverse=False, coset=True)
    assert np.array_equal(fwd, want)
    ctx_bn254.ntt(dev, log_m, inverse=True, coset=True)
    assert np.array_equal(dev.to_host(), x)
    dev.free()


def test_concurrent_lanes_match_sequential_and_are_deterministic(ctx_bn254):
    """compute_responses proves from several OS threads (mpi-snark/src/bin/node.rs:745-795): 8 host threads on
    one context must give, for every subcircuit, exactly the bytes a lone sequential call gives — also a
    determinism check (the digit sort uses atomics, the proof must not depend on their order)."""
    from concurrent.futures import ThreadPoolExecutor
    fc = FrCodec("bn254")
    circ = make_config("bn254", "big-merkle-4x1")
    pk, _td = generate_parameters(circ, "bn254", SeededRng(b"HEKATON2" * 4), ctx_bn254)
    dpk = pk.upload(ctx_bn254)
    zs, w0s = [], []
    for k in range(4):
        circ.set_witness_seed(500 + k)
        zs.append(capi.DeviceBuffer.from_host(ctx_bn254, circ.full_assignment_bytes()))
        w0s.append(circ.stage0_witness_bytes())
    r_b, s_b, kap = fc.enc1(3), fc.enc1(5), fc.enc([7])

    def one(i):
        k = i % 4
        com = dpk.commit(0, w0s[k], kap)
        a, b, c = dpk.prove(zs[k], r_b, s_b, kap, n_v=circ.n_v)
        return com.tobytes() + a.tobytes() + b.tobytes() + c.tobytes()

    seq = [one(i) for i in range(4)]
    with ThreadPoolExecutor(max_workers=8) as pool:
        par = list(pool.map(one, range(32)))
    for i, p in enumerate(par):
        assert p == seq[i % 4], i
    assert len(set(seq)) == 4
    for z in zs:
        z.free()
    dpk.free()


def test_config0_bls12_381_bit_exact_vs_cpu_oracle(ctx_bls):
    """Same shape on the curve BASELINE.json's north_star names: BLS12-381 (6-limb Fq)."""
    _run_config(ctx_bls, "bls12_381", "big-merkle-4x1", check_oracle_prove=True)


def test_config1_bls12_381_full_size_properties(ctx_bls):
    """BASELINE configs[1] shape (m = 2^21) on BLS12-381: proof valid under the trapdoor, quotient polynomial
    bit-exact vs the CPU oracle."""
    _run_config(ctx_bls, "bls12_381", "big-merkle-64x32", check_oracle_prove=False)


@pytest.mark.parametrize("kind", ["leaf", "parent", "root", "padding"])
def test_real_sha256_subcircuits_prove_and_verify(kind, ctx_bn254):
    """subcircuits of the re-implemented big-merkle gadget set (hekaton_system_amd/sha_circuit.py:
    real SHA-256 chains, digest <-> field packing, ROM running evaluations; 2 iterations, m = 2^16 / 2^17): the assignment comes
    from the trace generator, commit + prove on the GPU, and the proof passes the trapdoor form of the verifier
    equation with h recomputed by hk_witness_map; the statement proved is a hashlib-checked SHA-256 chain."""
    from hekaton_system_amd.cp_groth16 import trapdoor_verify
    from hekaton_system_amd.sha_circuit import ShaMerkleSubcircuit, example_witness, iterated_sha256, INNER_HASH_SIZE
    cname = "bn254"
    fc = FrCodec(cname)
    circ = ShaMerkleSubcircuit(cname, kind, ns=2, n_portals=4, first=False, last=(kind == "padding"))
    pk, td = generate_parameters(circ, cname, SeededRng(b"SHA-MERKLE-CLASS" * 2), ctx_bn254)
    dpk = pk.upload(ctx_bn254)
    w = example_witness(circ, seed=11)
    _bits, _full, digests = circ.witness_batch([w])
    data = w["leaf"] if kind in ("leaf", "padding") else b"".join(int(w["time"][k][1]).to_bytes(INNER_HASH_SIZE, "little") for k in range(2))
    assert digests[0] == iterated_sha256(data, 2)
    z_ints = circ.assignment_ints(w)[0]
    zb = circ.assignment_bytes(w)[0]
    kappa, r_, s_ = 0xabcdef, 0x1357_9bdf_2468, 0x2222_1111
    w0 = fc.enc(z_ints[circ.N_INST:circ.N_INST + circ.n0])
    com = dpk.commit(0, w0, fc.enc1(kappa))
    a, b, c = dpk.prove(zb, fc.enc1(r_), fc.enc1(s_), fc.enc([kappa]), n_v=circ.n_v)
    A, B, C = pk.matrices
    h_b, m = ctx_bn254.witness_map(A, B, C, circ.N_INST, circ.n_c, zb, n_v=circ.n_v)
    h = fc.dec(h_b)
    assert h[-1] == 0 and m >= circ.n_c + circ.N_INST and m & (m - 1) == 0
    trapdoor_verify(ctx_bn254, cname, td, circ.N_INST, td.stage_ranges, z_ints, h, [com], [kappa], r_, s_, (a, b, c))
    # a wrong digest bit is not provable: the quotient is no longer a polynomial
    bad = list(z_ints)
    bad[-5] = 1 - bad[-5] if bad[-5] in (0, 1) else bad[-5] + 1
    hb, _ = ctx_bn254.witness_map(A, B, C, circ.N_INST, circ.n_c, fc.enc(bad), n_v=circ.n_v)
    assert fc.dec(hb)[-1] != 0
    dpk.free()


def test_assignment_materialised_on_the_device_equals_the_host_bytes(ctx_bn254):
    """hk_assignment_from_bits: one byte per variable + the full-width values over PCIe, Montgomery form in HBM - bit
    for bit what the host-side table lookup (`assignment_bytes`) produces."""
    from hekaton_system_amd.sha_circuit import ShaMerkleSubcircuit, example_witness, packed_assignments
    circ = ShaMerkleSubcircuit("bn254", "parent", ns=1, n_portals=4)
    ws = [example_witness(circ, seed=s, entry_chal=3, tr_chal=4) for s in (1, 2)]
    want = circ.assignment_bytes(ws)
    for k, (bits, cols, vals) in enumerate(packed_assignments(circ, ws)):
        buf = ctx_bn254.assignment_from_bits(bits, cols, vals)
        assert np.array_equal(buf.to_host(), want[k])
        buf.free()
    bad_cols = np.array([circ.n_v], np.uint32)
    with pytest.raises(capi.HekatonError):
        ctx_bn254.assignment_from_bits(np.zeros(circ.n_v, np.uint8), bad_cols, FrCodec("bn254").enc([1]))


@pytest.mark.parametrize("kind,macro", [("leaf", True), ("parent", True), ("parent", False)])
def test_witness_generated_on_the_device_equals_the_host_trace(kind, macro, ctx_bn254, monkeypatch):
    """hk_wprog_upload / hk_wprog_run + hk_poseidon_path (csrc/witness.cuh, csrc/poseidon.cuh): the class's word program interpreted on the
    GPU from the subcircuits' inputs, and the Poseidon membership block computed on the GPU from the execution leaf and
    its path, give bit for bit the assignments the host trace emits (themselves checked against hashlib, poseidon.py and
    the R1CS on the CPU); then a proof from the device-generated assignment verifies."""
    from hekaton_system_amd.cp_groth16 import trapdoor_verify
    from hekaton_system_amd.poseidon import device_params
    from hekaton_system_amd.sha_circuit import (ShaMerkleSubcircuit, example_witness, full_values, poseidon_inputs,
                                                program_inputs)
    cname = "bn254"
    fc = FrCodec(cname)
    if not macro:               # one program entry per gadget (XOR, Ch, Maj, additions) instead of one per round / schedule step
        monkeypatch.setenv("HK_WPROG_NO_MACRO", "1")
    circ = ShaMerkleSubcircuit(cname, kind, ns=2, n_portals=4, depth=5)
    ws = [example_witness(circ, seed=s, entry_chal=31, tr_chal=41) for s in range(5)]
    ops, refs, vmap = circ.tape.word_program(circ.n_v)
    assert bool(np.any(ops[:, 0] >= 8)) == macro
    wp = ctx_bn254.wprog_upload(ops, refs, vmap, circ.tape.n_values, circ.tape.n_inputs)
    cols, vals = full_values(circ, ws)
    zdev = wp.run(program_inputs(circ, ws), cols, vals)
    leaves, sibs, idx = poseidon_inputs(circ, ws)
    ctx_bn254.poseidon_path(device_params(cname, fc), leaves, sibs, idx, circ.n_v, circ.pos_col0, zdev)
    got = zdev.to_host().reshape(len(ws), -1)
    want = circ.assignment_bytes(ws)
    assert np.array_equal(got, want)
    # the same assignments in two steps: the program alone first (what a worker can run before the round's challenges
    # are known), the full-width values afterwards (hk_assignment_scatter)
    z2 = wp.run(program_inputs(circ, ws), [], [])
    wp.scatter(cols, vals, z2)
    ctx_bn254.poseidon_path(device_params(cname, fc), leaves, sibs, idx, circ.n_v, circ.pos_col0, z2)
    assert np.array_equal(z2.to_host().reshape(len(ws), -1), want)
    z2.free()
    if not macro:
        bad = ops.copy()
        bad[int(np.nonzero(bad[:, 0] == 2)[0][0]), 1] = circ.tape.n_values - 1
        with pytest.raises(capi.HekatonError) as e:
            ctx_bn254.wprog_upload(bad, refs, vmap, circ.tape.n_values, circ.tape.n_inputs)
        assert e.value.status == capi.HK_ERR_ARG
        zdev.free()
        return
    # a malformed program (operand reference beyond the values defined so far) is refused, not interpreted
    from hekaton_system_amd.sha_circuit import OP_SHA_ROUND, OP_SHA_SCHED
    for opcode, n_operands in ((OP_SHA_ROUND, 9), (OP_SHA_SCHED, 4)):
        k = int(np.nonzero(ops[:, 0] == opcode)[0][0])                  # the first round / schedule step of the program
        for j in (0, n_operands - 1):
            bad_refs = refs.copy()
            bad_refs[ops[k, 1] + j] = circ.tape.n_values - 1
            with pytest.raises(capi.HekatonError) as e:
                ctx_bn254.wprog_upload(ops, bad_refs, vmap, circ.tape.n_values, circ.tape.n_inputs)
            assert e.value.status == capi.HK_ERR_ARG
    bad = ops.copy()
    bad[int(np.nonzero(ops[:, 0] == OP_SHA_ROUND)[0][-1]), 1] = len(refs) - 3   # operand table runs past the reference array
    with pytest.raises(capi.HekatonError) as e:
        ctx_bn254.wprog_upload(bad, refs, vmap, circ.tape.n_values, circ.tape.n_inputs)
    assert e.value.status == capi.HK_ERR_ARG
    # prove straight from the device-generated assignment of subcircuit 3
    pk, td = generate_parameters(circ, cname, SeededRng(b"WPROG-CLASS-KEY!" * 2), ctx_bn254)
    dpk = pk.upload(ctx_bn254)
    z3 = capi.DeviceBuffer.from_host(ctx_bn254, got[3].copy())
    z_ints = circ.assignment_ints(ws[3])[0]
    kappa, r_, s_ = 5, 6, 7
    com = dpk.commit(0, fc.enc(z_ints[circ.N_INST:circ.N_INST + circ.n0]), fc.enc1(kappa))
    a, b, c = dpk.prove(z3, fc.enc1(r_), fc.enc1(s_), fc.enc([kappa]), n_v=circ.n_v)
    A, B, C = pk.matrices
    h_b, _m = ctx_bn254.witness_map(A, B, C, circ.N_INST, circ.n_c, z3, n_v=circ.n_v)
    trapdoor_verify(ctx_bn254, cname, td, circ.N_INST, td.stage_ranges, z_ints, fc.dec(h_b), [com], [kappa], r_, s_, (a, b, c))
    for x in (zdev, z3):
        x.free()
    wp.free(); dpk.free()
