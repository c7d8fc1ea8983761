"""GPU: device key generation (hk_qap_eval, hk_keygen, cp_groth16.generate_parameters_device) against the golden keys, the
host setup path, a hand-built uneven CSR, a full-size class, the resident proving chain and every refusal."""
import ctypes as C

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import (CURVE_PARAMS, CommitmentBuilder, FrCodec, Proof, SeededRng,
                                           generate_parameters, generate_parameters_device, prepare_verifying_key,
                                           qap_instance_map_with_evaluation, setup_device, setup_host, verify_proof)
from hekaton_system_amd.workload import make_config
from tests import golden_util as gu

pytestmark = pytest.mark.gpu


def _ctx(name, ctx_bn254, ctx_bls):
    return ctx_bn254 if name == "bn254" else ctx_bls


def _bytes(x):
    if isinstance(x, capi.DeviceBuffer):
        return x.to_host().tobytes()
    return np.asarray(x, dtype=np.uint8).tobytes()


def _rows(fc, M):
    rp, col, val = M
    vals = fc.dec(val)
    return [[(vals[k], int(col[k])) for k in range(int(rp[i]), int(rp[i + 1]))] for i in range(len(rp) - 1)]


def _case_keygen(ctx, case, **over):
    td = case["trapdoor"]
    n_v = len(case["z_mont"]) // 2 // ctx.fr_bytes
    kw = dict(matrices=(gu.csr(case["A"]), gu.csr(case["B"]), gu.csr(case["C"])), n_inst=case["n_inst"],
              n_constraints=case["n_constraints"], n_v=n_v, stage_ranges=[tuple(x) for x in case["stage_ranges"]],
              alpha=td["alpha"], beta=td["beta"], gamma=td["gamma"], deltas=list(td["deltas"]), t=td["t"],
              g1_scalar=td["g1_scalar"], g2_scalar=td["g2_scalar"])
    kw.update(over)
    return ctx.keygen(**kw)


@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_keygen_reproduces_golden_keys(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    fc = FrCodec(cname)
    g2 = ctx.g2_bytes
    for case in gu.load("groth16.json")[cname]:
        pk = case["pk"]
        res = _case_keygen(ctx, case, with_qap=True)
        for key in ("a_g", "b_g", "b_h", "h_g", "deltas_g", "alpha_g", "beta_g", "beta_h", "gamma_h", "gamma_abc_g",
                    "deltas_h"):
            assert _bytes(res[key]).hex() == pk[key], (cname, case["label"], key)
        assert [_bytes(c).hex() for c in res["ck"]] == pk["ck"], (cname, case["label"])
        assert _bytes(res["deltas_h"])[-g2:].hex() == pk["last_delta_h"]
        # hk_qap_eval == the host's instance_map_with_evaluation on the same matrices
        A, B, Cm = (_rows(fc, gu.csr(case[k])) for k in "ABC")
        n_v = len(case["z_mont"]) // 2 // fc.nb
        n_inst, n_c, t = case["n_inst"], case["n_constraints"], case["trapdoor"]["t"]
        a, b, c, zt, m = qap_instance_map_with_evaluation(cname, A, B, Cm, n_inst, n_v - n_inst, n_c, t)
        ga, gb, gc, gzt, gm = ctx.qap_eval(gu.csr(case["A"]), gu.csr(case["B"]), gu.csr(case["C"]), n_inst, n_c, n_v, t)
        assert (fc.dec(ga), fc.dec(gb), fc.dec(gc), fc.dec(gzt)[0], gm) == (a, b, c, zt, m), (cname, case["label"])
        assert fc.dec(res["qap_abc"]) == a + b + c
        assert res["m"] == m


def _same_key(pk1, pk2):
    for key in ("a_g", "b_g", "b_h", "h_g", "beta_g", "deltas_g"):
        assert _bytes(getattr(pk1, key)) == _bytes(getattr(pk2, key)), key
    for key in ("alpha_g", "beta_h", "gamma_h", "last_delta_h", "gamma_abc_g", "deltas_h"):
        assert _bytes(getattr(pk1.vk, key)) == _bytes(getattr(pk2.vk, key)), key
    assert [_bytes(c) for c in pk1.ck.deltas_abc_g] == [_bytes(c) for c in pk2.ck.deltas_abc_g]
    assert _bytes(pk1.ck.last_delta_g) == _bytes(pk2.ck.last_delta_g)
    assert (pk1.n_inst, pk1.n_constraints) == (pk2.n_inst, pk2.n_constraints)


@pytest.mark.parametrize("cname,config,rep,resident", [
    ("bn254", "tiny", None, False), ("bn254", "tiny", None, True), ("bls12_381", "tiny", None, False),
    ("bls12_381", "tiny", None, True), ("bn254", "big-merkle-4x1", None, True),
    ("bn254", "big-merkle-sha-8x1", 1, False), ("bn254", "big-merkle-sha-8x1", 5, True)])
def test_device_setup_equals_host_setup(cname, config, rep, resident, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    seed = b"KEYGEN-SAME-KEY-0123456789abcdef"
    pk_h, td_h = generate_parameters(make_config(cname, config, rep), cname, SeededRng(seed), ctx)
    pk_d, td_d = generate_parameters_device(make_config(cname, config, rep), cname, SeededRng(seed), ctx,
                                            keep_on_device=resident, with_qap=True)
    _same_key(pk_h, pk_d)
    ints = lambda xs: [int(x) for x in xs]
    assert [ints(x) for x in (td_d.a, td_d.b, td_d.c)] == [ints(x) for x in (td_h.a, td_h.b, td_h.c)]
    assert (td_d.zt, td_d.m) == (int(td_h.zt), td_h.m)
    assert all(isinstance(getattr(pk_d, k), capi.DeviceBuffer) == resident for k in ("a_g", "b_g", "b_h", "h_g"))


def test_uneven_matrices(ctx_bn254):
    """One column in every row, a 4096-entry row, empty rows and columns, duplicates, zero coefficients, n_inst > 1."""
    ctx, cname = ctx_bn254, "bn254"
    fc = FrCodec(cname)
    r = CURVE_PARAMS[cname]["r"]
    n_c, n_inst, n_v = (1 << 18) + 3, 5, 9000
    rng = np.random.default_rng(7)
    empty_cols = {17, 4000, n_v - 1}

    def matrix(seed_col):
        rows = []
        for i in range(n_c):
            if i % 97 == 5:
                rows.append([])                                              # empty row
                continue
            row = [(1 if i % 3 else (i * 7919) % r, seed_col)]               # the heavy column
            if i == 1234:
                row += [(int(v), int(cc)) for v, cc in zip(rng.integers(0, 1 << 62, 4096), rng.integers(0, n_v, 4096))
                        if int(cc) not in empty_cols]
            else:
                cc = int(rng.integers(0, n_v))
                if cc not in empty_cols:
                    row += [(int(rng.integers(0, 1 << 62)), cc), (0, cc)]   # a zero coefficient
                    if i % 5 == 0:
                        row.append((i + 1, cc))                              # duplicate (row, col)
            rows.append(row)
        return rows
    A, B, Cm = matrix(0), matrix(2), matrix(n_inst + 3)
    csr = lambda rows: (np.array([0] + list(np.cumsum([len(x) for x in rows])), dtype=np.uint64),
                        np.array([j for x in rows for _, j in x], dtype=np.uint32), fc.enc([v for x in rows for v, _ in x]))
    t = 0x1234567890abcdef1234567890abcdef % r
    want = qap_instance_map_with_evaluation(cname, A, B, Cm, n_inst, n_v - n_inst, n_c, t)
    ga, gb, gc, gzt, gm = ctx.qap_eval(csr(A), csr(B), csr(Cm), n_inst, n_c, n_v, t)
    assert (fc.dec(ga), fc.dec(gb), fc.dec(gc), fc.dec(gzt)[0], gm) == want
    assert want[0][17] == 0 and want[1][4000] == 0


def test_full_size_class_proves_and_verifies(ctx_bn254):
    """big-merkle-64x32 (m = 2^21): the device key equals the host path's; a proof under it passes hk_verify_batch and
    the Groth16 equation holds in the exponent under the trapdoor."""
    ctx, cname = ctx_bn254, "bn254"
    fc = FrCodec(cname)
    r = CURVE_PARAMS[cname]["r"]
    seed = b"KEYGEN-FULL-SIZE-0123456789abcde"
    pk, td = generate_parameters_device(make_config(cname, "big-merkle-64x32"), cname, SeededRng(seed), ctx,
                                        with_qap=True)
    assert td.m == 1 << 21
    pk_h, td_h = setup_device(setup_host(make_config(cname, "big-merkle-64x32"), cname, SeededRng(seed)), ctx)
    _same_key(pk, pk_h)
    assert [list(map(int, x)) for x in (td.a, td.b, td.c)] == [list(map(int, x)) for x in (td_h.a, td_h.b, td_h.c)]
    del pk_h, td_h

    circ = make_config(cname, "big-merkle-64x32")
    circ.set_witness_seed(4242)
    pk.upload(ctx)
    cb = CommitmentBuilder.new(circ, pk)
    com, kappa = cb.commit(SeededRng(b"KEYGEN-COMMIT-0123456789abcdef!!"))
    rr = SeededRng(b"KEYGEN-PROVE-0123456789abcdef!!!")
    proof = cb.prove([com], [kappa], rr)
    z = circ.assignment_ints()
    n_inst = circ.N_INST
    assert verify_proof(prepare_verifying_key(ctx, pk.vk), proof, z[1:n_inst])

    # the verifier's equation in the exponent: log A log B = alpha beta + ic gamma + log D delta_0 + log C delta_1
    rr2 = SeededRng(b"KEYGEN-PROVE-0123456789abcdef!!!")
    r_, s_ = rr2.fr(r), rr2.fr(r)
    inv = lambda x: pow(x, -1, r)
    d0, dl = td.deltas
    abc = [(td.beta * a + td.alpha * b + c) % r for a, b, c in zip(td.a, td.b, td.c)]
    (s0, e0), _ = td.stage_ranges
    log_a = (td.alpha + sum(x * y for x, y in zip(z, td.a)) + r_ * dl) % r
    log_b = (td.beta + sum(x * y for x, y in zip(z, td.b)) + s_ * dl) % r
    ic = sum(z[i] * abc[i] for i in range(n_inst)) * inv(td.gamma) % r
    log_d = (sum(z[i] * abc[i] for i in range(n_inst + s0, n_inst + e0)) * inv(d0) + kappa * dl) % r
    log_c = (log_a * log_b - td.alpha * td.beta - ic * td.gamma - log_d * d0) * inv(dl) % r
    G1, G2 = fc.g1(CURVE_PARAMS[cname]["g1"]), fc.g2(CURVE_PARAMS[cname]["g2"])
    want1 = np.asarray(ctx.fixed_base(1, G1, fc.enc([x * td.g1_scalar % r for x in (log_a, log_c, log_d)])))
    want2 = np.asarray(ctx.fixed_base(2, G2, fc.enc([log_b * td.g2_scalar % r])))
    g1 = ctx.g1_bytes
    assert _bytes(proof.a) == want1[:g1].tobytes()
    assert _bytes(proof.c) == want1[g1:2 * g1].tobytes()
    assert _bytes(com) == want1[2 * g1:].tobytes()
    assert _bytes(proof.b) == want2.tobytes()
    pk.device.free()


@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_resident_key_proves_like_host_key(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    fc = FrCodec(cname)
    seed = b"KEYGEN-RESIDENT-0123456789abcdef"
    circ = make_config(cname, "tiny")
    pk_h, _ = generate_parameters(circ, cname, SeededRng(seed), ctx)
    pk_d, _ = generate_parameters_device(make_config(cname, "tiny"), cname, SeededRng(seed), ctx, keep_on_device=True)
    assert isinstance(pk_d.a_g, capi.DeviceBuffer) and isinstance(pk_d.h_g, capi.DeviceBuffer)
    circ.set_witness_seed(77)
    z = circ.full_assignment_bytes()
    args = (z, fc.enc1(0x1111), fc.enc1(0x2222), fc.enc([0x3333]))
    got = [pk.upload(ctx).prove(*args) for pk in (pk_h, pk_d)]
    assert [_bytes(x) for x in got[0]] == [_bytes(x) for x in got[1]]
    for pk in (pk_h, pk_d):
        pk.device.free()


def _status(fn):
    try:
        fn()
    except capi.HekatonError as e:
        return e.status
    return capi.HK_OK


def test_keygen_refusals_leave_the_context_usable(ctx_bn254):
    ctx, cname = ctx_bn254, "bn254"
    p = CURVE_PARAMS[cname]
    r = p["r"]
    case = gu.load("groth16.json")[cname][0]
    n_inst, n_c = case["n_inst"], case["n_constraints"]
    m = 1
    while m < n_c + n_inst:
        m *= 2
    omega = pow(pow(p["gen"], (r - 1) >> p["two_adicity"], r), (1 << p["two_adicity"]) // m, r)
    good = lambda: _case_keygen(ctx, case)
    want_a_g = case["pk"]["a_g"]
    A = gu.csr(case["A"])
    bad_col = (A[0], A[1].copy(), A[2])
    bad_col[1][3] = 1 << 20
    n_v = len(case["z_mont"]) // 2 // ctx.fr_bytes
    gap = [tuple(x) for x in case["stage_ranges"]]
    gap[1] = (gap[1][0] + 1, gap[1][1])
    refusals = [
        (capi.HK_ERR_ARG, dict(t=1)),
        (capi.HK_ERR_ARG, dict(t=omega)),
        (capi.HK_ERR_ARG, dict(deltas=[case["trapdoor"]["deltas"][0], 0])),
        (capi.HK_ERR_ARG, dict(gamma=0)),
        (capi.HK_ERR_ARG, dict(stage_ranges=gap)),
        (capi.HK_ERR_ARG, dict(matrices=(bad_col, gu.csr(case["B"]), gu.csr(case["C"])))),
        (capi.HK_ERR_ARG, dict(n_constraints=n_c + 1)),
    ]
    for want, over in refusals:
        assert _status(lambda: _case_keygen(ctx, case, **over)) == want, over
        assert _bytes(good()["a_g"]).hex() == want_a_g, over
    # hk_qap_eval refuses t in the domain too
    assert _status(lambda: ctx.qap_eval(A, gu.csr(case["B"]), gu.csr(case["C"]), n_inst, n_c, n_v, omega)) == capi.HK_ERR_ARG
    # the domain check comes from the sizes alone: NULL arrays and a row count that matches nothing are not looked at
    null = capi.hk_csr(None, None, None, 3, 5)
    d = capi.hk_keygen_desc(C.pointer(null), C.pointer(null), C.pointer(null), n_inst, (1 << p["two_adicity"]) + 1, n_v,
                            None, 0, None, None, None, None, None, None, None)
    o = capi.hk_keygen_out()
    assert ctx.lib.hk_keygen(ctx.handle, C.byref(d), C.byref(o), None) == capi.HK_ERR_DOMAIN_TOO_LARGE
    assert ctx.lib.hk_qap_eval(ctx.handle, C.byref(null), C.byref(null), C.byref(null), n_inst, (1 << p["two_adicity"]) + 1,
                               n_v, None, None, None, None, None, None) == capi.HK_ERR_DOMAIN_TOO_LARGE
    # no point output is written when the device finds a bad column
    out = np.full(n_v * ctx.g1_bytes, 0xAB, dtype=np.uint8)
    keep = []
    csrs = capi.Context._csrs((bad_col, gu.csr(case["B"]), gu.csr(case["C"])), keep)
    fc = FrCodec(cname)
    td = case["trapdoor"]
    sc = [fc.enc1(td[k]) for k in ("alpha", "beta", "gamma", "t", "g1_scalar", "g2_scalar")]
    dl = np.concatenate([fc.enc1(x) for x in td["deltas"]])
    sr = np.array([v for be in case["stage_ranges"] for v in be], dtype=np.uint64)
    d = capi.hk_keygen_desc(C.pointer(csrs[0]), C.pointer(csrs[1]), C.pointer(csrs[2]), n_inst, n_c, n_v, sr.ctypes.data,
                            len(case["stage_ranges"]), *[x.ctypes.data for x in sc], dl.ctypes.data)
    bufs = {k: np.full(1 << 14, 0xAB, dtype=np.uint8) for k in ("b_g", "b_h", "h_g", "deltas_g", "alpha_g", "beta_g",
                                                              "gamma_abc_g", "beta_h", "gamma_h", "deltas_h", "ck0", "ck1")}
    ck = (C.c_void_p * 2)(bufs["ck0"].ctypes.data, bufs["ck1"].ctypes.data)
    o = capi.hk_keygen_out(out.ctypes.data, bufs["b_g"].ctypes.data, bufs["b_h"].ctypes.data, bufs["h_g"].ctypes.data, ck,
                           *[bufs[k].ctypes.data for k in ("deltas_g", "alpha_g", "beta_g", "gamma_abc_g", "beta_h", "gamma_h",
                                                           "deltas_h")], None)
    assert ctx.lib.hk_keygen(ctx.handle, C.byref(d), C.byref(o), None) == capi.HK_ERR_ARG
    assert (out == 0xAB).all() and all((b == 0xAB).all() for b in bufs.values())
    assert _bytes(good()["a_g"]).hex() == want_a_g
