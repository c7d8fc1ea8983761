"""GPU: a proving key that holds its H query in the coset's evaluation basis (csrc/h_basis.cuh: four transforms per proof, no
C pass) proves byte for byte what the same key material gives in the coefficient basis (HK_H_BASIS=coeff at upload).  The
identity behind it is linear in the key's points and holds for every assignment, so the keys here are arbitrary curve points
and the assignments satisfy the system or not; one trapdoor key per curve also passes the verifier equation."""
import random
import zlib

import numpy as np
import pytest

from hekaton_system_amd.cp_groth16 import (CURVE_PARAMS, FrCodec, SeededRng, csr_from_rows, generate_parameters,
                                           trapdoor_verify)
from hekaton_system_amd.workload import make_config

pytestmark = pytest.mark.gpu


def _points(ctx, fc, cname, group, rnd, n):
    """n arbitrary points of the group: random multiples of its generator (packed affine bytes)."""
    P = CURVE_PARAMS[cname]
    base = fc.g1(P["g1"]) if group == 1 else fc.g2(P["g2"])
    if n == 0:
        return np.zeros(0, np.uint8)
    return ctx.fixed_base(group, base, fc.enc([rnd.randrange(1, P["r"]) for _ in range(n)]))


def _system(rnd, r, n_inst, stages, n_c, dense_c_col=None, zero_c=False, c_only_var=None):
    """Random sparse rows [(coeff, col)] of A, B, C over n_v = n_inst + sum(stages) variables, and an assignment that
    satisfies them when every C row is its own product variable (the last n_c variables) - else just a random one."""
    n_v = n_inst + sum(stages)
    small = [1, r - 1, 2, r - 3]
    coeff = lambda: rnd.choice(small) if rnd.random() < 0.5 else rnd.randrange(1, r)
    free = max(1, n_v - n_c)                               # A and B read the variables in front of the product variables
    row = lambda: [(coeff(), rnd.randrange(free)) for _ in range(rnd.randrange(0, 4))]
    A = [row() for _ in range(n_c)]
    B = [row() for _ in range(n_c)]
    z = [1] + [rnd.randrange(r) for _ in range(n_v - 1)]
    ev = lambda rw: sum(c * z[j] for c, j in rw) % r
    C = []
    for i in range(n_c):
        if zero_c:
            C.append([])
            continue
        k = n_v - n_c + i
        if k >= free and k >= n_inst:                       # the row's own product variable
            C.append([(1, k)])
            z[k] = ev(A[i]) * ev(B[i]) % r
        else:
            C.append([(coeff(), rnd.randrange(n_v))])
    if dense_c_col is not None:                             # one variable in every row of C (the "one" variable's role)
        for rw in C:
            rw.append((coeff(), dense_c_col))
    if c_only_var is not None:                              # a variable that A and B never read
        A = [[(c, j) for c, j in rw if j != c_only_var] for rw in A]
        B = [[(c, j) for c, j in rw if j != c_only_var] for rw in B]
        C[0].append((coeff(), c_only_var))
    return A, B, C, z


def _key_material(ctx, fc, cname, rnd, n_inst, stages, n_c, h_inf=()):
    n_v = n_inst + sum(stages)
    m = 1
    while m < n_c + n_inst:
        m *= 2
    g1b = ctx.g1_bytes
    h_g = _points(ctx, fc, cname, 1, rnd, m - 1)
    for i in h_inf:
        if i < m - 1:
            h_g[i * g1b:(i + 1) * g1b] = 0
    return dict(a_g=_points(ctx, fc, cname, 1, rnd, n_v), b_g=_points(ctx, fc, cname, 1, rnd, n_v),
                b_h=_points(ctx, fc, cname, 2, rnd, n_v), h_g=h_g,
                ck_stages=[_points(ctx, fc, cname, 1, rnd, n) for n in stages],
                deltas_g=_points(ctx, fc, cname, 1, rnd, len(stages)), last_delta_h=_points(ctx, fc, cname, 2, rnd, 1),
                alpha_g=_points(ctx, fc, cname, 1, rnd, 1), beta_g=_points(ctx, fc, cname, 1, rnd, 1),
                beta_h=_points(ctx, fc, cname, 2, rnd, 1)), m


def _upload_both(ctx, monkeypatch, heavy=None, **kw):
    """The same key material in the coefficient basis and in the evaluation basis."""
    monkeypatch.setenv("HK_H_BASIS", "coeff")
    coeff = ctx.pk_upload(**kw)
    monkeypatch.delenv("HK_H_BASIS")
    if heavy is not None:
        monkeypatch.setenv("HK_H_BASIS_HEAVY_COL", str(heavy))
    ev = ctx.pk_upload(**kw)
    monkeypatch.delenv("HK_H_BASIS_HEAVY_COL", raising=False)
    return coeff, ev


def _same_proofs(ctx, fc, rnd, r, coeff, ev, zs, n_v, n_kappas):
    """hk_prove row by row and hk_prove_batch over all rows: A, B and C byte for byte between the two forms."""
    k = len(zs)
    rs = fc.enc([rnd.randrange(r) for _ in range(k)])
    ss = fc.enc([rnd.randrange(r) for _ in range(k)])
    kap = fc.enc([rnd.randrange(r) for _ in range(k * n_kappas)])
    fr = ctx.fr_bytes
    zb = np.ascontiguousarray(np.concatenate([fc.enc(z) for z in zs]))
    for j in range(k):
        args = (zb[j * n_v * fr:(j + 1) * n_v * fr], rs[j * fr:(j + 1) * fr], ss[j * fr:(j + 1) * fr],
                kap[j * n_kappas * fr:(j + 1) * n_kappas * fr])
        want = coeff.prove(*args, n_v=n_v)
        got = ev.prove(*args, n_v=n_v)
        for name, g, w in zip("ABC", got, want):
            assert g.tobytes() == w.tobytes(), (name, j)
    want = coeff.prove_batch(zb, rs, ss, kap, n_v, k)
    got = ev.prove_batch(zb, rs, ss, kap, n_v, k)
    for name, g, w in zip("ABC", got, want):
        assert g.tobytes() == w.tobytes(), ("batch", name)
    return want


# n_inst, stage lengths, n_c, and what is special about the case.  m = 2, 8, 64 (n_c + n_inst a power of two), 1024.
CASES = {
    "m2": dict(n_inst=1, stages=[2, 3], n_c=1),
    "m8": dict(n_inst=2, stages=[3, 9], n_c=5),
    "m8_single_stage_one_instance": dict(n_inst=1, stages=[9], n_c=6),                 # N_INST = 1, no earlier stage
    "m64_exact_power_of_two": dict(n_inst=4, stages=[5, 70], n_c=60),
    "m64_two_earlier_stages": dict(n_inst=3, stages=[4, 6, 64], n_c=50),
    "m64_h_infinities": dict(n_inst=2, stages=[3, 70], n_c=55, h_inf=(0, 1, 17, 40, 62)),
    "m64_zero_c": dict(n_inst=2, stages=[3, 70], n_c=55, zero_c=True),
    "m64_dense_c_column_both_paths": dict(n_inst=2, stages=[3, 70], n_c=55, dense_c_col=0, heavy=4),
    "m64_dense_witness_column": dict(n_inst=2, stages=[3, 70], n_c=55, dense_c_col=30, heavy=4),
    "m64_variable_only_in_c": dict(n_inst=2, stages=[3, 70], n_c=55, c_only_var=4),
    "m1024": dict(n_inst=3, stages=[16, 1100], n_c=1000, dense_c_col=0),
}


def _run_case(ctx, cname, spec, monkeypatch, seed):
    fc = FrCodec(cname)
    r = CURVE_PARAMS[cname]["r"]
    rnd = random.Random(seed)
    n_inst, stages, n_c = spec["n_inst"], spec["stages"], spec["n_c"]
    n_v = n_inst + sum(stages)
    A, B, C, z = _system(rnd, r, n_inst, stages, n_c, dense_c_col=spec.get("dense_c_col"), zero_c=spec.get("zero_c", False),
                         c_only_var=spec.get("c_only_var"))
    cols = {j for rw in C for _c, j in rw}
    assert len(cols) < n_v                                   # some columns of C are empty in every case
    if spec.get("c_only_var") is not None:
        assert all(j != spec["c_only_var"] for M in (A, B) for rw in M for _c, j in rw)
    mat, m = _key_material(ctx, fc, cname, rnd, n_inst, stages, n_c, h_inf=spec.get("h_inf", ()))
    coeff, ev = _upload_both(ctx, monkeypatch, heavy=spec.get("heavy"), matrices=tuple(csr_from_rows(fc, M) for M in (A, B, C)),
                             n_inst=n_inst, n_constraints=n_c, **mat)
    try:
        bad = list(z)
        bad[n_v - 1] = (bad[n_v - 1] + 1) % r               # an assignment that does not satisfy the system
        bad[1 % n_v] = (bad[1 % n_v] + 5) % r if n_v > 1 else bad[0]
        other = [1] + [rnd.randrange(r) for _ in range(n_v - 1)]
        _same_proofs(ctx, fc, rnd, r, coeff, ev, [z, bad, other], n_v, len(stages) - 1)
    finally:
        coeff.free()
        ev.free()


@pytest.mark.parametrize("case", sorted(CASES))
def test_both_forms_prove_the_same_bytes_bn254(case, ctx_bn254, monkeypatch):
    _run_case(ctx_bn254, "bn254", CASES[case], monkeypatch, seed=zlib.crc32(case.encode()))


def test_both_forms_prove_the_same_bytes_bls12_381(ctx_bls, monkeypatch):
    _run_case(ctx_bls, "bls12_381", CASES["m64_dense_c_column_both_paths"], monkeypatch, seed=381)


@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_trapdoor_key_evaluation_basis_proof_verifies(cname, ctx_bn254, ctx_bls, monkeypatch):
    """A real key of the tiny big-merkle class: the evaluation-basis proof equals the coefficient-basis one and satisfies
    the verifier equation in its trapdoor form, with h from hk_witness_map (which is unchanged)."""
    ctx = ctx_bn254 if cname == "bn254" else ctx_bls
    fc = FrCodec(cname)
    circ = make_config(cname, "tiny")
    pk, td = generate_parameters(circ, cname, SeededRng(b"H-BASIS-TRAPDOOR-KEY-0123456789A"), ctx)
    kw = dict(a_g=pk.a_g, b_g=pk.b_g, b_h=pk.b_h, h_g=pk.h_g, ck_stages=pk.ck.deltas_abc_g, deltas_g=pk.deltas_g,
              last_delta_h=pk.vk.last_delta_h, alpha_g=pk.vk.alpha_g, beta_g=pk.beta_g, beta_h=pk.vk.beta_h,
              matrices=pk.matrices, n_inst=pk.n_inst, n_constraints=pk.n_constraints)
    coeff, ev = _upload_both(ctx, monkeypatch, heavy=8, **kw)
    try:
        circ.set_witness_seed(77)
        z = circ.full_assignment_bytes()
        z_ints = circ.assignment_ints()
        r_, s_, kappa = 0x1234567, 0x7654321, 0x55AA55
        args = (z, fc.enc1(r_), fc.enc1(s_), fc.enc1(kappa))
        want = coeff.prove(*args, n_v=circ.n_v)
        got = ev.prove(*args, n_v=circ.n_v)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        com = ev.commit(0, circ.stage0_witness_bytes(), fc.enc1(kappa))
        assert com.tobytes() == coeff.commit(0, circ.stage0_witness_bytes(), fc.enc1(kappa)).tobytes()
        A, B, C = pk.matrices
        h_b, _m = ctx.witness_map(A, B, C, circ.N_INST, circ.n_c, z, n_v=circ.n_v)
        trapdoor_verify(ctx, cname, td, circ.N_INST, td.stage_ranges, z_ints, fc.dec(h_b), [com], [kappa], r_, s_, got)
    finally:
        coeff.free()
        ev.free()
