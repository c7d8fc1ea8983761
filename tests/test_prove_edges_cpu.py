"""The cases of tests/prove_edges.py are what they claim - shown with the reference alone, so that the GPU test
(tests/test_prove_edges_gpu.py) cannot pass vacuously: nothing the directed scalars divide by vanishes, every directed case
meets its own condition in discrete logs with exactly the intended output at infinity, the GLV halves of the named and
directed scalars have the shapes the cases rely on (csrc/endo.cuh's endo_decompose, host-compiled), and the exponent
reference equals the oracle's MSM-based prover and committer point for point."""
import ctypes

import numpy as np
import pytest

from oracle.pyref import groth16
from tests import host_build
from tests import prove_edges as pe
from tests.util import oracle_commit, oracle_prove


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim") / "field_shim.so")
    host_build.build("field_shim.cpp", out, "-O1", *host_build.SHARED)
    lib = host_build.load(out)
    lib.shim_endo_decompose.restype = ctypes.c_uint
    return lib


def _split(lib, cname, c):
    """(k0, k1) signed and the sign mask of the G1 split of c, as k_finish_ab's lanes read them"""
    cl = np.array([(c >> (32 * i)) & 0xffffffff for i in range(8)], np.uint32)
    mag = np.zeros(12, np.uint32)
    neg = lib.shim_endo_decompose(0 if cname == "bn254" else 1, 1, cl.ctypes.data_as(ctypes.c_void_p),
                                  mag.ctypes.data_as(ctypes.c_void_p))
    m = [sum(int(mag[6 * j + l]) << (32 * l) for l in range(6)) for j in range(2)]
    return tuple(-m[j] if (neg >> j) & 1 else m[j] for j in range(2)), neg


@pytest.mark.parametrize("cname", pe.CURVE_NAMES)
def test_nothing_the_cases_divide_by_vanishes(cname):
    su = pe.setup(cname)
    for name, v in pe.denominators(su).items():
        assert v % su.cp.r != 0, name
    assert len(su.cases) <= pe.MAX_PROOFS
    # the circuit: n_v = 40, m = 32, two stages (one kappa), four instance variables - far below the 4096 bases at which A
    # and B would leave the dense lists
    assert (su.n_v, su.td.m, len(su.cs.stage_ranges), su.cs.num_instance) == (40, 32, 2, 4)


@pytest.mark.parametrize("cname", pe.CURVE_NAMES)
def test_every_directed_case_meets_its_condition(cname):
    su = pe.setup(cname)
    mod = su.cp.r
    directed = 0
    for case in su.cases:
        p = su.parts(case)
        la, lb, lc = pe.proof_logs(su.td, su.cs, case["z"], [case["kappa"]], case["r"], case["s"])
        assert (la, lb, lc) == (p["log_a"], p["log_b"], p["log_c"])
        got_inf = {k for k, v in (("a", la), ("b", lb), ("c", lc)) if v == 0}
        if case["cond"] is not None:
            directed += 1
            assert case["cond"](p, mod), case["name"]
            assert got_inf == set(case["inf"]), case["name"]
        points = pe.proof_points(cname, su.td, su.cs, case)
        assert {k for k, P in zip("abc", points) if P is None} == got_inf, case["name"]
    assert directed == 20
    # the unit vector without blinding: the three big queries and L all come back at infinity
    unit = su.parts(next(c for c in su.cases if c["name"] == "z_unit_no_blinding"))
    assert unit["ma"] == unit["mb"] == unit["l_log"] == unit["cc"] == 0
    # the changed witness no longer satisfies the circuit: h's top coefficient is non-zero, the others' is zero
    assert pe._h_of(su.cp, su.cs, su.z)[-1] == 0
    assert pe._h_of(su.cp, su.cs, next(c for c in su.cases if c["name"] == "z_spoiled")["z"])[-1] != 0
    assert sum(1 for c in su.cases if not pe.satisfying(su, c)) == 4


@pytest.mark.parametrize("cname", pe.CURVE_NAMES)
def test_named_pairs_hold_every_scalar_and_every_single_zero(cname):
    su = pe.setup(cname)
    named = pe.se.split_scalars(pe.G1_GID[cname])
    pairs = {(c["r"], c["s"]) for c in su.cases if c["name"].startswith("named_")}
    n = len(named)
    assert all((named[i], named[(i + 3) % n]) in pairs for i in range(n))
    for x in named[1:7]:
        assert (0, x) in pairs and (x, 0) in pairs
    assert (0, 0) not in pairs


@pytest.mark.parametrize("cname", pe.CURVE_NAMES)
def test_glv_halves_of_the_case_scalars(cname, shim):
    """What k_finish_ab's four lanes read for the r and s of the cases, through the host-compiled endo_decompose.  The
    split TRUNCATES its two quotients (t_j = floor(c g_j / 2^256)), it does not round them: a scalar below 2^126 keeps
    itself as the first half with a zero second half (3 -> (3, 0)), every other scalar lands in one fixed fundamental cell,
    so lambda does NOT come out as (0, +-1), the first half is zero for c = 0 alone, and the sign mask is one constant per
    curve (0 on BN254, 2 on BLS12-381 - masks 1 and 3 are unreachable, as 2 is on BN254).  Asserted here: the cases hold
    every shape the split can produce - a zero second half under r and under s, both halves non-zero, every mask that
    2000 random scalars give - and each recombines to its scalar."""
    import random
    su = pe.setup(cname)
    mod = su.cp.r
    lam = pe.se.lam(pe.G1_GID[cname])
    assert _split(shim, cname, 3) == ((3, 0), 0)                              # lane 3 (lane 1) of the join cases gives infinity
    assert _split(shim, cname, 0) == ((0, 0), 0)
    for c in (lam, mod - lam):                                                # both halves of lambda itself are long
        (k0, k1), _ = _split(shim, cname, c)
        assert (k0 + k1 * lam) % mod == c and k0 != 0 and abs(k0).bit_length() > 120
    rnd = random.Random("prove_edges/glv")
    reachable = {0}
    for _ in range(2000):
        c = rnd.randrange(1, mod)
        (k0, k1), neg = _split(shim, cname, c)
        assert k0 != 0
        reachable.add(neg)
    assert reachable == ({0} if cname == "bn254" else {0, 2})
    masks = {"r": set(), "s": set()}
    zero_second, both = set(), set()
    for case in su.cases:
        for which in ("r", "s"):
            c = case[which]
            (k0, k1), neg = _split(shim, cname, c)
            assert (k0 + k1 * lam) % mod == c and (k0 != 0 or c == 0), (case["name"], which)
            masks[which].add(neg)
            if c and k1 == 0:
                zero_second.add(which)
            if k0 and k1:
                both.add(which)
    assert masks["r"] == masks["s"] == reachable
    assert zero_second == both == {"r", "s"}


@pytest.mark.parametrize("cname", pe.CURVE_NAMES)
def test_reference_equals_the_msm_based_oracle(cname):
    """groth16.prove forms every output from MSMs over the key; proof_logs from the trapdoor alone.  Every case, the ones
    with another assignment included (the oracle's prover is a map of z, not a check)."""
    su = pe.setup(cname)
    for case in su.cases:
        want = oracle_prove(su.cp, su.cs, su.pk, case["z"], [case["kappa"]], case["r"], case["s"])
        assert (want.a, want.b, want.c) == pe.proof_points(cname, su.td, su.cs, case), case["name"]
    # the exceptional proofs of the satisfying assignment are proofs: the trapdoor check accepts them
    for name in ("ma_a0_neg_alpha", "mb_b0_neg_beta", "a_and_b_inf", "ma_eq_a0", "ma_a0_eq_alpha", "part_c_neg_mh",
                 "join_r3_dbl", "join_s3_cancel"):
        case = next(c for c in su.cases if c["name"] == name)
        assert pe.satisfying(su, case)
        a, b, c = pe.proof_points(cname, su.td, su.cs, case)
        com = pe.point(cname, 1, su.td, pe.commit_log(su.td, su.cs, su.cs.stage_witness(0), case["kappa"]))
        proof = groth16.Proof(a, b, c, [com])
        assert groth16.verify_proof_trapdoor(su.cp, su.cs, su.pk, su.td, proof, [case["kappa"]], case["r"], case["s"]), name


@pytest.mark.parametrize("cname", pe.CURVE_NAMES)
def test_commit_cases(cname):
    su = pe.setup(cname)
    assert [c["inf"] for c in su.commit_cases] == [False, True, False, True, False]
    for c in su.commit_cases:
        log = pe.commit_log(su.td, su.cs, c["w"], c["kappa"])
        assert (log == 0) == c["inf"], c["name"]
        assert oracle_commit(su.cp, su.cs, su.pk, 0, c["w"], c["kappa"]) == pe.point(cname, 1, su.td, log), c["name"]
    cancels = su.commit_cases[1]
    assert pe.commit_log(su.td, su.cs, cancels["w"], 0) != 0 and cancels["kappa"] != 0


@pytest.mark.parametrize("rows", [11])
@pytest.mark.parametrize("cname", pe.CURVE_NAMES)
def test_batch_order_alternates_infinite_and_finite_rows(cname, rows):
    su = pe.setup(cname)
    calls = pe.batch_order(su.cases, rows)
    assert all(len(c) == rows for c in calls)
    assert sorted({i for c in calls for i in c}) == list(range(len(su.cases)))
    chunk = rows - pe.BATCH_ROWS_OVER_CHUNK
    mixed_full = mixed_ragged = 0
    for call in calls:
        inf = [bool(su.cases[i]["inf"]) for i in call]
        mixed_full += any(inf[:chunk]) and not all(inf[:chunk])
        mixed_ragged += any(inf[chunk:]) and not all(inf[chunk:])
        for p, f in enumerate(inf):                                            # an infinite row has finite neighbours
            if f:
                assert not any(inf[q] for q in (p - 1, p + 1) if 0 <= q < rows)
    assert mixed_full >= 2 and mixed_ragged >= 1
