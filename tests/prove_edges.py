"""Deterministic cases for the tests of the proof finish (k_prep_ext, k_finish_ab, k_finish_c of csrc/prove_impl.cuh, and the
"ext" slots that carry r, s, r s and the kappa_i through the big MSMs) and of hk_commit / hk_commit_batch:
tests/test_prove_edges_cpu.py checks every premise stated here, tests/test_prove_edges_gpu.py runs the device on them.  A
plain module with fixed seeds, like tests/sweep_edges.py, whose named scalars it takes; nothing here needs a GPU.

The key comes from the oracle with its toxic waste kept, so the discrete log of every output is a polynomial in Fr that is
LINEAR in r, in s and in kappa:

    MA  = S_a + r dl                    A  = MA + a_0 + alpha         (S_a = sum_{i >= 1} z_i a_i, dl = delta_last)
    MB  = S_b + s dl                    B  = B1 = MB + b_0 + beta
    Cc  = s A + r B1                    ML' = l - r s dl - kappa d_0   part_c = Cc + ML'      C = part_c + MH

and every exceptional branch of the finish (an operand at infinity, P + P, P + (-P), a zero GLV half) is one linear
equation in one of them.  The reference `proof_logs` reads nothing from the device and nothing from the key: an expected
point is ONE scalar multiplication of the key's generator.
"""
import random

from oracle.pyref import curve, groth16
from oracle.pyref.params import CURVES
from tests import sweep_edges as se
from tests.util import synthetic_r1cs

CURVE_NAMES = ("bn254", "bls12_381")
G1_GID = {"bn254": 0, "bls12_381": 2}                 # group ids of tests/msm_edges.py
SEED = 7                                              # tests/test_prove_edges_cpu.py asserts what the seed has to give
ALPHA, BETA, GAMMA, DELTAS, TAU, G1_SCALAR, G2_SCALAR = 5, 7, 11, (13, 17), 19, 2, 3
MAX_PROOFS = 64
BATCH_ROWS_OVER_CHUNK = 3


def _cp_of(cs):
    return next(cp for cp in CURVES.values() if cp.r == cs.r)


# ---- the reference ----------------------------------------------------------------------------------------------------
_h_cache = {}


def _h_of(cp, cs, z):
    key = (id(cs), tuple(z))                           # a Setup's circuit lives as long as the module
    if key not in _h_cache:
        A, B, C = cs.matrices()
        _h_cache[key] = groth16.witness_map_from_matrices(cp, A, B, C, cs.num_instance, cs.num_constraints, list(z))
    return _h_cache[key]


def proof_parts(td, cs, z, kappas, r, s):
    """Every discrete log on the way to a proof, by the exponent formula of groth16.verify_proof_trapdoor without its
    satisfaction check, for ANY assignment z: a dict with s_a, s_b (the sums over i >= 1), ma, mb (the A and B query
    results with their ext slot), log_a, log_b, cc = s log_a + r log_b, ml (the L query with its ext slots), h_log,
    part_c = cc + ml and log_c.  Variable 0 enters A and B as query[0], i.e. as 1 (groth16.calculate_coeff); h's top
    coefficient has no base (prover.rs:128-129)."""
    cp = _cp_of(cs)
    mod = cp.r
    n_in = cs.num_instance
    assert len(z) == n_in + cs.num_witness and len(kappas) + 1 == len(td.deltas)
    inv = lambda x: pow(x, -1, mod)
    dl = td.deltas[-1]
    h = _h_of(cp, cs, z)
    s_a = sum(zi * ai for zi, ai in zip(z[1:], td.a[1:])) % mod
    s_b = sum(zi * bi for zi, bi in zip(z[1:], td.b[1:])) % mod
    ma = (s_a + r * dl) % mod
    mb = (s_b + s * dl) % mod
    log_a = (ma + td.a[0] + td.alpha) % mod
    log_b = (mb + td.b[0] + td.beta) % mod
    abc = lambda i: (td.beta * td.a[i] + td.alpha * td.b[i] + td.c[i]) % mod
    s_last, e_last = cs.stage_ranges[-1]
    l_log = sum(z[n_in + j] * abc(n_in + j) for j in range(s_last, e_last)) % mod * inv(dl) % mod
    h_log = sum(h[i] * pow(td.t, i, mod) for i in range(td.m - 1)) % mod * td.zt % mod * inv(dl) % mod
    cc = (s * log_a + r * log_b) % mod
    ml = (l_log - r * s % mod * dl - sum(k * d for k, d in zip(kappas, td.deltas))) % mod
    part_c = (cc + ml) % mod
    return dict(s_a=s_a, s_b=s_b, ma=ma, mb=mb, log_a=log_a, log_b=log_b, l_log=l_log, h_log=h_log, cc=cc, ml=ml,
                part_c=part_c, log_c=(part_c + h_log) % mod, sa=s * log_a % mod, rb=r * log_b % mod)


def proof_logs(td, cs, z, kappas, r, s):
    """(log_a, log_b, log_c): A = log_a g1, B = log_b g2, C = log_c g1 for the key's generators td.g1, td.g2"""
    p = proof_parts(td, cs, z, kappas, r, s)
    return p["log_a"], p["log_b"], p["log_c"]


def commit_log(td, cs, w, kappa, stage=0):
    """the discrete log of committer.rs:87-91's commitment to the stage witness w under randomness kappa"""
    mod = cs.r
    n_in = cs.num_instance
    s0, e0 = cs.stage_ranges[stage]
    assert len(w) == e0 - s0
    abc = lambda i: (td.beta * td.a[i] + td.alpha * td.b[i] + td.c[i]) % mod
    d = sum(wj * abc(n_in + j) for wj, j in zip(w, range(s0, e0))) % mod * pow(td.deltas[stage], -1, mod) % mod
    return (d + kappa * td.deltas[-1]) % mod


_pts = {}


def point(cname, group, td, log):
    """log td.g1 (group 1) or log td.g2 (group 2) as an affine tuple, None at infinity; one oracle multiplication, cached"""
    cp = CURVES[cname]
    key = (cname, group, log % cp.r)
    if key not in _pts:
        G = (curve.G1 if group == 1 else curve.G2)(cp)
        _pts[key] = G.mul(td.g1 if group == 1 else td.g2, log % cp.r)
    return _pts[key]


def proof_points(cname, td, cs, case):
    la, lb, lc = proof_logs(td, cs, case["z"], [case["kappa"]], case["r"], case["s"])
    return point(cname, 1, td, la), point(cname, 2, td, lb), point(cname, 1, td, lc)


# ---- circuit and key -------------------------------------------------------------------------------------------------
class Setup:
    """One curve's circuit (n_v = 40, m = 32, two stages, one kappa), key, trapdoor and case lists; `setup` caches it."""

    def __init__(self, cname):
        self.cname = cname
        self.cp = cp = CURVES[cname]
        self.cs = cs = synthetic_r1cs(cp, random.Random("prove_edges/%s/%d" % (cname, SEED)), n_inst=4, n_free=12, n_c=24,
                                      two_stage_split=5)
        assert cs.is_satisfied() and len(cs.stage_ranges) == 2
        self.pk, self.td = groth16.generate_parameters(cp, cs, ALPHA, BETA, GAMMA, list(DELTAS), TAU, G1_SCALAR, G2_SCALAR)
        self.z = cs.full_assignment()
        self.n_v = len(self.z)
        assert self.n_v == 40 and self.td.m == 32
        self.cases = _proof_cases(self)
        self.commit_cases = _commit_cases(self)
        assert len(self.cases) <= MAX_PROOFS and len({c["name"] for c in self.cases}) == len(self.cases)

    def parts(self, case):
        return proof_parts(self.td, self.cs, case["z"], [case["kappa"]], case["r"], case["s"])


_setups = {}


def setup(cname):
    if cname not in _setups:
        _setups[cname] = Setup(cname)
    return _setups[cname]


def denominators(su):
    """everything a directed case divides by, and the operands that must not be at infinity by accident: all non-zero for
    the seed above (tests/test_prove_edges_cpu.py)"""
    td, mod = su.td, su.cp.r
    p = proof_parts(td, su.cs, su.z, [0], 0, 0)
    return dict(dl=td.deltas[-1], d0=td.deltas[0], a_0=td.a[0], b_0=td.b[0], alpha=td.alpha, beta=td.beta, h_log=p["h_log"],
                l_log=p["l_log"], a_fixed=p["log_a"], b_fixed=p["log_b"], a_fixed_6dl=(p["log_a"] + 6 * td.deltas[-1]) % mod,
                b_fixed_6dl=(p["log_b"] + 6 * td.deltas[-1]) % mod)


# ---- the proof cases -------------------------------------------------------------------------------------------------
def _proof_cases(su):
    """[dict(name, z, r, s, kappa, inf, cond)]: `inf` is the set of outputs ('a', 'b', 'c') at infinity, `cond` a predicate
    on proof_parts (and the modulus) that states the branch the case is there for"""
    cp, td, cs, z = su.cp, su.td, su.cs, su.z
    mod = cp.r
    inv = lambda x: pow(x, -1, mod)
    rn = random.Random("prove_edges/%s/scalars" % su.cname)
    rand = lambda: rn.randrange(1, mod)
    dl, d0, a_0, b_0, alpha, beta = td.deltas[-1], td.deltas[0], td.a[0], td.b[0], td.alpha, td.beta
    base = proof_parts(td, cs, z, [0], 0, 0)
    s_a, s_b = base["s_a"], base["s_b"]
    cases = []

    def add(name, r, s, kappa, inf=(), cond=None, zz=None):
        cases.append(dict(name=name, z=list(zz if zz is not None else z), r=r % mod, s=s % mod, kappa=kappa % mod,
                          inf=frozenset(inf), cond=cond))

    # r for the A side, s for the B side: the five rows of each, then both at infinity at once
    a_rows = [("ma_inf", -s_a, lambda p, m: p["ma"] == 0, ()),
              ("ma_neg_a0", -a_0 - s_a, lambda p, m: (p["ma"] + a_0) % m == 0 and p["ma"] != 0, ()),
              ("ma_eq_a0", a_0 - s_a, lambda p, m: p["ma"] == a_0, ()),
              ("ma_a0_eq_alpha", alpha - a_0 - s_a, lambda p, m: (p["ma"] + a_0) % m == alpha, ()),
              ("ma_a0_neg_alpha", -alpha - a_0 - s_a, lambda p, m: (p["ma"] + a_0 + alpha) % m == 0 and p["log_a"] == 0, "a")]
    b_rows = [("mb_inf", -s_b, lambda p, m: p["mb"] == 0, ()),
              ("mb_neg_b0", -b_0 - s_b, lambda p, m: (p["mb"] + b_0) % m == 0 and p["mb"] != 0, ()),
              ("mb_eq_b0", b_0 - s_b, lambda p, m: p["mb"] == b_0, ()),
              ("mb_b0_eq_beta", beta - b_0 - s_b, lambda p, m: (p["mb"] + b_0) % m == beta, ()),
              ("mb_b0_neg_beta", -beta - b_0 - s_b, lambda p, m: (p["mb"] + b_0 + beta) % m == 0 and p["log_b"] == 0, "b")]
    for name, num, cond, inf in a_rows:
        add(name, num * inv(dl), rand(), rand(), inf, cond)
    for name, num, cond, inf in b_rows:
        add(name, rand(), num * inv(dl), rand(), inf, cond)
    add("a_and_b_inf", a_rows[4][1] * inv(dl), b_rows[4][1] * inv(dl), rand(), "ab",
        lambda p, m: p["log_a"] == 0 and p["log_b"] == 0 and p["cc"] == 0)

    # kappa for C, with r, s generic: ml(kappa) = ml(0) - kappa d_0 is linear in kappa
    for name, target, cond, inf in (
            ("ml_inf", lambda p: 0, lambda p, m: p["ml"] == 0 and p["cc"] != 0, ()),
            ("cc_eq_ml", lambda p: p["cc"], lambda p, m: p["cc"] == p["ml"] != 0, ()),
            ("cc_neg_ml", lambda p: -p["cc"], lambda p, m: p["part_c"] == 0 and p["cc"] != 0, ()),
            ("part_c_eq_mh", lambda p: p["h_log"] - p["cc"], lambda p, m: p["part_c"] == p["h_log"] != 0, ()),
            ("part_c_neg_mh", lambda p: -p["h_log"] - p["cc"], lambda p, m: (p["part_c"] + p["h_log"]) % m == 0 and p["part_c"] != 0,
             "c")):
        r, s = rand(), rand()
        p0 = proof_parts(td, cs, z, [0], r, s)
        add(name, r, s, (p0["ml"] - target(p0)) * inv(d0), inf, cond)              # ml(0) - kappa d_0 = target

    # the join of the four partial products.  r = 3 has a zero second half: lane 3 gives infinity, lane 2 gives 3 B1, and
    # lanes 0 + 1 give s A, so `sum + part[2]` meets s A == 3 B1 or s A == -3 B1; s = 3 mirrors it (3 A + infinity, then
    # r B1's two halves one by one: the cancellation falls on the LAST add of the join, the equality on no single add -
    # the sum is 6 A all the same).
    a_f, b_f = base["log_a"], base["log_b"]                                    # a_0 + S_a + alpha, b_0 + S_b + beta
    add("join_r3_dbl", 3, 3 * b_f * inv(a_f), rand(), (), lambda p, m: p["sa"] == p["rb"] != 0)
    add("join_r3_cancel", 3, -3 * b_f * inv((a_f + 6 * dl) % mod), rand(), (), lambda p, m: p["cc"] == 0 and p["sa"] != 0)
    add("join_s3_dbl", 3 * a_f * inv(b_f), 3, rand(), (), lambda p, m: p["sa"] == p["rb"] != 0)
    add("join_s3_cancel", -3 * a_f * inv((b_f + 6 * dl) % mod), 3, rand(), (), lambda p, m: p["cc"] == 0 and p["sa"] != 0)

    # named scalars, paired cyclically (r_i with s_(i+3)), then every pair of a named scalar with 0 on either side
    named = se.split_scalars(G1_GID[su.cname])
    n = len(named)
    pairs = [(named[i], named[(i + 3) % n]) for i in range(n)]
    for x in named[1:7]:
        pairs += [p for p in ((0, x), (x, 0)) if p not in pairs]
    for i, (r, s) in enumerate(pairs):
        add("named_%02d" % i, r, s, rand())

    # other assignments: h's top coefficient non-zero, the unit vector, all r - 1
    spoiled = list(z)
    spoiled[cs.num_instance + 7] = (spoiled[cs.num_instance + 7] + 1) % mod
    e0 = [1] + [0] * (len(z) - 1)
    big = [1] + [mod - 1] * (len(z) - 1)
    add("z_spoiled", rand(), rand(), rand(), zz=spoiled)
    add("z_unit", rand(), rand(), rand(), zz=e0)
    add("z_unit_no_blinding", 0, 0, 0, zz=e0)
    add("z_all_r_minus_1", rand(), rand(), rand(), zz=big)
    return cases


def satisfying(su, case):
    return case["z"] == su.z


def batch_order(cases, rows):
    """The calls of the batch test: lists of `rows` case indices each, every case in at least one, with the cases that have
    an output at infinity spread over the calls at odd rows - row 1 of the full chunk or row rows - 2 of the ragged one
    first, call by call in turn - so that infinite and finite results sit next to each other inside a chunk.  The last call takes the last
    `rows` cases again where the list is no multiple of `rows`."""
    inf = [i for i, c in enumerate(cases) if c["inf"]]
    fin = [i for i, c in enumerate(cases) if not c["inf"]]
    n_calls = (len(cases) + rows - 1) // rows
    slots = [1, rows - 2] + [p for p in range(3, rows - 2, 2)]
    calls = [[None] * rows for _ in range(n_calls)]
    for j, i in enumerate(inf):
        call, turn = j % n_calls, j // n_calls
        assert turn < len(slots)
        if turn < 2 and call % 2:                              # odd calls start in the ragged chunk
            turn = 1 - turn
        calls[call][slots[turn]] = i
    it = iter(fin)
    flat = []
    for call in calls:
        for p in range(rows):
            if call[p] is None:
                call[p] = next(it, None)
        flat += [i for i in call if i is not None]
    assert sorted(flat) == list(range(len(cases)))
    out = [flat[o:o + rows] for o in range(0, len(flat), rows)]
    if len(out[-1]) < rows:
        out[-1] = flat[-rows:]
    return out


# ---- the commit cases --------------------------------------------------------------------------------------------------
def _commit_cases(su):
    """[dict(name, w, kappa, inf)] for stage 0, five rows with the infinities at rows 1 and 3 (the batch takes them in this
    order)"""
    cp, td, cs = su.cp, su.td, su.cs
    mod = cp.r
    rn = random.Random("prove_edges/%s/commit" % su.cname)
    n = len(cs.stage_witness(0))
    dl = td.deltas[-1]
    rand_w = lambda: [rn.randrange(mod) for _ in range(n)]
    w1 = rand_w()
    d1 = commit_log(td, cs, w1, 0)
    rows = [("random", rand_w(), rn.randrange(1, mod), False),
            ("kappa_cancels", w1, -d1 * pow(dl, -1, mod), True),
            ("zero_w_kappa_1", [0] * n, 1, False),
            ("zero_w_kappa_0", [0] * n, 0, True),
            ("kappa_r_minus_1", cs.stage_witness(0), mod - 1, False)]
    return [dict(name=nm, w=[x % mod for x in w], kappa=k % mod, inf=inf) for nm, w, k, inf in rows]
