"""CPU: the premises of tests/verify_edges.py, and its forge against the oracle's pairing.

Every case states why it exists (IC at infinity, the join doubles, M == 17, row 990 lies past the split, sum r_i == 0, ...):
each statement is asserted here in Python integers, so a changed seed or constant cannot turn a directed case into a random
one unnoticed.  The cofactors come from the curve parameter and are asserted with the oracle ([n] T == O on curve points), as
is the order of every small-order point.

The expected verdicts rest on one congruence mod r.  test_forge_matches_oracle_pairing ties it to the verifier's equation
(oracle/pyref/pairing.verify_proof) on the cases marked `oracle`: per curve 13 proofs - a valid and an invalid one from the
public-input, infinity and commitment-count groups (n_deltas <= 3) and one valid proof with n_deltas = 15 - i.e. 80 oracle
pairings per curve, 160 in all (each verification is one product of n_deltas + 2 pairs and one e(alpha, beta)).
"""
import pytest

from oracle.pyref import curve, groth16 as og, pairing
from oracle.pyref.params import CURVES, _is_probable_prime
from tests import verify_edges as ve

CURVE_NAMES = list(ve.CURVE_NAMES)
ORACLE_PAIRINGS_PER_CURVE = 80


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_every_premise_holds(cname):
    cases = ve.cases(cname)
    assert {c["group"] for c in cases} == set(range(1, 9))
    keys = {}
    for c in cases:
        assert keys.setdefault(c["key"].name, c["key"]) is c["key"]          # the GPU test prepares a key once per name
        assert c["premise"]() is True, (c["name"], c["why"])
        assert len(c["want"]) == len(c["proofs"]) and set(c["want"]) <= {0, 1, 2}
        assert "proof" in c["modes"] and set(c["modes"]) <= {"proof", "batch"}
        if c["rand"] is not None:
            assert "batch" in c["modes"]


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_named_premises(cname):
    """the premises the issue names, stated once more without the case's own lambda"""
    cp = CURVES[cname]
    mod, S = cp.r, ve.STEPS[cname]
    for name in ("ic_join_ic_inf", "ic_inf_nk1", "member_ic_inf"):
        c = ve.case(cname, name)
        assert c["key"].ic(c["inputs"][0]) == 0 and c["want"][0] == 1 and c["want"][1] == 0
        assert point_of(cname, c["key"], c["inputs"][0]) is None               # the oracle's prepare_inputs agrees
    c = ve.case(cname, "ic_join_dbl")
    k, x = c["key"], c["inputs"][0]
    first = (k.w[0] + sum(x[i] * k.w[i + 1] for i in range(4))) % mod
    assert first == sum(x[i] * k.w[i + 1] for i in range(4, 8)) % mod != 0
    assert ve.members_of(ve.case(cname, "nd14")["key"]) == 16 and ve.members_of(ve.case(cname, "nd15")["key"]) == 17
    assert ve.members_of(ve.case(cname, "nd255")["key"]) == 257 == 16 * 16 + 1
    c = ve.case(cname, "split_nd15_n1000")
    assert len(c["proofs"]) == 1000 and [i for i, v in enumerate(c["want"]) if v != 1] == [100, 990]
    assert 990 * S > ve.GRID_ROWS > 101 * S and ve.members_of(c["key"]) == 17
    for name in ("rand_sums_vanish_same_proof", "rand_sum_r_zero"):
        c = ve.case(cname, name)
        assert sum(c["rand"]) % mod == 0 and all(v % mod for v in c["rand"]) and c["want"] == [1, 1]
    c = ve.case(cname, "rand_input_sum_zero")
    assert sum(r * x[0] for r, x in zip(c["rand"], c["inputs"])) % mod == 0
    for c in ve.cases(cname):
        if c["group"] == 7:
            assert [v % mod for v in c["rand"]].count(0) == 1


def point_of(cname, key, x):
    cp = CURVES[cname]
    vk = og.VerifyingKey(alpha_g=None, beta_h=None, gamma_h=None, last_delta_h=None,
                         gamma_abc_g=[ve.point(cname, 1, v) for v in key.w], deltas_h=[])
    return og.prepare_inputs(cp, vk, x)


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_batch_model_is_the_congruence_but_for_the_contract_cases(cname):
    for c in ve.cases(cname):
        if "batch" not in c["modes"]:
            continue
        rand = c["rand"] if c["rand"] is not None else ve.seeded_rand(c)
        assert all(0 < v < CURVES[cname].r for v in rand) or c["group"] == 7
        model = ve.batch_model(c, rand)
        if c["contract"]:
            assert model == [1] * len(model) and c["want"] == [0] * len(model), c["name"]
        else:
            assert model == c["want"], c["name"]
    c = ve.case(cname, "batch_seam_1023")
    assert c["want"].index(0) == 1023 and c["want"].count(1) == 1024


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_group_orders_and_cofactors(cname):
    cp = CURVES[cname]
    n1, n2 = ve.group_orders(cname)
    x = ve.CURVE_X[cname]
    for group, n in ((1, n1), (2, n2)):
        G = (curve.G1 if group == 1 else curve.G2)(cp)
        assert n % cp.r == 0
        for k in range(2):
            T = ve.curve_point(cname, group, 7 + 100 * k)
            assert G.on_curve(T) and G.mul(T, n) is None
    if cname == "bn254":
        assert n1 == cp.r and ve.cofactor_points(cname, 1) is None          # cofactor 1: nothing to test on G1
        assert n2 // cp.r == 2 * cp.q - cp.r
    else:
        assert 3 * (n1 // cp.r) == (x - 1) ** 2
        assert ve.cofactor_points(cname, 1)["h"] == 0x396c8c005555e1568c00aaab0000aaab
    for group, n in ((1, n1), (2, n2)):
        cof = ve.cofactor_points(cname, group)
        if cof is None:
            continue
        G = (curve.G1 if group == 1 else curve.G2)(cp)
        assert cof["h"] * cp.r == n and cof["factors"] and set(cof["V"]) == {l for l, _e in cof["factors"]}
        rest = cof["h"]
        for l, e in cof["factors"]:
            assert l < ve.SMALL_PRIME_BOUND and _is_probable_prime(l) and rest % l ** e == 0 and rest // l ** e % l != 0
            rest //= l ** e
            V = cof["V"][l]
            assert V is not None and G.on_curve(V) and G.mul(V, l) is None    # l is prime: the order is exactly l
            assert G.mul(V, cp.r) is not None
        assert cof["U"] is not None and G.on_curve(cof["U"]) and G.mul(cof["U"], cof["h"]) is None and G.mul(cof["U"], cp.r) is not None
    if cname == "bls12_381":
        assert [l for l, _e in ve.cofactor_points(cname, 1)["factors"]] == [3, 11, 10177, 859267]
        assert [l for l, _e in ve.cofactor_points(cname, 2)["factors"]] == [13, 23, 2713, 11953, 262069]
    else:
        assert [l for l, _e in ve.cofactor_points(cname, 2)["factors"]] == [10069, 5864401]


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_check_points_expectations(cname):
    cp = CURVES[cname]
    for group in (1, 2):
        pts = dict(ve.check_points(cname, group))
        want = {nm: ve.in_subgroup(cname, group, P) for nm, P in pts.items()}
        assert want["infinity"] and all(want["subgroup_%d" % i] for i in range(3)) and not want["off_curve"]
        outside = [nm for nm in pts if nm.startswith(("U", "V_", "neg_V_", "S_plus_V_", "order3"))]
        if (cname, group) == ("bn254", 1):
            assert not outside and all(want["curve_%d" % k] for k in range(3))
        else:
            assert outside and not any(want[nm] for nm in outside)
            G = (curve.G1 if group == 1 else curve.G2)(cp)
            assert all(G.on_curve(pts[nm]) for nm in outside)                 # rejected by the subgroup test alone
    if cname == "bls12_381":
        G1 = curve.G1(cp)
        for y in (2, cp.q - 2):
            assert G1.on_curve((0, y)) and G1.mul((0, y), 3) is None


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_forge_matches_oracle_pairing(cname):
    pairings, seen = 0, set()
    for c in ve.cases(cname):
        if not c["oracle"]:
            continue
        key = c["key"]
        assert key.nd <= 3 or (key.nd == 15 and len(c["oracle"]) == 1)
        vk = og.VerifyingKey(alpha_g=ve.point(cname, 1, key.alpha), beta_h=ve.point(cname, 2, key.beta),
                             gamma_h=ve.point(cname, 2, key.gamma), last_delta_h=ve.point(cname, 2, key.deltas[-1]),
                             gamma_abc_g=[ve.point(cname, 1, v) for v in key.w],
                             deltas_h=[ve.point(cname, 2, d) for d in key.deltas])
        for i in c["oracle"]:
            p, x = c["proofs"][i], c["inputs"][i]
            assert p.valid_points()
            proof = og.Proof(ve.point(cname, 1, p.a), ve.point(cname, 2, p.b), ve.point(cname, 1, p.c),
                             [ve.point(cname, 1, d) for d in p.ds])
            assert pairing.verify_proof(cname, vk, proof, x) is bool(c["want"][i]), (c["name"], i)
            pairings += key.nd + 2 + 1
            seen.add((c["group"], c["want"][i]))
    assert {(g, v) for g in (1, 2, 3) for v in (0, 1)} <= seen
    assert pairings == ORACLE_PAIRINGS_PER_CURVE


def test_pack_shapes():
    cname = "bn254"
    cp = CURVES[cname]
    c = ve.pack(ve.case(cname, "ic_nk0"))
    assert c["x"] is None and c["n"] == 3 and len(c["a"]) == 3 * 64 and len(c["b"]) == 3 * 128 and len(c["ds"]) == 3 * 64
    c = ve.pack(ve.case(cname, "nd1"))
    assert c["ds"] is None and len(c["x"]) == 3 * 2 * 32
    c = ve.pack(ve.case(cname, "nd255"))
    assert len(c["ds"]) == 3 * 254 * 64
    vk = ve.case(cname, "nd255")["key"].vk_bytes()
    assert len(vk["deltas_h"]) == 255 * 128 and len(vk["gamma_abc_g"]) == 3 * 64
    c = ve.pack(ve.case(cname, "rand_zero_on_wrong"))
    assert len(c["rand"]) == 3 * 32 and not c["rand"][32:64].any() and c["rand"][:32].any()
    assert cp.r > 1 << 253
