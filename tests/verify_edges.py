"""Deterministic cases for the tests of proof verification (hk_vk_prepare / hk_verify_batch / hk_points_check_* of
csrc/verify.cuh): tests/test_verify_edges_cpu.py checks every premise stated here, tests/test_verify_edges_gpu.py runs the
device on them.  A plain module with fixed seeds, like tests/prove_edges.py; nothing here needs a GPU and no device call goes
into an expected value.

A proof forge.  The key's trapdoor is known: alpha G, beta H, gamma H, delta_j H, w_k G for logs chosen here (G, H the curve's
generators), so a proof with logs (a, b, d_0 .. d_{nd-2}, c) and public inputs x satisfies the verifier's equation iff

    a b == alpha beta + (w_0 + sum_k x_k w_{k+1}) gamma + sum_j d_j delta_j + c delta_last      (mod r)

`Key.solve` solves that for one member, `Key.holds` evaluates it in Python integers: that congruence is the expected
verdict of every case (2 where a point is off its curve or outside the prime-order subgroup).  The CPU test ties it to the
oracle's pairing on a named subset (`oracle` cases).

Batch mode gives a verdict of 1 from the exact equation or from a batch equation that holds, so `batch_model` states what a
chunk has to return: the per-proof verdicts where a point is invalid, an r_i is 0 or sum r_i (a_i b_i - rhs_i) != 0, else all
1.  For every case but the `contract` ones (whose tampers cancel under r_i the forger knows - the caller's side of the
contract: the r_i are drawn after the proofs are fixed) that model IS the congruence; the CPU test asserts so.  The contract
cases make the batch pipeline visible from outside: a wrong r_i A_i or column sum turns their [1, 1] into [0, 0].
"""
import random

import numpy as np

from oracle.pyref import curve
from oracle.pyref.codec import Codec
from oracle.pyref.params import CURVES

CURVE_NAMES = ("bn254", "bls12_381")
CHUNK = 1024                                            # VERIFY_CHUNK of csrc/verify.cuh
GRID_ROWS = 65535                                       # rows of one tree launch (verify_products)
WAVE_MEMBERS = 16                                       # members one wave multiplies (c of k_verify_tree_lines)
STEPS = {"bn254": 88, "bls12_381": 68}                  # Miller steps S, pinned by tests/test_pairing_cpu.py
CURVE_X = {"bn254": 4965661367192848881, "bls12_381": -0xd201000000010000}
SMALL_PRIME_BOUND = 1 << 23
DELTA_POOL, D_POOL = 7, 11                              # distinct delta_j / D logs before they cycle


class Bad:
    """A proof member that is no multiple of the generator: `pt` is off its curve or outside the prime-order subgroup."""

    def __init__(self, pt, why):
        self.pt, self.why = pt, why


class Pr:
    """One proof: a, b, c and ds are logs (ints mod r; 0 is the point at infinity) or Bad points."""

    def __init__(self, a, b, ds, c):
        self.a, self.b, self.ds, self.c = a, b, tuple(ds), c

    def with_(self, **kw):
        p = Pr(self.a, self.b, self.ds, self.c)
        for k, v in kw.items():
            setattr(p, k, tuple(v) if k == "ds" else v)
        return p

    def members(self):
        return (self.a, self.b, self.c) + self.ds

    def valid_points(self):
        return not any(isinstance(m, Bad) for m in self.members())


# ---- points ----------------------------------------------------------------------------------------------------------
_pts, _bytes = {}, {}


def point(cname, group, log):
    """log G (group 1) or log H (group 2) as an affine tuple, None at infinity; one oracle multiplication, cached"""
    cp = CURVES[cname]
    key = (cname, group, log % cp.r)
    if key not in _pts:
        G = (curve.G1 if group == 1 else curve.G2)(cp)
        _pts[key] = G.mul(G.gen, log % cp.r)
    return _pts[key]


def member_bytes(cname, group, m):
    """the packed affine bytes of a proof member (a log or a Bad point)"""
    cd = Codec(CURVES[cname])
    enc = cd.g1 if group == 1 else cd.g2
    if isinstance(m, Bad):
        return enc(m.pt)
    key = (cname, group, m % CURVES[cname].r)
    if key not in _bytes:
        _bytes[key] = enc(point(cname, group, m))
    return _bytes[key]


# ---- the key -----------------------------------------------------------------------------------------------------------
class Key:
    """A verifying key by its logs.  deltas[-1] is delta_last; w has n_abc entries (0: that base is at infinity)."""

    def __init__(self, cname, name, alpha, beta, gamma, deltas, w):
        self.cname, self.name = cname, name
        self.mod = mod = CURVES[cname].r
        self.alpha, self.beta, self.gamma = alpha % mod, beta % mod, gamma % mod
        self.deltas = [d % mod for d in deltas]
        self.w = [v % mod for v in w]
        self.nd, self.n_abc, self.nk = len(deltas), len(w), len(w) - 1
        assert self.alpha and self.beta and self.gamma and all(self.deltas)

    def ic(self, x):
        assert len(x) == self.nk
        return (self.w[0] + sum(xk * wk for xk, wk in zip(x, self.w[1:]))) % self.mod

    def rhs(self, pr, x):
        assert len(pr.ds) == self.nd - 1
        return (self.alpha * self.beta + self.ic(x) * self.gamma + sum(d * dl for d, dl in zip(pr.ds, self.deltas))
                + pr.c * self.deltas[-1]) % self.mod

    def defect(self, pr, x):
        return (pr.a * pr.b - self.rhs(pr, x)) % self.mod

    def holds(self, pr, x):
        return self.defect(pr, x) == 0

    def verdict(self, pr, x):
        return 2 if not pr.valid_points() else int(self.holds(pr, x))

    def solve(self, x, a, b, ds, c=None, for_="c"):
        """The valid proof with the given logs and the member `for_` ('c', 'a' or 'd0') solved for; the member solved for is
        passed as None (c by default)."""
        mod, inv = self.mod, lambda v: pow(v, -1, self.mod)
        ds = list(ds)
        if for_ == "c":
            rest = Pr(a, b, ds, 0)
            c = (a * b - self.rhs(rest, x)) * inv(self.deltas[-1]) % mod
        elif for_ == "a":
            a = self.rhs(Pr(0, b, ds, c), x) * inv(b) % mod
        elif for_ == "d0":
            ds[0] = 0
            ds[0] = (a * b - self.rhs(Pr(a, b, ds, c), x)) * inv(self.deltas[0]) % mod
        else:
            raise ValueError(for_)
        pr = Pr(a, b, ds, c)
        assert self.holds(pr, x)
        return pr

    def vk_bytes(self):
        """dict(alpha_g, beta_h, gamma_h, deltas_h, gamma_abc_g) of packed affine bytes (hk_vk_desc; deltas_h ends with
        delta_last)"""
        cn = self.cname
        u8 = lambda b: np.frombuffer(b, np.uint8).copy()
        return dict(alpha_g=u8(member_bytes(cn, 1, self.alpha)), beta_h=u8(member_bytes(cn, 2, self.beta)),
                    gamma_h=u8(member_bytes(cn, 2, self.gamma)),
                    deltas_h=u8(b"".join(member_bytes(cn, 2, d) for d in self.deltas)),
                    gamma_abc_g=u8(b"".join(member_bytes(cn, 1, v) for v in self.w)))


def pack(case):
    """The operands of hk_verify_batch for a case: dict(n, a, b, c, ds, x, rand) of uint8 arrays (ds None for n_deltas == 1,
    x None for n_abc == 1, rand None where the case names no scalars)."""
    key = case["key"]
    cn = key.cname
    cd = Codec(CURVES[cn])
    u8 = lambda parts: np.frombuffer(b"".join(parts), np.uint8).copy()
    ps = case["proofs"]
    return dict(n=len(ps), a=u8(member_bytes(cn, 1, p.a) for p in ps), b=u8(member_bytes(cn, 2, p.b) for p in ps),
                c=u8(member_bytes(cn, 1, p.c) for p in ps),
                ds=u8(member_bytes(cn, 1, d) for p in ps for d in p.ds) if key.nd > 1 else None,
                x=cd.fr_vec_mont([v for x in case["inputs"] for v in x]) if key.nk else None,
                rand=cd.fr_vec_mont(case["rand"]) if case["rand"] is not None else None)


def seeded_rand(case):
    """nonzero 128-bit r_i for a case without explicit scalars (what the Python wrapper draws)"""
    rn = random.Random("verify_edges/rand/" + case["name"])
    return [rn.getrandbits(128) | 1 for _ in case["proofs"]]


def batch_model(case, rand):
    """what batch mode has to return under the scalars `rand` (module docstring)"""
    key, ps, xs = case["key"], case["proofs"], case["inputs"]
    out = []
    for o in range(0, len(ps), CHUNK):
        rows = range(o, min(o + CHUNK, len(ps)))
        per_proof = [key.verdict(ps[i], xs[i]) for i in rows]
        if 2 in per_proof or any(rand[i] % key.mod == 0 for i in rows):
            out += per_proof
        elif sum(rand[i] * key.defect(ps[i], xs[i]) for i in rows) % key.mod == 0:
            out += [1] * len(rows)
        else:
            out += per_proof
    return out


# ---- on-curve points outside the subgroup ----------------------------------------------------------------------------
def _sqrt_fq(a, q):
    s = pow(a, (q + 1) // 4, q)                          # q = 3 mod 4 on both curves
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


def curve_point(cname, group, start):
    """a point on the G1 curve (x = start upward) or on the twist (x = (start, 1) upward), the cofactor NOT cleared"""
    cp = CURVES[cname]
    G = (curve.G1 if group == 1 else curve.G2)(cp)
    F = G.F
    x = start if group == 1 else (start, 1)
    while True:
        rhs = F.add(F.mul(F.mul(x, x), x), G.b)
        y = _sqrt_fq(rhs, cp.q) if group == 1 else _sqrt_fq2(rhs, cp.q)
        if y:
            assert G.on_curve((x, y))
            return (x, y)
        x = x + 1 if group == 1 else (x[0] + 1, 1)


def off_curve(cname, group, log):
    """log G (or H) with its y moved by one: off the curve"""
    P = point(cname, group, log)
    q = CURVES[cname].q
    bad = (P[0], (P[1] + 1) % q) if group == 1 else (P[0], (P[1][0], (P[1][1] + 1) % q))
    assert not (curve.G1 if group == 1 else curve.G2)(CURVES[cname]).on_curve(bad)
    return Bad(bad, "off the curve")


def _isqrt_exact(n):
    import math
    s = math.isqrt(n)
    assert s * s == n
    return s


_orders = {}


def group_orders(cname):
    """(n1, n2): the orders of E(Fq) and of the twist E'(Fq2), from the curve's parameter x: q + 1 - t for the trace t of
    the family, and the one sextic twist of E over Fq2 whose order r divides.  The CPU test asserts [n] T == O on curve
    points T with the oracle."""
    if cname in _orders:
        return _orders[cname]
    cp, x = CURVES[cname], CURVE_X[cname]
    q, r = cp.q, cp.r
    if cname == "bn254":
        assert q == 36 * x ** 4 + 36 * x ** 3 + 24 * x ** 2 + 6 * x + 1 and r == 36 * x ** 4 + 36 * x ** 3 + 18 * x ** 2 + 6 * x + 1
        t = 6 * x * x + 1
    else:
        assert r == x ** 4 - x * x + 1 and 3 * q == (x - 1) ** 2 * r + 3 * x
        t = x + 1
    n1 = q + 1 - t
    t2 = t * t - 2 * q                                   # the trace over Fq2
    f2 = _isqrt_exact((4 * q * q - t2 * t2) // 3)        # t2^2 - 4 q^2 = -3 f2^2
    assert (4 * q * q - t2 * t2) % 3 == 0
    cands = [q * q + 1 - tau // 2 for tau in (t2 + 3 * f2, t2 - 3 * f2, -t2 + 3 * f2, -t2 - 3 * f2) if tau % 2 == 0]
    cands = [n for n in cands if n % r == 0]
    assert len(cands) == 1 and n1 % r == 0
    _orders[cname] = (n1, cands[0])
    return _orders[cname]


_primes = []


def small_prime_factors(h):
    """[(l, e)] for every prime l < 2^23 with l^e exactly dividing h, by trial division"""
    if not _primes:
        sieve = np.ones(SMALL_PRIME_BOUND, dtype=bool)
        sieve[:2] = False
        for i in range(2, int(SMALL_PRIME_BOUND ** 0.5) + 1):
            if sieve[i]:
                sieve[i * i::i] = False
        _primes.extend(np.nonzero(sieve)[0].tolist())
    out = []
    for l in _primes:
        if h % l == 0:
            e = 0
            while h % l == 0:
                h //= l
                e += 1
            out.append((l, e))
    return out


_cof = {}


def cofactor_points(cname, group):
    """dict(h, factors, U, V): h the cofactor (group order / r), factors its primes below 2^23, U = [r] T a point of the
    cofactor part for a curve point T, V[l] a point of order exactly l for each such prime (from the first curve points
    that have a component there).  None on BN254 G1, whose cofactor is 1."""
    key = (cname, group)
    if key in _cof:
        return _cof[key]
    cp = CURVES[cname]
    G = (curve.G1 if group == 1 else curve.G2)(cp)
    n = group_orders(cname)[group - 1]
    h = n // cp.r
    if h == 1:
        _cof[key] = None
        return None
    factors = small_prime_factors(h)
    U, V = None, {}
    start = 2
    while U is None or len(V) < len(factors):
        T = curve_point(cname, group, start)
        start = (T[0] if group == 1 else T[0][0]) + 1
        Ut = G.mul(T, cp.r)
        if Ut is None:
            continue
        U = U or Ut
        for l, e in factors:
            if l in V:
                continue
            W = G.mul(Ut, h // l ** e)
            while W is not None and G.mul(W, l) is not None:
                W = G.mul(W, l)
            if W is not None:
                V[l] = W
    _cof[key] = dict(h=h, factors=factors, U=U, V=V)
    return _cof[key]


def check_points(cname, group):
    """[(name, point)] for hk_points_check_g1 / _g2: subgroup points, infinity, curve points with the cofactor not cleared,
    a point off the curve, and - where the cofactor is not 1 - U, every V_l, -V_l, S + V_l for a subgroup point S, and on
    BLS12-381 G1 the order-3 points (0, +-2).  The expected value of each is the oracle's on-curve and [r] P == O."""
    cp = CURVES[cname]
    G = (curve.G1 if group == 1 else curve.G2)(cp)
    rn = random.Random("verify_edges/%s/points%d" % (cname, group))
    sub = [point(cname, group, rn.randrange(1, cp.r)) for _ in range(3)]
    pts = [("subgroup_%d" % i, P) for i, P in enumerate(sub)] + [("infinity", None)]
    pts += [("curve_%d" % k, curve_point(cname, group, 5 + 1000 * k)) for k in range(3)]
    pts.append(("off_curve", off_curve(cname, group, 12345).pt))
    cof = cofactor_points(cname, group)
    if cof:
        pts.append(("U", cof["U"]))
        for l, V in sorted(cof["V"].items()):
            pts += [("V_%d" % l, V), ("neg_V_%d" % l, G.neg(V)), ("S_plus_V_%d" % l, G.add(sub[0], V))]
    if (cname, group) == ("bls12_381", 1):
        pts += [("order3_plus", (0, 2)), ("order3_minus", (0, cp.q - 2))]
    return pts


def in_subgroup(cname, group, P):
    """the oracle's test: on the curve and [r] P == O"""
    cp = CURVES[cname]
    G = (curve.G1 if group == 1 else curve.G2)(cp)
    return G.on_curve(P) and G.mul(P, cp.r) is None


# ---- the cases -------------------------------------------------------------------------------------------------------
def members_of(key):
    """members of a per-proof product: A, IC, the D_j, C"""
    return key.nd + 2


def _cases(cname):
    cp = CURVES[cname]
    mod = cp.r
    S = STEPS[cname]
    inv = lambda v: pow(v, -1, mod)
    rn = random.Random("verify_edges/%s" % cname)
    rand = lambda: rn.randrange(2, mod - 1)
    alpha, beta, gamma = rand(), rand(), rand()
    dpool = [rand() for _ in range(DELTA_POOL)]
    dlog_pool = [rand() for _ in range(D_POOL)]
    top_bit = 1 << (mod.bit_length() - 1)                  # bit 253 on BN254, bit 254 on BLS12-381
    cases = []

    def make_key(name, nd, w):
        return Key(cname, name, alpha, beta, gamma, [dpool[j % DELTA_POOL] for j in range(nd)], w)

    def ds_of(key, i):
        """the D logs of the i-th forged proof of a key: cycled from the pool, shifted by i"""
        return [dlog_pool[(3 * i + j) % D_POOL] for j in range(key.nd - 1)]

    def forge(key, x, i=0, **kw):
        return key.solve(x, kw.pop("a", None) or rand(), kw.pop("b", None) or rand(), kw.pop("ds", None) or ds_of(key, i), **kw)

    def add(name, group, key, proofs, inputs, premise, why, rand=None, modes=("proof", "batch"), oracle=(), contract=False):
        assert len(proofs) == len(inputs) and (rand is None or len(rand) == len(proofs))
        cases.append(dict(name=name, group=group, key=key, proofs=list(proofs), inputs=[list(x) for x in inputs], rand=rand,
                          want=[key.verdict(p, x) for p, x in zip(proofs, inputs)], premise=premise, why=why, modes=modes,
                          oracle=tuple(oracle), contract=contract))

    def bump(x, pos):
        y = list(x)
        y[pos] = (y[pos] + 1) % mod
        return y

    # -- 1. public inputs (k_verify_ic), nd = 2 ----------------------------------------------------------------------
    for nk in (0, 1, 3, 4, 5, 8, 9):
        key = make_key("nk%d" % nk, 2, [rand() for _ in range(nk + 1)])
        x0, x1 = [rand() for _ in range(nk)], [rand() for _ in range(nk)]
        p0, p1 = forge(key, x0, 0), forge(key, x1, 1)
        if nk:
            add("ic_nk%d" % nk, 1, key, [p0, p1, p1], [x0, x1, bump(x1, nk - 1)],
                lambda key=key, nk=nk: key.nk == nk, "nk = %d: the last group has %d of 4 scalars" % (nk, nk % 4 or 4),
                oracle=(0, 2) if nk == 3 else ())
        else:
            add("ic_nk0", 1, key, [p0, p1, p1.with_(c=p1.c + 1)], [x0, x1, x1], lambda key=key: key.n_abc == 1,
                "no public input: IC = abc[0], inputs == NULL", oracle=(0, 2))
    k5 = make_key("nk5_values", 2, [rand() for _ in range(6)])
    for nm, val in (("zero", 0), ("one", 1), ("r_minus_1", mod - 1), ("top_bit", top_bit + rn.randrange(mod - top_bit))):
        x = [val] * 5
        p = forge(k5, x)
        add("ic_inputs_" + nm, 1, k5, [p, p, p], [x, bump(x, 4), bump(x, 1)],
            lambda x=x, val=val, nm=nm: all(v == val for v in x) and 0 <= val < mod
            and (nm != "top_bit" or val >> (mod.bit_length() - 1) == 1),
            "every input %s; the second proof's input 4 and the third's input 1 are one more" % nm)
    w = [rand() for _ in range(6)]
    w[3] = 0
    key = make_key("nk5_w3_inf", 2, w)
    x = [rand() for _ in range(5)]
    p = forge(key, x)
    add("ic_base_inf", 1, key, [p, p, p], [x, bump(x, 2), bump(x, 3)],
        lambda key=key, x=x: key.w[3] == 0 and x[2] != 0 and key.ic(x) == key.ic(bump(x, 2)) != key.ic(bump(x, 3)),
        "abc[3] at infinity under a nonzero input: input 2 does not enter IC (the second proof still holds), input 3 does")
    w = [0] + [rand() for _ in range(5)]
    key = make_key("nk5_w0_inf", 2, w)
    p = forge(key, x)
    add("ic_abc0_inf", 1, key, [p, p], [x, bump(x, 0)], lambda key=key: key.w[0] == 0, "abc[0] at infinity")
    for nm, sign in (("dbl", 1), ("cancel", -1)):
        w = [rand() for _ in range(6)]
        w[2] = sign * w[1] % mod
        key = make_key("nk5_w2_%s" % nm, 2, w)
        x = [rand() for _ in range(5)]
        x[1] = x[0]
        p = forge(key, x)
        add("ic_chain_" + nm, 1, key, [p, p], [x, bump(x, 1)],
            lambda key=key, x=x, sign=sign: key.w[2] == sign * key.w[1] % mod and x[0] == x[1] != 0,
            "abc[2] = %sabc[1] under equal inputs: the chain's first two additions are P + P%s" % (
                "" if sign == 1 else "-", "" if sign == 1 else " then back from infinity (P + (-P))"))
    k8 = make_key("nk8_join", 2, [rand() for _ in range(9)])
    for nm, sign in (("dbl", 1), ("ic_inf", -1)):
        x = [rand() for _ in range(8)]
        first = (k8.w[0] + sum(x[k] * k8.w[k + 1] for k in range(4))) % mod
        x[7] = (sign * first - sum(x[k] * k8.w[k + 1] for k in range(4, 7))) * inv(k8.w[8]) % mod
        second = sum(x[k] * k8.w[k + 1] for k in range(4, 8)) % mod
        p = forge(k8, x)
        add("ic_join_" + nm, 1, k8, [p, p], [x, bump(x, 7)],
            lambda first=first, second=second, sign=sign, x=x: first != 0 and second == sign * first % mod
            and (k8.ic(x) == 0) == (sign == -1),
            "nk = 8: the second group's sum is %s the running total, the join %s" % (
                "" if sign == 1 else "minus", "doubles" if sign == 1 else "gives IC at infinity"),
            oracle=(0, 1) if sign == -1 else ())
    k1 = make_key("nk1_ic_inf", 2, [rand(), rand()])
    x = [-k1.w[0] * inv(k1.w[1]) % mod]
    p = forge(k1, x)
    add("ic_inf_nk1", 1, k1, [p, p], [x, bump(x, 0)], lambda x=x: k1.ic(x) == 0 and x[0] != 0, "nk = 1 and IC at infinity")

    # -- 2. members at infinity, each alone; the second copy differs in C ------------------------------------------------
    std = make_key("std", 2, [rand(), rand(), rand()])
    sx = [[rand(), rand()] for _ in range(8)]
    x = sx[0]
    x_ic0 = [x[0], -(std.w[0] + x[0] * std.w[1]) * inv(std.w[2]) % mod]
    inf_rows = [("a_inf", std.solve(x, 0, rand(), [rand()]), x, lambda p, x: p.a == 0 and p.b and p.c and p.ds[0]),
                ("b_inf", std.solve(x, rand(), 0, [rand()]), x, lambda p, x: p.b == 0 and p.a and p.c and p.ds[0]),
                ("c_inf", std.solve(x, None, rand(), [rand()], c=0, for_="a"), x, lambda p, x: p.c == 0 and p.a and p.b and p.ds[0]),
                ("d_inf", std.solve(x, rand(), rand(), [0]), x, lambda p, x: p.ds[0] == 0 and p.a and p.b and p.c),
                ("ic_inf", std.solve(x_ic0, rand(), rand(), [rand()]), x_ic0, lambda p, x: std.ic(x) == 0 and p.a and p.b and p.c),
                ("a_and_b_inf", std.solve(x, 0, 0, [rand()]), x, lambda p, x: p.a == 0 and p.b == 0 and p.c and p.ds[0])]
    for nm, p, xx, cond in inf_rows:
        add("member_" + nm, 2, std, [p, p.with_(c=p.c + 1)], [xx, xx], lambda p=p, xx=xx, cond=cond: bool(cond(p, xx)),
            nm + " alone, the equation holding; the copy's C is one generator more", oracle=(0, 1) if nm in ("b_inf", "c_inf") else ())

    # -- 3. commitment counts: M = nd + 2 members per product ---------------------------------------------------------------
    other = rand()
    nd_keys = {}
    for nd in (1, 2, 3, 14, 15, 16, 255):
        key = nd_keys[nd] = make_key("nd%d" % nd, nd, [rand(), rand(), rand()])
        ps = [forge(key, sx[i], i) for i in range(3)]
        if nd == 1:
            ps[1] = ps[1].with_(c=ps[1].c + 1)
        else:
            last = list(ps[1].ds)
            last[-1] = other
            first = list(ps[2].ds)
            first[0] = other
            ps[1], ps[2] = ps[1].with_(ds=last), ps[2].with_(ds=first)
        M = members_of(key)
        add("nd%d" % nd, 3, key, ps, sx[:3],
            lambda key=key, nd=nd, M=M: key.nd == nd and M == nd + 2 and {1: 3, 2: 4, 3: 5, 14: 16, 15: 17, 16: 18, 255: 257}[nd] == M,
            "M = %d members: %d first-level group(s), the last of %d" % (M, -(-M // WAVE_MEMBERS), M % WAVE_MEMBERS or WAVE_MEMBERS),
            oracle={3: (0, 1), 15: (0,)}.get(nd, ()))
    for nd in (3, 15):
        key = nd_keys[nd]
        base = [forge(key, sx[i], i) for i in range(4)]
        ps = [base[i % 4] for i in range(16)]
        xs = [sx[i % 4] for i in range(16)]
        for row, col in ((0, 0), (1, nd - 2), (15, nd - 2)):
            ds = list(ps[row].ds)
            ds[col] = off_curve(cname, 1, ds[col])
            ps[row] = ps[row].with_(ds=ds)
        add("nd%d_bad_d" % nd, 3, key, ps, xs,
            lambda ps=ps, nd=nd: [i for i, p in enumerate(ps) if not p.valid_points()] == [0, 1, 15]
            and isinstance(ps[0].ds[0], Bad) and isinstance(ps[1].ds[-1], Bad) and isinstance(ps[15].ds[-1], Bad)
            and len(ps[15].ds) == nd - 1,
            "an off-curve D at (0, 0), (1, last) and the matrix's last element: verdict 2 there and 1 on every other row")

    # -- 4. split launches with g > 1: count * S rows cross 65535 ------------------------------------------------------------
    key = nd_keys[15]
    base = [forge(key, sx[i], i) for i in range(8)]
    n_big = 1000
    ps = [base[i % 8] for i in range(n_big)]
    xs = [sx[i % 8] for i in range(n_big)]
    for row in (100, 990):
        ps[row] = ps[row].with_(c=ps[row].c + 1)
    add("split_nd15_n1000", 4, key, ps, xs,
        lambda key=key: members_of(key) == 17 and 100 * S + S <= GRID_ROWS < 990 * S and n_big * S > GRID_ROWS and n_big <= CHUNK,
        "n = 1000, M = 17 (two groups): the wrong row 100 is in the first launch, row 990 lies past the split", modes=("proof",))

    # -- 5. batch product bounds: M = m + nd + 1 ---------------------------------------------------------------------------
    base = [forge(std, sx[i], i) for i in range(8)]
    wrong = [p.with_(c=p.c + 1) for p in base]
    for m in (13, 14, 253, 254):
        for nm, bad in (("valid", None), ("last_wrong", m - 1)):
            ps = [wrong[i % 8] if i == bad else base[i % 8] for i in range(m)]
            add("batch_m%d_%s" % (m, nm), 5, std, ps, [sx[i % 8] for i in range(m)],
                lambda m=m: m + std.nd + 1 == {13: 16, 14: 17, 253: 256, 254: 257}[m],
                "batch product of M = %d members" % (m + std.nd + 1))
    for bad in (1023, 1024):
        n = 1025
        ps = [wrong[i % 8] if i == bad else base[i % 8] for i in range(n)]
        add("batch_seam_%d" % bad, 5, std, ps, [sx[i % 8] for i in range(n)],
            lambda bad=bad: CHUNK == 1024 and (bad // CHUNK, bad % CHUNK) in ((0, 1023), (1, 0)),
            "n = 1025: the wrong proof is the %s; the other chunk passes by its batch equation" % (
                "last of chunk 0" if bad == 1023 else "only row of chunk 1"))

    # -- 6. explicit batching scalars --------------------------------------------------------------------------------------
    p0, p1, p2 = base[0], base[1], base[2]
    x0, x1, x2 = sx[0], sx[1], sx[2]
    full = [rand() for _ in range(3)]
    for nm, rr in (("r_minus_1", [mod - 1] * 3), ("two_128", [1 << 128] * 3), ("full_width", full)):
        add("rand_%s" % nm, 6, std, [p0, p1, p2], [x0, x1, x2], lambda rr=rr: all(0 < v < mod and v >> 127 for v in rr),
            "three valid proofs under r_i = %s" % nm, rand=rr)
        add("rand_%s_wrong" % nm, 6, std, [p0, wrong[1], p2], [x0, x1, x2], lambda rr=rr: all(0 < v < mod for v in rr),
            "the same with the middle proof wrong", rand=rr)
        # visible from outside: tampers t G and -t (r_0 / r_1) G on C cancel under exactly these r_i (distinct for full_width)
        r0, r1 = (rr[0], rr[1]) if nm == "full_width" else (rr[0], rr[0])
        t = rand()
        pair = [p0.with_(c=p0.c + t), p1.with_(c=p1.c - t * r0 * inv(r1))]
        add("rand_%s_cancelling" % nm, 6, std, pair, [x0, x1],
            lambda pair=pair, r0=r0, r1=r1: (r0 * std.defect(pair[0], x0) + r1 * std.defect(pair[1], x1)) % mod == 0
            and std.defect(pair[0], x0) != 0,
            "two wrong proofs whose defects cancel under r_i = %s: the batch equation holds (caller contract)" % nm,
            rand=[r0, r1], contract=True)
    add("rand_sums_vanish_same_proof", 6, std, [p0, p0], [x0, x0], lambda: (1 + mod - 1) % mod == 0,
        "(1, r - 1) over two identical valid proofs: every sum is infinity or 0, the right side e(alpha, beta)^0",
        rand=[1, mod - 1])
    add("rand_sum_r_zero", 6, std, [p0, p1], [x0, x1],
        lambda: (1 + mod - 1) % mod == 0 and (x0[0] - x1[0]) % mod != 0 and (p0.c - p1.c) % mod != 0,
        "(1, r - 1) over two different valid proofs: sum r_i == 0 only", rand=[1, mod - 1])
    ra = rand()
    rb = -ra * x0[0] * inv(x1[0]) % mod
    add("rand_input_sum_zero", 6, std, [p0, p1], [x0, x1],
        lambda: (ra * x0[0] + rb * x1[0]) % mod == 0 and (ra + rb) % mod != 0 and (ra * x0[1] + rb * x1[1]) % mod != 0,
        "sum r_i x_i0 == 0: abc[1] meets a zero coefficient", rand=[ra, rb])
    comp = [p0.with_(c=p0.c + 1), p1.with_(c=p1.c - 1)]
    add("rand_complementary_distinct", 6, std, comp, [x0, x1], lambda: (full[0] - full[1]) % mod != 0,
        "C_0 + G and C_1 - G under distinct r_i: [0, 0]", rand=full[:2])
    add("rand_complementary_equal", 6, std, comp, [x0, x1],
        lambda: (std.defect(comp[0], x0) + std.defect(comp[1], x1)) % mod == 0,
        "the same pair under equal r_i: the batch equation holds, so batch mode accepts (caller contract: the r_i are random)",
        rand=[full[0], full[0]], contract=True)
    # e(alpha, beta) to the power of the wrong coefficient: a proof forged for alpha beta x_0 in place of alpha beta
    scaled = p0.with_(c=p0.c - (x0[0] - 1) * alpha * beta * inv(std.deltas[-1]))
    add("rand_alpha_beta_power", 6, std, [scaled], [x0],
        lambda: (scaled.a * scaled.b - std.rhs(scaled, x0) - (x0[0] - 1) * alpha * beta) % mod == 0 and x0[0] != 1,
        "one proof that holds with e(alpha, beta)^(x_0) on the right: the exponent must be sum r_i, not sum r_i x_i0",
        rand=[1])

    # -- 7. a zero r_i: the chunk takes the per-proof path -----------------------------------------------------------------
    add("rand_zero_on_wrong", 7, std, [p0, wrong[1], p2], [x0, x1, x2], lambda: True,
        "r_1 == 0 on a wrong proof: its terms vanish from both sides of the batch equation", rand=[full[0], 0, full[2]])
    add("rand_zero_on_valid", 7, std, [p0, wrong[1], p2], [x0, x1, x2], lambda: True,
        "r_0 == 0 on a valid proof beside a wrong one", rand=[0, full[1], full[2]])
    add("rand_zero_all_valid", 7, std, [p0, p1, p2], [x0, x1, x2], lambda: True,
        "r_2 == 0 and every proof valid", rand=[full[0], full[1], 0])

    # -- 8. points of the cofactor part inside proofs --------------------------------------------------------------------------
    c1, c2 = cofactor_points(cname, 1), cofactor_points(cname, 2)
    v2 = Bad(c2["V"][min(c2["V"])], "order %d on the twist" % min(c2["V"]))
    ps = [p0, p1.with_(b=v2), p2, base[3], base[4], base[5]]
    bad_rows = [1]
    if c1:
        ls = sorted(c1["V"])
        ps[3] = ps[3].with_(a=Bad(c1["V"][ls[0]], "order %d" % ls[0]))
        ps[5] = ps[5].with_(ds=[Bad(c1["V"][ls[-1]], "order %d" % ls[-1])])
        bad_rows = [1, 3, 5]
    add("cofactor_members", 8, std, ps, sx[:6],
        lambda ps=ps, bad_rows=bad_rows: [i for i, p in enumerate(ps) if not p.valid_points()] == bad_rows,
        "a small-order point as B%s: verdict 2 there, 1 beside it" % (", as A and as D" if c1 else " (G1 has cofactor 1)"))
    return cases


_case_lists = {}


def cases(cname):
    if cname not in _case_lists:
        _case_lists[cname] = _cases(cname)
        names = [c["name"] for c in _case_lists[cname]]
        assert len(set(names)) == len(names)
    return _case_lists[cname]


def case(cname, name):
    return next(c for c in cases(cname) if c["name"] == name)
