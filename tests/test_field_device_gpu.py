"""GPU: the DEVICE build of csrc/field.cuh, operand by operand, against Python integers (Fq2: the tower oracle's f2_*).

The host-compiled shim (tests/host_shim) never runs the inline assembly of mont_asm.h nor the lazy [0, 2p) branches;
tests/device_shim/field_dev_shim.hip compiles both for gfx950, as shipped ("asm") and with -DHK_NO_ASM_MUL ("noasm":
the C++ fallback under the same lazy representation, dead code otherwise).  Operands are the edge sets of
tests/field_edges.py, loaded as raw limbs so that representatives in [p, 2p) sit on either side.  Every comparison is
exact: the canonicalised output equals the integer result, the raw register output is below the representative bound
B and congruent to it.  Nothing is compared with the host C++ build of the same code.
"""
import random

import pytest

from oracle.pyref import pairing
from tests import dev_shim as ds
from tests import field_edges as fe

pytestmark = pytest.mark.gpu

FIELD_NAMES = list(fe.FIELDS)
FP2 = {"bn254": (4, "BN254_FQ"), "bls12_381": (5, "BLS12_381_FQ")}


@pytest.fixture(scope="module", params=["asm", "noasm"])
def shim(request):
    return ds.load(request.param)


_pairs = {}


def pairs_of(f):
    if f.name not in _pairs:
        ps = fe.pair_list(f) + fe.lazy_alias_pairs(f)
        _pairs[f.name] = ([a for a, _b in ps], [b for _a, b in ps])
    return _pairs[f.name]


def check(f, got0, got1, want, what):
    """got0: canonicalised output, got1: raw registers; want: integers mod p (one component list per element for Fq2)"""
    assert len(got0) == len(got1) == len(want)
    for k, (g0, g1, w) in enumerate(zip(got0, got1, want)):
        if isinstance(w, int):
            g0, g1, w = (g0,), (g1,), (w,)
        for c0, c1, cw in zip(g0, g1, w):
            assert c0 == cw, "%s #%d: canonical output %#x, want %#x" % (what, k, c0, cw)
            assert c1 < f.B and (c1 - cw) % f.p == 0, "%s #%d: raw output %#x (B = %#x), want %#x" % (what, k, c1, f.B, cw)


def run_both(shim, fid, op, nb, a, b=None, chain=0):
    return (shim.field_op(fid, op, nb, a, b, raw=0, chain=chain), shim.field_op(fid, op, nb, a, b, raw=1, chain=chain))


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_base_field_binary_and_unary_ops(shim, name):
    f = fe.FIELDS[name]
    fid, nb, p = fe.FIELD_IDS[name], 4 * f.N, f.p
    a, b = pairs_of(f)
    what = "%s/%s " % (shim.variant, name)
    check(f, *run_both(shim, fid, ds.ADD, nb, a, b), [(x + y) % p for x, y in zip(a, b)], what + "add")
    check(f, *run_both(shim, fid, ds.SUB, nb, a, b), [(x - y) % p for x, y in zip(a, b)], what + "sub")
    check(f, *run_both(shim, fid, ds.MUL, nb, a, b), [x * y * f.Rinv % p for x, y in zip(a, b)], what + "mul")
    u = fe._dedup(fe.all_values(f) + a[-512:] + b[-512:])
    check(f, *run_both(shim, fid, ds.SQR, nb, u), [x * x * f.Rinv % p for x in u], what + "sqr")
    check(f, *run_both(shim, fid, ds.DBL, nb, u), [2 * x % p for x in u], what + "dbl")
    check(f, *run_both(shim, fid, ds.CANON, nb, u), [x % p for x in u], what + "canon")
    # neg: -0 = 0 and, on a lazy field, -p is a representative of 0 below the bound
    g0, g1 = run_both(shim, fid, ds.NEG, nb, u)
    check(f, g0, g1, [(-x) % p for x in u], what + "neg")
    assert g1[u.index(0)] % p == 0 and (not f.lazy or g1[u.index(p)] % p == 0)
    # halve: 2 halve(x) = x
    h0, h1 = run_both(shim, fid, ds.HALVE, nb, u)
    check(f, h0, h1, [x * pow(2, -1, p) % p for x in u], what + "halve")
    assert all((2 * h - x) % p == 0 and h < f.B for h, x in zip(h1, u))


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_base_field_predicates(shim, name):
    f = fe.FIELDS[name]
    fid, nb, p = fe.FIELD_IDS[name], 4 * f.N, f.p
    a, b = pairs_of(f)
    u = fe.all_values(f)
    assert shim.field_op(fid, ds.IS_ZERO, nb, u) == [1 if x % p == 0 else 0 for x in u]
    assert sum(x % p == 0 for x in u) == (2 if f.lazy else 1)                 # 0, and p where it is a representative
    eq = shim.field_op(fid, ds.EQ, nb, a, b)
    assert eq == [1 if (x - y) % p == 0 else 0 for x, y in zip(a, b)]
    assert sum(eq) > (100 if f.lazy else 50) and sum(1 for x, y, e in zip(a, b, eq) if e and x != y) >= (64 if f.lazy else 0)


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_base_field_montgomery_conversions_and_inverse(shim, name):
    f = fe.FIELDS[name]
    fid, nb, p = fe.FIELD_IDS[name], 4 * f.N, f.p
    what = "%s/%s " % (shim.variant, name)
    u = fe.all_values(f)
    t0, t1 = run_both(shim, fid, ds.TO_MONT, nb, u)
    check(f, t0, t1, [x * f.R % p for x in u], what + "to_mont")
    f0, f1 = run_both(shim, fid, ds.FROM_MONT, nb, u)
    check(f, f0, f1, [x * f.Rinv % p for x in u], what + "from_mont")
    assert f1 == f0, "from_mont leaves a canonical integer in the registers (its limbs get read as bits)"
    # from_mont(to_mont(x)) = x, fed the raw (possibly lazy) output of to_mont
    assert shim.field_op(fid, ds.FROM_MONT, nb, t1, raw=1) == [x % p for x in u]
    rnd = random.Random("inv/" + name)
    xs = [0, 1, 2, p - 1, f.one] + ([p, p + 1] if f.lazy else []) + [rnd.randrange(1, f.B) for _ in range(57)]
    want = [0 if x % p == 0 else pow(x, -1, p) * f.R * f.R % p for x in xs]
    check(f, *run_both(shim, fid, ds.INV, nb, xs), want, what + "fp_inv")


def chain_ref(x, y, n, p, Rinv):
    r = x
    for _ in range(n):
        r = (r * y * Rinv + x - 2 * y) % p
    return r


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_base_field_chain_keeps_the_bound(shim, name):
    """r <- r y + x - 2 y with nothing canonicalised in between: the lazy bound has to close under composition"""
    f = fe.FIELDS[name]
    fid, nb, p = fe.FIELD_IDS[name], 4 * f.N, f.p
    e = fe.edge_values(f)
    rnd = random.Random("chain/" + name)
    ps = [(x, y) for x in e for y in e] + [(rnd.randrange(f.B), rnd.randrange(f.B)) for _ in range(64)]
    a, b = [x for x, _y in ps], [y for _x, y in ps]
    for n in (64, 1000):
        want = [chain_ref(x, y, n, p, f.Rinv) for x, y in ps]
        check(f, *run_both(shim, fid, ds.CHAIN, nb, a, b, chain=n), want, "%s/%s chain %d" % (shim.variant, name, n))


# ---- Fq2 -------------------------------------------------------------------------------------------------------------
_fp2 = {}


def fp2_pairs(f):
    if f.name not in _fp2:
        ps = fe.fp2_pair_list(f)
        _fp2[f.name] = ([a for a, _b in ps], [b for _a, b in ps])
    return _fp2[f.name]


@pytest.mark.parametrize("cname", list(FP2))
def test_fq2_ops(shim, cname):
    fid, name = FP2[cname]
    f = fe.FIELDS[name]
    T = pairing.tower(cname)
    assert T.p == f.p
    nb, p = 4 * f.N, f.p
    a, b = fp2_pairs(f)
    # sqr goes through (a0 + a1)(a0 - a1): a0 = a1, (p - 1, 1) and lazy components have to be among the operands
    assert (f.p - 1, 1) in a and (f.p - 1, f.p - 1) in a and (f.p + 1, f.p) in a and (f.B - 1, f.B - 1) in a
    what = "%s/%s " % (shim.variant, cname)
    mont = lambda z: T.f2_scale(z, f.Rinv)
    check(f, *run_both(shim, fid, ds.ADD, nb, a, b), [T.f2_add(x, y) for x, y in zip(a, b)], what + "f2 add")
    check(f, *run_both(shim, fid, ds.SUB, nb, a, b), [T.f2_sub(x, y) for x, y in zip(a, b)], what + "f2 sub")
    check(f, *run_both(shim, fid, ds.MUL, nb, a, b), [mont(T.f2_mul(x, y)) for x, y in zip(a, b)], what + "f2 mul")
    u = fe._dedup(a)
    check(f, *run_both(shim, fid, ds.SQR, nb, u), [mont(T.f2_sqr(x)) for x in u], what + "f2 sqr")
    check(f, *run_both(shim, fid, ds.NEG, nb, u), [T.f2_neg(x) for x in u], what + "f2 neg")
    check(f, *run_both(shim, fid, ds.DBL, nb, u), [T.f2_dbl(x) for x in u], what + "f2 dbl")
    check(f, *run_both(shim, fid, ds.HALVE, nb, u), [T.f2_scale(x, T.two_inv) for x in u], what + "f2 halve")
    check(f, *run_both(shim, fid, ds.CANON, nb, u), [(x[0] % p, x[1] % p) for x in u], what + "f2 canon")
    assert [z[0] for z in shim.field_op(fid, ds.IS_ZERO, nb, u)] == [1 if x[0] % p == 0 and x[1] % p == 0 else 0 for x in u]
    assert [z[0] for z in shim.field_op(fid, ds.EQ, nb, a, b)] == [
        1 if (x[0] - y[0]) % p == 0 and (x[1] - y[1]) % p == 0 else 0 for x, y in zip(a, b)]
    # inverse: a^-1 in Montgomery form, (0, 0) -> (0, 0)
    xs = u[::7]
    R2 = f.R * f.R % p
    want = [(0, 0) if x[0] % p == 0 and x[1] % p == 0 else T.f2_scale(T.f2_inv(x), R2) for x in xs]
    check(f, *run_both(shim, fid, ds.INV, nb, xs), want, what + "f2 inv")


@pytest.mark.parametrize("cname", list(FP2))
def test_fq2_chain_keeps_the_bound(shim, cname):
    fid, name = FP2[cname]
    f = fe.FIELDS[name]
    T = pairing.tower(cname)
    a, b = fp2_pairs(f)
    a, b = a[::97] + a[-24:], b[::97] + b[-24:]
    for n in (64, 1000):
        want = []
        for x, y in zip(a, b):
            r, y2 = x, T.f2_dbl(y)
            for _ in range(n):
                r = T.f2_sub(T.f2_add(T.f2_scale(T.f2_mul(r, y), f.Rinv), x), y2)
            want.append(r)
        check(f, *run_both(shim, fid, ds.CHAIN, 4 * f.N, a, b, chain=n), want, "%s/%s f2 chain %d" % (shim.variant, cname, n))


def test_the_shim_refuses_what_it_does_not_implement(shim):
    out = bytes(64)
    assert shim.lib.dshim_field_op(4, ds.TO_MONT, out, out, out, 1, 0, 0) != 0       # no Montgomery conversion on Fq2
    assert shim.lib.dshim_field_op(9, ds.ADD, out, out, out, 1, 0, 0) != 0
    assert shim.lib.dshim_field_op(0, 99, out, out, out, 1, 0, 0) != 0
