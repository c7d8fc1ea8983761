"""GPU: the wave-parallel Fq12 code of csrc/pairing_wave.cuh (DPP quad sums, LDS slots, generated PRE / POST tables) in
isolation, against the tower oracle (oracle/pyref/pairing.py).  It cannot be compiled for the host; the pairing tests
reach it only end to end on generic elements, where every table entry contributes at once.  Here:

  * all 144 products e_i e_j of basis elements (and with (p - 1) e_i): each exercises a handful of table entries alone;
  * structured operands, also shifted by +p into the lazy range [p, 2p) that LDS values may hold;
  * every aliasing mode `mul` documents (dst == a, dst == b, a == b == dst) and the in-place forms the final
    exponentiation uses of sqr, cyc_sqr, conj and frob;
  * cyc_sqr on elements of the cyclotomic subgroup only (it is specified nowhere else);
  * the 13th (padding) slot of every result, which the operand tables read as zero.

One 64-lane workgroup per element (tests/device_shim/field_dev_shim.hip), both shim builds; all comparisons exact.
"""
import random

import pytest

from oracle.pyref import pairing
from oracle.pyref.params import CURVES
from tests import dev_shim as ds
from tests import field_edges as fe

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "bls12_381"]
FQ = {"bn254": "BN254_FQ", "bls12_381": "BLS12_381_FQ"}


@pytest.fixture(scope="module", params=["asm", "noasm"])
def shim(request):
    return ds.load(request.param)


class Wave:
    """plain Fq12 coefficient lists <-> what the shim takes and gives"""

    def __init__(self, shim, cname):
        self.shim, self.cname = shim, cname
        self.cid = CURVES[cname].cid
        self.f = fe.FIELDS[FQ[cname]]
        self.T = pairing.tower(cname)
        assert self.T.p == self.f.p and self.f.lazy
        self.nb = 4 * self.f.N

    def enc(self, flat, shift=False):
        f = self.f
        return tuple(c % f.p * f.R % f.p + (f.p if shift else 0) for c in flat)

    def run(self, op, xs, ys=None, alias=ds.ALIAS_NONE, shift=False):
        """-> list of 12-coefficient lists (plain integers); asserts the padding slot of every result"""
        a = [self.enc(x, shift) for x in xs]
        b = None if ys is None else [self.enc(y, shift) for y in ys]
        out = self.shim.wave_op(self.cid, op, self.nb, a, b, alias)
        f = self.f
        for k, o in enumerate(out):
            assert o[12] == 0, "%s op %d alias %d #%d: padding slot reads %#x" % (self.cname, op, alias, k, o[12])
            assert all(c < f.p for c in o)
        return [[c * f.Rinv % f.p for c in o[:12]] for o in out]

    def want(self, fn, xs, ys=None):
        T = self.T
        if ys is None:
            return [T.f12_flat(fn(T.f12_from_flat(x))) for x in xs]
        return [T.f12_flat(fn(T.f12_from_flat(x), T.f12_from_flat(y))) for x, y in zip(xs, ys)]


_cache = {}


def randoms(cname, n=32, tag="rnd"):
    key = (cname, n, tag)
    if key not in _cache:
        rnd = random.Random("%s/%s" % (cname, tag))
        q = CURVES[cname].q
        _cache[key] = [[rnd.randrange(q) for _ in range(12)] for _ in range(n)]
    return _cache[key]


def sparse_elements(cname):
    """few non-zero coefficients: single ones, one Fq2 / Fq6 half, the shapes of the line values"""
    q = CURVES[cname].q
    rnd = random.Random(cname + "/sparse")
    out = []
    for k in range(12):
        e = [0] * 12
        e[k] = rnd.randrange(1, q)
        out.append(e)
    for idx in ((0, 1), (6, 7, 8, 9, 10, 11), (0, 1, 2, 3, 4, 5), (0, 1, 6, 7, 8, 9), (0, 1, 2, 3, 8, 9), (0, 11)):
        e = [0] * 12
        for k in idx:
            e[k] = rnd.randrange(1, q)
        out.append(e)
    return out


def basis(k, c=1):
    e = [0] * 12
    e[k] = c
    return e


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_basis_products(shim, cname):
    W = Wave(shim, cname)
    q = W.f.p
    for c in (1, q - 1):
        xs = [basis(i, c) for i in range(12) for _j in range(12)]
        ys = [basis(j) for _i in range(12) for j in range(12)]
        got, want = W.run(ds.W_MUL, xs, ys), W.want(W.T.f12_mul, xs, ys)
        bad = [(k // 12, k % 12) for k in range(144) if got[k] != want[k]]
        assert not bad, "%s/%s: %d e_i e_j products differ (c = %s): (i, j) = %s" % (
            shim.variant, cname, len(bad), "1" if c == 1 else "p-1", bad[:12])
    # both factors (p - 1) e_k, and the squaring path on the same
    xs = [basis(i, q - 1) for i in range(12)]
    assert W.run(ds.W_SQR, xs) == W.want(W.T.f12_sqr, xs)


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_structured_operands(shim, cname):
    W = Wave(shim, cname)
    q = W.f.p
    one, zero, full = basis(0), [0] * 12, [q - 1] * 12
    structured = [full, one, zero]
    xs = [x for x in structured for _y in structured]
    ys = [y for _x in structured for y in structured]
    rx, ry = randoms(cname), randoms(cname, tag="rnd-b")
    for shift in (False, True):                 # True: every coefficient of both operands enters as its value + p
        assert W.run(ds.W_MUL, xs, ys, shift=shift) == W.want(W.T.f12_mul, xs, ys), (shim.variant, cname, shift)
        assert W.run(ds.W_SQR, structured, shift=shift) == W.want(W.T.f12_sqr, structured), (shim.variant, cname, shift)
        assert W.run(ds.W_MUL, rx, ry, shift=shift) == W.want(W.T.f12_mul, rx, ry), (shim.variant, cname, shift)
        assert W.run(ds.W_SQR, rx, shift=shift) == W.want(W.T.f12_sqr, rx), (shim.variant, cname, shift)
    # random against structured, both orders
    assert W.run(ds.W_MUL, rx[:3], structured) == W.want(W.T.f12_mul, rx[:3], structured)
    assert W.run(ds.W_MUL, structured, rx[:3]) == W.want(W.T.f12_mul, structured, rx[:3])


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_aliasing(shim, cname):
    W = Wave(shim, cname)
    T = W.T
    rx, ry = randoms(cname), randoms(cname, tag="rnd-b")
    want = W.want(T.f12_mul, rx, ry)
    for alias in (ds.ALIAS_NONE, ds.ALIAS_A, ds.ALIAS_B):
        assert W.run(ds.W_MUL, rx, ry, alias=alias) == want, (shim.variant, cname, alias)
    assert W.run(ds.W_MUL, rx, ry, alias=ds.ALIAS_ALL) == W.want(T.f12_sqr, rx)        # a == b == dst
    # the in-place forms the final exponentiation and the GT powers use
    assert W.run(ds.W_SQR, rx, alias=ds.ALIAS_A) == W.want(T.f12_sqr, rx)
    assert W.run(ds.W_CONJ, rx, alias=ds.ALIAS_A) == W.want(T.f12_conj, rx)
    for k, op in ((1, ds.W_FROB1), (2, ds.W_FROB2), (3, ds.W_FROB3)):
        assert W.run(op, rx, alias=ds.ALIAS_A) == W.want(lambda x, k=k: T.f12_frob(x, k), rx), (shim.variant, cname, k)


def cyclotomic(cname):
    """f^((q^6 - 1)(q^2 + 1)) for 16 random f, one, and e(G1, G2)"""
    if ("cyc", cname) not in _cache:
        T, cp = pairing.tower(cname), CURVES[cname]
        out = []
        for flat in randoms(cname, 16, "cyc"):
            f = T.f12_from_flat(flat)
            t = T.f12_mul(T.f12_conj(f), T.f12_inv(f))
            out.append(T.f12_flat(T.f12_mul(T.f12_frob(t, 2), t)))
        out.append(basis(0))
        out.append(T.f12_flat(T.pairing(cp.g1_gen, cp.g2_gen)))
        _cache[("cyc", cname)] = out
    return _cache[("cyc", cname)]


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_cyclotomic_square(shim, cname):
    W = Wave(shim, cname)
    xs = cyclotomic(cname)
    want = W.want(W.T.f12_sqr, xs)
    # the inputs are in the subgroup: conj(x) x = 1
    assert all(T12 == basis(0) for T12 in W.want(lambda x: W.T.f12_mul(x, W.T.f12_conj(x)), xs))
    assert W.run(ds.W_CYC_SQR, xs) == want, (shim.variant, cname)
    assert W.run(ds.W_CYC_SQR, xs, alias=ds.ALIAS_A) == want, (shim.variant, cname, "in place")
    assert W.run(ds.W_CYC_SQR, xs, shift=True) == want, (shim.variant, cname, "lazy")


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_conj_frobenius_and_inverse(shim, cname):
    W = Wave(shim, cname)
    T = W.T
    xs = randoms(cname, 16) + sparse_elements(cname)
    for shift in (False, True):
        assert W.run(ds.W_CONJ, xs, shift=shift) == W.want(T.f12_conj, xs), (shim.variant, cname, shift)
        for k, op in ((1, ds.W_FROB1), (2, ds.W_FROB2), (3, ds.W_FROB3)):
            assert W.run(op, xs, shift=shift) == W.want(lambda x, k=k: T.f12_frob(x, k), xs), (shim.variant, cname, k, shift)
    # conj of zero coefficients stays a representative of zero; inv(one) = one
    assert W.run(ds.W_CONJ, [[0] * 12], shift=True) == [[0] * 12]
    assert W.run(ds.W_INV, [basis(0)]) == [basis(0)]
    inv = W.run(ds.W_INV, xs)
    assert inv == W.want(T.f12_inv, xs), (shim.variant, cname)
    assert W.run(ds.W_INV, xs, shift=True) == inv
    assert W.run(ds.W_MUL, xs, inv) == [basis(0)] * len(xs)            # a inv(a) = one through the device mul


def test_the_shim_refuses_alias_modes_an_op_does_not_have(shim):
    buf = bytes(13 * 48)
    assert shim.lib.dshim_wave_op(0, ds.W_INV, buf, buf, buf, 1, ds.ALIAS_A) != 0    # inv: dst, a, tmp distinct
    assert shim.lib.dshim_wave_op(0, ds.W_SQR, buf, buf, buf, 1, ds.ALIAS_B) != 0
    assert shim.lib.dshim_wave_op(2, ds.W_MUL, buf, buf, buf, 1, 0) != 0
