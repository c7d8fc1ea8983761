"""GPU: hk_multi_pairing / hk_pairing_products / hk_pairing_pairs at the seams of PairRun<P>::run that the shapes of
tests/test_pairing_gpu.py (n in {0, 1, 2, 64, 1024}) miss:

  * n in {15, 16, 17, 33}: a partial last group of the 16-ary product tree, a last group of one element, three groups - bit
    for bit against the oracle, with infinities at a group's first slot, over a whole group and in every slot;
  * n in {255, 256, 257} (257: 17 first-level values, so the SECOND level has a group of one) and n = 4097 with four rhs
    vectors (four tree levels, and 4097 * 4 * 4 lanes > 65 536: the lane-per-point form of k_pair_lines without any
    environment setting) through bilinearity: all points are known multiples of the generators, so every product must be
    e(G, H)^(sum a_i b_i) over the slots where neither member is infinity;
  * the lane-per-point form at n in {17, 33} (HK_ENDO_NO_QUAD, read per call), byte for byte the quad form's result;
  * infinities in ONE lhs / rhs vector of a 3 x 2 grid, and the same through a pair list;
  * host, device and mixed pointers.

The oracle side of the bit-exact grids multiplies per-pair Miller values (T.multi_miller_loop of one pair, cached): the
Miller value of a multi-pairing is the product of its pairs' values in a commutative field, exactly."""
import random

import numpy as np
import pytest

from oracle.pyref import curve, pairing
from oracle.pyref.params import CURVES
from tests.test_pairing_cpu import Enc

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "bls12_381"]
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _ctx(cname, ctx_bn254, ctx_bls):
    return ctx_bn254 if cname == "bn254" else ctx_bls


class Ora:
    def __init__(self, cname):
        self.cname = cname
        self.cp = cp = CURVES[cname]
        self.T = pairing.tower(cname)
        self.E = Enc(cp)
        G1, G2 = curve.G1(cp), curve.G2(cp)
        rnd = random.Random(cname + "/edges")
        self.ps = [G1.mul(cp.g1_gen, rnd.randrange(1, cp.r)) for _ in range(33)]
        self.qs = [G2.mul(cp.g2_gen, rnd.randrange(1, cp.r)) for _ in range(33)]
        self._miller = {}

    def g1(self, ps): return np.frombuffer(b"".join(self.E.g1(p) for p in ps), np.uint8)
    def g2(self, qs): return np.frombuffer(b"".join(self.E.g2(q) for q in qs), np.uint8)
    def dec(self, arr): return self.E.f12_dec(np.ascontiguousarray(arr).tobytes())

    def miller(self, i, j):
        """Miller value of (ps[i], qs[j])"""
        if (i, j) not in self._miller:
            self._miller[(i, j)] = self.T.multi_miller_loop([(self.ps[i], self.qs[j])])
        return self._miller[(i, j)]

    def product(self, li, ri):
        """li, ri: indices into ps / qs (None: infinity) -> the flat GT value of prod_k e(ps[li[k]], qs[ri[k]])"""
        f = self.T.f12_one()
        for i, j in zip(li, ri):
            if i is not None and j is not None:
                f = self.T.f12_mul(f, self.miller(i, j))
        return self.T.f12_flat(self.T.final_exponentiation(f))


def ora(cname):
    return cached(("ora", cname), lambda: Ora(cname))


def small_cases(n):
    """(name, infinity slots of the G1 vector, of the G2 vector)"""
    cases = [("index 0 (G1), index 16 (G2)", {0}, {16} if n > 16 else set())]
    if n == 33:
        cases.append(("group 1", set(range(16, 32, 2)), set(range(17, 32, 2))))
    cases.append(("every slot", set(range(0, n, 2)) | {1}, set(range(1, n, 2))))
    return cases


def small_vectors(O, n, inf1, inf2):
    return [None if i in inf1 else O.ps[i] for i in range(n)], [None if i in inf2 else O.qs[i] for i in range(n)]


def small_want(O, n, name, inf1, inf2):
    def make():
        ps, qs = small_vectors(O, n, inf1, inf2)
        return O.T.f12_flat(O.T.multi_pairing(list(zip(ps, qs))))
    return cached(("small", O.cname, n, name), make)


@pytest.mark.parametrize("n", [15, 16, 17, 33])
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_partial_groups_with_infinities_bit_exact(cname, n, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    O = ora(cname)
    for name, inf1, inf2 in small_cases(n):
        ps, qs = small_vectors(O, n, inf1, inf2)
        got = O.dec(ctx.multi_pairing(O.g1(ps), O.g2(qs), n=n))
        assert got == small_want(O, n, name, inf1, inf2), (cname, n, name)
        if name == "every slot":
            assert got == O.T.f12_flat(O.T.f12_one())


@pytest.mark.parametrize("n", [17, 33])
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_lane_per_point_lines_at_small_sizes(cname, n, ctx_bn254, ctx_bls, monkeypatch):
    """HK_ENDO_NO_QUAD makes PairRun<P>::run (which reads it at every call) take k_pair_lines<Fp2<P>> where 4 n n_r lanes
    would fit the quad form.  The MSM paths read the same variable, so every input exists before it is set."""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    O = ora(cname)
    cases = small_cases(n)
    inputs = [(O.g1(ps), O.g2(qs)) for ps, qs in (small_vectors(O, n, i1, i2) for _, i1, i2 in cases)]
    lhs = [O.g1([None if i == 3 else O.ps[i] for i in range(n)]), O.g1(O.ps[n - 1::-1])]
    rhs = [O.g2(O.qs[:n]), O.g2([None if i == 16 else O.qs[32 - i] for i in range(n)])]
    quad = [ctx.multi_pairing(a, b, n=n) for a, b in inputs]
    quad_grid = ctx.pairing_products(lhs, rhs, n=n)
    with monkeypatch.context() as m:
        m.setenv("HK_ENDO_NO_QUAD", "1")
        lane = [ctx.multi_pairing(a, b, n=n) for a, b in inputs]
        lane_grid = ctx.pairing_products(lhs, rhs, n=n)
    for (name, i1, i2), x, y in zip(cases, quad, lane):
        assert O.dec(y) == small_want(O, n, name, i1, i2), (cname, n, name)
        assert np.array_equal(x, y), (cname, n, name)
    assert np.array_equal(quad_grid, lane_grid)
    assert O.dec(lane_grid[0, 1]) == O.product([None if i == 3 else i for i in range(n)],
                                                [None if i == 16 else 32 - i for i in range(n)])


def grid_vectors(cname):
    """3 lhs x 2 rhs vectors of 17 slots as indices into a pool of 4 G1 and 4 G2 points (16 Miller values in all).  lhs
    infinities in vector 0 only (slots 4 and 16), rhs infinities in vector 1 only (slots 4 - the same index - and 9)."""
    rnd = random.Random(cname + "/grid")
    n = 17
    li = [[rnd.randrange(4) for _ in range(n)] for _ in range(3)]
    ri = [[rnd.randrange(4) for _ in range(n)] for _ in range(2)]
    li[0][4] = li[0][16] = None
    ri[1][4] = ri[1][9] = None
    return n, li, ri


def grid_arrays(O, li, ri):
    return ([O.g1([None if i is None else O.ps[i] for i in v]) for v in li],
            [O.g2([None if j is None else O.qs[j] for j in v]) for v in ri])


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_infinities_of_one_vector_in_a_grid(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    O = ora(cname)
    n, li, ri = grid_vectors(cname)
    lhs, rhs = grid_arrays(O, li, ri)
    want = cached(("grid", cname), lambda: [[O.product(a, b) for b in ri] for a in li])
    out = ctx.pairing_products(lhs, rhs, n=n)
    assert out.shape == (3, 2, ctx.gt_bytes)
    for a in range(3):
        for b in range(2):
            assert O.dec(out[a, b]) == want[a][b], (cname, a, b)
    assert len({tuple(w) for row in want for w in row}) == 6
    pairs = [(2, 1), (0, 1), (0, 0), (2, 1), (1, 1), (0, 1)]
    sel = ctx.pairing_pairs(lhs, rhs, pairs, n=n)
    for k, (a, b) in enumerate(pairs):
        assert np.array_equal(sel[k], out[a, b]), (cname, k, a, b)


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_host_device_and_mixed_pointers_agree(cname, ctx_bn254, ctx_bls):
    from hekaton_system_amd.capi import DeviceBuffer
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    O = ora(cname)
    n, li, ri = grid_vectors(cname)
    lhs, rhs = grid_arrays(O, li, ri)
    host = ctx.pairing_products(lhs, rhs, n=n)
    dl = [DeviceBuffer.from_host(ctx, v) for v in lhs]
    dr = [DeviceBuffer.from_host(ctx, v) for v in rhs]
    try:
        dev = ctx.pairing_products(dl, dr, n=n)                              # all device: the packed k_gather_rows path
        mixed = ctx.pairing_products([dl[0], lhs[1], dl[2]], [rhs[0], dr[1]], n=n)
        dev_pairs = ctx.pairing_pairs(dl, dr, [(0, 1), (2, 0)], n=n)
    finally:
        for b in dl + dr:
            b.free()
    assert np.array_equal(dev, host) and np.array_equal(mixed, host)
    assert np.array_equal(dev_pairs[0], host[0, 1]) and np.array_equal(dev_pairs[1], host[2, 0])
    assert O.dec(host[0, 1]) == cached(("grid01", cname), lambda: O.product(li[0], ri[1]))


# ---- bilinearity ---------------------------------------------------------------------------------------------------------
class Multiples:
    """vectors of known multiples of the generators, made on the device by hk_fixed_base (as tests/test_pairing_gpu.py does)"""

    def __init__(self, cname, ctx):
        from hekaton_system_amd.cp_groth16 import FrCodec
        self.ctx, self.cp = ctx, CURVES[cname]
        self.T, self.E = pairing.tower(cname), Enc(self.cp)
        self.fc = FrCodec(cname)
        self.gen = {1: np.frombuffer(self.E.g1(self.cp.g1_gen), np.uint8), 2: np.frombuffer(self.E.g2(self.cp.g2_gen), np.uint8)}
        self.e_gen = cached(("e_gen", cname), lambda: self.T.pairing(self.cp.g1_gen, self.cp.g2_gen))
        self.rnd = random.Random(cname + "/multiples")

    def vec(self, group, n, inf=()):
        """-> (scalars with 0 at the infinity slots, the points with (0, 0) there)"""
        ks = [self.rnd.randrange(1, self.cp.r) for _ in range(n)]
        pts = np.array(self.ctx.fixed_base(group, self.gen[group], self.fc.enc(ks)), dtype=np.uint8)
        pb = self.ctx.g1_bytes if group == 1 else self.ctx.g2_bytes
        for i in inf:
            ks[i] = 0
            pts[i * pb:(i + 1) * pb] = 0
        return ks, pts

    def want(self, a, b, n=None):
        n = len(a) if n is None else n
        return self.T.f12_flat(self.T.f12_pow(self.e_gen, sum(x * y for x, y in zip(a[:n], b[:n])) % self.cp.r))


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_second_level_partial_group_by_bilinearity(cname, ctx_bn254, ctx_bls):
    """n = 257: 17 first-level values, the second level has a full group and a group of ONE; 255 and 256 on BN254 are its
    neighbours (a partial and a full last first-level group).  Then 257 with infinities at slot 0 (the G2 side) and at slot
    256 (the G1 side): the value that is alone in its group at both levels is 1."""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    M = Multiples(cname, ctx)
    a, A = M.vec(1, 257)
    b, B = M.vec(2, 257)
    g1b, g2b = ctx.g1_bytes, ctx.g2_bytes
    for n in (255, 256, 257) if cname == "bn254" else (257,):
        got = M.E.f12_dec(ctx.multi_pairing(A[:n * g1b], B[:n * g2b], n=n).tobytes())
        assert got == M.want(a, b, n), (cname, n)
    a2, A2 = list(a), A.copy()
    b2, B2 = list(b), B.copy()
    a2[256], b2[0] = 0, 0
    A2[256 * g1b:] = 0
    B2[:g2b] = 0
    got = M.E.f12_dec(ctx.multi_pairing(A2, B2, n=257).tobytes())
    assert got == M.want(a2, b2), (cname, "257 with infinities")
    assert got != M.want(a, b)


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_four_tree_levels_and_lane_per_point_lines_by_bilinearity(cname, ctx_bn254, ctx_bls):
    """n = 4097, one lhs vector against four rhs vectors: 4097 * 4 * 4 lanes are more than the quad form's 65 536, so the
    lines come from the lane-per-point kernel, and the tree has the levels 257, 17, 2, 1.  Infinities: lhs slot 0 (every
    product), rhs vector 1 slot 4096 (the last first-level group's lone element), rhs vector 2 slot 256."""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    M = Multiples(cname, ctx)
    n = 4097
    assert n * 4 * 4 > 65536
    a, A = M.vec(1, n, inf=(0,))
    rhs = [M.vec(2, n, inf=inf) for inf in ((), (4096,), (256,), ())]
    out = ctx.pairing_products([A], [B for _, B in rhs], n=n)
    assert out.shape == (1, 4, ctx.gt_bytes)
    for j, (b, _) in enumerate(rhs):
        assert M.E.f12_dec(out[0, j].tobytes()) == M.want(a, b), (cname, j)
