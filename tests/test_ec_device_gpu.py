"""GPU: the DEVICE build of csrc/ec.cuh, case by case, against the big-int group law of oracle.pyref.curve, and the
product's k_batch_affine with infinities inside a chunk.

The host shim (tests/host_shim/field_shim.cpp) compiles the canonical C++ only.  On the device ec_madd and ec_add decide
P == Q, P == -Q and infinity with is_zero() on the result of a LAZY sub and on a zz that may sit in [p, 2p); the accumulate
loop reaches those corners only when a bucket happens to hold the same base twice in a row, in an order that atomics pick.
tests/device_shim/ec_dev_shim.hip runs one lane per case instead: operands enter as raw limbs, as XYZZ representatives
(x l^2, y l^3, l^2, l^3) for l in {1, 2, random} with coordinates optionally shifted by +p (never at or above the
representative bound of tests/field_edges.py).  Affine operands are canonical: they come from memory, and memory is
canonical by the st_vec contract.  A == B with y = 0 cannot occur: both curves have odd order, so no point has order 2.

Checks on every output: zz^3 = zzz^2, infinity iff zz = 0, the normalised point equals the oracle's, and raw registers
stay below the representative bound.  All comparisons are exact.  Runs on both builds of the shim; the -DHK_NO_ASM_MUL one
lacks the forms whose C++ fallback outgrows the code-object bounds (dev_shim.EC_NOASM_NOT_BUILT), which is asserted.
"""
import random

import pytest

from tests import dev_shim as ds
from tests import field_edges as fe
from tests import msm_edges as me

pytestmark = pytest.mark.gpu

FQ = {0: "BN254_FQ", 1: "BN254_FQ", 2: "BLS12_381_FQ", 3: "BLS12_381_FQ"}
X, Y, ZZ, ZZZ = 1, 2, 4, 8            # coordinate masks of a +p shift
TWO_POINT_OPS = {ds.G_MADD: "ec_madd (accumulate loop)", ds.G_MADD_NI: "ec_madd_ni", ds.G_ADD: "ec_add", ds.G_ADD_NI: "ec_add_ni"}


@pytest.fixture(scope="module", params=["asm", "noasm"])
def shim(request):
    return ds.load_ec(request.param)


class Grp:
    """coordinate encoding of one group: Montgomery limbs of ints (G1) or (c0, c1) tuples (G2)"""

    def __init__(self, gid):
        self.gid = gid
        self.f = fe.FIELDS[FQ[gid]]
        assert self.f.lazy                                  # every coordinate field is lazy: +p shifts exist
        self.nb = 4 * self.f.N
        self.G = me.group(gid)
        self.F = self.G.F
        self.g2 = gid in (1, 3)
        self.pts = me.points(gid, me.pool_ks(gid)[:8])
        rnd = random.Random("ec_device/%d" % gid)
        rl = (rnd.randrange(1, self.f.p), rnd.randrange(1, self.f.p)) if self.g2 else rnd.randrange(1, self.f.p)
        self.lams = [self.F.one, self.F.from_int(2), rl]

    def enc(self, e):
        f = self.f
        return tuple(c * f.R % f.p for c in e) if self.g2 else e * f.R % f.p

    def dec(self, e):
        f = self.f
        return tuple(c * f.Rinv % f.p for c in e) if self.g2 else e * f.Rinv % f.p

    def shift(self, e):
        return tuple(c + self.f.p for c in e) if self.g2 else e + self.f.p

    def zero_slot(self):
        z = self.F.zero
        return (z, z, z, z)

    def xyzz(self, P, lam=None, mask=0):
        """raw XYZZ slot of P under lambda, the coordinates in `mask` shifted by +p; P None: infinity as all zero, or with
        zz (and zzz) = p when the mask names them"""
        F = self.F
        if P is None:
            c = [F.zero] * 4
        else:
            lam = F.one if lam is None else lam
            l2 = F.mul(lam, lam)
            l3 = F.mul(l2, lam)
            c = [F.mul(P[0], l2), F.mul(P[1], l3), l2, l3]
        c = [self.enc(e) for e in c]
        return tuple(self.shift(e) if (mask >> i) & 1 else e for i, e in enumerate(c))

    def affine(self, P):
        """canonical affine operand in the first half of a slot ((0, 0) for infinity)"""
        z = self.F.zero
        if P is None:
            return (z, z, z, z)
        return (self.enc(P[0]), self.enc(P[1]), z, z)

    def scalar_slot(self, s):
        z = self.F.zero
        return ((s, 0) if self.g2 else s, z, z, z)

    def comps(self, e):
        return e if self.g2 else (e,)

    def point_of(self, slot, raw, what):
        """checks the slot (bounds, zz^3 = zzz^2) and returns its affine point, None for infinity"""
        f, F = self.f, self.F
        bound = f.B if raw else f.p
        for e in slot:
            assert all(c < bound for c in self.comps(e)), "%s: limb value at or above %s" % (what, "B" if raw else "p")
        x, y, zz, zzz = (self.dec(tuple(c % f.p for c in e) if self.g2 else e % f.p) for e in slot)
        assert F.mul(F.mul(zz, zz), zz) == F.mul(zzz, zzz), "%s: zz^3 != zzz^2" % what
        if F.is_zero(zz):
            return None
        return (F.mul(x, F.inv(zz)), F.mul(y, F.inv(zzz)))


_grp = {}


def grp(gid):
    if gid not in _grp:
        _grp[gid] = Grp(gid)
    return _grp[gid]


def run_checked(shim, g, op, a, b, want, what, k=0):
    """runs op raw and through st_vec and compares every lane with `want` (affine points)"""
    if not shim.built(g.gid, op):
        st, _ = shim.group_op_status(g.gid, op, g.nb, a, b, raw=1, k=k)
        assert st == -ds.HIP_NOT_SUPPORTED, "%s: expected to be left out of this build" % what
        return None
    outs = {}
    for raw in (1, 0):
        out = shim.group_op(g.gid, op, g.nb, a, b, raw=raw, k=k)
        assert len(out) == len(want)
        for i, (slot, w) in enumerate(zip(out, want)):
            got = g.point_of(slot, raw, "%s #%d raw=%d" % (what, i, raw))
            assert got == w, "%s #%d raw=%d: got %r, want %r" % (what, i, raw, got, w)
        outs[raw] = out
    return outs[1]


def pair_cases(g, mixed):
    """(A slot, B slot, A + B) over the exceptional cases; mixed: B is a canonical affine operand, else an XYZZ one"""
    G, P = g.G, g.pts
    masks_a = [0, X, Y, ZZ, ZZ | ZZZ, X | Y | ZZ | ZZZ]
    masks_b = [0] if mixed else [0, X, ZZ, X | Y | ZZ | ZZZ]
    bslot = (lambda Q, lam, m: g.affine(Q)) if mixed else (lambda Q, lam, m: g.xyzz(Q, lam, m))
    lams_b = [None] if mixed else g.lams
    cases = []
    s01, d2, n3 = G.add(P[0], P[1]), G.dbl(P[2]), G.neg(P[3])
    for la in g.lams:
        for lb in lams_b:
            for ma in masks_a:
                for mb in masks_b:
                    cases.append((g.xyzz(P[0], la, ma), bslot(P[1], lb, mb), s01))          # generic
                    cases.append((g.xyzz(P[2], la, ma), bslot(P[2], lb, mb), d2))                # B == A
                    cases.append((g.xyzz(P[3], la, ma), bslot(n3, lb, mb), None))                # B == -A
            # A infinity (zz = 0 and zz = p), B infinity, both
            for ma in (0, ZZ, ZZ | ZZZ):
                for mb in masks_b:
                    cases.append((g.xyzz(None, None, ma), bslot(P[4], lb, mb), P[4]))
                    cases.append((g.xyzz(None, None, ma), bslot(None, None, mb & (ZZ | ZZZ)), None))
            for ma in masks_a:
                for mb in ([0] if mixed else [0, ZZ, ZZ | ZZZ]):
                    cases.append((g.xyzz(P[5], la, ma), bslot(None, None, mb), P[5]))
    return cases


@pytest.mark.parametrize("gid", range(4))
def test_two_point_ops_exceptional_cases(shim, gid):
    g = grp(gid)
    for op, name in TWO_POINT_OPS.items():
        cases = pair_cases(g, mixed=op in (ds.G_MADD, ds.G_MADD_NI))
        a, b, want = zip(*cases)
        run_checked(shim, g, op, list(a), list(b), list(want), "%s/%s g%d" % (shim.variant, name, gid))


@pytest.mark.parametrize("gid", range(4))
def test_unary_ops(shim, gid):
    g = grp(gid)
    G = g.G
    reps = [(P, g.xyzz(P, lam, m)) for P in g.pts[:3] for lam in g.lams for m in (0, X, Y, ZZ, ZZZ, X | Y | ZZ | ZZZ)]
    reps += [(None, g.xyzz(None, None, m)) for m in (0, ZZ, ZZ | ZZZ)]
    a = [s for _P, s in reps]
    what = "%s/g%d " % (shim.variant, gid)
    for op in (ds.G_DBL, ds.G_DBL_NI):
        run_checked(shim, g, op, a, None, [G.dbl(P) for P, _s in reps], what + "ec_dbl")
    run_checked(shim, g, ds.G_NEG, a, None, [G.neg(P) for P, _s in reps], what + "ec_neg")
    # ec_dbl_affine: only reached from the P == Q corner, with a canonical non-infinity affine operand
    b = [g.affine(P) for P in g.pts]
    run_checked(shim, g, ds.G_DBL_AFFINE, [g.zero_slot()] * len(b), b, [G.dbl(P) for P in g.pts], what + "ec_dbl_affine")
    # ec_to_affine: (x, y) canonical through st_vec, (0, 0) for infinity
    for raw in (1, 0):
        out = shim.group_op(gid, ds.G_TO_AFFINE, g.nb, a, None, raw=raw)
        for i, ((P, _s), slot) in enumerate(zip(reps, out)):
            bound = g.f.B if raw else g.f.p
            assert all(c < bound for e in slot for c in g.comps(e))
            x, y = (g.dec(tuple(c % g.f.p for c in e) if g.g2 else e % g.f.p) for e in slot[:2])
            assert ((x, y) == (g.F.zero, g.F.zero)) if P is None else ((x, y) == P), "%sec_to_affine #%d raw=%d" % (what, i, raw)
            assert slot[2] == g.F.zero and slot[3] == g.F.zero


@pytest.mark.parametrize("gid", range(4))
def test_chains_keep_raw_intermediates(shim, gid):
    """((P + P) + P) - P - P - P + P step by step from infinity: restart from infinity, corner, generic, three
    subtractions down to the cancellation, restart - the raw registers of each step are the next step's operand"""
    g = grp(gid)
    G = g.G
    pts = g.pts
    steps = [+1, +1, +1, -1, -1, -1, +1]
    for op, name in TWO_POINT_OPS.items():
        mixed = op in (ds.G_MADD, ds.G_MADD_NI)
        acc = [g.xyzz(None)] * len(pts)
        mult = 0
        for n_step, sgn in enumerate(steps):
            Q = [P if sgn > 0 else G.neg(P) for P in pts]
            b = [g.affine(q) for q in Q] if mixed else [g.xyzz(q, g.lams[(n_step + j) % 3], 0) for j, q in enumerate(Q)]
            mult += sgn
            want = [G.mul(P, mult) for P in pts]
            acc = run_checked(shim, g, op, acc, b, want, "%s/%s g%d chain step %d" % (shim.variant, name, gid, n_step))
            if acc is None:
                break
        assert mult == 1 or acc is None
    # 64 mixed adds of the same P in one lane: corner once, then generic, registers never leave the lane
    for k in (1, 2, 3, 64):
        run_checked(shim, g, ds.G_MADD_CHAIN, [g.xyzz(None)] * len(pts), [g.affine(P) for P in pts],
                    [G.mul(P, k) for P in pts], "%s/madd chain x%d g%d" % (shim.variant, k, gid), k=k)
    # ... and from P + (-P): cancellation in mid-run, then the restart
    run_checked(shim, g, ds.G_MADD_CHAIN, [g.xyzz(G.neg(P), g.lams[2], X) for P in pts], [g.affine(P) for P in pts],
                [G.mul(P, 4) for P in pts], "%s/madd chain from -P g%d" % (shim.variant, gid), k=5)


@pytest.mark.parametrize("gid", range(4))
def test_mul_small_and_mul_limbs(shim, gid):
    g = grp(gid)
    G = g.G
    cname = me.GROUPS[gid][0]
    reps = [(P, g.xyzz(P, lam, m)) for P, lam, m in ((g.pts[0], g.lams[0], 0), (g.pts[1], g.lams[2], X | ZZ),
                                                     (g.pts[2], g.lams[1], X | Y | ZZ | ZZZ))]
    reps += [(None, g.xyzz(None, None, 0)), (None, g.xyzz(None, None, ZZ | ZZZ))]
    a = [s for _P, s in reps]
    # bucket-reduction weights wgt = j K (K = 8): lanes j = 1, 2, 3, 255, 256 and the last lane of a c = 16 window, 4095;
    # 4: c = 3 has K = B = 4 (one lane per window, weight 0, but the one K that is no multiple of 8)
    for k in [0, 1, 2, 4, 7] + [8 * j for j in (1, 2, 3, 255, 256, 4095)] + [1 << 15]:
        run_checked(shim, g, ds.G_MUL_SMALL, a, None, [G.mul(P, k) for P, _s in reps],
                    "%s/ec_mul_small(%d) g%d" % (shim.variant, k, gid), k=k)
    scalars = me.named_scalars(cname, 3)[:12] + me.named_scalars(cname, 16)[:12]
    scalars += [me.all_min(cname, 16), me.all_max(cname, 16), me.all_min(cname, 5), me.alternating(cname, 7, 1)]
    scalars = fe._dedup(scalars)
    P, slot = reps[1]
    run_checked(shim, g, ds.G_MUL_LIMBS, [slot] * len(scalars), [g.scalar_slot(s) for s in scalars],
                [G.mul(P, s) for s in scalars], "%s/ec_mul_limbs g%d" % (shim.variant, gid))
    run_checked(shim, g, ds.G_MUL_LIMBS, [g.xyzz(None, None, ZZ)] * 2, [g.scalar_slot(s) for s in scalars[3:5]], [None, None],
                "%s/ec_mul_limbs(infinity) g%d" % (shim.variant, gid))


def _inf_patterns(n, chunk):
    """index sets of the points at infinity: none, first / last / middle of a chunk, a whole chunk, a consecutive pair,
    every position"""
    pats = [set(), {i for i in (n // 2, n // 2 + 1) if i < n}, set(range(n))]
    for base in {0, chunk if chunk < n else 0, (n - 1) // chunk * chunk}:          # the first, second and last chunk
        pats += [{base}, {min(base + chunk - 1, n - 1)}, {min(base + chunk // 2, n - 1)},
                 set(range(base, min(base + chunk, n)))]
    out = []
    for p in pats:
        if p not in out:
            out.append(p)
    return out


@pytest.mark.parametrize("gid", range(4))
def test_batch_affine_with_infinities_inside_a_chunk(shim, gid):
    """k_batch_affine (Montgomery's trick inside a lane) with chunk > 1 is otherwise reached only above 65 536 points:
    an infinity must neither enter the lane's prefix product nor shift its neighbours' inverses"""
    g = grp(gid)
    rnd = random.Random("batch_affine/%d" % gid)
    f = g.f
    pool = []
    for i in range(50):
        lam = (rnd.randrange(1, f.p), rnd.randrange(f.p)) if g.g2 else rnd.randrange(1, f.p)
        pool.append((g.pts[i % 8], g.xyzz(g.pts[i % 8], lam if i % 5 else g.F.one, 0)))      # memory: canonical
    infs = [g.xyzz(None, None, 0), g.xyzz(None, None, ZZ | ZZZ)]                               # zz = 0 and zz = p
    zero = g.F.zero
    for n in (1, 15, 16, 17, 50):
        for chunk in (1, 2, 16):
            for pat in _inf_patterns(n, chunk):
                pts = [infs[i % 2] if i in pat else pool[i][1] for i in range(n)]
                out = shim.batch_affine(gid, g.nb, pts, chunk)
                assert len(out) == n
                for i, (x, y) in enumerate(out):
                    what = "%s/g%d n=%d chunk=%d inf=%s #%d" % (shim.variant, gid, n, chunk, sorted(pat)[:4], i)
                    if i in pat:
                        assert (x, y) == (zero, zero), what
                    else:
                        assert all(c < f.p for e in (x, y) for c in g.comps(e)), what
                        assert (g.dec(x), g.dec(y)) == pool[i][0], what
