"""Deterministic cases for the tests of the group sweeps over caller-supplied points - the kernels of csrc/fixed_base.cuh and
csrc/endo.cuh and the MsmRun entry points in front of them: tests/test_sweep_edges_cpu.py checks every premise stated here,
tests/test_sweep_device_gpu.py and tests/test_sweep_entries_gpu.py run the device on them.  A plain module with fixed seeds,
like tests/msm_edges.py, whose groups, pool of bases and `point` cache it shares; nothing here needs a GPU.

Every point is k G with a known k, so every expected value is ONE oracle multiplication of a scalar combination mod r
(msm_edges.point).  The case lists keep their discrete logs periodic in the element index, so that a vector of 65 elements
costs a dozen oracle multiplications, not 65.  The walks the kernels make (k_fb_mul's digit walk, k_points_sum_seg's strided loop
and LDS tree) are modelled here in discrete logs, so that a family can say "this add meets P == Q" and assert it.
"""
import random

import numpy as np

from hekaton_system_amd.endo import phi2, psi4
from oracle.pyref.codec import Codec
from oracle.pyref.params import CURVES
from tests import msm_edges as me

GROUPS = me.GROUPS
FB_WINDOWS = 32
# EndoOf<F>::K / STEPS and SplitDigits<F>::ND of csrc/endo.cuh by group id (the device shim reports them too)
SPLIT_K = {0: 2, 1: 4, 2: 2, 3: 4}
SPLIT_STEPS = {0: 131, 1: 68, 2: 131, 3: 68}
SPLIT_ND = {g: (s + 3) // 4 + 1 for g, s in SPLIT_STEPS.items()}
SPLIT_MAX_LANES = 65536
# PointsSum<F>::THREADS by group id: 256, or 128 where an XYZZ point is larger than 256 bytes (BLS12-381 G2); the device
# shim's getter is compared with this table in tests/test_sweep_device_gpu.py
SUM_THREADS = {0: 256, 1: 256, 2: 256, 3: 128}


def order(gid):
    return me.order(gid)


def cname(gid):
    return GROUPS[gid][0]


def rnd(gid, tag):
    return random.Random("sweep_edges/%d/%s" % (gid, tag))


def lam(gid):
    """the eigenvalue of the group's endomorphism: phi = [lam] on G1, psi = [lam] on G2"""
    return (phi2 if GROUPS[gid][1] == "g1" else psi4)(cname(gid)).lam


# ---- fixed base -------------------------------------------------------------------------------------------------------
def windows(s):
    """the 32 byte digits k_fb_mul reads from the canonical scalar"""
    assert 0 <= s < 1 << 256
    return [(s >> (8 * w)) & 255 for w in range(FB_WINDOWS)]


def fb_window_scalars(gid):
    """[(w, d, s)]: s = d 2^(8w) mod r for d in {1, 255} and every window, plus the largest digit the top window of a
    canonical scalar can hold.  Only 255 2^248 is reduced by r (the top byte of r is 0x30 / 0x73)."""
    r = order(gid)
    out = [(w, d, (d << (8 * w)) % r) for w in range(FB_WINDOWS) for d in (1, 255)]
    out.append((FB_WINDOWS - 1, r >> 248, (r >> 248) << 248))
    return out


def fb_walk(table_logs, s, r):
    """k_fb_mul in discrete logs: table_logs[w * 256 + d] -> (result log, events); an event is (w, 'dbl' | 'cancel' | 'inf')
    where the mixed add of window w met acc == entry, acc == -entry or an entry at infinity; acc = None is infinity"""
    acc, events = None, []
    for w, d in enumerate(windows(s)):
        if d == 0:
            continue
        e = table_logs[w * 256 + d] % r
        if e == 0:
            events.append((w, "inf"))
        elif acc is None:
            acc = e
        elif acc == e:
            events.append((w, "dbl"))
            acc = 2 * e % r
        elif (acc + e) % r == 0:
            events.append((w, "cancel"))
            acc = None
        else:
            acc = (acc + e) % r
        if acc == 0:
            acc = None
    return (acc or 0), events


def real_table_logs(k, r):
    return [(j << (8 * w)) * k % r for w in range(FB_WINDOWS) for j in range(256)]


def crafted_table(gid, kind):
    """logs of a 32 x 256 table no base generates: every entry f G but (0, 1) = a G, (1, 1) = a G ('dbl') or -a G ('cancel')
    and (2, 1) = b G.  The scalar 0x0101 then adds two equal / opposite entries, 0x010101 goes on into window 2."""
    r = order(gid)
    f, a, b = me.pool_ks(gid)[2:5]
    logs = [f] * (FB_WINDOWS * 256)
    logs[0 * 256 + 1] = a
    logs[1 * 256 + 1] = a if kind == "dbl" else r - a
    logs[2 * 256 + 1] = b
    return logs


CRAFTED_SCALARS = (0x0101, 0x010101, 0x01, 0x0100, 0x010000, 0, 0x0201)


# ---- linear combinations -------------------------------------------------------------------------------------------------
LINCOMB_PERIOD = 13


def lincomb_vecs(gid, k, n):
    """k vectors of n logs, periodic in the element; element 0 is infinity everywhere, element 1 in all but the last vector"""
    pool = me.pool_ks(gid)
    vecs = [[pool[(i + 3 * j) % LINCOMB_PERIOD] for i in range(n)] for j in range(k)]
    for j in range(k):
        vecs[j][0] = 0
        if n > 1 and j != k - 1:
            vecs[j][1] = 0
    return vecs


def lincomb_cases(gid, k, n):
    """[(name, vec_logs, coeffs)]; the cases that need two vectors are left out at k = 1"""
    r = order(gid)
    rn = rnd(gid, "lincomb/%d/%d" % (k, n))
    base = lincomb_vecs(gid, k, n)
    top_bit = r.bit_length() - 1                              # 253 on BN254, 254 on BLS12-381
    assert (1 << top_bit) < r
    cases = [("zeros", base, [0] * k),
             ("one_r_minus_1", base, [r - 1 if j == k // 2 else 0 for j in range(k)]),
             ("random", base, [rn.randrange(r) for _ in range(k)])]
    if k >= 2:
        same = [list(v) for v in base]
        same[1][2:] = same[0][2:]                             # elements 0 and 1 keep their infinities
        opp = [list(v) for v in base]
        opp[1][2:] = [(r - x) % r for x in opp[0][2:]]
        pad = [0] * (k - 2)
        cases += [("identical", same, [1, 1] + pad), ("opposite", opp, [1, 1] + pad),
                  ("top_bit", base, [1 << top_bit, 1] + pad)]
    return cases


def lincomb_expected(gid, vec_logs, coeffs):
    r = order(gid)
    n = len(vec_logs[0])
    return [sum(c * v[i] for c, v in zip(coeffs, vec_logs)) % r for i in range(n)]


def lincomb_last_step(vec_logs, coeffs, i, r):
    """what the LAST mixed add of element i meets in k_points_lincomb's shared chain: 'dbl', 'cancel' or None"""
    top = max((c.bit_length() for c in coeffs), default=0) - 1
    acc, last = 0, None
    for b in range(top, -1, -1):
        acc = 2 * acc % r
        for c, v in zip(coeffs, vec_logs):
            if (c >> b) & 1 and v[i] % r:
                e = v[i] % r
                last = "dbl" if acc == e else "cancel" if (acc + e) % r == 0 and acc else None
                acc = (acc + e) % r
    return last


# ---- sums --------------------------------------------------------------------------------------------------------------
SUM_FAMILIES = ("same_affine", "same_scaled", "plus_minus", "all_inf", "last_finite", "random")


def sum_family(gid, name, n, slot=0):
    """-> [(log, scale)] of n XYZZ inputs: log 0 is infinity; scale None is the from_affine form (zz = zzz = 1), an integer
    lambda the same point as (x lambda^2, y lambda^3, lambda^2, lambda^3).  `slot` picks the point (one per segment)."""
    r = order(gid)
    pool = me.pool_ks(gid, max(me.POOL, n))
    k = pool[1 + slot]
    rn = rnd(gid, "sum/%s/%d/%d" % (name, n, slot))
    if name == "same_affine":
        return [(k, None)] * n
    if name == "same_scaled":
        return [(k, rn.randrange(2, 1 << 200)) for _ in range(n)]
    if name == "plus_minus":
        return [(k if i % 2 == 0 else r - k, None if i % 3 else rn.randrange(2, 1 << 200)) for i in range(n)]
    if name == "all_inf":
        return [(0, None)] * n
    if name == "last_finite":
        return [(0, None)] * (n - 1) + [(k, 7)]
    assert name == "random"
    return [(pool[(i + 5 * slot) % len(pool)], rn.randrange(2, 1 << 200) if i % 2 else None) for i in range(n)]


def sum_walk(logs, T, r):
    """k_points_sum_seg (T lanes: PointsSum<F>::THREADS over one segment, or 64) in discrete logs -> (result log, events of the LDS tree): an event is
    (off, 'dbl' | 'cancel') where a tree add met equal or opposite finite operands"""
    acc = [sum(logs[t::T]) % r for t in range(T)]
    events = []
    off = T // 2
    while off:
        for t in range(off):
            a, b = acc[t], acc[t + off]
            if a and b:
                if a == b:
                    events.append((off, "dbl"))
                elif (a + b) % r == 0:
                    events.append((off, "cancel"))
            acc[t] = (a + b) % r
        off //= 2
    return acc[0], events


def xyzz(gid, k, scale=None):
    """the XYZZ slot (x, y, zz, zzz) of k G as field values of oracle.pyref (ints, or pairs in G2); infinity: all zero"""
    G = me.group(gid)
    F = G.F
    P = me.point(gid, k)
    if P is None:
        z = F.from_int(0)
        return (z, z, z, z)
    if scale is None:
        return (P[0], P[1], F.from_int(1), F.from_int(1))
    l1 = F.from_int(scale)
    l2 = F.mul(l1, l1)
    l3 = F.mul(l2, l1)
    return (F.mul(P[0], l2), F.mul(P[1], l3), l2, l3)


def xyzz_to_affine(gid, slot):
    G = me.group(gid)
    F = G.F
    x, y, zz, zzz = slot
    if F.is_zero(zz):
        return None
    return (F.mul(x, F.inv(zz)), F.mul(y, F.inv(zzz)))


# ---- the element-wise product ------------------------------------------------------------------------------------------------
SPLIT_PERIOD = 3


def split_scalars(gid):
    """the per-element scalars: 0, 1, r - 1, lam, r - lam, 2^64, 2^128 - 1 and four random ones"""
    r, l = order(gid), lam(gid)
    rn = rnd(gid, "split/scalars")
    return [0, 1, r - 1, l, r - l, 1 << 64, (1 << 128) - 1] + [rn.randrange(r) for _ in range(4)]


def split_points(gid, n, inf_at=()):
    """n logs with period SPLIT_PERIOD (coprime to the 11 scalars), infinity at the given elements"""
    pool = me.pool_ks(gid)
    return [0 if i in inf_at else pool[6 + i % SPLIT_PERIOD] for i in range(n)]


def mag_limit(gid):
    """the largest magnitude the K-lane form reads whole: 0x77..7 over ND nibbles"""
    return int("7" * SPLIT_ND[gid], 16)


def uniform_mags(gid):
    st = SPLIT_STEPS[gid]
    rn = rnd(gid, "split/mags")
    return [0, 7, 8, 9, (1 << st) - 1, mag_limit(gid)] + [rn.randrange(1 << st) for _ in range(3)]


def uniform_cases(gid):
    """[(mags, neg_mask)]: case i takes the magnitudes i, i + 2, ... of uniform_mags (cyclically) for its K parts and the sign
    mask i mod 2^K, for as many i as there are magnitudes or masks, whichever is more: every listed magnitude meets every
    part and every mask occurs (tests/test_sweep_edges_cpu.py asserts both); then the all-zero scalar"""
    K, mags = SPLIT_K[gid], uniform_mags(gid)
    count = max(len(mags), 1 << K)
    return [([mags[(i + 2 * j) % len(mags)] for j in range(K)], i % (1 << K)) for i in range(count)] + [([0] * K, 0)]


def fold_scalar(gid, mags, neg_mask):
    """c with  c P = sum_j (+-) mags[j] endo^j(P)"""
    r, l = order(gid), lam(gid)
    return sum((-m if (neg_mask >> j) & 1 else m) * pow(l, j, r) for j, m in enumerate(mags)) % r


def fold_vectors(gid, c, n, tag=0):
    """(lo logs, hi logs) of n elements: by (i + tag) % 5 - a generic pair, lo = c hi (the trailing add doubles), lo = -c hi
    (it gives infinity), lo at infinity, hi at infinity; the vectors of one launch differ by `tag`"""
    r = order(gid)
    pool = me.pool_ks(gid)
    lo, hi = [], []
    for i in range(n):
        h = pool[10 + i % 2]
        l = pool[20]
        kind = (i + tag) % 5
        if kind == 1:
            l = c * h % r
        elif kind == 2:
            l = (r - c * h) % r
        elif kind == 3:
            l = 0
        elif kind == 4:
            h = 0
        lo.append(l)
        hi.append(h)
    return lo, hi


def fold_expected(gid, c, lo, hi):
    r = order(gid)
    return [(l + c * h) % r for l, h in zip(lo, hi)]


# ---- vectors for the library's entry points -----------------------------------------------------------------------------
def progression(gid, n, tag):
    """n discrete logs k_0 + i d (the bases hk_fixed_base makes for the long entry tests)"""
    r = order(gid)
    rn = rnd(gid, "progression/%s/%d" % (tag, n))
    k0, d = rn.randrange(1, r), rn.randrange(1, r)
    return [(k0 + i * d) % r for i in range(n)]


# ---- bytes <-> oracle values -------------------------------------------------------------------------------------------------
class Io:
    """The memory forms of one group for both GPU test files: affine points and Fr scalars as the kernels and the C ABI read
    them, XYZZ slots as the kernels store them.  One instance per group id, so that every encoded point is made once."""
    _cache = {}

    def __new__(cls, gid):
        if gid not in cls._cache:
            self = super().__new__(cls)
            self.gid = gid
            self.cd = Codec(CURVES[cname(gid)])
            self.g2 = GROUPS[gid][1] == "g2"
            self.group = 2 if self.g2 else 1                  # the C ABI's group argument
            self.pb = self.cd.g2_bytes if self.g2 else self.cd.g1_bytes
            self.r = order(gid)
            self.F = me.group(gid).F
            self.dec = self.cd.g2_from if self.g2 else self.cd.g1_from
            self._aff, self._xy = {}, {}
            cls._cache[gid] = self
        return cls._cache[gid]

    def point_bytes(self, k):
        k %= self.r
        if k not in self._aff:
            self._aff[k] = (self.cd.g2 if self.g2 else self.cd.g1)(me.point(self.gid, k))
        return self._aff[k]

    def aff(self, logs):
        """the affine points k G, packed, as bytes"""
        return b"".join(self.point_bytes(k) for k in logs)

    def pts(self, logs):
        """the same as a numpy array"""
        return np.frombuffer(self.aff(logs), np.uint8).copy()

    def tiled(self, logs, idx):
        """the points logs[idx[i]] as one array, for long periodic vectors"""
        table = np.stack([np.frombuffer(self.point_bytes(k), np.uint8) for k in logs])
        return np.ascontiguousarray(table[idx]).reshape(-1)

    def fr(self, xs, mont=True):
        return (self.cd.fr_vec_mont if mont else self.cd.fr_vec_canon)(xs)

    def _fe(self, e):
        return b"".join(self.cd.fq_mont(c) for c in e) if self.g2 else self.cd.fq_mont(e)

    def xyzz(self, fam):
        """[(log, scale)] -> packed XYZZ slots (see `xyzz`)"""
        out = []
        for k, scale in fam:
            if (k, scale) not in self._xy:
                self._xy[(k, scale)] = b"".join(self._fe(e) for e in xyzz(self.gid, k, scale))
            out.append(self._xy[(k, scale)])
        return b"".join(out)

    def from_aff(self, buf):
        return [self.dec(buf[i:i + self.pb]) for i in range(0, len(buf), self.pb)]

    def from_xyzz(self, buf):
        """XYZZ slots as stored -> affine oracle points (zz = 0: None); asserts zz^3 = zzz^2 in every slot"""
        fb, F = self.cd.fq_bytes, self.F
        w = 2 if self.g2 else 1
        out = []
        for o in range(0, len(buf), 2 * self.pb):
            ints = [self.cd.fq_from_mont(buf[o + i * fb:o + (i + 1) * fb]) for i in range(4 * w)]
            slot = [tuple(ints[i:i + w]) if self.g2 else ints[i] for i in range(0, 4 * w, w)]
            zz, zzz = slot[2], slot[3]
            assert F.mul(F.mul(zz, zz), zz) == F.mul(zzz, zzz), "zz^3 != zzz^2 in slot %d" % (o // (2 * self.pb))
            out.append(xyzz_to_affine(self.gid, slot))
        return out

    def want(self, logs):
        return [me.point(self.gid, k) for k in logs]
