"""Deterministic scalars, scalar vectors and bases for the tests of the device curve arithmetic (csrc/ec.cuh) and of the
MSM bucket pass (csrc/msm.cuh, csrc/msm_driver_impl.cuh): tests/test_msm_edges_cpu.py checks every premise stated here,
tests/test_ec_device_gpu.py, tests/test_msm_plan_device_gpu.py and tests/test_msm_edges_gpu.py run the device on them.
A plain module with fixed seeds, like tests/field_edges.py; nothing here needs a GPU.

Scalars are built FROM the signed digits the device splits them into (`recode` is the Python model of msm_num_windows,
msm_load_scalar and msm_digit), so a family can say "every window below the top holds the digit -2^(c-1)" and assert it.
Bases are P_i = k_i G with known k_i, so the reference of any MSM is one scalar multiplication,
reference(ks, scalars) = ((sum s_i k_i) mod r) G, independent of every bucket schedule.
"""
import random

from oracle.pyref import curve
from oracle.pyref.params import CURVES

CURVE_NAMES = ("bn254", "bls12_381")
C_ALL = tuple(range(3, 17))
# group ids of shim_group_op / dshim_group_op
GROUPS = (("bn254", "g1"), ("bn254", "g2"), ("bls12_381", "g1"), ("bls12_381", "g2"))
GROUP_IDS = {g: i for i, g in enumerate(GROUPS)}
MSM_LDS_COUNTERS = 32768          # msm.cuh: W * 2^(c-1) counters of a plain plan must fit the sort's LDS histogram
MSM_LVL_L = 16                    # msm.cuh: entries per lane on levels >= 1
MSM_TAIL_THREADS = 256
POOL = 257                        # bases per group (pool_ks gives more on request)


# ---- recoding model ---------------------------------------------------------------------------------------------------
def kconst(c, W):
    return sum(1 << (c * w + c - 1) for w in range(W))


def num_windows(c, cname):
    """The rule of test_msm_window_count_is_the_smallest_that_holds_every_scalar: W windows hold every scalar iff
    (r - 1) + kconst(W) < 2^(cW); the plan takes ceil((bits + 2) / c), or one fewer when that already does."""
    r = CURVES[cname].r
    upper = (r.bit_length() + 2 + c - 1) // c
    fits = lambda w: (r - 1) + kconst(c, w) < (1 << (c * w))
    assert fits(upper)
    return upper - 1 if fits(upper - 1) else upper


def recode(s, c, cname):
    """(W, digits): digit_w = ((s + kconst) >> cw & (2^c - 1)) - 2^(c-1), each in [-2^(c-1), 2^(c-1) - 1]"""
    W = num_windows(c, cname)
    sp = s + kconst(c, W)
    assert 0 <= s < CURVES[cname].r and sp >> (c * W) == 0
    digits = [((sp >> (c * w)) & ((1 << c) - 1)) - (1 << (c - 1)) for w in range(W)]
    assert from_digits(digits, c) == s
    return W, digits


def from_digits(digits, c):
    return sum(d << (c * w) for w, d in enumerate(digits))


def _checked(s, digits, c, cname):
    """s is a valid non-zero scalar and the device's recoding gives exactly `digits` (zero-extended to W windows)"""
    r = CURVES[cname].r
    assert 0 < s < r, (cname, c, s)
    W, got = recode(s, c, cname)
    assert got == list(digits) + [0] * (W - len(digits)), (cname, c, digits, got)
    return s


# ---- directed scalar families: (cname, c) -> s with 0 < s < r ----------------------------------------------------------
def all_max(cname, c):
    """digit 2^(c-1) - 1 in windows 0 .. m-1, m the largest for which s < r (m = W - 1 for every c on both curves)"""
    r, W = CURVES[cname].r, num_windows(c, cname)
    d = (1 << (c - 1)) - 1
    m = max(k for k in range(1, W + 1) if from_digits([d] * k, c) < r)
    assert m == W - 1, (cname, c, m, W)
    return _checked(from_digits([d] * m, c), [d] * m, c, cname)


def all_min(cname, c):
    """digit -2^(c-1) in windows 0 .. m-1 and +1 in window m, m the largest for which s < r (m = W - 1 again): at c = 16
    the one int16 digit whose magnitude needs msm_mag's unsigned form, and every entry lands in a window's LAST bucket"""
    r, W = CURVES[cname].r, num_windows(c, cname)
    d = -(1 << (c - 1))
    m = max(k for k in range(1, W) if from_digits([d] * k + [1], c) < r)
    assert m == W - 1, (cname, c, m, W)
    return _checked(from_digits([d] * m + [1], c), [d] * m + [1], c, cname)


def one_bucket(cname, c, d):
    """the same digit d in every window below the top (d > 0); for d < 0 in windows 0 .. m-1 with +1 in window m, m the
    largest for which s < r (W - 1, or W - 2 where a +1 in the top window already passes r)"""
    r, W = CURVES[cname].r, num_windows(c, cname)
    assert d != 0 and -(1 << (c - 1)) <= d < (1 << (c - 1))
    if d > 0:
        digits = [d] * (W - 1)
    else:
        m = max(k for k in range(1, W) if from_digits([d] * k + [1], c) < r)
        assert m >= W - 2, (cname, c, d, m, W)
        digits = [d] * m + [1]
    return _checked(from_digits(digits, c), digits, c, cname)


def alternating(cname, c, d):
    """digits +d, -d, +d, ... ending in +d: the longest odd run that stays below r"""
    r, W = CURVES[cname].r, num_windows(c, cname)
    assert 0 < d < (1 << (c - 1))
    run = lambda k: [d if w % 2 == 0 else -d for w in range(k)]
    k = max(k for k in range(1, W + 1, 2) if 0 < from_digits(run(k), c) < r)
    assert k >= W - 2, (cname, c, k, W)
    return _checked(from_digits(run(k), c), run(k), c, cname)


def named_scalars(cname, c):
    """0, 1, 2, r - 1, r - 2, the digit edges of window 0 and 2^(cw) for every window w"""
    r, W = CURVES[cname].r, num_windows(c, cname)
    v = [0, 1, 2, r - 1, r - 2, (1 << (c - 1)) - 1, 1 << (c - 1), (1 << c) - 1]
    v += [1 << (c * w) for w in range(W) if (1 << (c * w)) < r]
    out = []
    for s in v:
        recode(s, c, cname)
        if s not in out:
            out.append(s)
    return out


# ---- bases ------------------------------------------------------------------------------------------------------------
_groups = {}
_points = {}


def group(gid):
    if gid not in _groups:
        cname, g = GROUPS[gid]
        _groups[gid] = (curve.G1 if g == "g1" else curve.G2)(CURVES[cname])
    return _groups[gid]


def order(gid):
    return CURVES[GROUPS[gid][0]].r


def pool_ks(gid, n=POOL):
    """n fixed discrete logs k_i = k_0 + i d in [1, r) for a seeded random k_0 and d: distinct, none the negative of
    another, and cheap to turn into points (one addition each; the cache of `point` is filled here).  A progression has
    linear coincidences that random logs lack - at small c a bucket's running sum now and then EQUALS the next base's
    shifted multiple (8 k_54 = eight window-0 entries whose indices sum to 432) - so even `uniform` reaches the P == Q
    corner of the accumulate loop there; the reference does not care."""
    rnd = random.Random("msm_edges/ks/%d" % gid)
    r, G = order(gid), group(gid)
    k0, d = rnd.randrange(1, r), rnd.randrange(1, r)
    ks = [(k0 + i * d) % r for i in range(n)]
    assert 0 not in ks and len(set(ks) | {r - k for k in ks}) == 2 * n
    if (gid, ks[-1]) not in _points:
        P, D = point(gid, k0), point(gid, d)
        for k in ks:
            _points.setdefault((gid, k), P)
            P = G.add(P, D)
    return ks


def point(gid, k):
    """k G as an affine tuple (None for k = 0 mod r), cached; -P costs a negation when P is known"""
    G, r = group(gid), order(gid)
    k %= r
    key = (gid, k)
    if key not in _points:
        if k == 0:
            _points[key] = None
        elif (gid, r - k) in _points:
            _points[key] = G.neg(_points[(gid, r - k)])
        else:
            _points[key] = G.mul(G.gen, k)
    return _points[key]


def points(gid, ks):
    return [point(gid, k) for k in ks]


def reference(gid, ks, scalars, idx_off=0):
    """sum_j scalars[j + idx_off] * (ks[j] G): base j goes with scalar j + idx_off (the L-query form; 0: one to one)"""
    r = order(gid)
    acc = 0
    for j, k in enumerate(ks):
        if 0 <= j + idx_off < len(scalars):
            acc += scalars[j + idx_off] * k
    return point(gid, acc % r)


# ---- vector families: each returns a dict(name, ks, scalars, idx_off) with len(scalars) = n --------------------------
def _vec(name, ks, scalars, idx_off=0):
    return dict(name=name, ks=list(ks), scalars=list(scalars), idx_off=idx_off)


def _rnd(gid, tag):
    return random.Random("msm_edges/%d/%s" % (gid, tag))


def uniform(gid, n, tag="uniform"):
    rnd, r = _rnd(gid, "%s/%d" % (tag, n)), order(gid)
    return _vec("uniform", pool_ks(gid)[:n], [rnd.randrange(r) for _ in range(n)])


def all_equal(gid, n, s, name="all_equal"):
    return _vec(name, pool_ks(gid)[:n], [s] * n)


def one_base(gid, n, scalars=None):
    """every base the same point: consecutive entries of a bucket are then equal (the P == Q corner of ec_madd)"""
    if scalars is None:
        rnd, r = _rnd(gid, "one_base/%d" % n), order(gid)
        scalars = [rnd.randrange(r) for _ in range(n)]
    return _vec("one_base", [pool_ks(gid)[0]] * n, scalars)


def plus_minus(gid, n, s):
    """bases P, -P, P, ... with equal scalars: infinity for even n, s P for odd n; partial sums cancel in mid-run"""
    k, r = pool_ks(gid)[1], order(gid)
    return _vec("plus_minus", [k if j % 2 == 0 else r - k for j in range(n)], [s] * n)


def inf_bases(gid, n, every=False):
    """the first half of the bases at infinity (k = 0), or all of them"""
    ks = pool_ks(gid)[:n]
    cut = n if every else (n + 1) // 2
    v = uniform(gid, n, "inf_bases")
    return _vec("inf_bases_all" if every else "inf_bases_half", [0] * cut + ks[cut:], v["scalars"])


def zeros(gid, n):
    """every scalar 0: no non-zero digit, E = 0"""
    return _vec("zeros", pool_ks(gid)[:n], [0] * n)


def slice_aligned(gid, k, c, n_max=POOL):
    """scalars d = 1 .. m, each k times: one non-zero digit each (d < 2^(c-1)), so bucket d - 1 of window 0 holds exactly k
    entries and E = m k.  With the default slice floor of 32 the first bucket ends one before (k = 31), at (32) or one
    after (33) the first slice end, and the later ends drift across the slices from there."""
    m = min(n_max // k, (1 << (c - 1)) - 1)
    scalars = [d for d in range(1, m + 1) for _ in range(k)]
    return _vec("slice_aligned_%d" % k, pool_ks(gid)[:len(scalars)], scalars)


def window(gid, n, idx_off, n_bases):
    """the L-query form: only scalars idx_off <= i < idx_off + n_bases have a base"""
    v = uniform(gid, n, "window")
    return _vec("window_%d_%d" % (idx_off, n_bases), pool_ks(gid)[:n_bases], v["scalars"], idx_off)


def sprinkle(scalars, named, tag):
    """a copy of `scalars` with the named values at fixed pseudo-random positions"""
    rnd = random.Random("msm_edges/sprinkle/%s/%d" % (tag, len(scalars)))
    out = list(scalars)
    for pos, s in zip(rnd.sample(range(len(out)), min(len(named), len(out))), named):
        out[pos] = s
    return out


def vector_families(gid, n, c):
    """every vector family at length n (n >= 2) for window size c"""
    cname = GROUPS[gid][0]
    r = order(gid)
    s_min, s_max = all_min(cname, c), all_max(cname, c)
    fams = [
        uniform(gid, n),
        all_equal(gid, n, s_min, "all_equal_all_min"),
        all_equal(gid, n, s_max, "all_equal_all_max"),
        all_equal(gid, n, r - 1, "all_equal_r_minus_1"),
        one_base(gid, n),
        one_base(gid, n, [one_bucket(cname, c, 1)] * n),
        plus_minus(gid, n, alternating(cname, c, 1)),
        plus_minus(gid, n - 1, s_min),
        inf_bases(gid, n),
        inf_bases(gid, n, every=True),
        zeros(gid, n),
    ]
    fams += [slice_aligned(gid, k, c, n) for k in (31, 32, 33) if n >= k]
    fams += [window(gid, n, o, nb) for o, nb in ((0, n), (1, n - 1), (n - 1, 1), (5, 0), (7, 40)) if o + nb <= n]
    return fams


# ---- the accumulate schedule (msm_set_lanes / msm_level_info of msm.cuh) ----------------------------------------------
# AccumOcc<F>::waves per group id: the device reports the lanes it plans for among dshim_msm's plan words, and
# tests/test_msm_plan_device_gpu.py compares them with `lanes` below on every call
ACCUM_WAVES = {0: 4, 1: 2, 2: 3, 3: 1}


def lane_plan(gid, n, c, WP, batch=1, lmin0=32):
    """W, WP, F, NB, T (lanes per level), n_levels of the plan MsmRun<F>::run derives"""
    W = num_windows(c, GROUPS[gid][0])
    WP = min(WP, W)
    lanes = max(ACCUM_WAVES[gid] * 65536 // batch, 1)
    T = [max(min((n * W + lmin0 - 1) // lmin0, lanes), 1)]
    while T[-1] > 1 and len(T) < 16:
        T.append((2 * T[-1] + MSM_LVL_L - 1) // MSM_LVL_L)
    return dict(W=W, WP=WP, F=(W + WP - 1) // WP, NB=WP << (c - 1), T=T, n_levels=len(T), lmin0=lmin0, lanes=lanes)


def level0_slices(plan, E):
    """(L, active): entries per lane and live lanes of level 0 for E sorted entries"""
    L = max((E + plan["T"][0] - 1) // plan["T"][0], plan["lmin0"])
    return L, (E + L - 1) // L


def bucket_ends(scalars, c, cname, WP):
    """exclusive end position of every non-empty bucket in the sorted entry list (bucket = (w % WP) B + |digit| - 1)"""
    B = 1 << (c - 1)
    count = {}
    for s in scalars:
        for w, d in enumerate(recode(s, c, cname)[1]):
            if d:
                b = (w % WP) * B + abs(d) - 1
                count[b] = count.get(b, 0) + 1
    ends, pos = [], 0
    for b in sorted(count):
        pos += count[b]
        ends.append(pos)
    return ends
