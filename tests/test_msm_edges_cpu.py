"""CPU: the premises of tests/msm_edges.py - the directed scalars really have the digits they claim under the device's
recoding, for every window size on both curves; `reference` (one scalar multiplication from known discrete logs) equals the
naive MSM of the oracle on every vector family; the slice_aligned vectors put their bucket ends where they say."""
import pytest

from oracle.pyref.params import CURVES
from tests import msm_edges as me


@pytest.mark.parametrize("cname", me.CURVE_NAMES)
def test_scalar_families_have_the_digits_they_claim(cname):
    r = CURVES[cname].r
    for c in me.C_ALL:
        W = me.num_windows(c, cname)
        lo, hi = -(1 << (c - 1)), (1 << (c - 1)) - 1
        _, d = me.recode(me.all_max(cname, c), c, cname)
        assert d == [hi] * (W - 1) + [0]
        _, d = me.recode(me.all_min(cname, c), c, cname)
        assert d == [lo] * (W - 1) + [1]
        for dig in (1, hi, lo, -1):
            _, d = me.recode(me.one_bucket(cname, c, dig), c, cname)
            m = max(w for w in range(W) if d[w] == dig) + 1
            assert d[:m] == [dig] * m and m >= W - 2
            assert d[m:] == ([0] * (W - m) if dig > 0 else [1] + [0] * (W - m - 1))
            assert dig < 0 or m == W - 1
        for dig in (1, hi):
            s = me.alternating(cname, c, dig)
            _, d = me.recode(s, c, cname)
            run = [x for x in d if x]
            assert 0 < s < r and len(run) % 2 == 1 and len(run) >= W - 2
            assert run == [dig if w % 2 == 0 else -dig for w in range(len(run))]
        named = me.named_scalars(cname, c)
        assert {0, 1, 2, r - 1, r - 2, hi, hi + 1, 2 * hi + 1} <= set(named)
        for s in named:
            _, d = me.recode(s, c, cname)
            assert all(lo <= x <= hi for x in d) and me.from_digits(d, c) == s
        # 2^(c-1) is the smallest scalar whose window-0 digit is the extreme negative one (with a carry into window 1)
        assert me.recode(1 << (c - 1), c, cname)[1][:2] == [lo, 1]


@pytest.mark.parametrize("cname", me.CURVE_NAMES)
def test_window_count_model_is_the_rule_of_the_plan(cname):
    r = CURVES[cname].r
    for c in me.C_ALL:
        W = me.num_windows(c, cname)
        assert (r - 1) + me.kconst(c, W) < 1 << (c * W)
        assert W == 1 or not (r - 1) + me.kconst(c, W - 1) < 1 << (c * (W - 1))
    assert me.num_windows(16, cname) == 16


@pytest.mark.parametrize("gid", range(4))
def test_reference_equals_the_naive_msm(gid):
    G = me.group(gid)
    for c, n in ((5, 16), (16, 7)):
        for v in me.vector_families(gid, n, c):
            bases = me.points(gid, v["ks"])
            assert all(G.on_curve(P) for P in bases)
            off = v["idx_off"]
            want = G.msm(bases, v["scalars"][off:off + len(bases)])
            assert me.reference(gid, v["ks"], v["scalars"], off) == want, (gid, c, v["name"])
    # what the families promise about their sums
    cname = me.GROUPS[gid][0]
    s = me.all_min(cname, 5)
    for n in (2, 16):
        v = me.plus_minus(gid, n, s)
        assert me.reference(gid, v["ks"], v["scalars"]) is None
    v = me.plus_minus(gid, 15, s)
    assert me.reference(gid, v["ks"], v["scalars"]) == G.mul(me.point(gid, v["ks"][0]), s)
    for v in (me.zeros(gid, 16), me.inf_bases(gid, 16, every=True)):
        assert me.reference(gid, v["ks"], v["scalars"]) is None
    assert me.points(gid, me.inf_bases(gid, 16)["ks"])[:8] == [None] * 8


@pytest.mark.parametrize("cname", me.CURVE_NAMES)
def test_slice_aligned_bucket_ends_sit_where_the_family_says(cname):
    gid = me.GROUP_IDS[(cname, "g1")]
    for c in (4, 5, 11, 16):
        for WP in (1, me.num_windows(c, cname)):
            if WP << (c - 1) > me.MSM_LDS_COUNTERS:
                continue
            for k in (31, 32, 33):
                v = me.slice_aligned(gid, k, c)
                n = len(v["scalars"])
                m = n // k
                assert m == min(me.POOL // k, (1 << (c - 1)) - 1) and m >= 7
                # exactly one non-zero digit each: bucket d - 1 of window 0 holds k entries, E = n
                for s in v["scalars"]:
                    d = me.recode(s, c, cname)[1]
                    assert d[0] == s and not any(d[1:])
                ends = me.bucket_ends(v["scalars"], c, cname, WP)
                assert ends == [k * (j + 1) for j in range(m)]
                plan = me.lane_plan(gid, n, c, WP)
                L, active = me.level0_slices(plan, ends[-1])
                assert L == 32 and active == (n + 31) // 32
                slice_ends = {L * (t + 1) for t in range(active)}
                assert ends[0] - L == k - 32
                if k == 32:
                    assert all(e in slice_ends for e in ends)
                else:
                    # the distance to the nearest slice end below grows by one per bucket: every offset 1 .. m is met
                    assert sorted(abs(e - L * (j + 1)) for j, e in enumerate(ends)) == list(range(1, m + 1))


def test_lane_plan_model_at_the_slice_floors():
    """floor 1 at n = 257: the level chain is longer than the fused tail reaches (T[1] > 256)"""
    for gid in range(4):
        p = me.lane_plan(gid, 257, 5, 1, lmin0=1)
        assert p["T"][0] == 257 * p["W"] and p["T"][1] > me.MSM_TAIL_THREADS
        p = me.lane_plan(gid, 257, 5, 1, lmin0=32)
        assert p["T"][1] <= me.MSM_TAIL_THREADS
        p = me.lane_plan(gid, 257, 5, 1, lmin0=4096)
        assert p["T"] == [4, 1]
