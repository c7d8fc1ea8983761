"""GPU: the group sweeps of csrc/fixed_base.cuh and csrc/endo.cuh, ONE kernel launch per call through
tests/device_shim/sweep_dev_shim.hip, on the directed cases of tests/sweep_edges.py (whose premises
tests/test_sweep_edges_cpu.py asserts), in all four groups.

Through the library these kernels sit behind MsmRun's choices: the window table always comes from the base, the form of the
element-wise product from n, and only random vectors reach the sums.  Here a crafted table makes k_fb_mul's mixed add double
and cancel in mid-walk, equal and opposite points meet at every level of k_points_sum_seg's LDS tree, the trailing add of the
split forms meets lo = c hi and lo = -c hi, and every size sits around the workgroup of its kernel (the sizes come from the
shim's getters).  Every result is compared exactly with the big-int oracle: points are k G with known k, the expected value
is ((combination of the logs) mod r) G.  Every XYZZ result must also satisfy zz^3 = zzz^2.
"""
import pytest

from tests import dev_shim as ds
from tests import msm_edges as me
from tests import sweep_edges as se

pytestmark = pytest.mark.gpu

FORMS = [(0, ds.SPLIT_K_LANE), (1, ds.SPLIT_K_LANE), (1, ds.SPLIT_QUAD), (2, ds.SPLIT_K_LANE), (3, ds.SPLIT_K_LANE),
         (3, ds.SPLIT_QUAD)]
FORM_IDS = ["g%d-%s" % (g, "quad" if f else "klane") for g, f in FORMS]


@pytest.fixture(scope="module")
def shim():
    return ds.load_sweep()


Io = se.Io


def _check(got, want, what):
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, "%s: elements %r differ (of %d)" % (what, bad[:8], len(want))


# ---- getters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", range(4))
def test_getters_match_the_tables_the_cpu_premises_use(gid, shim):
    g2 = gid in (1, 3)
    assert shim.sum_threads(gid) == se.SUM_THREADS[gid]
    assert shim.split_elems(gid, ds.SPLIT_K_LANE) == 64 // se.SPLIT_K[gid] == (16 if g2 else 32)
    assert shim.split_elems(gid, ds.SPLIT_QUAD) == (4 if g2 else 0)
    assert (shim.split_nd(gid), shim.split_steps(gid)) == (se.SPLIT_ND[gid], se.SPLIT_STEPS[gid])
    if not g2:                                               # no quad form in G1: refused, nothing launched
        io = Io(gid)
        st, _ = shim.mul_split_status(gid, io.pb, ds.SPLIT_QUAD, 0, io.aff([1]), io.fr([1]), 1)
        assert st == -ds.HIP_NOT_SUPPORTED


# ---- k_fb_table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", range(4))
def test_window_table_entries(gid, shim):
    io = Io(gid)
    k = me.pool_ks(gid)[0]
    table = shim.fb_table(gid, io.pb, io.aff([k]))
    rn = se.rnd(gid, "table")
    picks = [(w, j) for w in (0, 1, 31) for j in (0, 1, 2, 255)] + [(rn.randrange(32), rn.randrange(256)) for _ in range(16)]
    for w, j in picks:
        e = table[(w * 256 + j) * io.pb:(w * 256 + j + 1) * io.pb]
        assert io.from_aff(e) == io.want([(j << (8 * w)) * k]), (gid, w, j)
        if j == 0:
            assert e == bytes(io.pb)
    assert shim.fb_table(gid, io.pb, bytes(io.pb)) == bytes(32 * 256 * io.pb)


# ---- k_fb_mul ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", range(4))
def test_digit_walk_one_window_at_a_time(gid, shim):
    """1 2^(8w) and 255 2^(8w) for every window, the top window's largest digit, 0 and r - 1, in both scalar forms"""
    io = Io(gid)
    k = me.pool_ks(gid)[0]
    table = shim.fb_table(gid, io.pb, io.aff([k]))
    scalars = [s for _, _, s in se.fb_window_scalars(gid)] + [0, io.r - 1]
    want = io.want([s * k for s in scalars])
    assert want[-2] is None
    for mont in (True, False):
        got = io.from_xyzz(shim.fb_mul(gid, io.pb, table, io.fr(scalars, mont), mont))
        _check(got, want, "g%d k_fb_mul mont=%d" % (gid, mont))


@pytest.mark.parametrize("kind", ["dbl", "cancel"])
@pytest.mark.parametrize("gid", range(4))
def test_digit_walk_over_a_crafted_table(gid, kind, shim):
    """two windows' entries equal (the mixed add doubles) or opposite (it gives infinity and the walk goes on)"""
    io = Io(gid)
    logs = se.crafted_table(gid, kind)
    table = io.aff(logs)
    for n in (1, 63, 64, 65):
        scalars = [se.CRAFTED_SCALARS[i % len(se.CRAFTED_SCALARS)] for i in range(n)]
        want = io.want([se.fb_walk(logs, s, io.r)[0] for s in scalars])
        for mont in ((False, True) if n == 65 else (False,)):
            got = io.from_xyzz(shim.fb_mul(gid, io.pb, table, io.fr(scalars, mont), mont))
            _check(got, want, "g%d %s n=%d mont=%d" % (gid, kind, n, mont))


# ---- k_points_lincomb -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("gid", range(4))
def test_lincomb_cases(gid, k, n, shim):
    io = Io(gid)
    for name, vecs, coeffs in se.lincomb_cases(gid, k, n):
        buf = b"".join(io.aff(v) for v in vecs)
        got = io.from_xyzz(shim.lincomb(gid, io.pb, buf, io.fr(coeffs), k, n))
        want = io.want(se.lincomb_expected(gid, vecs, coeffs))
        assert want[0] is None
        _check(got, want, "g%d lincomb %s k=%d n=%d" % (gid, name, k, n))


# ---- k_points_sum_seg: one segment of PointsSum<F>::THREADS lanes, segments of 64 -----------------------------------------
@pytest.mark.parametrize("gid", range(4))
def test_points_sum_around_the_workgroup(gid, shim):
    io = Io(gid)
    T = shim.sum_threads(gid)
    for n in (1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 5 * T + 3):
        for name in se.SUM_FAMILIES:
            fam = se.sum_family(gid, name, n)
            got = io.from_xyzz(shim.points_sum(gid, io.pb, io.xyzz(fam)))
            assert got == io.want([sum(k for k, _ in fam)]), "g%d k_points_sum_seg, one segment, %s n=%d" % (gid, name, n)


@pytest.mark.parametrize("gid", range(4))
def test_points_sum_seg_keeps_the_segments_apart(gid, shim):
    io = Io(gid)
    names = list(se.SUM_FAMILIES)
    for seg in (1, 17, 63, 64, 65, 129):
        for batch in (1, 3):
            # every family in every segment, and a row of three different families
            rows = [[se.sum_family(gid, name, seg, slot=b) for b in range(batch)] for name in names]
            rows.append([se.sum_family(gid, names[(b + seg) % len(names)], seg, slot=b) for b in range(batch)])
            for row in rows:
                data = b"".join(io.xyzz(fam) for fam in row)
                got = io.from_xyzz(shim.points_sum_seg(gid, io.pb, data, seg, batch))
                want = io.want([sum(k for k, _ in fam) for fam in row])
                _check(got, want, "g%d k_points_sum_seg seg=%d batch=%d" % (gid, seg, batch))


# ---- k_points_mul_split ------------------------------------------------------------------------------------------------------
def _sizes(E):
    return sorted({1, E - 1, E, E + 1, 2 * E + 1} - {0})


@pytest.mark.parametrize("gid,form", FORMS, ids=FORM_IDS)
def test_split_per_element_scalars(gid, form, shim):
    """out[i] = s_i P_i, the split done by every lane: against the oracle at every element and against both one-lane kernels"""
    io = Io(gid)
    E = shim.split_elems(gid, form)
    named = se.split_scalars(gid)
    for n in _sizes(E):
        scalars = [named[(i + n) % len(named)] for i in range(n)]
        logs = se.split_points(gid, n, inf_at=(2,))
        pts = io.aff(logs)
        want = io.want([s * k for s, k in zip(scalars, logs)])
        for mont in (1, 0):
            got = io.from_xyzz(shim.mul_split(gid, io.pb, form, 0, pts, io.fr(scalars, mont), n, mont=mont))
            _check(got, want, "g%d form %d n=%d mont=%d" % (gid, form, n, mont))
        for kind in (ds.MUL_PLAIN, ds.MUL_ENDO):
            got = io.from_xyzz(shim.scalar_mul(gid, io.pb, kind, pts, io.fr(scalars)))
            _check(got, want, "g%d one-lane kind %d n=%d" % (gid, kind, n))
    # with lo: the trailing add after a per-element product
    n = E + 1
    scalars = [named[i % len(named)] for i in range(n)]
    logs = se.split_points(gid, n)
    lo = [0 if i % 4 == 3 else (s * k if i % 4 == 1 else -s * k if i % 4 == 2 else me.pool_ks(gid)[40]) % io.r
          for i, (s, k) in enumerate(zip(scalars, logs))]
    got = io.from_xyzz(shim.mul_split(gid, io.pb, form, 0, io.aff(logs), io.fr(scalars), n, lo=io.aff(lo)))
    _check(got, io.want([l + s * k for l, s, k in zip(lo, scalars, logs)]), "g%d form %d with lo" % (gid, form))


@pytest.mark.parametrize("gid,form", FORMS, ids=FORM_IDS)
def test_split_uniform_scalar_every_sign_mask(gid, form, shim):
    """out_y[i] = lo_y[i] + c hi_y[i] with c given as K magnitudes and a sign mask: every mask, the magnitudes at the digit
    edges up to 0x77..7, `vectors` in {1, 3, 4}; lo = c hi, lo = -c hi, lo and hi at infinity inside every vector"""
    io = Io(gid)
    E = shim.split_elems(gid, form)
    cases = se.uniform_cases(gid)
    assert {m for _, m in cases} == set(range(1 << se.SPLIT_K[gid]))
    assert se.mag_limit(gid) in {m for mags, _ in cases for m in mags}
    runs = [(E + 1, 1, c) for c in range(len(cases))]
    turn = 0
    for n in _sizes(E):
        for vectors in (1, 3, 4):
            for _ in range(2):
                runs.append((n, vectors, turn % len(cases)))
                turn += 1
    for n, vectors, ci in runs:
        mags, mask = cases[ci]
        c = se.fold_scalar(gid, mags, mask)
        pairs = [se.fold_vectors(gid, c, n, tag=y) for y in range(vectors)]
        lo = b"".join(io.aff(l) for l, _ in pairs)
        hi = b"".join(io.aff(h) for _, h in pairs)
        got = io.from_xyzz(shim.mul_split(gid, io.pb, form, 1, hi, io.fr(mags), n, lo=lo, neg=mask, vectors=vectors))
        want = [p for l, h in pairs for p in io.want(se.fold_expected(gid, c, l, h))]
        what = "g%d form %d n=%d vectors=%d mags=%r mask=%d" % (gid, form, n, vectors, [hex(m) for m in mags], mask)
        _check(got, want, what)
        # the one-lane kernel on the first pair
        one = io.from_xyzz(shim.fold_endo(gid, io.pb, io.aff(pairs[0][0]), io.aff(pairs[0][1]), io.fr(mags), mask))
        _check(one, want[:n], "k_points_fold_endo " + what)
    # no lo vector at all
    mags, mask = cases[1]
    c = se.fold_scalar(gid, mags, mask)
    _, h = se.fold_vectors(gid, c, E + 1)
    got = io.from_xyzz(shim.mul_split(gid, io.pb, form, 1, io.aff(h), io.fr(mags), E + 1, neg=mask))
    _check(got, io.want([c * x for x in h]), "g%d form %d uniform, lo = null" % (gid, form))


@pytest.mark.parametrize("gid,form", FORMS, ids=FORM_IDS)
def test_split_rows_over_one_short_base_set(gid, form, shim):
    """pts_mod = 17 under 5 rows of scalars (hk_commit_batch's shape): rows straddle workgroups, one base is at infinity;
    then the rows' sums through k_points_sum_seg"""
    io = Io(gid)
    seg, batch = 17, 5
    n = seg * batch
    assert n % shim.split_elems(gid, form) != 0 and seg % shim.split_elems(gid, form) != 0
    named = se.split_scalars(gid)
    bases = [0 if t == 5 else me.pool_ks(gid)[30 + t] for t in range(seg)]
    scalars = [named[(3 * i + 1) % len(named)] for i in range(n)]
    logs = [s * bases[i % seg] for i, s in enumerate(scalars)]
    out = shim.mul_split(gid, io.pb, form, 0, io.aff(bases), io.fr(scalars), n, pts_mod=seg)
    _check(io.from_xyzz(out), io.want(logs), "g%d form %d pts_mod" % (gid, form))
    rows = io.from_xyzz(shim.points_sum_seg(gid, io.pb, out, seg, batch))
    _check(rows, io.want([sum(logs[b * seg:(b + 1) * seg]) for b in range(batch)]), "g%d form %d row sums" % (gid, form))
