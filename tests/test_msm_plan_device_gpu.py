"""GPU: the product's MSM launch sequence (msm_make_plan, MsmRun::build_tables, MsmSort::run, MsmRun::run, to_affine of
csrc/msm_driver_impl.cuh) under plans the TEST forces, through dshim_msm of tests/device_shim/ec_dev_shim.hip.

The pickers give the suite's sizes c = 4, 6, 10, 11, 12 (plain) and 12, 13, 16 (tables); here every window size 3 .. 16 runs
with shift tables (WP = 1, F = W) and every one whose W 2^(c-1) counters fit the sort's LDS histogram runs plain (WP = W),
on all four groups, over the directed scalars and vectors of tests/msm_edges.py: one bucket holding every entry, the extreme
digit -2^(c-1), bucket ends on slice ends, equal partial sums meeting in the level chain, P and -P cancelling in mid-run,
no non-zero digit at all (E = 0), bases at infinity, the L-query's index window, three proofs in lock-step.  Shapes stay
at n <= 257: the schedule's regimes come from c, WP and the slice floor, not from n.

Every result is compared exactly with reference(ks, scalars) = ((sum s_i k_i) mod r) G - one Python scalar
multiplication from the bases' known discrete logs, independent of any bucket schedule.
"""
import json
import os
import subprocess
import sys

import pytest

from oracle.pyref.codec import Codec
from oracle.pyref.params import CURVES
from tests import dev_shim as ds
from tests import msm_edges as me

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HK_ERR_ARG = 4
N = 65
TABLES, PLAIN = "tables", "plain"
FAMILY_PLANS = ((5, TABLES), (16, TABLES), (4, PLAIN), (11, PLAIN))

_codecs = {}
_enc_cache = {}


def codec(gid):
    cname = me.GROUPS[gid][0]
    if cname not in _codecs:
        _codecs[cname] = Codec(CURVES[cname])
    return _codecs[cname]


def enc_bases(gid, ks):
    key = (gid, tuple(ks))
    if key not in _enc_cache:
        cd = codec(gid)
        pts = me.points(gid, ks)
        _enc_cache[key] = (cd.g1_vec(pts) if me.GROUPS[gid][1] == "g1" else cd.g2_vec(pts)).tobytes()
    return _enc_cache[key]


def point_bytes(gid):
    cd = codec(gid)
    return cd.g1_bytes if me.GROUPS[gid][1] == "g1" else cd.g2_bytes


def decode(gid, buf):
    cd = codec(gid)
    return cd.g1_from(buf) if me.GROUPS[gid][1] == "g1" else cd.g2_from(buf)


def wp_of(gid, c, kind):
    return 1 if kind == TABLES else me.num_windows(c, me.GROUPS[gid][0])


def run_vec(shim, gid, c, WP, v, mont):
    """one MSM over vector v -> (status, affine point or None, plan words)"""
    cd = codec(gid)
    sc = (cd.fr_vec_mont if mont else cd.fr_vec_canon)(v["scalars"]).tobytes()
    st, out, plan = shim.msm(gid, c, WP, len(v["scalars"]), enc_bases(gid, v["ks"]), sc, mont, n_bases=len(v["ks"]),
                             idx_off=v["idx_off"], point_bytes=point_bytes(gid))
    return st, (decode(gid, out) if st == 0 else None), plan


BOTH_FORMS = ("uniform", "named")


def batches(gid, c, vecs):
    """How a list of vectors is sent to the device: vectors over the same bases share one call (and one build of the shift
    tables) as a lock-step batch of up to 4, alternately with Montgomery and canonical scalars; the others run alone; the
    `uniform` and `named` vectors then run once more, alone, in the OTHER scalar form, so every plan sees both forms.
    -> [(part, ks, idx_off, n, mont)], the same list in the test process and in a child."""
    groups = {}
    for v in vecs:
        groups.setdefault((tuple(v["ks"]), v["idx_off"], len(v["scalars"])), []).append(v)
    out, again = [], []
    for call, ((ks, off, n), vs) in enumerate(groups.items()):
        for lo in range(0, len(vs), 4):
            mont = (call + lo // 4 + c) % 2 == 0
            out.append((vs[lo:lo + 4], ks, off, n, mont))
            again += [([v], ks, off, n, not mont) for v in vs[lo:lo + 4] if v["name"] in BOTH_FORMS]
    return out + again


def run_batch(shim, gid, c, WP, batch):
    """-> (status, result bytes or None, plan words)"""
    part, ks, off, n, mont = batch
    cd = codec(gid)
    sc = b"".join((cd.fr_vec_mont if mont else cd.fr_vec_canon)(v["scalars"]).tobytes() for v in part)
    return shim.msm(gid, c, WP, n, enc_bases(gid, ks), sc, mont, batch=len(part), n_bases=len(ks), idx_off=off,
                    point_bytes=point_bytes(gid))


def check_batch(gid, c, WP, batch, st, out, plan, lmin0=32, tag=""):
    """each proof of the batch against its own reference; the plan words against the Python model of the schedule"""
    part, ks, off, n, mont = batch
    pb = point_bytes(gid)
    what = "%sg%d c=%d WP=%d n=%d %s" % (tag, gid, c, WP, n, "mont" if mont else "canon")
    assert st == 0, "%s %s: status %d" % (what, [v["name"] for v in part], st)
    for b, v in enumerate(part):
        got, want = decode(gid, out[b * pb:(b + 1) * pb]), me.reference(gid, v["ks"], v["scalars"], off)
        assert got == want, "%s %s (proof %d of %d): got %r, want %r" % (what, v["name"], b, len(part), got, want)
        if v["name"] in ("zeros", "inf_bases_all") or (v["name"] == "plus_minus" and n % 2 == 0):
            assert want is None                 # the E = 0 pass and the full cancellation: the reference is infinity
    model = me.lane_plan(gid, n, c, WP, batch=len(part), lmin0=lmin0)
    T1 = model["T"][1] if model["n_levels"] > 1 else 0
    assert list(plan[:7]) == [model["W"], model["F"], model["NB"], model["n_levels"], model["T"][0], T1, lmin0], what
    assert plan[8] == model["lanes"], "%s: the device plans for %d lanes, the model for %d" % (what, plan[8], model["lanes"])


def check_vecs(shim, gid, c, WP, vecs):
    """every vector of `vecs` (see `batches`), each against its own reference.  Returns the plan words of the last call."""
    plan = None
    for batch in batches(gid, c, vecs):
        st, out, plan = run_batch(shim, gid, c, WP, batch)
        check_batch(gid, c, WP, batch, st, out, plan)
    return plan


@pytest.fixture(scope="module")
def shim():
    return ds.load_ec("asm")


def window_size_vectors(gid, c, n=N):
    """the vectors every window size runs: uniform, one scalar everywhere (every digit extreme, every digit equal), and the
    named scalars in one vector"""
    cname = me.GROUPS[gid][0]
    named = me.named_scalars(cname, c)
    u = me.uniform(gid, n, "named")
    u["scalars"] = me.sprinkle(u["scalars"], named[:n], "c%d" % c)
    u["name"] = "named"
    assert set(named[:n]) <= set(u["scalars"])
    return [
        me.uniform(gid, n),
        me.all_equal(gid, n, me.all_min(cname, c), "all_equal_all_min"),
        me.all_equal(gid, n, me.all_max(cname, c), "all_equal_all_max"),
        me.all_equal(gid, n, me.one_bucket(cname, c, 1), "all_equal_one_bucket_first"),
        me.all_equal(gid, n, me.one_bucket(cname, c, -(1 << (c - 1)) + 1), "all_equal_one_bucket_inner"),
        u,
    ]


@pytest.mark.parametrize("gid", range(4))
def test_every_window_size_with_tables(shim, gid):
    cname = me.GROUPS[gid][0]
    for c in me.C_ALL:
        plan = check_vecs(shim, gid, c, 1, window_size_vectors(gid, c))
        assert plan[0] == plan[1] == me.num_windows(c, cname) and plan[2] == 1 << (c - 1)


@pytest.mark.parametrize("gid", range(4))
def test_every_window_size_plain(shim, gid):
    """WP = W: every window keeps its own buckets and the result goes through bucket_reduce / window_sum / the Horner
    tail; W 2^(c-1) counters must fit the LDS histogram, and MsmSort::run refuses the plan (HK_ERR_ARG) when they do not"""
    cname = me.GROUPS[gid][0]
    ran, refused = [], []
    for c in me.C_ALL:
        W = me.num_windows(c, cname)
        if W << (c - 1) > me.MSM_LDS_COUNTERS:
            st, _got, _plan = run_vec(shim, gid, c, W, me.uniform(gid, N), mont=True)
            assert st == HK_ERR_ARG, "c=%d WP=%d: status %d, want HK_ERR_ARG" % (c, W, st)
            refused.append(c)
            continue
        plan = check_vecs(shim, gid, c, W, window_size_vectors(gid, c))
        assert plan[0] == W and plan[1] == 1 and plan[2] == W << (c - 1)
        ran.append(c)
    assert ran == list(range(3, 12)) and refused == list(range(12, 17))


def family_vectors(gid, c, n):
    if n >= 33:
        return me.vector_families(gid, n, c)
    cname = me.GROUPS[gid][0]
    out = [me.uniform(gid, n), me.all_equal(gid, n, me.all_min(cname, c), "all_equal_all_min"), me.zeros(gid, n),
           me.one_base(gid, n), me.inf_bases(gid, n, every=True), me.window(gid, n, 0, n)]
    return out


@pytest.mark.parametrize("c,kind", FAMILY_PLANS)
@pytest.mark.parametrize("gid", range(4))
def test_vector_families(shim, gid, c, kind):
    WP = wp_of(gid, c, kind)
    for n in SIZES:
        check_vecs(shim, gid, c, WP, family_vectors(gid, c, n))


@pytest.mark.parametrize("gid", range(4))
def test_batch_of_three_proofs(shim, gid):
    """three MSMs over one table in lock-step launches: per-proof strides of every buffer, and the ticket behind each
    proof's buckets; one proof has no non-zero digit, one has every digit extreme"""
    cname = me.GROUPS[gid][0]
    cd = codec(gid)
    ks = me.pool_ks(gid)[:N]
    for c, kind in ((5, TABLES), (16, TABLES), (11, PLAIN)):
        WP = wp_of(gid, c, kind)
        vecs = [me.uniform(gid, N)["scalars"], [0] * N, [me.all_min(cname, c)] * N]
        for order in (vecs, vecs[::-1], [vecs[1], vecs[0], vecs[2]]):
            sc = b"".join(cd.fr_vec_mont(s).tobytes() for s in order)
            st, out, _plan = shim.msm(gid, c, WP, N, enc_bases(gid, ks), sc, True, batch=3, point_bytes=point_bytes(gid))
            assert st == 0
            pb = point_bytes(gid)
            for b, s in enumerate(order):
                got = decode(gid, out[b * pb:(b + 1) * pb])
                assert got == me.reference(gid, ks, s), "g%d c=%d %s proof %d" % (gid, c, kind, b)


# ---- slice floor: HK_MSM_LMIN0 is read once per process -----------------------------------------------------------------
CHILD_GROUPS = (0, 3)                                  # BN254 G1, BLS12-381 G2
SIZES = (1, 63, 64, 65, 257)
_CHILD = "import sys; sys.path.insert(0, %(root)r); from tests import test_msm_plan_device_gpu as t; t.child_main(%(gid)d)"


def child_cases(gid):
    """the whole vector-family block of test_vector_families for one group: four plans, five sizes"""
    for c, kind in FAMILY_PLANS:
        for n in SIZES:
            for batch in batches(gid, c, family_vectors(gid, c, n)):
                yield c, wp_of(gid, c, kind), batch


def child_main(gid):
    """runs the block and prints [[status, result bytes as hex, plan words], ...] as one JSON line"""
    shim = ds.load_ec("asm")
    out = []
    for c, WP, batch in child_cases(gid):
        st, res, plan = run_batch(shim, gid, c, WP, batch)
        out.append([st, res.hex() if st == 0 else None, plan])
        if st != 0:
            break                                       # nothing further on the GPU after a failed run
    print(json.dumps(out))


@pytest.mark.parametrize("gid", CHILD_GROUPS)
@pytest.mark.parametrize("floor", [1, 32, 4096])
def test_slice_floor_in_a_child_process(floor, gid):
    """floor 1: one entry per lane, the longest level chain (k_msm_accum_lvl launches before the fused tail); 32: the
    default; 4096: a few lanes own everything, every run spans many buckets.  One child per floor and group, each running
    the whole block of test_vector_families for its group."""
    env = dict(os.environ)
    env["HK_MSM_LMIN0"] = str(floor)
    res = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "gid": gid}], env=env, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, "child (floor %d, g%d) exited with %d: %s" % (floor, gid, res.returncode, res.stderr[-2000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    cases = list(child_cases(gid))
    assert len(got) == len(cases)
    wide = 0
    for (c, WP, batch), (st, hexres, plan) in zip(cases, got):
        check_batch(gid, c, WP, batch, st, bytes.fromhex(hexres) if hexres else None, plan, lmin0=floor, tag="floor %d " % floor)
        wide += plan[5] > me.MSM_TAIL_THREADS
    if floor == 1:
        # at n = 257 level 1 is too wide for the fused tail under every plan: k_msm_accum_lvl launches ran
        for c, kind in FAMILY_PLANS:
            assert me.lane_plan(gid, 257, c, wp_of(gid, c, kind), batch=4, lmin0=1)["T"][1] > me.MSM_TAIL_THREADS
        assert wide >= len(FAMILY_PLANS)
