"""CPU: the plan rule of a compacted query (hekaton_system_amd/csrc/msm.cuh msm_sub_plan, msm_compact_rule, msm_rank_table,
compiled for the host: tests/host_shim/msm_sublist_driver.cpp).  A sub-list reuses the digits of the assignment's one sort,
so its plan shares c, W, WP, F, B, NB, K and kconst with plan_z even where a vector of its own length would pick another
window; n, gshift and the lane counts are its own.  The rank table is the inverse of the index list."""
import subprocess

import pytest

from tests import host_build

NONE = 0xFFFFFFFF
FIELDS = ("c", "W", "WP", "F", "B", "NB", "K", "n", "gshift", "chunk", "T0", "n_levels", "kconst")
# (n, n_sub): the default bench class and its A / B lists, the smallest class that compacts, a sub-list far shorter than its
# source, one of a single scalar, and one as long as its source
SHAPES = [(1300007, 717000), (1300007, 673000), (4100, 2200), (23007, 12000), (200000, 4097), (70000, 1), (5000, 5000)]


def pick_c_tables(n, bits=254):
    """Python copy of msm_pick_c_tables (csrc/curve_ops_impl.cuh), the window hk_pk_upload gives plan_z"""
    best, best_cost = 6, 1e300
    for c in range(5, 17):
        W = (bits + 2 + c - 1) // c
        cost = n * W + 6.0 * (1 << (c - 1))
        if cost < best_cost:
            best, best_cost = c, cost
    return best


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msm_sublist") / "msm_sublist_driver")
    host_build.build("msm_sublist_driver.cpp", exe, "-O1", "-Wall", "-Werror")
    args = [str(v) for n, k in SHAPES for v in (n, pick_c_tables(n), k)]
    plans, rules, rank = {}, {}, None
    for line in subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        if f[0] == "plan":
            parts = line.split("|")
            plans[int(f[1]), int(f[3])] = tuple(dict(zip(FIELDS, map(int, p.split()))) for p in parts[1:3])
        elif f[0] == "rule":
            rules[int(f[1]), int(f[2])] = int(f[3])
        else:
            _, idx, rk = line.split(":")
            rank = (list(map(int, idx.split())), list(map(int, rk.split())))
    return plans, rules, rank


def test_sub_plan_shares_the_windows_and_buckets_of_its_source(out):
    plans, _, _ = out
    assert sorted(plans) == sorted(SHAPES)
    differs = 0
    for (n, k), (pz, ps) in plans.items():
        assert pz["n"] == n and pz["c"] == pick_c_tables(n)
        for f in ("c", "W", "WP", "F", "B", "NB", "K", "kconst"):
            assert ps[f] == pz[f], (n, k, f)
        assert ps["n"] == k
        assert ps["gshift"] == max(1, (k - 1).bit_length()) and (1 << ps["gshift"]) >= k
        assert ps["gshift"] <= pz["gshift"]
        # its lanes are planned for its own longest list, k W entries, as msm_make_plan would
        assert ps["T0"] == min(262144, max(1, -(-k * ps["W"] // 32)))
        assert ps["chunk"] == max(1024, -(-k // 512))
        differs += pick_c_tables(k) != pz["c"]
    assert differs >= 3, "no shape left where the sub-list's own length would pick another window"


def test_compact_rule(out):
    _, rules, _ = out
    assert rules == {(4095, 0): 0, (4096, 0): 1, (4096, 3071): 1, (4096, 3072): 0, (4096, 3073): 0, (100000, 74999): 1,
                     (100000, 75000): 0}


def test_rank_table_is_the_inverse_of_the_index_list(out):
    _, _, (idx, rank) = out
    assert len(rank) == 50 and len(set(idx)) == len(idx)
    for k, i in enumerate(idx):
        assert rank[i] == k
    for i, r in enumerate(rank):
        assert (r == NONE) == (i not in idx)
        if r != NONE:
            assert idx[r] == i
