"""CPU: the NTT pass plan (hekaton_system_amd/csrc/ntt_plan.h) - which stages each launch of k_ntt_pass4 takes, and the
normalisation of HK_NTT_TILE_LOG / HK_NTT_UPPER_MAX.  Every plan must satisfy the kernel's contract (nst >= 1,
cols_bits <= lo, nst + cols_bits == the tile), for every transform size and every value the two knobs can be given."""
import pytest

from tests import ntt_plan


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return ntt_plan.load(tmp_path_factory.mktemp("ntt_plan"))


def test_knobs(plan):
    knobs, _ = plan
    for (rt, ru), (t, u) in knobs.items():
        assert t == min(max(rt, 8), 11)
        assert u == min(max(ru, 1), 10, t)
    assert knobs[11, 6] == (11, 6) and knobs[0, 0] == (8, 1) and knobs[13, 13] == (11, 10) and knobs[8, 10] == (8, 8)


def test_every_plan_meets_the_kernel_contract(plan):
    """The combination (tile_log 8, upper_max 10, logn 18) fails on the arithmetic NttHost::passes had before ntt_plan.h:
    upper_max was clamped to 10 whatever the tile, so rest = 10 went into one pass of nst = 10 and cols_bits = 8 - 10 wrapped
    to 0xFFFFFFFE (then `1u << cols_bits` in the kernel).  The clamp of upper_max to tile_log is what this loop pins: every
    (tile_log, raw upper_max) with raw upper_max > tile_log and logn - tile_log > tile_log fails without it."""
    _, plans = plan
    assert len(plans) == 33 * 4 * 13
    for (logn, tile_log, raw_um), (um, ps) in plans.items():
        tag = (logn, tile_log, raw_um, ps)
        assert um == min(max(raw_um, 1), 10, tile_log), tag
        assert len(ps) <= 34, tag
        if logn == 0:
            assert ps == [], tag
            continue
        lo = 0
        for p_lo, nst, cols_bits in ps:
            assert p_lo == lo and nst >= 1, tag
            lo += nst
        assert lo == logn, tag
        assert ps[0] == (0, min(logn, tile_log), 0), tag
        for p_lo, nst, cols_bits in ps[1:]:
            assert nst <= um, tag
            assert nst + cols_bits == tile_log, tag
            assert cols_bits <= p_lo and cols_bits < 32, tag


def test_wrapping_combination_is_legal_now(plan):
    _, plans = plan
    assert plans[18, 8, 10] == (8, [(0, 8, 0), (8, 5, 3), (13, 5, 3)])


def test_default_schedule(plan):
    """the lists of ntt_plan.h's header comment, literally"""
    _, plans = plan
    t, u = ntt_plan.DEFAULT_TILE_LOG, ntt_plan.DEFAULT_UPPER_MAX
    want = {11: [(0, 11, 0)],
            12: [(0, 11, 0), (11, 1, 10)],
            16: [(0, 11, 0), (11, 5, 6)],
            17: [(0, 11, 0), (11, 6, 5)],
            21: [(0, 11, 0), (11, 5, 6), (16, 5, 6)],
            22: [(0, 11, 0), (11, 6, 5), (17, 5, 6)]}
    for logn, ps in want.items():
        assert plans[logn, t, u] == (u, ps), logn
