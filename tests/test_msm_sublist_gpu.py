"""GPU: MsmSort::sublist (csrc/msm.cuh k_msm_sub_mark / k_msm_sub_emit / k_msm_sub_starts, scan_u32 between them) - the
A and B queries' entry lists, derived from the one digit sort of the assignment by stream compaction.

Part 1 drives the launch sequence through tests/device_shim/sublist_dev_shim.hip on sorted lists built here, and compares
`sorted` and `start` of the sub-list word for word with a numpy filter of the source: kept entries in the source's order,
index renumbered through the rank table, group field moved to the sub-list's gshift, sign bit kept; every word behind the
kept entries as it lay before the call.  n <= 4096 scalars and c = 4 .. 8, so that NB is 8 .. 128 and buckets are long.

Part 2: hk_prove on a key whose A and B queries both run compacted, and on one where neither meets the rule, against the
C oracle's proof of the same inputs, byte for byte.
"""
import numpy as np
import pytest

from tests import dev_shim as ds

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
TILE = 1024
SENTINEL = 0xA5A5A5A5


class Plan:
    def __init__(self, c, n, n_dst):
        self.c, self.n, self.n_dst = c, n, n_dst
        self.W, self.NB, self.gs_src, self.gs_dst, self.stride_src, self.stride_dst, self.tiles = ds.load_sublist().plan(c, n, n_dst)
        assert self.NB == 1 << (c - 1) and self.stride_src == n * self.W + 1 and self.stride_dst == n_dst * self.W + 1
        assert self.tiles == n * self.W // TILE + 1


def make_list(plan, counts, rnd, idx=None):
    """a sorted list with counts[b] entries in bucket b: random scalar index (or idx), table group and sign per entry"""
    counts = np.asarray(counts, dtype=np.int64)
    assert len(counts) == plan.NB
    E = int(counts.sum())
    assert E <= plan.n * plan.W
    if idx is None:
        idx = rnd.integers(0, plan.n, E)
    idx = np.asarray(idx, dtype=np.uint32)
    grp = rnd.integers(0, plan.W, E).astype(np.uint32)            # WP = 1: W table groups
    sign = rnd.integers(0, 2, E).astype(np.uint32)
    entries = (sign << np.uint32(31)) | (grp << np.uint32(plan.gs_src)) | idx
    start = np.zeros(plan.NB + 1, dtype=np.uint32)
    start[1:] = np.cumsum(counts)
    return entries.astype(np.uint32), start


def reference(plan, entries, start, rank):
    """the filter: kept entries in order, renumbered; start_dst[b] = kept entries below start_src[b]"""
    idx = entries & np.uint32((1 << plan.gs_src) - 1)
    grp = (entries & np.uint32(0x7FFFFFFF)) >> np.uint32(plan.gs_src)
    keep = rank[idx] != NONE
    out = (entries[keep] & np.uint32(0x80000000)) | (grp[keep] << np.uint32(plan.gs_dst)) | rank[idx[keep]]
    below = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint32)
    return out.astype(np.uint32), below[start]


def run_sublist(plan, lists, rank):
    """lists: one (entries, start) per proof -> [(sorted slice, start slice)] as the device left them"""
    batch = len(lists)
    src = np.full(batch * plan.stride_src, SENTINEL, dtype=np.uint32)
    st = np.zeros(batch * (plan.NB + 1), dtype=np.uint32)
    for b, (e, s) in enumerate(lists):
        src[b * plan.stride_src:b * plan.stride_src + len(e)] = e
        st[b * (plan.NB + 1):(b + 1) * (plan.NB + 1)] = s
    dst = np.full(batch * plan.stride_dst, SENTINEL, dtype=np.uint32)
    dst_st = np.full(batch * (plan.NB + 1), SENTINEL, dtype=np.uint32)
    rank = np.ascontiguousarray(rank, dtype=np.uint32)
    ds.load_sublist().sublist(plan.c, batch, plan.n, plan.n_dst, src, st, rank, dst, dst_st)
    return [(dst[b * plan.stride_dst:(b + 1) * plan.stride_dst], dst_st[b * (plan.NB + 1):(b + 1) * (plan.NB + 1)])
            for b in range(batch)]


def check(plan, lists, rank):
    got = run_sublist(plan, lists, rank)
    kept_total = 0
    for (e, s), (gs, gst) in zip(lists, got):
        want, want_st = reference(plan, e, s, rank)
        assert np.array_equal(gst, want_st), "start"
        assert np.array_equal(gs[:len(want)], want), "sorted"
        assert (gs[len(want):] == SENTINEL).all(), "a word behind the kept entries was written"
        kept_total += len(want)
    return kept_total


def rank_all(n):
    return np.arange(n, dtype=np.uint32), n


def rank_even(n):
    r = np.full(n, NONE, dtype=np.uint32)
    r[0::2] = np.arange((n + 1) // 2, dtype=np.uint32)
    return r, (n + 1) // 2


def spread(rnd, NB, E):
    """E entries over NB buckets, every bucket long"""
    cuts = np.sort(rnd.integers(0, E + 1, NB - 1))
    return np.diff(np.concatenate([[0], cuts, [E]]))


@pytest.mark.parametrize("c", [4, 6, 8])
def test_keep_all_and_keep_none(c):
    rnd = np.random.default_rng(c)
    n = 1500
    p = Plan(c, n, n)
    lst = make_list(p, spread(rnd, p.NB, 5000), rnd)
    rank, _ = rank_all(n)
    assert check(p, [lst], rank) == 5000
    # the identity renumbering under one plan: the sub-list IS the source list
    got, got_st = run_sublist(p, [lst], rank)[0]
    assert np.array_equal(got[:5000], lst[0]) and np.array_equal(got_st, lst[1])
    # keep none: every bucket empty, nothing written
    p0 = Plan(c, n, 1)
    assert check(p0, [lst], np.full(n, NONE, dtype=np.uint32)) == 0
    assert (run_sublist(p0, [lst], np.full(n, NONE, dtype=np.uint32))[0][1] == 0).all()


@pytest.mark.parametrize("c,n", [(4, 4096), (5, 1025), (7, 333)])
def test_every_other_index_keeps_the_sign_and_moves_the_group(c, n):
    rnd = np.random.default_rng(100 + c)
    rank, n_dst = rank_even(n)
    p = Plan(c, n, n_dst)
    assert p.gs_dst == p.gs_src - 1                               # the group field really moves
    e, s = make_list(p, spread(rnd, p.NB, 7001), rnd)
    kept = check(p, [(e, s)], rank)
    assert 0 < kept < 7001
    want, _ = reference(p, e, s, rank)
    assert (want >> 31).any() and not (want >> 31).all()          # negative and positive digits among the kept entries


def test_heavy_bucket_over_three_tiles_with_both_boundaries_straddled():
    """scalar = 1 in most positions: bucket 0 holds 2500 entries; around positions 1023 | 1024 and 2047 | 2048 the entries
    alternate kept, dropped / dropped, kept, so both tile boundaries fall between a kept and a dropped entry"""
    rnd = np.random.default_rng(7)
    c, n = 5, 3000
    rank, n_dst = rank_even(n)
    p = Plan(c, n, n_dst)
    counts = np.zeros(p.NB, dtype=np.int64)
    counts[0], counts[1], counts[p.NB - 1] = 2500, 40, 3
    idx = rnd.integers(0, n, int(counts.sum()))
    idx[1022:1026] = [10, 12, 13, 14]        # kept, kept | dropped, kept
    idx[2046:2050] = [21, 23, 24, 25]        # dropped, dropped | kept, dropped
    e, s = make_list(p, counts, rnd, idx)
    assert s[1] == 2500 > 2 * TILE
    check(p, [(e, s)], rank)


def test_empty_buckets_at_the_start_the_end_and_on_a_tile_boundary():
    rnd = np.random.default_rng(8)
    c, n = 4, 2048
    rank, n_dst = rank_even(n)
    p = Plan(c, n, n_dst)
    assert p.NB == 8
    #         empty | ends at 1024 | empty on the boundary | all dropped | ... | ends at 2048 | empty | empty
    counts = [0, 1024, 0, 17, 500, 507, 0, 0]
    idx = rnd.integers(0, n, sum(counts))
    idx[1024:1041] |= 1                                              # bucket 3 loses every entry
    e, s = make_list(p, counts, rnd, idx)
    assert s[2] == s[3] == TILE and s[6] == 2 * TILE
    check(p, [(e, s)], rank)
    got_st = run_sublist(p, [(e, s)], rank)[0][1]
    assert got_st[0] == got_st[1] == 0 and got_st[2] == got_st[3] == got_st[4] and got_st[6] == got_st[7] == got_st[8]


@pytest.mark.parametrize("E", [2 * TILE - 1, 2 * TILE, 2 * TILE + 1, TILE, 1, 0])
def test_list_lengths_around_a_multiple_of_the_tile(E):
    rnd = np.random.default_rng(E)
    c, n = 6, 777
    rank, n_dst = rank_even(n)
    p = Plan(c, n, n_dst)
    check(p, [make_list(p, spread(rnd, p.NB, E), rnd)], rank)


def test_full_list_whose_length_is_a_multiple_of_the_tile():
    """no zero digit at all and n W = 1024 W: start[NB] lies on the first position of the tile behind the list"""
    rnd = np.random.default_rng(9)
    c, n = 8, 1024
    rank, n_dst = rank_even(n)
    p = Plan(c, n, n_dst)
    E = n * p.W
    assert E % TILE == 0 and p.tiles == E // TILE + 1
    idx = np.tile(np.arange(n), p.W)                                 # every scalar W times: the sub-list is full as well
    rnd.shuffle(idx)
    e, s = make_list(p, spread(rnd, p.NB, E), rnd, idx)
    assert check(p, [(e, s)], rank) == n_dst * p.W


def test_batch_of_two_proofs_with_different_list_lengths():
    rnd = np.random.default_rng(10)
    c, n = 7, 2000
    rank, n_dst = rank_even(n)
    p = Plan(c, n, n_dst)
    a = make_list(p, spread(rnd, p.NB, 3 * TILE + 5), rnd)
    b = make_list(p, spread(rnd, p.NB, 411), rnd)
    one = [run_sublist(p, [x], rank)[0] for x in (a, b)]
    check(p, [a, b], rank)
    both = run_sublist(p, [a, b], rank)
    for (s1, t1), (s2, t2) in zip(one, both):                         # a proof's sub-list does not depend on its neighbour
        assert np.array_equal(s1, s2) and np.array_equal(t1, t2)
    check(p, [b, a], rank)


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,compact", [(dict(n_c=20000, n_free=3000, n0=16), True), (dict(n_c=1000, n_free=100, n0=16), False)])
def test_prove_equals_the_c_oracle_with_and_without_compacted_queries(shape, compact, ctx_bn254):
    """A and B both compacted (n_v - 1 >= 4096, 55 % / 52 % of the bases not at infinity), and neither (a class below
    4096 variables: both queries read z's list as it is)"""
    from hekaton_system_amd.cp_groth16 import FrCodec, SeededRng, generate_parameters
    from hekaton_system_amd.workload import SyntheticSubcircuit
    from oracle.c_oracle import COracle
    fc = FrCodec("bn254")
    circ = SyntheticSubcircuit("bn254", **shape)
    da, db = circ.query_density()
    assert ((circ.n_v - 1 >= 4096) and da < 0.75 and db < 0.75) == compact
    pk, _ = generate_parameters(circ, "bn254", SeededRng(b"SUBLIST1" * 4), ctx_bn254)
    dpk = pk.upload(ctx_bn254)
    try:
        circ.set_witness_seed(5)
        zb = circ.full_assignment_bytes()
        kappa, r_, s_ = 0x77, 0x1234_5678_9ABC, 0xFEDC_BA98
        a, b, c = dpk.prove(zb, fc.enc1(r_), fc.enc1(s_), fc.enc([kappa]), n_v=circ.n_v)
        co = COracle("bn254")
        A, B, C = pk.matrices
        view = co.pk_view(a_g=pk.a_g, b_g=pk.b_g, b_h=pk.b_h, h_g=pk.h_g, ck_stages=pk.ck.deltas_abc_g,
                          deltas_g=pk.deltas_g, last_delta_h=pk.vk.last_delta_h, alpha_g=pk.vk.alpha_g,
                          beta_g=pk.beta_g, beta_h=pk.vk.beta_h)
        oa, ob, oc = co.prove(view, A, B, C, circ.N_INST, circ.n_c, zb, fc.enc1(r_), fc.enc1(s_), fc.enc([kappa]))
        assert np.array_equal(oa, a) and np.array_equal(ob, b) and np.array_equal(oc, c)
    finally:
        dpk.free()
