"""CPU: every premise tests/sweep_edges.py states - the single-byte scalars have one non-zero window, the crafted fixed-base
tables make the digit walk double or cancel where intended, the "equal partial sums" vectors meet P == Q at every level of
the LDS tree, the K-lane form reads a magnitude whole up to 0x77..7 and no further (the kernels' own split_window_chain
compiled for the host: tests/host_shim/field_shim.cpp; once more, under the sanitizers and over both table layouts, as the
stand-alone tests/host_shim/split_chain_driver.cpp), and the discrete-log reference agrees with the oracle's own
add / mul / msm."""
import ctypes
import subprocess

import numpy as np
import pytest

from tests import host_build
from tests import msm_edges as me
from tests import sweep_edges as se


@pytest.mark.parametrize("gid", range(4))
def test_window_scalars_have_one_non_zero_window(gid):
    r = se.order(gid)
    reduced = []
    for w, d, s in se.fb_window_scalars(gid):
        assert 0 < s < r
        if (d << (8 * w)) >= r:
            reduced.append((w, d))
            continue
        digits = se.windows(s)
        assert digits[w] == d and sum(1 for x in digits if x) == 1, (gid, w, d)
    assert reduced == [(31, 255)]
    # the top window: its largest digit is the top byte of r, and one more would pass r
    w, d, s = se.fb_window_scalars(gid)[-1]
    assert w == 31 and s < r <= ((d + 1) << 248) and d < 255
    assert {(w, d) for w, d, _ in se.fb_window_scalars(gid)} >= {(w, d) for w in range(32) for d in (1, 255)}


@pytest.mark.parametrize("gid", range(4))
def test_real_table_walk_is_the_scalar_multiple(gid):
    r = se.order(gid)
    k = me.pool_ks(gid)[0]
    logs = se.real_table_logs(k, r)
    for _, _, s in se.fb_window_scalars(gid) + [(0, 0, 0), (0, 0, r - 1)]:
        assert se.fb_walk(logs, s, r)[0] == s * k % r


@pytest.mark.parametrize("gid", range(4))
def test_crafted_tables_double_and_cancel_at_window_one(gid):
    r = se.order(gid)
    f, a, b = me.pool_ks(gid)[2:5]
    dbl, cancel = se.crafted_table(gid, "dbl"), se.crafted_table(gid, "cancel")
    assert se.fb_walk(dbl, 0x0101, r) == (2 * a % r, [(1, "dbl")])
    assert se.fb_walk(dbl, 0x010101, r) == ((2 * a + b) % r, [(1, "dbl")])
    assert se.fb_walk(cancel, 0x0101, r) == (0, [(1, "cancel")])
    # after the cancellation the walk goes on from infinity into window 2
    assert se.fb_walk(cancel, 0x010101, r) == (b, [(1, "cancel")])
    for s in se.CRAFTED_SCALARS:
        assert s < r and all(d in (0, 1, 2) for d in se.windows(s))
    assert se.fb_walk(dbl, 0x0201, r) == ((a + f) % r, [])        # a neighbouring entry is not the crafted one
    assert len({f, a, b, r - a, 2 * a % r}) == 5


@pytest.mark.parametrize("gid", range(4))
def test_lincomb_cases_meet_the_corner_at_the_last_step(gid):
    r = se.order(gid)
    for k in (2, 8):
        cases = {name: (v, c) for name, v, c in se.lincomb_cases(gid, k, 65)}
        v, c = cases["identical"]
        assert all(se.lincomb_last_step(v, c, i, r) == "dbl" for i in range(2, 65))
        assert se.lincomb_last_step(v, c, 0, r) is None
        v, c = cases["opposite"]
        assert all(se.lincomb_last_step(v, c, i, r) == "cancel" for i in range(2, 65))
        assert se.lincomb_expected(gid, v, c)[2:] == [0] * 63
        v, c = cases["top_bit"]
        assert c[0].bit_length() == r.bit_length() and c[0] < r
        v, c = cases["zeros"]
        assert not any(c)
        for name, (v, c) in cases.items():
            assert all(x[0] == 0 for x in v) and all(x[1] == 0 for x in v[:-1]) and v[-1][1] != 0, name
            assert len(v) == k and len(c) == k
    assert {name for name, _, _ in se.lincomb_cases(gid, 1, 64)} == {"zeros", "one_r_minus_1", "random"}


@pytest.mark.parametrize("gid", range(4))
def test_equal_partial_sums_meet_p_eq_q_at_every_tree_level(gid):
    r, T = se.order(gid), se.SUM_THREADS[gid]
    levels = T.bit_length() - 1
    for name in ("same_affine", "same_scaled"):
        for n in (T, 2 * T):
            logs = [k for k, _ in se.sum_family(gid, name, n)]
            total, events = se.sum_walk(logs, T, r)
            assert total == n * logs[0] % r
            # every add of every level has equal operands
            assert len(events) == T - 1 and {e for _, e in events} == {"dbl"}
            assert {off for off, _ in events} == {1 << l for l in range(levels)}
    # the scaled form really differs in its coordinates from one element to the next
    fam = se.sum_family(gid, "same_scaled", 4)
    assert len({se.xyzz(gid, k, s) for k, s in fam}) == 4
    assert {se.xyzz_to_affine(gid, se.xyzz(gid, k, s)) for k, s in fam} == {me.point(gid, fam[0][0])}
    # P, -P, ...: 2T elements double up to the last level, which cancels; T + 1 leaves one point
    logs = [k for k, _ in se.sum_family(gid, "plus_minus", 2 * T)]
    total, events = se.sum_walk(logs, T, r)
    assert total == 0 and events[-1] == (1, "cancel") and all(e == "dbl" for _, e in events[:-1]) and len(events) == T - 1
    logs = [k for k, _ in se.sum_family(gid, "plus_minus", T + 1)]
    assert se.sum_walk(logs, T, r)[0] == logs[0]
    # one 64-lane segment (k_points_sum_seg)
    for seg in (64, 129):
        logs = [k for k, _ in se.sum_family(gid, "same_affine", seg, slot=2)]
        total, events = se.sum_walk(logs, 64, r)
        assert total == seg * logs[0] % r and any(e == "dbl" for _, e in events)


@pytest.fixture(scope="module")
def host_shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim") / "field_shim.so")
    host_build.build("field_shim.cpp", out, "-O1", *host_build.SHARED)
    return host_build.load(out)


def _split_mul(lib, gid, pb, m):
    ml = np.array([(m >> (32 * i)) & 0xffffffff for i in range(6)], np.uint32)
    got = ctypes.create_string_buffer(len(pb))
    lib.shim_split_mul(gid, pb, ml.ctypes.data_as(ctypes.c_void_p), got)
    return got.raw


@pytest.mark.parametrize("gid", range(4))
def test_one_lane_of_the_k_lane_form_reads_a_magnitude_up_to_the_limit(gid, host_shim):
    """m <= 0x77..7 (ND nibbles) multiplies correctly; 0x77..7 + 1 and 2^190 do not: the bound hk_points_fold_* routes by"""
    io = se.Io(gid)
    dec = io.dec
    k = me.pool_ks(gid)[0]
    pb = io.aff([k])
    lim = se.mag_limit(gid)
    assert lim.bit_length() == 4 * se.SPLIT_ND[gid] - 1 and lim >= (1 << se.SPLIT_STEPS[gid]) - 1
    for m in se.uniform_mags(gid) + [lim - 1]:
        assert m <= lim
        assert dec(_split_mul(host_shim, gid, pb, m)) == me.point(gid, m * k), (gid, hex(m))
    for m in (lim + 1, 1 << 190):
        assert dec(_split_mul(host_shim, gid, pb, m)) != me.point(gid, m * k), (gid, hex(m))


def test_window_chain_runs_clean_under_the_sanitizers_and_gives_the_shim_bytes(host_shim, tmp_path):
    """split_window_chain + jac_to_xyzz as a stand-alone program built with -fsanitize=address,undefined, its tables in a row
    per lane and in one block strided by lane: 0x77..7 (the largest magnitude split_mag_fits admits), 0, 1 and 8 times a
    point of each group, and times the point at infinity, exit clean and print shim_split_mul's bytes."""
    exe = host_build.build("split_chain_driver.cpp", tmp_path / "split_chain_driver", "-O1", "-g", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    pts = {gid: [se.Io(gid).aff([k]) for k in me.pool_ks(gid)[:4]] for gid in range(4)}
    text = "".join("%d %s\n" % (gid, b"".join(bytes(p) for p in pts[gid]).hex()) for gid in range(4))
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    lines = [l.split() for l in run.stdout.splitlines()]
    assert [(int(g), int(i), int(t)) for g, i, t, _ in lines] == [(g, i, t) for g in range(4) for i in (0, 1) for t in range(4)]
    for g, inf, t, got in lines:
        gid, t = int(g), int(t)
        assert len({bytes(p) for p in pts[gid]}) == 4
        pb = bytes(len(pts[gid][t])) if int(inf) else bytes(pts[gid][t])
        m = [se.mag_limit(gid), 0, 1, 8][t]
        assert bytes.fromhex(got) == _split_mul(host_shim, gid, pb, m), (gid, inf, t)
        if int(inf) or m == 0:
            assert bytes.fromhex(got) == bytes(len(pb))
        elif m in (1, 8):                                    # independent of the shim: the oracle's multiple
            assert se.Io(gid).dec(bytes.fromhex(got)) == me.point(gid, m * me.pool_ks(gid)[t]), (gid, t)
            assert m != 1 or bytes.fromhex(got) == pb


@pytest.mark.parametrize("gid", range(4))
def test_split_mag_fits_is_true_up_to_the_limit_and_false_above(gid, host_shim):
    """split_mag_fits (csrc/endo.cuh), by which hk_points_fold_* picks the kernel: a bound too lax returns wrong points, one
    too strict quietly sends every fold to the slow one-lane kernel.  True exactly for m <= 0x77..7 (ND nibbles)."""
    lim = se.mag_limit(gid)
    r = se.order(gid)

    def fits(m):
        ml = np.array([(m >> (32 * i)) & 0xffffffff for i in range(8)], np.uint32)
        return host_shim.shim_split_mag_fits(gid, ml.ctypes.data_as(ctypes.c_void_p))

    for m in [0, 1, lim - 1, lim, (1 << se.SPLIT_STEPS[gid]) - 1, lim & ~0xf] + se.uniform_mags(gid):
        assert fits(m) == 1, (gid, hex(m))
    # one above, a set bit in every limb above the limit's top limb, a smaller low limb under a larger high one
    above = [lim + 1, lim + 0x10, 1 << 190, r - 1, (1 << 256) - 1, (lim + 1) << 4] + [1 << (32 * l) for l in range(8) if (1 << (32 * l)) > lim]
    for m in above:
        assert m > lim and fits(m) == 0, (gid, hex(m))
    # every part of the split the wrappers send stays inside: they are below 2^STEPS
    rn = se.rnd(gid, "fits")
    assert all(fits(rn.randrange(1 << se.SPLIT_STEPS[gid])) == 1 for _ in range(50))


@pytest.mark.parametrize("gid", range(4))
def test_uniform_cases_put_every_magnitude_at_every_part_under_every_mask(gid):
    K, mags = se.SPLIT_K[gid], se.uniform_mags(gid)
    cases = se.uniform_cases(gid)
    assert {0, 7, 8, 9, (1 << se.SPLIT_STEPS[gid]) - 1, se.mag_limit(gid)} <= set(mags) and len(set(mags)) == len(mags) == 9
    for j in range(K):
        assert {c[j] for c, _ in cases} == set(mags), (gid, j)
    assert {m for _, m in cases} == set(range(1 << K))
    assert all(len(c) == K and m < (1 << K) for c, m in cases) and cases[-1] == ([0] * K, 0)
    # the signed digits one lane reads (split_bias / split_digit): every value -8 .. 7 occurs at every part
    ND = se.SPLIT_ND[gid]
    bias = int("8" * ND, 16)
    for j in range(K):
        seen = {(((c[j] + bias) >> (4 * d)) & 15) - 8 for c, _ in cases for d in range(ND)}
        assert seen == set(range(-8, 8)), (gid, j, sorted(seen))


@pytest.mark.parametrize("gid", range(4))
def test_discrete_log_reference_agrees_with_the_oracle_group(gid):
    r, G = se.order(gid), me.group(gid)
    ks = me.pool_ks(gid)
    # lincomb
    _, v, c = se.lincomb_cases(gid, 2, 5)[2]
    want = se.lincomb_expected(gid, v, c)
    for i in (0, 1, 4):
        assert me.point(gid, want[i]) == G.msm([me.point(gid, x[i]) for x in v], c)
    # fold
    mags, mask = se.uniform_cases(gid)[3]
    c = se.fold_scalar(gid, mags, mask)
    lo, hi = se.fold_vectors(gid, c, 5)
    want = se.fold_expected(gid, c, lo, hi)
    for i in range(5):
        assert me.point(gid, want[i]) == G.add(me.point(gid, lo[i]), G.mul(me.point(gid, hi[i]), c) if hi[i] else None)
    assert want[2] == 0 and want[1] == 2 * lo[1] % r and lo[3] == 0 and hi[4] == 0
    # the eigenvalue: c P as the sum of the signed parts over the endomorphism's powers
    P = me.point(gid, ks[0])
    parts = [G.mul(P, m * pow(se.lam(gid), j, r) % r) if m else None for j, m in enumerate(mags)]
    acc = None
    for j, Q in enumerate(parts):
        acc = G.add(acc, G.neg(Q) if (mask >> j) & 1 and Q is not None else Q)
    assert acc == me.point(gid, c * ks[0])
    # sums
    fam = se.sum_family(gid, "random", 9)
    total = se.sum_walk([k for k, _ in fam], 4, r)[0]
    assert me.point(gid, total) == G.sum([se.xyzz_to_affine(gid, se.xyzz(gid, k, s)) for k, s in fam])
    # per-element scalars
    sc = se.split_scalars(gid)
    assert len(sc) == 11 and sc[3] == se.lam(gid)
    assert G.mul(P, sc[7]) == me.point(gid, sc[7] * ks[0])
