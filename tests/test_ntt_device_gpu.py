"""GPU: the Fr transform layer (csrc/ntt.cuh, k_spmv of csrc/csr.cuh) launch by launch, through
tests/device_shim/ntt_dev_shim.hip, against the stage-by-stage integers of tests/ntt_ref.py (proved against
oracle.pyref.poly in tests/test_ntt_ref_cpu.py).  NttHost::passes and QapHost::run derive stages, tiles, batch and epilogue
themselves and the end-to-end tests reach them at the workload's sizes; here the caller picks them:

  * the stage tables and the three power-table levels as NttHost::ensure builds them; pow_from_tables at the exponents
    where the second and the third level join in (the third needs no 2^23-point vector this way);
  * ONE k_ntt_pass4 launch, DIF and DIT: bottom passes of every size 2^1 .. 2^11 under four block sizes, upper passes of the
    default and of small tiles (top pass, middle pass, block-high part of `base` non-zero, lo == cols_bits), on inputs whose
    memory form is 0 or r - 1 everywhere, alternating, or in one place - they carry the lazy [0, 2r) representatives through
    up to 11 chained stages in LDS;
  * batch and stride (pad elements between the vectors must come back untouched), the fused epilogue under every mask and
    every npost, with a random scale, kc and sub;
  * whole DIF and DIT chains by the plans of csrc/ntt_plan.h, schedules of 3 and more passes included;
  * k_scale_pow, k_bitrev, k_mul_pointwise, and k_spmv's tail (instance copy and zero fill) at the power-of-two seams.

Everything is integer arithmetic: every comparison is equality of bytes."""
import random

import pytest

from oracle.pyref.params import CURVES
from oracle.pyref.poly import Domain
from tests import dev_shim as ds
from tests import ntt_plan
from tests import ntt_ref as nr

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "bls12_381"]
VARIANT_NAMES = sorted(ds.NTT_VARIANTS)
FB = ds.FR_BYTES
SENTINEL = b"\xEE" * FB                       # never read by a kernel; no canonical element (both r are below 0x74 << 248)
PAD = 64
CLASSES = ("random", "zero", "max", "alternating", "first", "last")

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.fixture(scope="module", params=VARIANT_NAMES)
def shim(request):
    return ds.load_ntt(request.param)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return ntt_plan.load(tmp_path_factory.mktemp("ntt_plan"))[1]


def tws(cname, logn, inverse):
    return cached(("tws", cname, logn, inverse), lambda: nr.to_bytes(CURVES[cname], nr.stage_tables(CURVES[cname], logn, inverse)))


def pw(cname, inverse):
    return cached(("pw", cname, inverse), lambda: nr.to_bytes(CURVES[cname], nr.pow_tables(CURVES[cname], inverse)))


def rand_vec(cp, n, seed):
    rng = random.Random(seed)
    return [rng.randrange(cp.r) for _ in range(n)]


def inputs(cname, n):
    """the input classes as plain residues.  "max" is the element whose MEMORY form (Montgomery limbs) is r - 1, the largest
    canonical operand a kernel can load: with it the sums in LDS reach 2r - 2."""
    def make():
        cp = CURVES[cname]
        top = (cp.r - 1) * pow(nr.MONT_R, -1, cp.r) % cp.r
        return {"random": rand_vec(cp, n, 77 * n + cp.cid),
                "zero": [0] * n,
                "max": [top] * n,
                "alternating": [0, top] * (n // 2) if n > 1 else [top],
                "first": [top] + [0] * (n - 1),
                "last": [0] * (n - 1) + [top]}
    return cached(("in", cname, n), make)


def in_bytes(cname, n, cls):
    return cached(("inb", cname, n, cls), lambda: nr.to_bytes(CURVES[cname], inputs(cname, n)[cls]))


def want_pass(cname, cls, logn, lo, nst, dit, inverse=0):
    cp = CURVES[cname]
    return cached(("pass", cname, cls, logn, lo, nst, dit, inverse),
                  lambda: nr.to_bytes(cp, nr.pass_ref(cp, inputs(cname, 1 << logn)[cls], logn, lo, nst, dit, inverse)))


def check_single_pass(shim, cname, logn, lo, nst, cols_bits, threads):
    cid = CURVES[cname].cid
    for dit in (0, 1):
        for cls in CLASSES:
            got = shim.ntt_pass(cid, dit, in_bytes(cname, 1 << logn, cls), 1 << logn, 1, tws(cname, logn, 0), logn, lo, nst,
                                cols_bits, threads)
            assert got == want_pass(cname, cls, logn, lo, nst, dit), (cname, cls, dit, logn, lo, nst, cols_bits, threads)


# ---- tables ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_stage_tables(shim, cname):
    cp = CURVES[cname]
    for log_table in (1, 2, 11, 16):
        for inverse in (0, 1):
            got = shim.ntt_tables(cp.cid, log_table, nr.to_bytes(cp, nr.squarings(cp, log_table, inverse)))
            assert got == nr.to_bytes(cp, nr.stage_tables(cp, log_table, inverse)), (log_table, inverse)


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_pow_table_levels(shim, cname):
    cp = CURVES[cname]
    for inverse in (0, 1):
        g = pow(cp.fr_generator, -1, cp.r) if inverse else cp.fr_generator
        sq = [pow(g, 1 << k, cp.r) for k in range(3 * nr.POW_TABLE_BITS)]
        got = b"".join(shim.pow_table(cp.cid, nr.to_bytes(cp, sq[11 * lvl:11 * lvl + 11]), nr.POW_TABLE_SIZE, nr.POW_TABLE_BITS)
                       for lvl in range(3))
        assert got == pw(cname, inverse), inverse


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_pow_from_tables(shim, cname):
    cp = CURVES[cname]
    g = cp.fr_generator
    rng = random.Random(5 + cp.cid)
    cases = [(11, [0, 1, 2047])]
    cases += [(logn, [2047, 2048, 2049, (1 << 22) - 1]) for logn in (12, 22)]
    for logn in (23, cp.two_adicity, 32):
        cases.append((logn, [(1 << 22) - 1, 1 << 22, (1 << 22) + 2049, (1 << logn) - 1] + [rng.randrange(1 << logn) for _ in range(12)]))
    for logn, js in cases:
        js = [j for j in js if j < (1 << logn)]
        got = shim.pow_from_tables(cp.cid, pw(cname, 0), js, logn)
        assert got == nr.to_bytes(cp, [pow(g, j, cp.r) for j in js]), (logn, js)


# ---- one pass -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("threads", [512, 64, 128, 256])
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_bottom_pass(shim, cname, threads):
    """lo = 0, cols_bits = 0: tiles smaller than the block down to one butterfly (tile_elems >> 2 == 0), odd and even nst; under
    2^(t - 2) lanes the tile is 2^min(logn, t) elements and the larger vectors take several blocks"""
    t = {512: 11, 64: 8, 128: 9, 256: 10}[threads]
    for logn in range(1, 12):
        check_single_pass(shim, cname, logn, 0, min(logn, t), 0, threads)


@pytest.mark.parametrize("nst", range(1, 7))
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_upper_pass_of_the_default_tile(shim, cname, nst):
    check_single_pass(shim, cname, 11 + nst, 11, nst, 11 - nst, 512)


@pytest.mark.parametrize("shape", [(14, 8, 3, 5, 64),       # a middle pass of 8+3+3: the block-high part of `base` is non-zero
                                   (14, 8, 2, 6, 64),
                                   (14, 11, 3, 5, 64),      # the top pass of 8+3+3
                                   (14, 11, 3, 8, 512),     # the same stages on the default tile
                                   (10, 5, 5, 5, 256)],     # lo == cols_bits, mid_bits = 0: no plan forms it, the contract allows it
                         ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_upper_pass_of_small_tiles(shim, cname, shape):
    check_single_pass(shim, cname, *shape)


def test_shapes_outside_the_contract_are_refused(shim):
    data, t = in_bytes("bn254", 1 << 12, "random"), tws("bn254", 12, 0)
    # cols_bits > lo; nst + cols_bits > 11 (twice); nst < 1
    for lo, nst, cols_bits in ((3, 2, 4), (11, 1, 11), (6, 6, 6), (11, 0, 10)):
        st, out = shim.ntt_pass_status(0, 0, data, 1 << 12, 1, t, 12, lo, nst, cols_bits, 512)
        assert st == ds.NTT_REFUSED and out is None, (lo, nst, cols_bits)


@pytest.mark.parametrize("shape", [(9, 0, 9, 0), (13, 11, 2, 9)], ids=["bottom", "upper"])
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_batch_and_stride(shim, cname, shape):
    logn, lo, nst, cols_bits = shape
    cp = CURVES[cname]
    n = 1 << logn
    vecs = [rand_vec(cp, n, 900 + 10 * logn + v) for v in range(3)]
    data = b"".join(nr.to_bytes(cp, v) + SENTINEL * PAD for v in vecs)
    for dit in (0, 1):
        got = shim.ntt_pass(cp.cid, dit, data, n + PAD, 3, tws(cname, logn, 0), logn, lo, nst, cols_bits, 512)
        want = b"".join(nr.to_bytes(cp, nr.pass_ref(cp, v, logn, lo, nst, dit, 0)) + SENTINEL * PAD for v in vecs)
        assert got == want, dit


# ---- the fused epilogue ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("logn", [1, 5, 11, 12])
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_epilogue_masks_and_npost(shim, cname, logn, plans):
    """On the last pass of a DIF chain (at 2^12 the upper pass runs first, without epilogue; the second power-table level feeds
    the bottom pass's).  2, 3 and 7 are the masks QapHost::run and hk_ntt use; 1, 4, 5 and 6 complete the documented contract."""
    cp = CURVES[cname]
    n = 1 << logn
    rng = random.Random(31 * logn + cp.cid)
    vecs = [rand_vec(cp, n, 500 + 10 * logn + v) for v in range(3)]
    sub = rand_vec(cp, n, 499 + logn)
    scale, kc = rng.randrange(2, cp.r), rng.randrange(2, cp.r)
    ps = plans[logn, ntt_plan.DEFAULT_TILE_LOG, ntt_plan.DEFAULT_UPPER_MAX][1]
    t = tws(cname, logn, 0)
    data = b"".join(nr.to_bytes(cp, v) for v in vecs)
    plain = list(vecs)
    for lo, nst, cols_bits in ps[:0:-1]:
        data = shim.ntt_pass(cp.cid, 0, data, n, 3, t, logn, lo, nst, cols_bits, 512)
        plain = [nr.pass_ref(cp, v, logn, lo, nst, 0, 0) for v in plain]
    lo, nst, cols_bits = ps[0]
    plain = [nr.pass_ref(cp, v, logn, lo, nst, 0, 0) for v in plain]
    without = [nr.to_bytes(cp, v) for v in plain]
    for post in (1, 2, 3, 2 | 4, 2 | 4 | 1, 4, 5):
        with_ep = [nr.to_bytes(cp, nr.epilogue_ref(cp, v, logn, post, scale, cp.fr_generator, sub, kc)) for v in plain]
        assert all(a != b for a, b in zip(with_ep, without))
        for npost in (0, 1, 2, 3, 0xffffffff):
            got = shim.ntt_pass(cp.cid, 0, data, n, 3, t, logn, lo, nst, cols_bits, 512, post=post, npost=npost,
                                scale=nr.to_bytes(cp, [scale]), pw=pw(cname, 0), sub=nr.to_bytes(cp, sub), kc=nr.to_bytes(cp, [kc]))
            want = b"".join(with_ep[v] if v < npost else without[v] for v in range(3))
            assert got == want, (post, npost)


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_epilogue_on_a_dit_pass(shim, cname):
    cp = CURVES[cname]
    logn, n = 5, 32
    vecs = [rand_vec(cp, n, 700 + v) for v in range(3)]
    scale = random.Random(9 + cp.cid).randrange(2, cp.r)
    data = b"".join(nr.to_bytes(cp, v) for v in vecs)
    got = shim.ntt_pass(cp.cid, 1, data, n, 3, tws(cname, logn, 0), logn, 0, logn, 0, 512, post=1, npost=2,
                        scale=nr.to_bytes(cp, [scale]))
    plain = [nr.pass_ref(cp, v, logn, 0, logn, 1, 0) for v in vecs]
    want = [nr.epilogue_ref(cp, v, logn, 1, scale, None, None, None) if k < 2 else v for k, v in enumerate(plain)]
    assert got == b"".join(nr.to_bytes(cp, v) for v in want)


# ---- whole chains ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("logn", [12, 13, 14])
@pytest.mark.parametrize("knobs", [(11, 6), (8, 1), (8, 3), (9, 2)], ids=lambda k: "tile%d-max%d" % k)
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_chains_by_the_plan(shim, cname, knobs, logn, plans):
    """DIF over x with the forward tables gives bitrev(fft(x)); DIT over that with the inverse tables gives m x.  The shim
    takes the block size as an argument, so no environment is involved."""
    cp = CURVES[cname]
    tile_log, raw_um = knobs
    um, ps = plans[logn, tile_log, raw_um]
    assert um == raw_um and len(ps) == 1 + -(-(logn - tile_log) // um)
    n, threads = 1 << logn, 1 << (tile_log - 2)
    x = inputs(cname, n)["random"]
    mid, back = cached(("chain", cname, logn), lambda: (nr.to_bytes(cp, nr.bitrev(Domain(cp, n).fft(x))),
                                                         nr.to_bytes(cp, [v * n % cp.r for v in x])))
    data = in_bytes(cname, n, "random")
    for lo, nst, cols_bits in ps[::-1]:
        data = shim.ntt_pass(cp.cid, 0, data, n, 1, tws(cname, logn, 0), logn, lo, nst, cols_bits, threads)
    assert data == mid
    for lo, nst, cols_bits in ps:
        data = shim.ntt_pass(cp.cid, 1, data, n, 1, tws(cname, logn, 1), logn, lo, nst, cols_bits, threads)
    assert data == back


# ---- the pointwise kernels ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("logn", [0, 1, 8, 12])
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_scale_pow(shim, cname, logn):
    cp = CURVES[cname]
    n = 1 << logn
    g = cp.fr_generator
    vecs = [rand_vec(cp, n, 300 + 10 * logn + v) for v in range(2)]
    scale = random.Random(3 + logn).randrange(2, cp.r)
    data = b"".join(nr.to_bytes(cp, v) + SENTINEL * 8 for v in vecs)
    for bitrev_index in (0, 1):
        for use_pow in (0, 1):
            got = shim.scale_pow(cp.cid, data, n + 8, 2, pw(cname, 0), nr.to_bytes(cp, [scale]), logn, bitrev_index, use_pow)
            def idx(i):
                return nr.bitrev_index(i, logn) if bitrev_index else i
            want = [[x * scale * (pow(g, idx(i), cp.r) if use_pow else 1) % cp.r for i, x in enumerate(v)] for v in vecs]
            assert got == b"".join(nr.to_bytes(cp, v) + SENTINEL * 8 for v in want), (bitrev_index, use_pow)


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_bitrev(shim, cname):
    cp = CURVES[cname]
    for logn in (0, 1, 2, 8, 9):
        x = rand_vec(cp, 1 << logn, 40 + logn)
        assert shim.bitrev(cp.cid, nr.to_bytes(cp, x), logn) == nr.to_bytes(cp, nr.bitrev(x)), logn


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_mul_pointwise(shim, cname):
    cp = CURVES[cname]
    for m in (1, 255, 256, 257):
        a, b = rand_vec(cp, m, 60 + m), rand_vec(cp, m, 61 + m)
        a[0], b[-1] = cp.r - 1, cp.r - 1
        got = shim.mul_pointwise(cp.cid, nr.to_bytes(cp, a), nr.to_bytes(cp, b))
        assert got == nr.to_bytes(cp, [x * y % cp.r for x, y in zip(a, b)]), m


# ---- k_spmv ---------------------------------------------------------------------------------------------------------

def random_csr(cp, n_rows, n_z, seed):
    """rows of 0 .. 4 non-zeros: row 1 (and every ninth) empty, row 2 (and every seventh) of coefficients one only - the
    product-skipping branch of csr_dot -, row 3 a single coefficient r - 1"""
    rng = random.Random(seed)
    row_ptr, col, val = [0], [], []
    for i in range(n_rows):
        if i % 9 == 1:
            k, coef = 0, None
        elif i % 7 == 2:
            k, coef = 3, 1
        elif i == 3:
            k, coef = 1, cp.r - 1
        else:
            k, coef = rng.randrange(1, 5), None
        for _ in range(k):
            col.append(rng.randrange(n_z))
            val.append(coef if coef is not None else rng.choice([1, rng.randrange(cp.r)]))
        row_ptr.append(len(col))
    return row_ptr, col, val


@pytest.mark.parametrize("case", [(5, 0, 8), (5, 2, 8), (5, 3, 8),
                                  (252, 4, 256),           # the instance rows end exactly at m
                                  (256, 3, 512),           # n_rows a power of two: the domain doubles for the instance rows alone
                                  (257, 2, 512)],
                         ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_spmv_writes_every_row_of_the_domain(shim, cname, case):
    n_rows, n_copy, m = case
    cp = CURVES[cname]
    n_z = 11
    z = rand_vec(cp, n_z, 800 + n_rows)
    z[0] = 1
    row_ptr, col, val = random_csr(cp, n_rows, n_z, 810 + n_rows)
    got = shim.spmv(cp.cid, row_ptr, col, nr.to_bytes(cp, val), nr.to_bytes(cp, z), SENTINEL * m, n_copy)
    want = [sum(val[k] * z[col[k]] for k in range(row_ptr[i], row_ptr[i + 1])) % cp.r for i in range(n_rows)]
    want += z[:n_copy] + [0] * (m - n_rows - n_copy)
    assert len(want) == m
    assert got == nr.to_bytes(cp, want)
