"""GPU: scan_u32 (csrc/scan.cuh) handed a vector, through tests/device_shim/ntt_dev_shim.hip, against numpy's cumulative sum
in uint32.  Its users reach it with the sizes of their own data and check it by a proof verifying; here the sizes sit on the
seams of its three launches: the 16 elements of a lane, the 4096 of a tile, and the 256 tiles after which k_scan_u32_tops
loops with a carry.  `out` is longer than n and filled with a sentinel: nothing at or past n may be written."""
import numpy as np
import pytest

from tests import dev_shim as ds

pytestmark = pytest.mark.gpu

TILE = 4096
SIZES = [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 256 * TILE - 1, 256 * TILE, 256 * TILE + 1,
         2 * 256 * TILE + TILE + 1]
SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module")
def shim():
    return ds.load_ntt("asm")                # scan_u32 holds no field arithmetic: one build is every build


def exclusive(counts):
    want = np.zeros(len(counts), dtype=np.uint32)
    if len(counts) > 1:
        want[1:] = np.cumsum(counts[:-1], dtype=np.uint32)
    return want


def check(shim, counts):
    n = len(counts)
    out = np.full(n + shim.scan_pad, SENTINEL, dtype=np.uint32)
    shim.scan_u32(counts, out)
    assert np.array_equal(out[:n], exclusive(counts))
    assert (out[n:] == SENTINEL).all(), "written past n"


@pytest.mark.parametrize("n", SIZES)
def test_scan_u32(shim, n):
    rng = np.random.default_rng(n)
    check(shim, rng.integers(0, 1 << 10, size=n, dtype=np.uint32))
    check(shim, np.ones(n, dtype=np.uint32))
    check(shim, np.zeros(n, dtype=np.uint32))
    last = np.zeros(n, dtype=np.uint32)
    if n:
        last[-1] = 0xFFFFFFFF
    check(shim, last)


def test_scan_u32_total_wraps(shim):
    n = 2 * 256 * TILE + TILE + 1
    counts = np.random.default_rng(1).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    assert int(counts.astype(np.uint64).sum()) >> 32
    check(shim, counts)
