"""GPU: hk_prove's coalescer with its gather window on: 8 looping threads of one proving key settle
into chunks of 8 / PROVE_COALESCE_RUNNING = 4 proofs, every call still gets, byte for byte, what a lone sequential
hk_prove gives, and a lone caller right after the burst runs alone, at once."""
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from hekaton_system_amd import capi
from tests.test_prove_coalesce_gpu import _Setup

pytestmark = pytest.mark.gpu

THREADS, CALLS = 8, 4
GATHER_US = 5000          # well above the re-entry gap of a Python caller (0.15 ms median, 0.45 ms at most in the bench)


@pytest.fixture(scope="module")
def setup():
    """A context of its own: hk_ctx_create reads HK_PROVE_GATHER_US once, when the context is made."""
    old = os.environ.get("HK_PROVE_GATHER_US")
    os.environ["HK_PROVE_GATHER_US"] = str(GATHER_US)
    try:
        ctx = capi.Context("bn254", 0)
    finally:
        if old is None:
            del os.environ["HK_PROVE_GATHER_US"]
        else:
            os.environ["HK_PROVE_GATHER_US"] = old
    st = _Setup(ctx, "bn254")
    yield st
    st.free()
    ctx.close()


def test_looping_threads_prove_in_chunks_of_four(setup):
    """8 threads x 4 calls on one key: every output equals the row's lone sequential proof, and most calls ran in a chunk
    of exactly 4 (the two callers that arrive first lead alone, and the chunks holding a thread's last call may be
    short); three lone calls right after the burst run alone and do not wait for the callers that left."""
    bar = threading.Barrier(THREADS)

    def loop(t):
        bar.wait()
        res = []
        for i in range(CALLS):
            j = (t + i) % setup.rows
            out = setup.prove(0, j, True)
            res.append((j, out, setup.ctx.last_timings()["batch_proofs"]))
        return res

    with ThreadPoolExecutor(max_workers=THREADS) as pool:
        got = [x for r in pool.map(loop, range(THREADS)) for x in r]
    sizes = [nb for _, _, nb in got]
    print("batch_proofs of the 32 calls:", sorted(sizes))
    for j, out, nb in got:
        assert out == setup.want[(0, j)], j
        assert 1 <= nb <= THREADS
    assert sum(nb == 4 for nb in sizes) > len(sizes) // 2, sizes

    t0 = time.perf_counter()
    for j in range(3):
        assert setup.prove(0, j, True) == setup.want[(0, j)]
        assert setup.ctx.last_timings()["batch_proofs"] == 1
    print("three lone calls after the burst: %.1f ms" % ((time.perf_counter() - t0) * 1e3))


def test_two_keys_with_a_window(setup):
    """Two key classes interleaved on 8 looping threads: keys never share a chunk, so every proof is its row's lone proof."""
    def loop(t):
        ok = True
        for i in range(CALLS):
            k, j = (t + i) % 2, (t + 2 * i) % setup.rows
            ok = ok and setup.prove(k, j, i % 2 == 0) == setup.want[(k, j)]
        return ok

    with ThreadPoolExecutor(max_workers=THREADS) as pool:
        assert all(pool.map(loop, range(THREADS)))


@pytest.mark.parametrize("on_device", [False, True])
def test_chunk_of_three_assignments_gives_each_row_its_lone_proof(setup, on_device):
    """Each proof of a chunk reads its own assignment, on the host or on the device: one hk_prove_batch of three rows with
    three different assignments (and blinders) equals the three lone proofs."""
    rows = [2, 0, 3]
    z = np.ascontiguousarray(np.concatenate([np.frombuffer(bytes(setup.zh[j]), np.uint8) for j in rows]))
    zbuf = capi.DeviceBuffer.from_host(setup.ctx, z) if on_device else z
    r = np.concatenate([setup.rsk[j][0] for j in rows])
    s = np.concatenate([setup.rsk[j][1] for j in rows])
    kap = np.concatenate([setup.rsk[j][2] for j in rows])
    try:
        a, b, c = setup.dpks[1].prove_batch(zbuf, r, s, kap, setup.circ.n_v, len(rows))
    finally:
        if on_device:
            zbuf.free()
    for i, j in enumerate(rows):
        assert a[i].tobytes() + b[i].tobytes() + c[i].tobytes() == setup.want[(1, j)], (i, j)
