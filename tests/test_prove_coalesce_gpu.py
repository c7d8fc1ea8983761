"""GPU: concurrent hk_prove calls of one proving key meet in the context's coalescer and run as lock-step batches
(DESIGN.md section 4e).  Every call must still get, byte for byte, what a lone sequential hk_prove gives; a bad call must
fail on its own; hk_timings must report the call's share of its chunk and how many proofs that chunk held."""
import math
import os
import re
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import FrCodec, SeededRng, generate_parameters
from hekaton_system_amd.workload import make_config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = int(re.search(r"#define\s+HK_PROVE_BATCH_CHUNK\s+(\d+)", open(os.path.join(ROOT, "include", "hekaton.h")).read()).group(1))
THREADS = 8
SEEDS = (b"COALESCE-CLASS-KEY-A-0123456789a", b"COALESCE-CLASS-KEY-B-0123456789b")


def _ctx(request, cname):
    return request.getfixturevalue("ctx_bn254" if cname == "bn254" else "ctx_bls")


class _Setup:
    """Two proving-key classes of big-merkle-4x1 (m = 2^16), four distinct assignments and blinders per class, each
    assignment on the host and on the device, and the sequential single-thread proof of every (class, row)."""

    def __init__(self, ctx, cname, rows=4):
        self.ctx, self.cname, self.fc = ctx, cname, FrCodec(cname)
        self.circ = make_config(cname, "big-merkle-4x1")
        self.dpks = [generate_parameters(self.circ, cname, SeededRng(s), ctx)[0].upload(ctx) for s in SEEDS]
        self.rows = rows
        self.zh, self.zd, self.rsk = [], [], []
        for j in range(rows):
            self.circ.set_witness_seed(900 + j)
            zb = np.ascontiguousarray(self.circ.full_assignment_bytes())
            self.zh.append(zb)
            self.zd.append(capi.DeviceBuffer.from_host(ctx, zb))
            self.rsk.append((self.fc.enc1(0x51 + 7 * j), self.fc.enc1(0x9d + 13 * j), self.fc.enc([0x3003 + 17 * j])))
        self.want = {(k, j): self.prove(k, j, True) for k in range(2) for j in range(rows)}
        assert len({v for v in self.want.values()}) == 2 * rows

    def prove(self, k, j, on_device):
        r, s, kap = self.rsk[j]
        z = self.zd[j] if on_device else self.zh[j]
        a, b, c = self.dpks[k].prove(z, r, s, kap, n_v=self.circ.n_v)
        return a.tobytes() + b.tobytes() + c.tobytes()

    def free(self):
        for z in self.zd:
            z.free()
        for d in self.dpks:
            d.free()


@pytest.fixture(scope="module", params=["bn254", "bls12_381"])
def setup(request):
    st = _Setup(_ctx(request, request.param), request.param)
    yield st
    st.free()


@pytest.mark.parametrize("mode", ["device", "host", "mixed"])
def test_concurrent_calls_are_byte_identical_to_sequential(setup, mode):
    """8 threads, 32 hk_prove calls over two key classes: every output equals that row's lone sequential proof."""
    def one(i):
        k, j = i % 2, (i // 2) % setup.rows
        on_dev = {"device": True, "host": False, "mixed": (i // 3) % 2 == 0}[mode]
        return (k, j), setup.prove(k, j, on_dev), setup.ctx.last_timings()["batch_proofs"]

    with ThreadPoolExecutor(max_workers=THREADS) as pool:
        got = list(pool.map(one, range(32)))
    for i, (key, out, nb) in enumerate(got):
        assert out == setup.want[key], (mode, i, key)
        assert 1 <= nb <= CHUNK


def test_keys_of_different_shapes_share_the_queue(setup):
    """Calls of key classes with different n_v interleave in the queue: whichever caller leads runs each key's chunk
    with that key's lengths, and every output equals the lone sequential proof."""
    ctx, cname = setup.ctx, setup.cname
    circ2 = make_config(cname, "vkd-256")
    assert circ2.n_v != setup.circ.n_v
    dpk2 = generate_parameters(circ2, cname, SeededRng(SEEDS[0]), ctx)[0].upload(ctx)
    circ2.set_witness_seed(77)
    z2 = capi.DeviceBuffer.from_host(ctx, circ2.full_assignment_bytes())
    r, s, kap = setup.rsk[0]

    def other():
        a, b, c = dpk2.prove(z2, r, s, kap, n_v=circ2.n_v)
        return a.tobytes() + b.tobytes() + c.tobytes()

    want2 = other()
    try:
        res = _released_together(setup, lambda t: other() == want2 if t % 2 else
                                 setup.prove(0, t % setup.rows, True) == setup.want[(0, t % setup.rows)])
        res += _released_together(setup, lambda t: other() == want2 if t % 3 == 0 else
                                  setup.prove(1, t % setup.rows, False) == setup.want[(1, t % setup.rows)])
    finally:
        z2.free()
        dpk2.free()
    assert all(res), res


def _released_together(setup, fn, n=THREADS):
    """n threads that wait at one barrier, then each call fn(thread index); returns the results in thread order."""
    bar = threading.Barrier(n)

    def run(t):
        bar.wait()
        return fn(t)

    with ThreadPoolExecutor(max_workers=n) as pool:
        return list(pool.map(run, range(n)))


def test_batching_happens(setup):
    """A lone thread always runs alone (batch_proofs == 1); 8 threads released together share chunks."""
    for j in range(3):
        assert setup.prove(0, j, True) == setup.want[(0, j)]
        assert setup.ctx.last_timings()["batch_proofs"] == 1

    def one(t):
        j = t % setup.rows
        out = setup.prove(0, j, True)
        return out == setup.want[(0, j)], setup.ctx.last_timings()["batch_proofs"]

    sizes = []
    for _ in range(3):
        res = _released_together(setup, one)
        assert all(ok for ok, _ in res)
        sizes += [nb for _, nb in res]
    assert all(1 <= nb <= THREADS for nb in sizes)
    assert max(sizes) > 1, sizes


def test_bad_calls_fail_alone(setup):
    """A wrong n_v, a wrong n_kappas and a NULL output get their own error while concurrent good calls get their proofs."""
    ctx, circ, lib = setup.ctx, setup.circ, setup.ctx.lib
    g1, g2 = ctx.g1_bytes, ctx.g2_bytes

    def raw(t, n_v, nk, null_c):
        r, s, kap = setup.rsk[t % setup.rows]
        a, b, c = np.zeros(g1, np.uint8), np.zeros(g2, np.uint8), np.zeros(g1, np.uint8)
        kap2 = np.concatenate([kap, kap])
        return lib.hk_prove(ctx.handle, setup.dpks[0].handle, capi.ptr(setup.zd[t % setup.rows]), n_v, r.ctypes.data,
                            s.ctypes.data, kap2.ctypes.data, nk, a.ctypes.data, b.ctypes.data,
                            None if null_c else c.ctypes.data)

    bad = {1: (circ.n_v - 1, 1, False, capi.HK_ERR_LEN), 4: (circ.n_v, 2, False, capi.HK_ERR_LEN),
           6: (circ.n_v, 0, False, capi.HK_ERR_LEN), 7: (circ.n_v, 1, True, capi.HK_ERR_ARG)}

    def one(t):
        if t in bad:
            n_v, nk, null_c, want = bad[t]
            return raw(t, n_v, nk, null_c) == want
        j = t % setup.rows
        return setup.prove(0, j, True) == setup.want[(0, j)]

    assert all(_released_together(setup, one))
    # the lanes are usable afterwards
    assert setup.prove(1, 0, False) == setup.want[(1, 0)]


def test_timings_are_per_proof_shares(setup):
    """With profiling on, every member of a coalesced chunk reports four accumulate launches and finite, positive
    per-proof shares of the chunk's phases."""
    ctx = setup.ctx

    def one(t):
        j = t % setup.rows
        out = setup.prove(1, j, True)
        return out == setup.want[(1, j)], ctx.last_timings()

    ctx.set_profiling(True)
    try:
        res = _released_together(setup, one)
    finally:
        ctx.set_profiling(False)
    assert all(ok for ok, _ in res)
    for _, t in res:
        assert t["accum_kernel_launches"] == 4, t
        assert 1 <= t["batch_proofs"] <= THREADS, t
        for f in ("total_ms", "digits_ms", "msm_a_ms", "msm_b_g1_ms", "msm_b_g2_ms", "msm_l_ms", "witness_map_ms",
                  "msm_h_ms", "finish_ms", "accum_kernel_ms", "accum_h_ms"):
            assert math.isfinite(t[f]) and t[f] > 0, (f, t)
    # a chunk's members share one set of figures
    by_size = {}
    for _, t in res:
        by_size.setdefault(t["batch_proofs"], []).append(t)
    for nb, ts in by_size.items():
        assert len(ts) % nb == 0, (nb, len(ts))


def test_full_size_concurrent_proofs_pass_the_trapdoor_check(ctx_bn254):
    """BASELINE configs[1] (m = 2^21): 8 threads released together prove 8 subcircuits of one class; the first two equal
    the lone sequential proofs and all eight satisfy the Groth16 equation in the exponent under the SRS trapdoor."""
    from hekaton_system_amd.cp_groth16 import trapdoor_verify
    ctx, cname = ctx_bn254, "bn254"
    fc = FrCodec(cname)
    circ = make_config(cname, "big-merkle-64x32")
    pk, td = generate_parameters(circ, cname, SeededRng(b"COALESCE-FULL-SIZE-KEY-012345678"), ctx)
    dpk = pk.upload(ctx)
    A, B, C = pk.matrices
    zs, ints, coms, hs = [], [], [], []
    for j in range(2):
        circ.set_witness_seed(4100 + j)
        ints.append(circ.assignment_ints())
        zs.append(capi.DeviceBuffer.from_host(ctx, circ.full_assignment_bytes()))
        coms.append(dpk.commit(0, circ.stage0_witness_bytes(), fc.enc1(0x4444 + j)))
        h_b, _m = ctx.witness_map(A, B, C, circ.N_INST, circ.n_c, zs[j], n_v=circ.n_v)
        hs.append(fc.dec(h_b))
    rsk = [(0x1234_5678 + 3 * t, 0x8765_4321 + 5 * t, 0x4444 + t % 2) for t in range(THREADS)]

    def one(t):
        r_, s_, kappa = rsk[t]
        a, b, c = dpk.prove(zs[t % 2], fc.enc1(r_), fc.enc1(s_), fc.enc([kappa]), n_v=circ.n_v)
        return a, b, c, ctx.last_timings()["batch_proofs"]

    seq = [one(t)[:3] for t in range(2)]
    par = _released_together(None, one)
    for t in range(2):
        assert all(np.array_equal(x, y) for x, y in zip(par[t][:3], seq[t])), t
    assert max(p[3] for p in par) > 1
    for t in range(THREADS):
        r_, s_, kappa = rsk[t]
        j = t % 2
        trapdoor_verify(ctx, cname, td, circ.N_INST, td.stage_ranges, ints[j], hs[j], [coms[j]], [kappa], r_, s_, par[t][:3])
    for z in zs:
        z.free()
    dpk.free()
