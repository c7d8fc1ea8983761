"""prove_batch_bench.py — K stage-1 proofs of one proving-key class, two ways, in one process: K hk_prove calls on a thread
pool (8 threads: how a host without the batched call proves a class) and one hk_prove_batch call (lock-step launches).
The two forms alternate, their outputs are compared row for row, and one JSON line reports per (curve, shape, K) the
proofs/s of each form (median over the repetitions) and the ratio batch / threads.

Shapes: one key class of every BASELINE config shape (hekaton_system_amd/workload.py CONFIGS), BN254; both curves at the
headline shape (big-merkle-64x32).  Assignments stay resident in HBM (one device buffer of K rows), as in bench.py.

usage:  python tools/prove_batch_bench.py [--shapes a,b,...] [--ks 8,32] [--reps 3] [--threads 8] [--distinct 4]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from hekaton_system_amd import capi  # noqa: E402
from hekaton_system_amd.cp_groth16 import FrCodec, SeededRng, generate_parameters  # noqa: E402
from hekaton_system_amd.workload import make_config  # noqa: E402

SHAPES = ["big-merkle-4x1", "vkd-256", "vm-1024x1024", "big-merkle-64x32", "big-merkle-512x64"]
HEADLINE = "big-merkle-64x32"


def bench_shape(ctx, curve, shape, ks, reps, threads, distinct):
    fc = FrCodec(curve)
    fr = ctx.fr_bytes
    circ = make_config(curve, shape)
    pk, _td = generate_parameters(circ, curve, SeededRng(b"PROVE-BATCH-BENCH-KEY-0123456789"), ctx)
    dpk = pk.upload(ctx)
    n_v = circ.n_v
    nb = n_v * fr
    base = []
    for j in range(distinct):                       # distinct assignments, tiled over the K rows
        circ.set_witness_seed(900 + j)
        base.append(np.frombuffer(bytes(circ.full_assignment_bytes()), np.uint8))
    m = 1 << max(0, (circ.n_c + circ.N_INST - 1).bit_length())
    out = []
    pool = ThreadPoolExecutor(threads)
    for k in ks:
        z = np.ascontiguousarray(np.concatenate([base[j % distinct] for j in range(k)]))
        zdev = capi.DeviceBuffer.from_host(ctx, z)
        r = fc.enc([0x1000_0001 + 7919 * j for j in range(k)])
        s = fc.enc([0x2000_0003 + 104729 * j for j in range(k)])
        kap = fc.enc([0x3000_0005 + 1299709 * j for j in range(k)])

        def one(j):
            return dpk.prove(zdev.view(j * nb, nb), r[j * fr:(j + 1) * fr], s[j * fr:(j + 1) * fr], kap[j * fr:(j + 1) * fr],
                             n_v=n_v)

        def singles():
            return list(pool.map(one, range(k)))

        def batched():
            return dpk.prove_batch(zdev, r, s, kap, n_v, k)

        want, got = singles(), batched()                                  # warm-up, and the equality check
        equal = all(got[0][j].tobytes() == want[j][0].tobytes() and got[1][j].tobytes() == want[j][1].tobytes() and
                    got[2][j].tobytes() == want[j][2].tobytes() for j in range(k))
        ts, tb = [], []
        for _ in range(reps):
            t0 = time.perf_counter(); singles(); ts.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); batched(); tb.append(time.perf_counter() - t0)
        ps, pb = k / statistics.median(ts), k / statistics.median(tb)
        out.append({"curve": curve, "shape": shape, "m": m, "n_v": n_v, "K": k, "threads_proofs_per_s": round(ps, 1),
                    "batch_proofs_per_s": round(pb, 1), "ratio": round(pb / ps, 3), "equal": equal})
        print("[prove_batch_bench] %s" % json.dumps(out[-1]), file=sys.stderr, flush=True)
        zdev.free()
    pool.shutdown()
    dpk.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ks", default="8,32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--distinct", type=int, default=4, help="distinct assignments per shape (tiled over the K rows)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    ks = [int(x) for x in args.ks.split(",")]
    plan = [("bn254", s) for s in args.shapes.split(",")]
    if HEADLINE in args.shapes.split(","):
        plan.append(("bls12_381", HEADLINE))
    ctxs, results = {}, []
    try:
        for curve, shape in plan:
            if curve not in ctxs:
                ctxs[curve] = capi.Context(curve, args.device)
            results += bench_shape(ctxs[curve], curve, shape, ks, args.reps, args.threads, args.distinct)
    finally:
        for c in ctxs.values():
            c.close()
    print(json.dumps({"tool": "prove_batch_bench", "threads": args.threads, "reps": args.reps, "results": results,
                      "all_equal": all(r["equal"] for r in results),
                      "min_ratio": min(r["ratio"] for r in results) if results else None}))


if __name__ == "__main__":
    main()
