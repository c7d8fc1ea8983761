"""prove_chunk_bench.py — which chunk shape the device wants: one proving-key class of big-merkle-64x32 (BN254 by default)
resident, the same proofs run as

  batch32     one hk_prove_batch of 32 proofs: chunks of HK_PROVE_BATCH_CHUNK = 8, one after another on one prove lane;
  2x<n>       two threads, each calling hk_prove_batch with n proofs four times in a row (a call of n <= 8 is one chunk of
              n on one prove lane, so two chunks of n run side by side), n = 4, 3 and 8;
  threads8    32 hk_prove calls on 8 threads: the coalesced path, whatever chunks it forms (their mean size is reported).

The forms alternate; the figure of each is the median over --reps repetitions.  One JSON line.

usage:  python tools/prove_chunk_bench.py [--curve bn254] [--shape big-merkle-64x32] [--reps 3]
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

ROWS = 32


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--curve", default="bn254")
    ap.add_argument("--shape", default="big-merkle-64x32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    curve = args.curve
    with capi.Context(curve, args.device) as ctx:
        fc, fr = FrCodec(curve), ctx.fr_bytes
        circ = make_config(curve, args.shape)
        pk, _td = generate_parameters(circ, curve, SeededRng(b"PROVE-CHUNK-BENCH-KEY-0123456789"), ctx)
        dpk = pk.upload(ctx)
        n_v = circ.n_v
        nb = n_v * fr
        base = []
        for j in range(args.distinct):
            circ.set_witness_seed(900 + j)
            base.append(np.frombuffer(bytes(circ.full_assignment_bytes()), np.uint8))
        zdev = capi.DeviceBuffer.from_host(ctx, np.ascontiguousarray(np.concatenate([base[j % args.distinct] for j in range(ROWS)])))
        r = fc.enc([0x1000_0001 + 7919 * j for j in range(ROWS)])
        s = fc.enc([0x2000_0003 + 104729 * j for j in range(ROWS)])
        kap = fc.enc([0x3000_0005 + 1299709 * j for j in range(ROWS)])
        pool8, pool2 = ThreadPoolExecutor(8), ThreadPoolExecutor(2)
        sizes = []

        def rows(j0, n):                                   # rows j0 .. j0 + n - 1 as one hk_prove_batch call
            return dpk.prove_batch(zdev.view(j0 * nb, n * nb), r[j0 * fr:(j0 + n) * fr], s[j0 * fr:(j0 + n) * fr],
                                   kap[j0 * fr:(j0 + n) * fr], n_v, n)

        def one(j):
            out = dpk.prove(zdev.view(j * nb, nb), r[j * fr:(j + 1) * fr], s[j * fr:(j + 1) * fr], kap[j * fr:(j + 1) * fr], n_v=n_v)
            sizes.append(ctx.last_timings()["batch_proofs"])
            return out

        def batch32():
            rows(0, ROWS)
            return ROWS

        def side_by_side(n):
            def f():
                def worker(t):
                    for i in range(4):
                        rows(((2 * i + t) * n) % (ROWS - n + 1), n)
                list(pool2.map(worker, range(2)))
                return 8 * n
            return f

        def threads8():
            list(pool8.map(one, range(ROWS)))
            return ROWS

        forms = [("threads8", threads8), ("batch32", batch32), ("2x4", side_by_side(4)), ("2x3", side_by_side(3)),
                 ("2x8", side_by_side(8))]
        # warm-up (arenas at their final size), and the forms must agree on a row
        want = one(5)
        got = rows(4, 4)
        equal = all(got[i][1].tobytes() == want[i].tobytes() for i in range(3))
        for _name, f in forms:
            f()
        sizes.clear()
        rates = {name: [] for name, _ in forms}
        for _ in range(args.reps):
            for name, f in forms:
                t0 = time.perf_counter()
                n = f()
                rates[name].append(n / (time.perf_counter() - t0))
        out = {"tool": "prove_chunk_bench", "curve": curve, "shape": args.shape, "reps": args.reps, "equal": equal,
               "lib": os.path.basename(os.path.dirname(capi.LIB_PATH)),
               "gather_us": os.environ.get("HK_PROVE_GATHER_US"),
               "proofs_per_s": {k: round(statistics.median(v), 1) for k, v in rates.items()},
               "proofs_per_s_runs": {k: [round(x, 1) for x in v] for k, v in rates.items()},
               "threads8_mean_chunk": round(len(sizes) / sum(1.0 / x for x in sizes), 2) if sizes else None}
        print(json.dumps(out))
        pool8.shutdown()
        pool2.shutdown()
        zdev.free()
        dpk.free()


if __name__ == "__main__":
    main()
