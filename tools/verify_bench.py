"""verify_bench.py — proofs verified per second by hk_verify_batch on one device, per curve: per-proof mode and batch mode
(one randomised equation), at n = 64 and n = 1024 proofs, with and without the point checks (batch mode always checks).

The proofs are distinct stage-1 proofs of one "tiny" hekaton key class (hk_prove_batch), repeated to n; every input
stays resident in HBM, so a timing covers the verification launches only.  Each configuration runs `warmup` untimed
calls, then `reps` timed ones (each call ends in a stream synchronisation); the figure is the median.  Every call's
verdicts are checked to be all 1.  One JSON line per (curve, n, mode, check) and a final summary line.

usage:  python tools/verify_bench.py [--curves bn254,bls12_381] [--ns 64,1024] [--reps 5] [--warmup 2] [--modes proof,batch]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from hekaton_system_amd import capi  # noqa: E402
from hekaton_system_amd.cp_groth16 import FrCodec, SeededRng, generate_parameters, prepare_verifying_key  # noqa: E402
from hekaton_system_amd.workload import make_config  # noqa: E402

DISTINCT = 32


def proofs_of_class(ctx, curve):
    fc = FrCodec(curve)
    fr = ctx.fr_bytes
    circ = make_config(curve, "tiny")
    pk, _td = generate_parameters(circ, curve, SeededRng(b"VERIFY-BENCH-KEY-0123456789abcde"), ctx)
    dpk = pk.upload(ctx)
    z, coms, xs = [], [], []
    kaps = [0x3000_0005 + 1299709 * j for j in range(DISTINCT)]
    for j in range(DISTINCT):
        circ.set_witness_seed(700 + j)
        zj = circ.full_assignment_bytes()
        z.append(zj)
        coms.append(dpk.commit(0, circ.stage0_witness_bytes(), fc.enc1(kaps[j])))
        xs.append(zj[fr:circ.N_INST * fr])
    a, b, c = dpk.prove_batch(np.concatenate(z), fc.enc([11 + j for j in range(DISTINCT)]),
                              fc.enc([13 + j for j in range(DISTINCT)]), fc.enc(kaps), circ.n_v, DISTINCT)
    dpk.free()
    return pk.vk, a, b, c, np.stack(coms), np.stack(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--ns", default="64,1024")
    ap.add_argument("--modes", default="proof,batch")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    summary = {}
    for curve in args.curves.split(","):
        ctx = capi.Context(curve, 0)
        vk, a, b, c, ds, xs = proofs_of_class(ctx, curve)
        pvk = prepare_verifying_key(ctx, vk)
        fc = FrCodec(curve)
        for n in [int(v) for v in args.ns.split(",")]:
            idx = [i % DISTINCT for i in range(n)]
            bufs = [capi.DeviceBuffer.from_host(ctx, np.ascontiguousarray(t[idx])) for t in (a, b, c, ds, xs)]
            rnd = random.Random(n)
            rand = fc.enc([rnd.getrandbits(128) | 1 for _ in range(n)])
            for mode in args.modes.split(","):
                for check in ((True, False) if mode == "proof" else (True,)):
                    times = []
                    for k in range(args.warmup + args.reps):
                        t0 = time.perf_counter()
                        v = pvk.device.verify(*bufs, n=n, check_points=check, rand=rand if mode == "batch" else None)
                        dt = time.perf_counter() - t0
                        assert v.tolist() == [1] * n, (curve, n, mode, check)
                        if k >= args.warmup:
                            times.append(dt)
                    ms = statistics.median(times) * 1e3
                    row = {"curve": curve, "n": n, "mode": mode, "check_points": check, "median_ms": round(ms, 3),
                           "min_ms": round(min(times) * 1e3, 3), "max_ms": round(max(times) * 1e3, 3),
                           "proofs_per_s": round(n / (ms / 1e3), 1), "reps": args.reps}
                    print(json.dumps(row), flush=True)
                    summary["%s/n=%d/%s%s" % (curve, n, mode, "" if check else "/nocheck")] = row["proofs_per_s"]
            for t in bufs:
                t.free()
        pvk.free()
        ctx.close()
    print(json.dumps({"summary_proofs_per_s": summary}))


if __name__ == "__main__":
    main()
