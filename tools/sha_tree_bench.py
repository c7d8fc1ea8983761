#!/usr/bin/env python3
"""The head of a big-merkle job on the device (hk_sha_tree) against the host path it replaces.

Per shape: the wall time of one hk_sha_tree call with the leaves resident on the device and the three outputs left there
(median of --reps runs after --warmup), and beside it the time of the host path on the same box for the same leaves, run
once - the ShaMerkleJob constructor (hashlib level by level, the trace in Python lists, its sort) and the flatten /
FrCodec.enc / upload Stage0Device.__init__ does.  The device outputs are compared with the host's before a row is written.
A call is a dependent chain of ns + 1 compressions for the leaf level and ns for each of the log2(n) - 1 levels above;
`compressions_in_chain` and the per-compression latency the wall time implies (an upper bound: launches, copies and the
trace kernel are in it) are in the row.  One JSON line per row, appended to profiles/sha_tree_bench.jsonl (--out).

    python tools/sha_tree_bench.py [--shapes bn254:64,bn254:1024,bn254:4096,bls12_381:64] [--ns 38] [--portals 4]
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hekaton_system_amd import capi  # noqa: E402
from hekaton_system_amd.cp_groth16 import FrCodec  # noqa: E402
from hekaton_system_amd.sha_circuit import ShaMerkleJob  # noqa: E402


def bench_shape(ctx, curve, n, ns, k, warmup, reps):
    fc = FrCodec(curve)
    rnd = random.Random(n * 1000003 + ns)
    leaves = [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(n // 2)]
    t0 = time.perf_counter()
    job = ShaMerkleJob(curve, n, ns, k, leaves)
    t1 = time.perf_counter()
    time_b = fc.enc([x for ops in job.time for e in ops for x in e])
    t2 = time.perf_counter()
    up = capi.DeviceBuffer.from_host(ctx, time_b)
    ctx.sync()
    t3 = time.perf_counter()
    up.free()
    want = [np.frombuffer(b"".join(job.digest), np.uint8), time_b, fc.enc([job.sha_root])]
    src = capi.DeviceBuffer.from_host(ctx, np.frombuffer(b"".join(leaves), np.uint8))
    outs = [capi.DeviceBuffer(ctx, x.size) for x in want]
    o = capi.hk_sha_tree_out(*[capi.ptr(x) for x in outs])
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t4 = time.perf_counter()
        capi.check(ctx.lib.hk_sha_tree(ctx.handle, src.ptr, n, ns, k, C.byref(o)), "hk_sha_tree")
        dt = time.perf_counter() - t4
        if i == 0:
            for name, g, w in zip(("digests", "trace", "sha_root"), outs, want):
                assert np.array_equal(g.to_host(), w), "%s differs from the host path" % name
        if i >= warmup:
            wall.append(dt * 1e3)
    for x in [src] + outs:
        x.free()
    chain = (ns + 1) + ns * (n.bit_length() - 2)                    # the leaf level, then log2(n) - 1 levels
    med = statistics.median(wall)
    row = dict(curve=curve, n_sub=n, ns=ns, n_portals=k, reps=reps, warmup=warmup, sha_tree_wall_ms=round(med, 3),
               sha_tree_wall_ms_min=round(min(wall), 3), compressions_in_chain=chain,
               us_per_compression_implied=round(med * 1e3 / chain, 2),
               host_constructor_ms=round((t1 - t0) * 1e3, 1), host_encode_ms=round((t2 - t1) * 1e3, 1),
               host_upload_ms=round((t3 - t2) * 1e3, 2), host_path_ms=round((t3 - t0) * 1e3, 1))
    row["device_faster"] = row["sha_tree_wall_ms"] < row["host_path_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bn254:64,bn254:1024,bn254:4096,bls12_381:64")
    ap.add_argument("--ns", type=int, default=38)
    ap.add_argument("--portals", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sha_tree_bench.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    shapes = [(s.split(":")[0], int(s.split(":")[1])) for s in a.shapes.split(",") if s]
    for curve in dict.fromkeys(c for c, _ in shapes):
        with capi.Context(curve, 0) as ctx:
            for n in [n for c, n in shapes if c == curve]:
                row = bench_shape(ctx, curve, n, a.ns, a.portals, a.warmup, a.reps)
                print(json.dumps(row), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
