#!/usr/bin/env python3
"""The coordinator's address sort on the device (hk_trace_sort) against the host path it replaces.

Per shape: the wall time of one hk_trace_sort call with the time-ordered trace resident on the device and both outputs (the
sorted entries and perm) left there (median of --reps runs after --warmup), and beside it the time of the host path on the
same box for the same input - transcript.sort_subtraces_by_addr plus the flatten_subtraces encode of the address order that
the device path makes unnecessary, run once.  The device output is compared with the host's before a row is written.
Shapes: ROM traces of 256, 4 096 and 1 048 576 entries and a RAM trace of 1 048 576, all with addresses below 2^20 (the
big-merkle range: 5 of 8 ROM passes are skipped), and a ROM trace of 1 048 576 full-width keys (no pass skipped).  One JSON
line per row, appended to profiles/trace_sort_bench.jsonl (--out).

    python tools/trace_sort_bench.py [--curve bn254] [--shapes rom:64x4,rom:1024x4,rom:1024x1024,ram:1024x1024,romfull:1024x1024]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hekaton_system_amd import capi, transcript  # noqa: E402
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec  # noqa: E402


def bench_shape(ctx, curve, kind, n_sub, per, warmup, reps):
    r = CURVE_PARAMS[curve]["r"]
    fc = FrCodec(curve)
    rnd = random.Random("%s %d %d" % (kind, n_sub, per))
    top = (1 << 64) if kind == "romfull" else (1 << 20)
    if kind == "ram":
        k = 4
        mk = lambda t: transcript.RamTranscriptEntry(rnd.randrange(top), rnd.getrandbits(250) % r, t, bool(rnd.getrandbits(1)))
    else:
        k = 2
        mk = lambda t: transcript.RomTranscriptEntry(rnd.randrange(top), rnd.getrandbits(250) % r)
    time_st = [[mk(i * per + j) for j in range(per)] for i in range(n_sub)]
    n = n_sub * per
    _, time_b = transcript.flatten_subtraces(fc, time_st)
    t0 = time.perf_counter()
    addr_st = transcript.sort_subtraces_by_addr(time_st)
    t1 = time.perf_counter()
    _, addr_b = transcript.flatten_subtraces(fc, addr_st)
    t2 = time.perf_counter()
    src = capi.DeviceBuffer.from_host(ctx, time_b)
    out, perm = capi.DeviceBuffer(ctx, n * k * ctx.fr_bytes), capi.DeviceBuffer(ctx, 4 * n)
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t3 = time.perf_counter()
        capi.check(ctx.lib.hk_trace_sort(ctx.handle, k, src.ptr, n, out.ptr, perm.ptr), "hk_trace_sort")
        dt = time.perf_counter() - t3
        if i == 0:
            assert (out.to_host() == addr_b).all(), "sorted entries differ from the host path"
            p = perm.to_host().view(np.uint32)
            assert (time_b.reshape(n, -1)[p] == addr_b.reshape(n, -1)).all(), "perm does not map the time order to the address order"
        if i >= warmup:
            wall.append(dt * 1e3)
    for x in (src, out, perm):
        x.free()
    row = dict(curve=curve, kind=kind, entry_fields=k, n_sub=n_sub, entries_per_subtrace=per, entries=n,
               addr_below="2^64" if kind == "romfull" else "2^20", reps=reps, warmup=warmup,
               trace_sort_wall_ms=round(statistics.median(wall), 3), trace_sort_wall_ms_min=round(min(wall), 3),
               host_sort_ms=round((t1 - t0) * 1e3, 1), host_encode_ms=round((t2 - t1) * 1e3, 1),
               host_path_ms=round((t2 - t0) * 1e3, 1))
    row["device_faster"] = row["trace_sort_wall_ms"] < row["host_path_ms"]
    row["device_faster_than_host_sort_alone"] = row["trace_sort_wall_ms"] < row["host_sort_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", default="bn254")
    ap.add_argument("--shapes", default="rom:64x4,rom:1024x4,rom:1024x1024,ram:1024x1024,romfull:1024x1024")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_sort_bench.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with capi.Context(a.curve, 0) as ctx:
        for s in a.shapes.split(","):
            kind, dims = s.split(":")
            n_sub, per = (int(x) for x in dims.split("x"))
            row = bench_shape(ctx, a.curve, kind, n_sub, per, a.warmup, a.reps)
            print(json.dumps(row), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
