#!/usr/bin/env python3
"""A partitioned R1CS job's witness on the device (hk_r1cs_job_trace / hk_r1cs_job_witness) beside its host mirror.

Per curve and shape PxTxW - P partitions of W wires each, T transactions with witnesses of their own; partition p owns 4
wires and borrows the 4 of partition p - 1; every other wire is defined by one imported constraint - in the same run:

  device   the witness blocks resident, then hk_r1cs_job_trace -> hk_trace_sort -> hk_exec_tree, and per partition one
           hk_r1cs_job_witness + one hk_stage1_witness over its T subcircuits (`R1csStage1Device.fill`): wall time of each
           step, median of --reps after --warmup, the context synchronised before each
  host     `PartitionedR1csJob(...)` (the trace and its address order), `set_challenges` (running evaluations, execution
           tree) and `assignment_bytes` of the P subcircuits of transaction 0, each once; the whole job's rows are that last
           figure times T (stated as an extrapolation)

The device rows of transaction 0 are compared with the host's byte for byte before a line is written.  One JSON line per
shape, appended to profiles/r1cs_job_bench.jsonl (--out).

    python tools/r1cs_job_bench.py [--curves bn254,bls12_381] [--shapes 4x4x130,4x256x1024]
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

from hekaton_system_amd import capi, circom  # noqa: E402
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS  # noqa: E402
from hekaton_system_amd.r1cs_circuit import Partition, PartitionedR1csJob  # noqa: E402

CHAL = (0x1234567, 0x7654321)
SHARED = 4


def _median_ms(ctx, fn, warmup, reps):
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(wall), 3)


def chain(p, n_wires):
    """(constraints, owned ids, borrowed ids) of partition p: x[w] = x[w-1] + x[1] + 7 + (a borrowed wire while any is
    unused), over the non-borrowed wires; the last SHARED of them are owned."""
    owned = [100 * p + j for j in range(SHARED)]
    borrowed = [100 * (p - 1) + j for j in range(SHARED)] if p else []
    last = n_wires - len(borrowed) - 1
    cons, pend = [], list(range(last + 1, n_wires))
    for w in range(2, last + 1):
        a = [(w - 1, 1), (1, 1), (0, 7)] + ([(pend.pop(0), 1)] if pend else [])
        cons.append((a, [(0, 1)], [(w, 1)]))
    return cons, owned, borrowed


def solve(cons, n_wires, owned, borrowed, shared, seed, r):
    x = [0] * n_wires
    x[0], x[1] = 1, random.Random(seed).randrange(1, r)
    for j, vid in enumerate(borrowed):
        x[n_wires - len(borrowed) + j] = shared[vid]
    for a, _b, c in cons:
        x[c[0][0]] = sum(k * x[i] for i, k in a) % r
    u = n_wires - len(owned) - len(borrowed)
    for i, vid in enumerate(owned):
        shared[vid] = x[u + i]
    return x


def bench_shape(ctx, curve, P, T, W, warmup, reps):
    r = CURVE_PARAMS[curve]["r"]
    shapes = [chain(p, W) for p in range(P)]
    wits = []
    for g in range(T):
        shared = {}
        wits.append([solve(c, W, o, b, shared, 1000 * g + p, r) for p, (c, o, b) in enumerate(shapes)])
    parts = []
    for (cons, owned, borrowed), w in zip(shapes, wits[0]):
        hdr = circom.Header(32, circom.BN254_R_LE, W, 0, 0, W - 1, W, len(cons))
        parts.append(Partition(circom.R1CSFile(1, hdr, cons), w, owned, borrowed))
    t0 = time.perf_counter()
    job = PartitionedR1csJob(curve, parts, T, witnesses=wits)
    t1 = time.perf_counter()
    job.set_challenges(CHAL)
    t2 = time.perf_counter()
    want = [job.assignment_bytes(p) for p in range(P)]
    t3 = time.perf_counter()
    tables, wit_b = job.tables(), job.witness_bytes()
    n = int(job.offsets[-1])
    t_up = time.perf_counter()
    wit_d = capi.DeviceBuffer.from_host(ctx, wit_b)
    ctx.sync()
    upload_ms = (time.perf_counter() - t_up) * 1e3
    trace_d = capi.DeviceBuffer(ctx, n * 2 * ctx.fr_bytes)
    trace_ms = _median_ms(ctx, lambda: ctx.r1cs_job_trace(tables, wit_d, out=trace_d), warmup, reps)
    assert (trace_d.to_host() == job.flat("time")).all(), "hk_r1cs_job_trace differs from the host trace"
    trace_d.free()
    wit_d.free()
    dev0 = job.stage0_device(ctx)
    sort_ms = _median_ms(ctx, lambda: ctx.trace_sort(2, dev0.traces[0], n, device_out=True).free(), warmup, reps)
    dev = job.stage1_device(ctx, dev0=dev0)
    tree_ms = _median_ms(ctx, lambda: [x.free() for x in ctx.exec_tree(dev.params, 2, job.offsets, dev0.traces[0], dev0.traces[1],
                                                                         dev.challenges, device_out=True)], warmup, reps)
    body_ms = stage1_ms = 0.0
    written = 0
    for p in range(P):
        members = np.arange(p, job.n, P, dtype=np.uint32)
        # the first and the last subcircuit have classes of their own with the same columns: one buffer per partition
        circ = job.make_class(int(members[min(1, T - 1)]))
        z = capi.DeviceBuffer(ctx, members.size * circ.n_v * ctx.fr_bytes)
        body_ms += _median_ms(ctx, lambda: ctx.r1cs_job_witness(tables, dev0.witness, members, circ.n_v, circ.body_col0, z),
                              warmup, reps)
        stage1_ms += _median_ms(ctx, lambda: ctx.stage1_witness(dev.params, circ.np_, job.offsets, dev0.traces[0], dev0.traces[1],
                                                                dev.challenges, dev.outs, members, circ.n_v,
                                                                (1, circ.N_INST, circ.pos_col0), z), warmup, reps)
        got = z.to_host()[:circ.n_v * ctx.fr_bytes]
        assert (got == want[p]).all(), "the device row of subcircuit %d differs from the host mirror" % p
        written += members.size * circ.n_v * ctx.fr_bytes
        z.free()
    dev.free()
    dev0.free()
    device_ms = trace_ms + sort_ms + tree_ms + body_ms + stage1_ms
    rows_ms = (t3 - t2) * 1e3
    return dict(curve=curve, partitions=P, txs=T, wires=W, n_sub=job.n, entries=n, reps=reps, warmup=warmup,
                witness_upload_ms=round(upload_ms, 3), r1cs_job_trace_wall_ms=trace_ms, trace_sort_wall_ms=sort_ms,
                exec_tree_wall_ms=tree_ms, r1cs_job_witness_wall_ms=round(body_ms, 3), stage1_witness_wall_ms=round(stage1_ms, 3),
                device_path_ms=round(device_ms, 3), assignment_mb=round(written / 1e6, 2),
                host_job_ms=round((t1 - t0) * 1e3, 1), host_set_challenges_ms=round((t2 - t1) * 1e3, 1),
                host_rows_one_tx_ms=round(rows_ms, 1), host_mirror_ms_extrapolated=round((t2 - t0) * 1e3 + rows_ms * T, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--shapes", default="4x4x130,4x256x1024")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_job_bench.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for curve in a.curves.split(","):
        with capi.Context(curve, 0) as ctx:
            for s in a.shapes.split(","):
                P, T, W = (int(x) for x in s.split("x"))
                row = bench_shape(ctx, curve, P, T, W, a.warmup, a.reps)
                print(json.dumps(row), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
