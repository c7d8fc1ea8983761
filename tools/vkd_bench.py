#!/usr/bin/env python3
"""A VKD job's trace and witness on the device (hk_vkd_trace / hk_vkd_witness) beside the host mirror.

Per curve and log2(number of subcircuits), at --depth / --split (128 / 4: the reference's), in the same run:

  device   everything resident (leaves, siblings, Poseidon constants, outputs), then hk_vkd_trace -> hk_trace_sort ->
           hk_exec_tree, and per class one hk_vkd_witness + one hk_stage1_witness over its members
           (`VkdStage1Device.fill`): wall time of each step, median of --reps after --warmup, the context synchronised
           before each
  host     `VkdJob(...)` - the value table and the trace, about 2 depth + 3 Poseidon permutations per update in Python -
           once; `VkdJob.random`'s sparse tree is not counted on either side

The device trace is compared with the host's byte for byte, and one device row per class with the host mirror's, before a
line is written.  One JSON line per job, appended to profiles/vkd_bench.jsonl (--out).

    python tools/vkd_bench.py [--curves bn254,bls12_381] [--log-n 5,8]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hekaton_system_amd import capi  # noqa: E402
from hekaton_system_amd.cp_groth16 import FrCodec  # noqa: E402
from hekaton_system_amd.poseidon import device_params  # noqa: E402
from hekaton_system_amd.vkd_circuit import VkdJob  # noqa: E402

CHAL = (0x1234567, 0x7654321)


def _median_ms(ctx, fn, warmup, reps):
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(wall), 3)


def bench_job(ctx, curve, log_n, depth, split, warmup, reps):
    made = VkdJob.random(curve, log_n, depth, split)
    t0 = time.perf_counter()
    job = VkdJob(curve, made.initial_root, made.final_root, made.updates, depth, split)
    host_trace_ms = (time.perf_counter() - t0) * 1e3
    job.set_challenges(CHAL)
    fr, n = ctx.fr_bytes, int(job.offsets[-1])
    t = job.tables()
    params = device_params(curve, FrCodec(curve))
    dev = [capi.DeviceBuffer.from_host(ctx, np.ascontiguousarray(x).reshape(-1).view(np.uint8))
           for x in (t["leaves"], t["siblings"], params[0])]
    t_d, params_d = dict(t, leaves=dev[0], siblings=dev[1]), (dev[2],) + tuple(params[1:])
    outs = (capi.DeviceBuffer(ctx, len(job.values) * fr), capi.DeviceBuffer(ctx, n * 2 * fr))
    trace_ms = _median_ms(ctx, lambda: ctx.vkd_trace(t_d, params_d, out=outs), warmup, reps)
    assert (outs[0].to_host() == job.values_bytes()).all() and (outs[1].to_host() == job.flat("time")).all(), \
        "hk_vkd_trace differs from the host mirror"
    for x in outs + tuple(dev):
        x.free()
    dev0 = job.stage0_device(ctx)
    sort_ms = _median_ms(ctx, lambda: ctx.trace_sort(2, dev0.traces[0], n, device_out=True).free(), warmup, reps)
    dev1 = job.stage1_device(ctx, dev0=dev0)
    tree_ms = _median_ms(ctx, lambda: [x.free() for x in ctx.exec_tree(dev1.params, 2, job.offsets, dev0.traces[0], dev0.traces[1],
                                                                          dev1.challenges, device_out=True)], warmup, reps)
    per_class, body_ms, stage1_ms, written = {}, 0.0, 0.0, 0
    for (kind, first, last), members in job.classes().items():
        circ = job.make_class(members[0])
        members = np.array(members, np.uint32)
        z = capi.DeviceBuffer(ctx, members.size * circ.n_v * fr)
        b = _median_ms(ctx, lambda: ctx.vkd_witness(dev1.tables, dev1.params, dev0.values, members, circ.n_v, circ.device_cols, z),
                       warmup, reps)
        s = _median_ms(ctx, lambda: ctx.stage1_witness(dev1.params, circ.np_, job.offsets, dev0.traces[0], dev0.traces[1],
                                                       dev1.challenges, dev1.outs, members, circ.n_v,
                                                       (1, circ.N_INST, circ.pos_col0), z), warmup, reps)
        assert (z.to_host()[:circ.n_v * fr] == job.assignment_bytes(int(members[0]))).all(), \
            "the device row of subcircuit %d differs from the host mirror" % members[0]
        z.free()
        name = kind + (" (first)" if first else "")
        per_class[name] = dict(rows=int(members.size), n_c=circ.n_c, n_v=circ.n_v, k=circ.np_, vkd_witness_wall_ms=b,
                               stage1_witness_wall_ms=s)
        body_ms, stage1_ms, written = body_ms + b, stage1_ms + s, written + members.size * circ.n_v * fr
    dev1.free()
    dev0.free()
    return dict(curve=curve, log_n=log_n, depth=depth, split=split, n_sub=job.n, updates=len(job.updates), entries=n, reps=reps,
                warmup=warmup, vkd_trace_wall_ms=trace_ms, trace_sort_wall_ms=sort_ms, exec_tree_wall_ms=tree_ms,
                vkd_witness_wall_ms=round(body_ms, 3), stage1_witness_wall_ms=round(stage1_ms, 3),
                device_path_ms=round(trace_ms + sort_ms + tree_ms + body_ms + stage1_ms, 3), assignment_mb=round(written / 1e6, 2),
                host_trace_ms=round(host_trace_ms, 1), classes=per_class)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--log-n", default="5,8")
    ap.add_argument("--depth", type=int, default=128)
    ap.add_argument("--split", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vkd_bench.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for curve in a.curves.split(","):
        with capi.Context(curve, 0) as ctx:
            for log_n in a.log_n.split(","):
                row = bench_job(ctx, curve, int(log_n), a.depth, a.split, a.warmup, a.reps)
                print(json.dumps(row), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
