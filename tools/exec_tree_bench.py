#!/usr/bin/env python3
"""The coordinator's step between the rounds on the device (hk_exec_tree) against the host path it replaces.

Per shape: the wall time of one hk_exec_tree call with the two traces and the Poseidon constants resident on the device and
the outputs left there (median of --reps runs after --warmup), and beside it the time of the host path on the same box for
the same input - transcript.running_evaluations + poseidon.ExecTree, run once (the Poseidon constants are generated
before either clock starts).  The device outputs are compared with the host's before a row is written.  Shapes: n_sub 64
and 1 024 with 4 entries per subtrace on each curve, and one long trace (n_sub 1 024 x 1 024 entries, BN254).  One JSON
line per row, appended to profiles/exec_tree_bench.jsonl (--out).

    python tools/exec_tree_bench.py [--curves bn254,bls12_381] [--shapes 64x4,1024x4] [--long 1024x1024]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hekaton_system_amd import capi, transcript  # noqa: E402
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec  # noqa: E402
from hekaton_system_amd.poseidon import ExecTree, device_params, merkle_params  # noqa: E402

COM = b"exec tree bench: the super commitment's bytes"


def bench_shape(ctx, curve, n_sub, per, warmup, reps):
    r = CURVE_PARAMS[curve]["r"]
    fc = FrCodec(curve)
    rnd = random.Random(n_sub * 1000003 + per)
    merkle_params(curve)                                            # cached from here on, for both paths
    time_st = [[transcript.RomTranscriptEntry(rnd.randrange(1 << 20), rnd.getrandbits(250) % r) for _ in range(per)]
               for _ in range(n_sub)]
    addr_st = transcript.sort_subtraces_by_addr(time_st)
    t0 = time.perf_counter()
    leaves = transcript.running_evaluations(transcript.ROM, COM, r, time_st, addr_st)
    t1 = time.perf_counter()
    fields = [[ev.time_ordered_eval, ev.addr_ordered_eval] + last.to_field_elements() for ev, last in leaves]
    tree = ExecTree(curve, fields)
    paths = [tree.path(i) for i in range(n_sub)]
    t2 = time.perf_counter()
    chal = transcript.RunningEvaluation.new(transcript.ROM, COM, r).challenges
    offsets, time_b = transcript.flatten_subtraces(fc, time_st)
    _, addr_b = transcript.flatten_subtraces(fc, addr_st)
    params = device_params(curve, fc)
    res = [capi.DeviceBuffer.from_host(ctx, x) for x in (time_b, addr_b, params[0])]
    params_d = (res[2],) + params[1:]
    chal_b = fc.enc(chal)
    depth = n_sub.bit_length() - 1
    outs = [capi.DeviceBuffer(ctx, k * ctx.fr_bytes) for k in (2 * n_sub, 4 * n_sub, 2 * n_sub - 1, n_sub * depth, 1)]
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t3 = time.perf_counter()
        ctx.exec_tree(params_d, 2, offsets, res[0], res[1], chal_b, out=outs)
        dt = time.perf_counter() - t3
        if i == 0:
            got = [fc.dec(x.to_host()) for x in outs]
            assert got[1] == [x for f in fields for x in f], "leaves differ from the host path"
            assert got[2] == [x for lvl in tree.levels for x in lvl], "tree differs from the host path"
            assert got[3] == [x for sib, _ in paths for x in sib] and got[4] == [tree.root], "paths differ from the host path"
        if i >= warmup:
            wall.append(dt * 1e3)
    for x in res + outs:
        x.free()
    row = dict(curve=curve, n_sub=n_sub, entries_per_subtrace=per, entries=n_sub * per, reps=reps, warmup=warmup,
               exec_tree_wall_ms=round(statistics.median(wall), 3), exec_tree_wall_ms_min=round(min(wall), 3),
               host_evals_ms=round((t1 - t0) * 1e3, 1), host_tree_ms=round((t2 - t1) * 1e3, 1),
               host_path_ms=round((t2 - t0) * 1e3, 1))
    row["device_faster"] = row["exec_tree_wall_ms"] < row["host_path_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--shapes", default="64x4,1024x4")
    ap.add_argument("--long", default="1024x1024", help="one long-trace shape, run on the first curve only ('' = none)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exec_tree_bench.jsonl"))
    a = ap.parse_args()
    shape = lambda s: tuple(int(x) for x in s.split("x"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for k, curve in enumerate(a.curves.split(",")):
        shapes = [shape(s) for s in a.shapes.split(",") if s] + ([shape(a.long)] if a.long and k == 0 else [])
        with capi.Context(curve, 0) as ctx:
            for n_sub, per in shapes:
                row = bench_shape(ctx, curve, n_sub, per, a.warmup, a.reps)
                print(json.dumps(row), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
