#!/usr/bin/env python3
"""A job's challenge-dependent witness on the device (hk_stage1_witness) against the path it replaces.

Per curve and shape (n_sub subcircuits x k entries per order, every subcircuit selected): the wall time of one
hk_stage1_witness call over hk_exec_tree's outputs and the two traces, all resident on the device (median of --reps runs
after --warmup), and beside it the parent path on the same inputs in the same run - sha_circuit.full_values +
poseidon_inputs on the host (run once), then hk_assignment_scatter + hk_poseidon_path with the host arrays they return
(median of --reps).  hk_poseidon_path over the device-resident leaves and siblings is timed too: the membership kernel
alone (the same quad kernel the new call launches; rows before this one in the jsonl timed the retired one-lane kernel
here), with the minimum and maximum over its repetitions as its spread.  The two assignments are compared byte for byte
before a row is written.  One JSON line per row, appended to profiles/stage1_witness_bench.jsonl (--out).

    python tools/stage1_witness_bench.py [--curves bn254,bls12_381] [--shapes 64x4,1024x4]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hekaton_system_amd import capi, transcript  # noqa: E402
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec  # noqa: E402
from hekaton_system_amd.poseidon import device_params  # noqa: E402
from hekaton_system_amd.sha_circuit import full_values, poseidon_inputs  # noqa: E402

COM = b"stage-1 witness bench: the super commitment's bytes"
N_INST = 4


def _median_ms(ctx, fn, warmup, reps):
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(wall), 3), round(min(wall), 3), round(max(wall), 3)


def bench_shape(ctx, curve, n_sub, k, warmup, reps):
    r = CURVE_PARAMS[curve]["r"]
    fc = FrCodec(curve)
    rnd = random.Random(n_sub * 1000003 + k)
    time_st = [[transcript.RomTranscriptEntry(rnd.randrange(1 << 20), rnd.getrandbits(250) % r) for _ in range(k)]
               for _ in range(n_sub)]
    addr_st = transcript.sort_subtraces_by_addr(time_st)
    chal = transcript.RunningEvaluation.new(transcript.ROM, COM, r).challenges
    offsets, time_b = transcript.flatten_subtraces(fc, time_st)
    _, addr_b = transcript.flatten_subtraces(fc, addr_st)
    params = device_params(curve, fc)
    res = [capi.DeviceBuffer.from_host(ctx, x) for x in (time_b, addr_b, params[0])]
    params_d = (res[2],) + params[1:]
    chal_b = fc.enc(chal)
    depth = n_sub.bit_length() - 1
    outs = ctx.exec_tree(params_d, 2, offsets, res[0], res[1], chal_b, device_out=True)
    # what each subcircuit's Stage1Request carries, decoded once from hk_exec_tree's outputs (not timed)
    ev, sib, root = fc.dec(outs[0].to_host()), fc.dec(outs[3].to_host()), fc.dec(outs[4].to_host())[0]
    pairs = lambda st: [(e.addr, e.val) for e in st]
    ws = [dict(entry_chal=chal[0], tr_chal=chal[1], root=root, time=pairs(time_st[i]), addr=pairs(addr_st[i]),
               time_eval0=ev[2 * i - 2] if i else 1, addr_eval0=ev[2 * i - 1] if i else 1,
               prev=pairs(addr_st[i - 1])[-1] if i else (0, 0), path=(sib[i * depth:(i + 1) * depth], i)) for i in range(n_sub)]
    pos_col0 = N_INST + 10 * k + 4
    circ = SimpleNamespace(r=r, N_INST=N_INST, pos_col0=pos_col0, kind="leaf", fc=fc)
    # the parent path: host values, then the two device calls
    t0 = time.perf_counter()
    cols, vals = full_values(circ, ws)
    t1 = time.perf_counter()
    leaves, sibs, idx = poseidon_inputs(circ, ws)
    t2 = time.perf_counter()
    vals = np.ascontiguousarray(vals)
    a, b = params[2], params[3]
    per_perm = lambda t, alpha, rf, rp, _off: rf * (t * (3 if alpha == 5 else 5) + t) + rp * ((3 if alpha == 5 else 5) + t)
    block = 2 * per_perm(*a) + depth * (3 + per_perm(*b))
    n_v = pos_col0 + block
    z_ref = capi.DeviceBuffer.from_host(ctx, np.zeros(n_sub * n_v * ctx.fr_bytes, np.uint8))
    z_new = capi.DeviceBuffer.from_host(ctx, np.zeros(n_sub * n_v * ctx.fr_bytes, np.uint8))
    scatter = lambda: capi.check(ctx.lib.hk_assignment_scatter(ctx.handle, cols.ctypes.data, vals.ctypes.data, cols.size, n_sub,
                                                               n_v, z_ref.ptr), "hk_assignment_scatter")
    scatter_ms, _, _ = _median_ms(ctx, scatter, warmup, reps)
    path_ms, _, _ = _median_ms(ctx, lambda: ctx.poseidon_path(params_d, leaves, sibs, idx, n_v, pos_col0, z_ref), warmup, reps)
    path_res = lambda: ctx.poseidon_path(params_d, outs[1], outs[3], idx, n_v, pos_col0, z_ref)
    path_res_ms, path_res_min, path_res_max = _median_ms(ctx, path_res, warmup, reps)
    rows = np.arange(n_sub, dtype=np.uint32)
    new = lambda: ctx.stage1_witness(params_d, k, offsets, res[0], res[1], chal_b, outs, rows, n_v, (1, N_INST, pos_col0), z_new)
    new_ms, new_min, new_max = _median_ms(ctx, new, warmup, reps)
    want, got = z_ref.to_host().reshape(n_sub, n_v, 32), z_new.to_host().reshape(n_sub, n_v, 32)
    assert (got[:, 1:] == want[:, 1:]).all(), "hk_stage1_witness differs from the parent path"
    for x in res + list(outs) + [z_ref, z_new]:
        x.free()
    host_ms = (t2 - t0) * 1e3
    row = dict(curve=curve, n_sub=n_sub, n_portals=k, depth=depth, n_v=n_v, reps=reps, warmup=warmup,
               stage1_witness_wall_ms=new_ms, stage1_witness_wall_ms_min=new_min, stage1_witness_wall_ms_max=new_max,
               host_full_values_ms=round((t1 - t0) * 1e3, 2), host_poseidon_inputs_ms=round((t2 - t1) * 1e3, 2),
               assignment_scatter_wall_ms=scatter_ms, poseidon_path_wall_ms=path_ms,
               parent_path_ms=round(host_ms + scatter_ms + path_ms, 3), poseidon_path_resident_wall_ms=path_res_ms,
               poseidon_path_resident_wall_ms_min=path_res_min, poseidon_path_resident_wall_ms_max=path_res_max)
    row["device_faster"] = row["stage1_witness_wall_ms"] < row["parent_path_ms"]
    row["call_faster_than_membership_alone"] = row["stage1_witness_wall_ms"] < row["poseidon_path_resident_wall_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--shapes", default="64x4,1024x4")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--build", default=None, help="a name for the library under test, kept in every row (HK_LIB builds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage1_witness_bench.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for curve in a.curves.split(","):
        with capi.Context(curve, 0) as ctx:
            for s in a.shapes.split(","):
                n_sub, k = (int(x) for x in s.split("x"))
                row = bench_shape(ctx, curve, n_sub, k, a.warmup, a.reps)
                if a.build:
                    row["build"] = a.build
                print(json.dumps(row), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
