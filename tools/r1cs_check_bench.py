#!/usr/bin/env python3
"""R1CS satisfaction of device-resident assignments (hk_r1cs_check) against the only device route to the same yes / no that
existed before it, and against its own memory traffic.

Per shape and batch: the wall time of one hk_r1cs_check call with the class's matrices and `batch` assignments resident on
the device, cap = 8 and the row list left on the device (median of --reps runs after --warmup).  Beside it, in the same run: one hk_witness_map call on the same resident matrices and one of the assignments, which answers
for a single assignment and names no row (the top coefficient of h is zero iff it is satisfied).  The achieved rate is given
against the call's own traffic in the grid.y form: 36 B per non-zero read once per assignment, plus n_c / 8 bytes written.
The last assignment of every batch has one witness value replaced; the call must report failing rows for it and satisfaction
for the others before a row is written.  Shapes: the leaf class of big-merkle-sha-64x32 (the
`with_synthesis` leg of bench.py, m = 2^20) and the synthetic big-merkle-64x32 class (m = 2^21).  One JSON line per row,
appended to profiles/r1cs_check_bench.jsonl (--out).

    python tools/r1cs_check_bench.py [--curve bn254] [--shapes sha,synthetic] [--batches 1,8,64]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hekaton_system_amd import capi, workload  # noqa: E402
from hekaton_system_amd.cp_groth16 import FrCodec  # noqa: E402

SHAPES = {"sha": ("big-merkle-sha-64x32", 1), "synthetic": ("big-merkle-64x32", None)}
CAP = 8


def timed(ctx, fn, warmup, reps):
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i >= warmup:
            wall.append(dt * 1e3)
    return round(statistics.median(wall), 3), round(min(wall), 3)


def bench_shape(ctx, curve, shape, batches, warmup, reps):
    name, rep = SHAPES[shape]
    fc = FrCodec(curve)
    fr = ctx.fr_bytes
    circ = workload.make_config(curve, name, rep)
    circ.set_witness_seed(1)
    z_row = np.ascontiguousarray(circ.full_assignment_bytes())
    n_v, n_c = circ.n_v, circ.n_c
    host = circ.csr(fc)
    nnz = sum(int(m[1].size) for m in host)
    mats = [tuple(capi.DeviceBuffer.from_host(ctx, x) for x in m) for m in host]
    keep = []
    csrs = ctx._csrs(mats, keep)
    m_dom = 1
    while m_dom < n_c + circ.N_INST:
        m_dom *= 2
    # the parent's route: one assignment, no row index
    z1 = capi.DeviceBuffer.from_host(ctx, z_row)
    h = capi.DeviceBuffer(ctx, m_dom * fr)
    m_out = C.c_size_t()

    def witness_map():
        capi.check(ctx.lib.hk_witness_map(ctx.handle, C.byref(csrs[0]), C.byref(csrs[1]), C.byref(csrs[2]), circ.N_INST, n_c, z1.ptr,
                                          n_v, h.ptr, m_dom, C.byref(m_out)), "hk_witness_map")
    wm_ms, wm_min = timed(ctx, witness_map, warmup, reps)
    assert not h.view((m_dom - 1) * fr, fr).to_host().any(), "the assignment does not satisfy its class"
    h.free()
    z1.free()
    rows_out = []
    tampered_col = int(host[2][1][-1])                              # the last column C mentions: its row's c moves, a b does not
    bad_val = fc.enc1(12345)
    for batch in batches:
        z = capi.DeviceBuffer(ctx, batch * n_v * fr)
        for b in range(batch):
            capi.check(ctx.lib.hk_dev_upload(ctx.handle, z.ptr + b * n_v * fr, z_row.ctypes.data, n_v * fr), "hk_dev_upload")
        capi.check(ctx.lib.hk_dev_upload(ctx.handle, z.ptr + ((batch - 1) * n_v + tampered_col) * fr, bad_val.ctypes.data, fr),
                   "hk_dev_upload")
        verdicts = np.zeros((batch, 2), np.uint32)
        bad_rows = capi.DeviceBuffer(ctx, batch * CAP * 4)

        def check():
            capi.check(ctx.lib.hk_r1cs_check(ctx.handle, C.byref(csrs[0]), C.byref(csrs[1]), C.byref(csrs[2]), z.ptr, n_v, batch,
                                             verdicts.ctypes.data, bad_rows.ptr, None, CAP), "hk_r1cs_check")
        ms, ms_min = timed(ctx, check, warmup, reps)
        assert (verdicts[:-1] == (0, 0xFFFFFFFF)).all() and verdicts[-1, 0] >= 1, verdicts[-3:]
        listed = np.frombuffer(bad_rows.to_host().tobytes(), np.uint32).reshape(batch, CAP)
        assert (listed[:-1] == 0xFFFFFFFF).all() and listed[-1, 0] == verdicts[-1, 1]
        traffic = batch * (36 * nnz + n_c // 8)
        row = dict(curve=curve, shape=shape, config=name, n_c=n_c, n_v=n_v, nnz=nnz, m=m_dom, batch=batch, cap=CAP, reps=reps,
                   warmup=warmup, r1cs_check_wall_ms=ms, r1cs_check_wall_ms_min=ms_min, per_assignment_ms=round(ms / batch, 4),
                   model_bytes=traffic, model_gb_per_s=round(traffic / ms / 1e6, 1), witness_map_one_assignment_ms=wm_ms,
                   witness_map_one_assignment_ms_min=wm_min, n_bad_last=int(verdicts[-1, 0]), first_bad_last=int(verdicts[-1, 1]))
        row["faster_than_witness_map_per_assignment"] = row["per_assignment_ms"] < wm_ms
        rows_out.append(row)
        print(json.dumps(row), flush=True)
        bad_rows.free()
        z.free()
    for m in mats:
        for x in m:
            x.free()
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", default="bn254")
    ap.add_argument("--shapes", default="sha,synthetic")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_check_bench.jsonl"))
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",") if x]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with capi.Context(a.curve, 0) as ctx:
        for shape in a.shapes.split(","):
            for row in bench_shape(ctx, a.curve, shape, ints(a.batches), a.warmup, a.reps):
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
