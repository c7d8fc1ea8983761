#!/usr/bin/env python3
"""A RAM subcircuit's whole assignment row on the device (hk_ram_stage1_witness), timed.

Per curve and shape (a VM job of n_sub subcircuits with `ops` operations per chunk, k = 32 + 3 ops entries per order in a
middle subcircuit, `batch` middle subcircuits selected): the wall time of one hk_ram_stage1_witness call over the two traces,
hk_exec_tree's outputs and the class's template row, all resident on the device (median of --reps runs after --warmup, the
context synchronised before each), and of one hk_ram_stage0_witness call over the same rows.  Beside it, for scale, the host
mirror of ONE row: `VmJob.assignment_bytes` of a middle-class subcircuit of the same k, taken from a two-subcircuit job
(depth 1: its membership block is nine levels shorter than the device rows'; everything that grows with k is the same).

The job's trace is the reference's default one (every `set` writes 1) built with numpy and taken to Montgomery form on the
device, so the k = 3 104 shape (3.2 M entries) needs no Python object per entry; hk_trace_sort and hk_exec_tree then make the
address order and the execution tree where hk_ram_stage1_witness reads them.  The first row of the call is compared with the
host mirror's time-ordered entry columns before a line is written.  One JSON line per row, appended to
profiles/ram_witness_bench.jsonl (--out).

    python tools/ram_witness_bench.py [--curves bn254] [--shapes 1024x1,1024x1024] [--batch 64]
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
from hekaton_system_amd.vm_circuit import REGISTER_NUM, VmJob, ram_class, vm_subtraces  # noqa: E402

CHAL = (0x1234567, 0x7654321, 0xabcdef1, 0x1fedcba)


def _median_ms(ctx, fn, warmup, reps):
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(wall), 3), round(min(wall), 3)


def vm_trace_fields(log_n_sub, ops):
    """(offsets uint32 [n + 1], fields uint64 [entries, 4]) of `vm_subtraces(log_n_sub, ops)`: (addr, val, timestamp, read)."""
    n = 1 << log_n_sub
    regs = np.arange(1, REGISTER_NUM + 1, dtype=np.uint64)
    op_addr, op_read = np.tile(np.uint64(2), 3 * ops), np.tile(np.array([0, 1, 1], np.uint64), ops)
    first = (np.concatenate([regs, op_addr]), np.concatenate([np.zeros(REGISTER_NUM, np.uint64), op_read]))
    later = (np.concatenate([regs, op_addr, regs]),
             np.concatenate([np.ones(REGISTER_NUM, np.uint64), op_read, np.zeros(REGISTER_NUM, np.uint64)]))
    addr = np.concatenate([first[0]] + [later[0]] * (n - 1))
    read = np.concatenate([first[1]] + [later[1]] * (n - 1))
    offsets = np.zeros(n + 1, np.uint32)
    offsets[1:] = len(first[0]) + len(later[0]) * np.arange(n)
    fields = np.stack([addr, np.ones_like(addr), np.arange(len(addr), dtype=np.uint64), read], axis=1)
    return offsets, fields


def bench_shape(ctx, curve, n_sub, ops, batch, warmup, reps):
    fc = FrCodec(curve)
    fr = ctx.fr_bytes
    log_n = n_sub.bit_length() - 1
    offsets, fields = vm_trace_fields(log_n, ops)
    small = vm_subtraces(2, 1)
    _, sf = vm_trace_fields(2, 1)
    assert [tuple(int(x) for x in row) for row in sf] == [(e.addr, e.val, e.i, int(e.read)) for st in small for e in st]
    n = fields.shape[0]
    canon = np.zeros((n * 4, fr), np.uint8)
    canon[:, :8] = fields.reshape(-1, 1).view(np.uint8)
    raw = capi.DeviceBuffer.from_host(ctx, canon.reshape(-1))
    del canon
    time_d = capi.DeviceBuffer(ctx, n * 4 * fr)
    capi.check(ctx.lib.hk_field_convert(ctx.handle, 0, raw.ptr, time_d.ptr, n * 4, 1), "hk_field_convert")
    raw.free()
    addr_d = ctx.trace_sort(4, time_d, n, device_out=True)
    consts, n_consts, ld, nd = device_params(curve, fc)
    params = (capi.DeviceBuffer.from_host(ctx, consts), n_consts, ld, nd)
    chal_b = fc.enc(list(CHAL))
    outs = ctx.exec_tree(params, 4, offsets, time_d, addr_d, chal_b, device_out=True)
    k = 2 * REGISTER_NUM + 3 * ops
    circ = ram_class(curve, k, False, False, log_n, 0)
    tmpl = capi.DeviceBuffer.from_host(ctx, fc.enc(circ.template_ints()))
    members = (1 + (np.arange(batch, dtype=np.uint32) * 7) % (n_sub - 2)).astype(np.uint32)
    z = capi.DeviceBuffer(ctx, batch * circ.n_v * fr)
    w = capi.DeviceBuffer(ctx, batch * 70 * k * fr)
    layout = (1, circ.N_INST, circ.col0, circ.pos_col0)
    s1 = lambda: ctx.ram_stage1_witness(params, k, offsets, time_d, addr_d, chal_b, outs, members, circ.n_v, layout, z, template=tmpl)
    s0 = lambda: ctx.ram_stage0_witness(offsets, k, time_d, addr_d, members, w)
    s1_ms, s1_min = _median_ms(ctx, s1, warmup, reps)
    s0_ms, s0_min = _median_ms(ctx, s0, warmup, reps)
    # the host mirror of one row of the same k, for scale (the class is built before the clock starts)
    host_job = VmJob(curve, 1, ops, 0)
    host_job.set_challenges(CHAL)
    host_job.make_class(1)
    t0 = time.perf_counter()
    host_row = host_job.assignment_bytes(1)
    host_ms = (time.perf_counter() - t0) * 1e3
    got = z.view(0, circ.n_v * fr).to_host().reshape(circ.n_v, fr)
    got0 = w.view(0, 70 * k * fr).to_host()
    assert (got[circ.N_INST:circ.N_INST + 70 * k].reshape(-1) == got0).all(), "the two calls disagree on the stage-0 columns"
    # a middle subcircuit of the big job and subcircuit 1 of the small one run the same accesses: val / addr / read of the
    # time-ordered entries agree (the address-ordered slices are cut from different sorted traces; tests/test_ram_witness_gpu.py
    # compares whole rows)
    want = host_row.reshape(-1, fr)
    cols = [c for e in range(k) for c in (circ.N_INST + 35 * e, circ.N_INST + 35 * e + 1, circ.N_INST + 35 * e + 34)]
    assert (got[cols] == want[cols]).all(), "hk_ram_stage1_witness differs from the host mirror"
    for x in [time_d, addr_d, params[0], tmpl, z, w] + list(outs):
        x.free()
    return dict(curve=curve, n_sub=n_sub, ops=ops, n_portals=k, batch=batch, n_v=circ.n_v, entries=int(n), reps=reps, warmup=warmup,
                ram_stage1_witness_wall_ms=s1_ms, ram_stage1_witness_wall_ms_min=s1_min,
                ram_stage0_witness_wall_ms=s0_ms, ram_stage0_witness_wall_ms_min=s0_min,
                row_mb=round(circ.n_v * fr / 1e6, 3), stage1_gb_per_s=round(batch * circ.n_v * fr / s1_ms / 1e6, 1),
                host_mirror_one_row_ms=round(host_ms, 1), host_mirror_batch_ms_extrapolated=round(host_ms * batch, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254")
    ap.add_argument("--shapes", default="1024x1,1024x1024", help="n_sub x operations per chunk")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ram_witness_bench.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for curve in a.curves.split(","):
        with capi.Context(curve, 0) as ctx:
            for s in a.shapes.split(","):
                n_sub, ops = (int(x) for x in s.split("x"))
                row = bench_shape(ctx, curve, n_sub, ops, a.batch, a.warmup, a.reps)
                print(json.dumps(row), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
