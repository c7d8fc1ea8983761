#!/usr/bin/env python3
"""Device key generation (hk_keygen) against the split host + device setup, per proving-key class and curve.

For every class: the device time of each hk_keygen phase (the QAP at t, the scalar assembly, the fixed-base sweeps; HIP
events on the lane, hk_timings), the wall time of hk_qap_eval and of the whole hk_keygen (bulk arrays kept on the device,
as a coordinator that uploads the key next would), each the median of --reps runs after --warmup; and setup_host +
setup_device for the same class - the host half only up to --host-max-log-m (it grows linearly with m, 1 s at 2^16),
once per class.  One JSON line per (curve, class) to profiles/keygen_bench.jsonl (--out).

    python tools/keygen_bench.py [--curves bn254,bls12_381] [--classes tiny,big-merkle-4x1,...]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hekaton_system_amd import capi  # noqa: E402
from hekaton_system_amd.cp_groth16 import (CURVE_PARAMS, FrCodec, MultiStageConstraintSystem, SeededRng,  # noqa: E402
                                           csr_from_rows, setup_device, setup_host)
from hekaton_system_amd.workload import make_config  # noqa: E402

CLASSES = ["tiny", "big-merkle-4x1", "vkd-256", "vm-1024x1024", "big-merkle-64x32", "big-merkle-512x64",
           "big-merkle-sha-64x32"]
SEED = b"KEYGEN-BENCH-0123456789abcdef!!!"


def _inputs(circ, curve):
    """What hk_keygen takes for this class: synthesis in setup mode and the matrices (host work outside the timing)."""
    r = CURVE_PARAMS[curve]["r"]
    fc = FrCodec(curve)
    rng = SeededRng(SEED)
    alpha, beta, gamma = rng.fr(r) or 1, rng.fr(r) or 1, rng.fr(r) or 1
    deltas = [rng.fr(r) or 1 for _ in range(circ.total_num_stages())]
    g1s, g2s = rng.fr(r) or 1, rng.fr(r) or 1
    fast = hasattr(circ, "qap_evaluate")
    cs = MultiStageConstraintSystem(r, construct_matrices=not fast)
    for stage in range(circ.total_num_stages()):
        circ.generate_constraints(stage, cs)
    n_inst, n_wit, n_c = cs.num_instance_variables(), cs.num_witness_variables(), cs.num_constraints()
    t = rng.fr(r)
    matrices = circ.csr(fc) if fast else tuple(csr_from_rows(fc, M) for M in cs.to_matrices())
    return dict(matrices=matrices, n_inst=n_inst, n_constraints=n_c, n_v=n_inst + n_wit,
                stage_ranges=list(cs.variable_range_for_stage), alpha=alpha, beta=beta, gamma=gamma, deltas=deltas, t=t,
                g1_scalar=g1s, g2_scalar=g2s)


def _free(res):
    for k in ("a_g", "b_g", "b_h", "h_g"):
        if isinstance(res[k], capi.DeviceBuffer):
            res[k].free()


def bench_class(ctx, curve, name, warmup, reps, host_max_log_m):
    t0 = time.perf_counter()
    circ = make_config(curve, name)
    kw = _inputs(circ, curve)
    prep_s = time.perf_counter() - t0
    # device matrices: what a coordinator that keeps the class resident hands over (no PCIe in the timings)
    dev_m = tuple(tuple(capi.DeviceBuffer.from_host(ctx, x) for x in M) for M in kw["matrices"])
    kw_d = dict(kw, matrices=dev_m)
    ctx.set_profiling(True)
    phases, whole, qap = [], [], []
    for i in range(warmup + reps):
        ctx.sync()
        t1 = time.perf_counter()
        res = ctx.keygen(on_device=True, **kw_d)
        ctx.sync()
        dt = time.perf_counter() - t1
        tm = ctx.last_timings()
        m = res["m"]
        _free(res)
        t1 = time.perf_counter()
        ctx.qap_eval(*dev_m, kw["n_inst"], kw["n_constraints"], kw["n_v"], kw["t"])
        dq = time.perf_counter() - t1
        if i >= warmup:
            whole.append(dt * 1e3)
            qap.append(dq * 1e3)
            phases.append((tm["keygen_qap_ms"], tm["keygen_scalars_ms"], tm["keygen_sweeps_ms"], tm["total_ms"]))
    ctx.set_profiling(False)
    for M in dev_m:
        for x in M:
            x.free()
    med = lambda xs: round(statistics.median(xs), 3)
    row = dict(curve=curve, cls=name, m=m, n_v=kw["n_v"], nnz=[int(len(M[1])) for M in kw["matrices"]],
               n_stages=len(kw["stage_ranges"]), reps=reps, warmup=warmup,
               qap_ms=med([p[0] for p in phases]), scalars_ms=med([p[1] for p in phases]),
               sweeps_ms=med([p[2] for p in phases]), keygen_device_ms=med([p[3] for p in phases]),
               keygen_wall_ms=med(whole), qap_eval_wall_ms=med(qap), synthesis_and_matrices_s=round(prep_s, 3))
    log_m = m.bit_length() - 1
    if log_m <= host_max_log_m:
        t1 = time.perf_counter()
        hs = setup_host(make_config(curve, name), curve, SeededRng(SEED))
        row["setup_host_s"] = round(time.perf_counter() - t1, 3)
        ctx.sync()
        t1 = time.perf_counter()
        pk, _ = setup_device(hs, ctx, keep_on_device=True)
        ctx.sync()
        row["setup_device_s"] = round(time.perf_counter() - t1, 3)
        for k in ("a_g", "b_g", "b_h", "h_g"):
            getattr(pk, k).free()
    else:
        row["setup_host_s"] = None                    # capped (--host-max-log-m)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--classes", default=",".join(CLASSES))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max-log-m", type=int, default=17)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keygen_bench.jsonl"))
    a = ap.parse_args()
    rows = []
    for curve in a.curves.split(","):
        with capi.Context(curve, 0) as ctx:
            for name in a.classes.split(","):
                row = bench_class(ctx, curve, name, a.warmup, a.reps, a.host_max_log_m)
                print(json.dumps(row), flush=True)
                rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
