#!/usr/bin/env python3
"""The aggregator's scalar vectors on the device (hk_scalar_powers, hk_ipa_quotient) against the Python loops they replace.

calls   per curve and n: the wall time of one hk_scalar_powers(n) and of one hk_ipa_quotient at l = log2 n with shift 0 (q_v)
        and shift n (q_w), outputs left on the device (median of --reps after --warmup, a host clock around a call that
        ends in its settle), and beside each the host path for the same inputs on the same box, run once: the power loop or
        ipa_polynomial_coeffs + _divide_by_linear, then enc_canon.  The device bytes are compared with the host's before a
        row is written.
prove   Tipp.prove's phase_times (set-up, rounds, openings) on random curve points at each --prove-n: HK_AGG_HOST_SCALARS=1
        and the default alternate in one process, --reps times each after a warm-up pair; medians and min / max per phase.
One JSON line per row, appended to profiles/agg_scalars_bench.jsonl (--out).

    python tools/agg_scalars_bench.py [--mode calls,prove] [--curves bn254,bls12_381] [--sizes 64,1024,16384,65536]
                                      [--prove-n 64,1024] [--prove-curves bn254]
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

from hekaton_system_amd import capi, tipa  # noqa: E402
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec  # noqa: E402


def _timed(ctx, fn, warmup, reps):
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(wall), 4), round(min(wall), 4), round(max(wall), 4)


def bench_calls(ctx, curve, n, warmup, reps):
    fc = FrCodec(curve)
    r = fc.r
    rnd = random.Random(n)
    l = n.bit_length() - 1
    x, rho, z = (rnd.randrange(2, r) for _ in range(3))
    ch = [rnd.randrange(1, r) for _ in range(l)]
    buf = capi.DeviceBuffer(ctx, 2 * n * ctx.fr_bytes)
    row = dict(mode="calls", curve=curve, n=n, reps=reps, warmup=warmup)
    # host paths, once each
    t0 = time.perf_counter()
    pw = [fc.R % r] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * x % r
    host_pw = fc.enc_canon(pw)
    t1 = time.perf_counter()
    host_qv = fc.enc_canon(tipa._divide_by_linear(tipa.ipa_polynomial_coeffs(ch, 1, r, fc.R), z, r))
    t2 = time.perf_counter()
    host_qw = fc.enc_canon(tipa._divide_by_linear([0] * n + tipa.ipa_polynomial_coeffs(ch, rho, r, fc.R), z, r))
    t3 = time.perf_counter()
    row.update(host_powers_ms=round((t1 - t0) * 1e3, 3), host_quotient_shift0_ms=round((t2 - t1) * 1e3, 3),
               host_quotient_shiftn_ms=round((t3 - t2) * 1e3, 3))
    for key, want, nfr, call in (
            ("powers", host_pw, n, lambda o: ctx.scalar_powers(x, n, 1, out=o)),
            ("quotient_shift0", host_qv, n, lambda o: ctx.ipa_quotient(ch, 1, z, 0, out=o)),
            ("quotient_shiftn", host_qw, 2 * n, lambda o: ctx.ipa_quotient(ch, rho, z, n, out=o))):
        out = buf.view(0, nfr * ctx.fr_bytes)
        call(out)
        assert out.to_host().tobytes() == want.tobytes(), key + " differs from the host path"
        med, lo, hi = _timed(ctx, lambda: call(out), warmup, reps)
        row.update({key + "_wall_ms": med, key + "_wall_ms_min": lo, key + "_wall_ms_max": hi})
        row[key + "_device_faster"] = med < row["host_" + key + "_ms"]
    buf.free()
    return row


def bench_prove(ctx, curve, n, reps):
    fc = FrCodec(curve)
    p = CURVE_PARAMS[curve]
    r = p["r"]
    rnd = random.Random(7 * n)
    alpha, beta, twist = (rnd.randrange(2, r) for _ in range(3))
    srs = tipa.setup(ctx, curve, n, alpha, beta)
    A = np.asarray(ctx.fixed_base(1, fc.g1(p["g1"]), fc.enc([rnd.randrange(1, r) for _ in range(n)])))
    B = np.asarray(ctx.fixed_base(2, fc.g2(p["g2"]), fc.enc([rnd.randrange(1, r) for _ in range(n)])))
    T = tipa.Tipp(ctx, curve)
    com = T.com.commit_with_ip(srs.ck, A, B)
    z_ab = T.F.decode(ctx.multi_pairing(A, ctx.scalar_pairing(2, B, fc.enc([pow(twist, i, r) for i in range(n)]), n), n))
    phases = {"host": [], "device": []}
    proofs = {}
    for i in range(1 + reps):                                              # a warm-up pair, then alternating
        for path in ("host", "device"):
            if path == "host":
                os.environ["HK_AGG_HOST_SCALARS"] = "1"
            else:
                os.environ.pop("HK_AGG_HOST_SCALARS", None)
            ctx.sync()
            t0 = time.perf_counter()
            proofs[path] = T.prove(srs, A, B, twist, com, z_ab)
            total = time.perf_counter() - t0
            if i:
                phases[path].append(tuple(x * 1e3 for x in T.phase_times) + (total * 1e3,))
    os.environ.pop("HK_AGG_HOST_SCALARS", None)
    assert proofs["host"]["rounds"] == proofs["device"]["rounds"]
    for k in ("open_v", "open_w"):
        assert np.array_equal(np.asarray(proofs["host"][k]), np.asarray(proofs["device"][k])), k
    assert T.verify(tipa.verifier_key(ctx, curve, srs), com, z_ab, twist, proofs["device"])
    for b in srs.resident.values():
        b.free()
    T.pool.shutdown()
    row = dict(mode="prove", curve=curve, n=n, reps=reps)
    for path, rows in phases.items():
        for j, name in enumerate(("setup", "rounds", "openings", "total")):
            col = [x[j] for x in rows]
            row["%s_%s_ms" % (path, name)] = round(statistics.median(col), 3)
            row["%s_%s_ms_min_max" % (path, name)] = [round(min(col), 3), round(max(col), 3)]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="calls,prove")
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--sizes", default="64,1024,16384,65536")
    ap.add_argument("--prove-n", default="64,1024")
    ap.add_argument("--prove-curves", default="bn254")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agg_scalars_bench.jsonl"))
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",") if x]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(row):
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")
    modes = a.mode.split(",")
    for curve in a.curves.split(","):
        with capi.Context(curve, 0) as ctx:
            if "calls" in modes:
                for n in ints(a.sizes):
                    emit(bench_calls(ctx, curve, n, a.warmup, a.reps))
            if "prove" in modes and curve in a.prove_curves.split(","):
                for n in ints(a.prove_n):
                    emit(bench_prove(ctx, curve, n, a.reps))


if __name__ == "__main__":
    main()
