#!/usr/bin/env python3
"""The aggregate verifier (agg_verify.verify_aggregate) and its device call hk_class_power_sums, timed.

verify  per curve and n: a big-merkle job of n tiny synthetic subcircuits in five key classes (one proof per class, repeated
        over the class's members) is aggregated, the key and the proof go through their wire forms, and the wall time of
        verify_aggregate is set beside Tipp.verify alone on the same instance in the same process - Tipp.verify is what
        existed before the verifier, the difference is what the verifier adds (the class sums, z_alpha_beta, com_lr, z_lr,
        two transcript passes).  Median of --reps after --warmup, a host clock around each call.
sums    per curve, n and class count: the wall time of one hk_class_power_sums with class_of (i mod C) and the sums on the
        device, the call ending in its settle.  Before a row is written the sums are compared with the closed form of that
        map: sigma_c = x^c (x^(C m_c) - 1) / (x^C - 1), m_c = the number of i < n with i mod C == c.
One JSON line per row, appended to profiles/agg_verify_bench.jsonl (--out).

    python tools/agg_verify_bench.py [--mode verify,sums] [--curves bn254] [--verify-n 64,1024]
                                     [--sums-n 1024,1048576,134217728] [--classes 5,64]
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

from hekaton_system_amd import agg_verify as av, aggregation as agg, capi, tipa  # noqa: E402
from hekaton_system_amd.chacha import ChaCha12Rng  # noqa: E402
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec, Proof, SeededRng, generate_parameters  # noqa: E402
from hekaton_system_amd.merlin import Transcript as Merlin  # noqa: E402
from hekaton_system_amd.workload import make_config, representative_subcircuit, unique_subcircuits  # noqa: E402

LABEL = b"agg-verify-bench"


def _timed(ctx, fn, warmup, reps):
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(wall), 4), round(min(wall), 4), round(max(wall), 4)


def bench_verify(ctx, curve, n, warmup, reps):
    fc = FrCodec(curve)
    r = fc.r
    rnd = random.Random(n)
    family = "big-merkle"
    made, pub = {}, None
    for rep in unique_subcircuits(family, n):
        circ = make_config(curve, "tiny", rep)
        pk, _td = generate_parameters(circ, curve, SeededRng(bytes([rep % 251 + 1]) * 32), ctx)
        dpk = pk.upload(ctx)
        circ.set_witness_seed(4)
        pub = pub or circ.assignment_ints()[1:4]
        kappa = ChaCha12Rng(bytes([rep % 251 + 2]) * 32).fr(r)
        com = dpk.commit(0, circ.stage0_witness_bytes(), fc.enc1(kappa))
        a, b, c = dpk.prove(circ.full_assignment_bytes(), fc.enc1(rnd.randrange(r)), fc.enc1(rnd.randrange(r)), fc.enc([kappa]),
                            n_v=circ.n_v)
        dpk.free()
        made[rep] = (Proof(a, b, c, [com]), com, pk.vk)
    members = [made[representative_subcircuit(family, n, idx)] for idx in range(n)]
    proofs, coms, vks = ([m[k] for m in members] for k in range(3))
    srs = tipa.setup(ctx, curve, n, rnd.randrange(2, r), rnd.randrange(2, r))
    try:
        apk = agg.AggProvingKey(ctx, curve, srs.ck, vks)
        super_com = apk.com.commit_only_left(srs.ck, np.concatenate(coms))
        tipp_proof, inst = apk.agg_subcircuit_proofs(Merlin(LABEL), super_com, proofs, pub, srs, check=False)
        key_bytes = av.AggVerifyingKey.from_proving_key(apk, tipa.verifier_key(ctx, curve, srs)).serialize()
        proof_bytes = av.AggProof.from_instance(tipp_proof, inst).serialize()
    finally:
        for b in srs.resident.values():
            b.free()
    avk = av.AggVerifyingKey.deserialize(ctx, curve, key_bytes)
    proof = av.AggProof.deserialize(ctx, curve, proof_bytes)
    verdict = av.verify_aggregate(ctx, avk, super_com, pub, proof, Merlin(LABEL))
    assert verdict, verdict
    T = tipa.Tipp(ctx, curve)
    assert T.verify(avk.tipp_vk, inst["commitment"], inst["output"], inst["twist"], proof.tipp)
    row = dict(mode="verify", curve=curve, n=n, classes=len(avk.alpha_beta), reps=reps, warmup=warmup,
               key_bytes=len(key_bytes), proof_bytes=len(proof_bytes))
    for key, call in (("verify_aggregate", lambda: av.verify_aggregate(ctx, avk, super_com, pub, proof, Merlin(LABEL))),
                      ("tipp_verify", lambda: T.verify(avk.tipp_vk, inst["commitment"], inst["output"], inst["twist"], proof.tipp)),
                      ("class_power_sums", lambda: ctx.class_power_sums(inst["twist"], avk.class_of, len(avk.alpha_beta)))):
        med, lo, hi = _timed(ctx, call, warmup, reps)
        row.update({key + "_wall_ms": med, key + "_wall_ms_min": lo, key + "_wall_ms_max": hi})
    row["added_ms"] = round(row["verify_aggregate_wall_ms"] - row["tipp_verify_wall_ms"], 4)
    T.pool.shutdown()
    return row


def closed_form_sums(x, n, C, r):
    """The class sums of the map i mod C."""
    xc = pow(x, C, r)
    inv = pow(xc - 1, -1, r)
    out = []
    for c in range(C):
        m = (n - c + C - 1) // C if n > c else 0
        out.append(pow(x, c, r) * (pow(xc, m, r) - 1) * inv % r)
    return out


def bench_sums(ctx, curve, n, C, warmup, reps):
    fc = FrCodec(curve)
    r = fc.r
    x = random.Random(n + C).randrange(2, r)
    cls = capi.DeviceBuffer.from_host(ctx, (np.arange(n, dtype=np.uint32) % np.uint32(C)).astype(np.uint32))
    out = capi.DeviceBuffer(ctx, C * ctx.fr_bytes)
    try:
        ctx.class_power_sums(x, cls, C, out=out)
        assert fc.dec(out.to_host()) == closed_form_sums(x, n, C, r), "the sums differ from the closed form"
        med, lo, hi = _timed(ctx, lambda: ctx.class_power_sums(x, cls, C, out=out), warmup, reps)
    finally:
        cls.free()
        out.free()
    return dict(mode="sums", curve=curve, n=n, classes=C, reps=reps, warmup=warmup, wall_ms=med, wall_ms_min=lo, wall_ms_max=hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="verify,sums")
    ap.add_argument("--curves", default="bn254")
    ap.add_argument("--verify-n", default="64,1024")
    ap.add_argument("--sums-n", default="1024,1048576,134217728")
    ap.add_argument("--classes", default="5,64")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agg_verify_bench.jsonl"))
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",") if v]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(row):
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")
    modes = a.mode.split(",")
    for curve in a.curves.split(","):
        with capi.Context(curve, 0) as ctx:
            if "sums" in modes:
                for n in ints(a.sums_n):
                    for C in ints(a.classes):
                        emit(bench_sums(ctx, curve, n, C, a.warmup, a.reps))
            if "verify" in modes:
                for n in ints(a.verify_n):
                    emit(bench_verify(ctx, curve, n, a.warmup, a.reps))


if __name__ == "__main__":
    main()
