#!/usr/bin/env python3
"""GT membership (hk_gt_check) and what it changes for the aggregate's verifier, timed.

kernel    per curve and n = 1, 64, 1024: one hk_gt_check beside one hk_fq12_pow with exponent r - 1 (the plain chain, the only
          membership test there was: x^(r - 1) x == 1) on n distinct members of GT resident on the device; both verdicts
          are checked before a row is written.
verifier  per curve, on the tiny job of tests/test_agg_verify_gpu.py: verify_aggregate with members_in_gt False and True;
          AggProof.deserialize and AggVerifyingKey.deserialize without a context, with the GT check stubbed out, and as
          they are.
Two warm-ups, then seven batches with the variants alternating; per call: median, min, max of the batches in ms.  One JSON
line per row, printed and written to profiles/gt_check_bench.jsonl (argv[1] names another file).

    python tools/gt_check_bench.py [out.jsonl]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hekaton_system_amd import agg_verify as av, capi  # noqa: E402
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec  # noqa: E402
from hekaton_system_amd.gt import GtField  # noqa: E402
from hekaton_system_amd.merlin import Transcript as Merlin  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gt_check_bench.jsonl")
lines = []


def timed(fns, reps, batches=7, warm=2):
    """fns: dict name -> callable; alternated; per-call ms: median (min - max) over batches of `reps` calls."""
    for _ in range(warm):
        for f in fns.values():
            f()
    res = {k: [] for k in fns}
    for _ in range(batches):
        for k, f in fns.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            res[k].append((time.perf_counter() - t0) * 1e3 / reps)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


def emit(**kw):
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def kernels(cname):
    ctx = capi.Context(cname, 0)
    F, fc, r = GtField(cname), FrCodec(cname), CURVE_PARAMS[cname]["r"]
    # a member of GT without the oracle: g = f^((q^12 - 1) / r) for a seeded f, on the host; the n inputs are powers of it
    import random
    rnd = random.Random(3)
    f = tuple(rnd.randrange(F.q) for _ in range(12))
    g = F.pow(f, (F.q ** 12 - 1) // r)
    assert F.in_gt(g) and g != F.one
    for n in (1, 64, 1024):
        exps = [rnd.randrange(1, r) for _ in range(n)]
        bases = ctx.gt_pow(np.tile(np.frombuffer(F.encode(g), np.uint8), n), fc.enc(exps))     # n distinct members
        dev_in = capi.DeviceBuffer.from_host(ctx, bases.reshape(-1))
        dev_e = capi.DeviceBuffer.from_host(ctx, fc.enc([r - 1] * n))
        want = ctx.gt_check(dev_in, n=n)
        assert want.all()
        pw = ctx.gt_pow(dev_in, dev_e, in_gt=False)                                             # x^(r - 1) = x^-1
        assert F.mul(F.decode(pw[0]), F.decode(bases[0])) == F.one
        reps = 20 if n < 1024 else 5
        t = timed({"gt_check": lambda: ctx.gt_check(dev_in, n=n),
                   "fq12_pow_r_minus_1": lambda: ctx.gt_pow(dev_in, dev_e, in_gt=False)}, reps)
        emit(what="kernel", curve=cname, n=n, reps=reps, ms={k: [round(x, 4) for x in v] for k, v in t.items()})
        dev_in.free()
        dev_e.free()
    ctx.close()


def verifier(cname):
    from tests.test_agg_verify_gpu import LABEL, _tiny_job
    ctx = capi.Context(cname, 0)
    j = _tiny_job(ctx, cname)
    avk = av.AggVerifyingKey.deserialize(ctx, cname, j.key_bytes)
    proof = av.AggProof.deserialize(ctx, cname, j.proof_bytes)

    def run(fast):
        v = av.verify_aggregate(ctx, avk, j.super_com, j.pub, proof, Merlin(LABEL), members_in_gt=fast)
        assert v.ok
    t = timed({"plain": lambda: run(False), "members_in_gt": lambda: run(True)}, 3)
    emit(what="verify_aggregate", curve=cname, n=j.n, ms={k: [round(x, 3) for x in v] for k, v in t.items()})
    real = av._check_gt

    def read(mode):
        av._check_gt = real if mode == "gt" else (lambda *a: None)
        try:
            av.AggProof.deserialize(None if mode == "none" else ctx, cname, j.proof_bytes)
        finally:
            av._check_gt = real
    t = timed({"no_ctx": lambda: read("none"), "points_only": lambda: read("points"), "points_and_gt": lambda: read("gt")}, 3)
    emit(what="AggProof.deserialize", curve=cname, n=j.n, gt_members=5 + 16 + 6 * (j.n.bit_length() - 1),
         ms={k: [round(x, 3) for x in v] for k, v in t.items()})

    def read_key(mode):
        av._check_gt = real if mode == "gt" else (lambda *a: None)
        try:
            av.AggVerifyingKey.deserialize(ctx, cname, j.key_bytes)
        finally:
            av._check_gt = real
    t = timed({"points_only": lambda: read_key("points"), "points_and_gt": lambda: read_key("gt")}, 3)
    emit(what="AggVerifyingKey.deserialize", curve=cname, ms={k: [round(x, 3) for x in v] for k, v in t.items()})
    for rb in j.srs.resident.values():
        rb.free()
    ctx.close()


if __name__ == "__main__":
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    for cname in ("bn254", "bls12_381"):
        kernels(cname)
    for cname in ("bn254", "bls12_381"):
        verifier(cname)
    with open(OUT, "w") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")
    print("bench done")
