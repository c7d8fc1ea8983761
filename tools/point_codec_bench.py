#!/usr/bin/env python3
"""Reading compressed points on the device (hk_points_decompress_*) against reading the same points uncompressed.

Per curve, group and n, outputs left on the device, median of --reps after --warmup (a host clock around calls that end
in their settle):
  decompress_ms        one hk_points_decompress call, x and flags on the host (the file's bytes), check = 0
  decompress_dev_ms    the same call with x and flags already on the device: the kernel and its launch
  checked_dev_ms       ... with check = 1 (ark's checked deserialize_compressed)
  uncompressed_ms      what the uncompressed file costs today: the H2D copy of twice the bytes + hk_field_convert in place
  mirror_ms            n = 2^10 only, once: the Python mirror (ArkCodec._decompress) on the same x
G1 rows also carry the Fq products per second the kernel time implies at PRODUCTS[curve] products per point (the weight of
the exponent (q - 3) / 4) and, on BN254, that rate as a fraction of the measured product ceiling.
The points are k G for random k (hk_fixed_base), compressed on the device; the decompressed bytes are compared with them
before a row is written.  One JSON line per row, appended to profiles/point_codec_bench.jsonl (--out).

    python tools/point_codec_bench.py [--curves bn254,bls12_381] [--groups 1,2] [--sizes 1024,65536,1048576]
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
from hekaton_system_amd.ark_serialize import ArkCodec  # noqa: E402
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec  # noqa: E402

PRODUCTS = {"bn254": 360, "bls12_381": 610}       # Fq products of one G1 decompression, from the exponent's weight
CEILING_BN254 = 134e9                             # Fq products / s, DESIGN.md (ubench)


def _timed(ctx, fn, warmup, reps):
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(wall), 4)


def bench(ctx, curve, group, n, warmup, reps):
    lib, h = ctx.lib, ctx.handle
    fc = FrCodec(curve)
    p = CURVE_PARAMS[curve]
    rng = np.random.default_rng(n + group)
    pb = ctx.g1_bytes if group == 1 else ctx.g2_bytes
    xb = pb // 2
    scalars = rng.integers(0, 256, size=(n, ctx.fr_bytes), dtype=np.uint8)
    scalars[:, -1] &= 0x0F                                            # canonical, below r on both curves
    gen = fc.g1(p["g1"]) if group == 1 else fc.g2(p["g2"])
    pts = ctx.fixed_base(group, gen, scalars.reshape(-1), n=n, montgomery=False)
    x, flags = ctx.points_compress(group, pts)
    out = capi.DeviceBuffer(ctx, n * pb)
    status = capi.DeviceBuffer(ctx, n)
    dx, df = capi.DeviceBuffer.from_host(ctx, x), capi.DeviceBuffer.from_host(ctx, flags)
    dec = lib.hk_points_decompress_g1 if group == 1 else lib.hk_points_decompress_g2

    def run(xs, fl, check):
        capi.check(dec(h, capi.ptr(xs), capi.ptr(fl), n, check, capi.ptr(out), capi.ptr(status)), "hk_points_decompress")
    row = dict(curve=curve, group=group, n=n, reps=reps, warmup=warmup)
    row["decompress_ms"] = _timed(ctx, lambda: run(x, flags, 0), warmup, reps)
    assert out.to_host().tobytes() == pts.tobytes() and (status.to_host() == 1).all()
    row["decompress_dev_ms"] = _timed(ctx, lambda: run(dx, df, 0), warmup, reps)
    row["checked_dev_ms"] = _timed(ctx, lambda: run(dx, df, 1), warmup, reps)
    assert (status.to_host() == 1).all()
    canon = ctx.field_convert(1, pts, False)                          # the uncompressed file's coordinates

    def uncompressed():
        capi.check(lib.hk_dev_upload(h, out.ptr, canon.ctypes.data, canon.nbytes), "hk_dev_upload")
        capi.check(lib.hk_field_convert(h, 1, out.ptr, out.ptr, canon.nbytes // ctx.fq_bytes, 1), "hk_field_convert")
    row["uncompressed_ms"] = _timed(ctx, uncompressed, warmup, reps)
    assert out.to_host().tobytes() == pts.tobytes()
    if n <= 1024:
        cd = ArkCodec(curve)
        xs = np.asarray(x).reshape(n, group, ctx.fq_bytes)
        t0 = time.perf_counter()
        got = cd._decompress(group, xs, np.zeros(n, bool), (flags & 2) != 0)
        row["mirror_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        assert got.tobytes() == canon.tobytes()
    if group == 1:
        rate = n * PRODUCTS[curve] / (row["decompress_dev_ms"] * 1e-3)
        row["fq_products_per_s"] = float("%.4g" % rate)
        if curve == "bn254":
            row["fraction_of_ceiling"] = round(rate / CEILING_BN254, 3)
    for b in (out, status, dx, df):
        b.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--groups", default="1,2")
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_codec_bench.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as f:
        for curve in a.curves.split(","):
            with capi.Context(curve, 0) as ctx:
                for group in (int(g) for g in a.groups.split(",")):
                    for n in (int(s) for s in a.sizes.split(",")):
                        row = bench(ctx, curve, group, n, a.warmup, a.reps)
                        print(json.dumps(row), flush=True)
                        f.write(json.dumps(row) + "\n")
                        f.flush()


if __name__ == "__main__":
    main()
