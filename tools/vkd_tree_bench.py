#!/usr/bin/env python3
"""A VKD batch applied to the directory on the device (hk_vkd_tree) beside the host mirror (`vkd_circuit.directory_paths`).

Per curve and number of updates U, at --depth (128: the reference's), a directory of M = 1 leaf (the genesis user) and the
batch of `VkdJob.random`: one append, then U - 1 updates of that user, in the same run:

  device   everything resident (both leaf tables, the Poseidon constants, the three outputs), then hk_vkd_tree: wall time,
           median of --reps after --warmup, the context synchronised before each
  host     `directory_paths` - one `lookup_path` and one `insert` of `depth` Poseidon hashes per update, in Python - once,
           over the first --host-updates updates of the batch (all of them by default); the building of the empty-subtree
           table is part of it

The device siblings of those updates (a path depends on the updates before it only), the status bytes and - when the host ran
the whole batch - the roots are compared with the host's byte for byte before a line is written.  One JSON line per batch,
appended to profiles/vkd_tree_bench.jsonl (--out).

    python tools/vkd_tree_bench.py [--curves bn254,bls12_381] [--updates 31,2047] [--host-updates N]
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
from hekaton_system_amd.vkd_circuit import Append, Update, concat, directory_paths, leaves_table  # noqa: E402


def _median_ms(ctx, fn, warmup, reps):
    wall = []
    for i in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(wall), 3)


def batch(n_updates):
    """`VkdJob.random`'s batch without its paths: an append of user [8; 32], then updates of that user."""
    username, key, counter = bytes([8]) * 32, bytes(32), 0
    changes = [Append(username, key)]
    for i in range(n_updates - 1):
        key2 = bytes([i % 256]) * 32
        changes.append(Update(username, counter, key, key2))
        counter, key = counter + 1, key2
    return changes


def bench_batch(ctx, curve, n_updates, depth, warmup, reps, host_updates):
    fc, fr = FrCodec(curve), ctx.fr_bytes
    leaves0, changes = [concat(bytes(32), bytes(32), 0)], batch(n_updates)
    n_host = n_updates if host_updates is None else min(host_updates, n_updates)
    t0 = time.perf_counter()
    initial, final, paths, status = directory_paths(curve, depth, leaves0, changes[:n_host])
    host_ms = (time.perf_counter() - t0) * 1e3
    consts, n_consts, ld, nd = device_params(curve, fc)
    dev = [capi.DeviceBuffer.from_host(ctx, np.ascontiguousarray(x).reshape(-1).view(np.uint8))
           for x in (np.frombuffer(b"".join(leaves0), np.uint8), leaves_table(changes), consts)]
    outs = (capi.DeviceBuffer(ctx, n_updates * depth * fr), capi.DeviceBuffer(ctx, 2 * fr), capi.DeviceBuffer(ctx, n_updates))
    kinds = [u.kind for u in changes]
    ms = _median_ms(ctx, lambda: ctx.vkd_tree(depth, dev[0], kinds, dev[1], (dev[2], n_consts, ld, nd), out=outs), warmup, reps)
    want = fc.enc([x for p in paths for x in p])
    assert (outs[0].to_host()[:want.size] == want).all(), "hk_vkd_tree's siblings differ from the host mirror's"
    assert outs[2].to_host()[:n_host].tobytes() == bytes(status), "hk_vkd_tree's status differs from the host mirror's"
    roots = fc.dec(outs[1].to_host())
    assert roots[0] == initial and (n_host < n_updates or roots[1] == final), "hk_vkd_tree's roots differ from the host mirror's"
    for x in outs + tuple(dev):
        x.free()
    return dict(curve=curve, depth=depth, n_leaves0=1, updates=n_updates, reps=reps, warmup=warmup, vkd_tree_wall_ms=ms,
                host_updates=n_host, host_mirror_ms=round(host_ms, 1), host_ms_per_update=round(host_ms / n_host, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--updates", default="31,2047")
    ap.add_argument("--depth", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-updates", type=int, default=None, help="run the host mirror over the first N updates only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vkd_tree_bench.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for curve in a.curves.split(","):
        with capi.Context(curve, 0) as ctx:
            for u in a.updates.split(","):
                row = bench_batch(ctx, curve, int(u), a.depth, a.warmup, a.reps, a.host_updates)
                print(json.dumps(row), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
