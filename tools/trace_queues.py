#!/usr/bin/env python3
"""Hardware-queue view of a rocprofv3 --kernel-trace CSV of bench.py: how prove_batch's chunks use the queues.

    rocprofv3 --kernel-trace --output-format csv -- python3 bench.py --steps 2 --warmup 1
    python tools/trace_queues.py <kernel_trace.csv> [--warmup 1] [--json out.json]

A chunk is the kernels one host thread submits from a k_prep_ext to the chunk's last finish kernel (k_finish, or
k_finish_c once the finish is split), in the order of the host calls (Correlation_Id).  Each kernel gets the role
prove_batch submits it for: main
(k_prep_ext, the z digit sort, A, the finish kernels), H (witness map, H sort, H), B1 (with a compact B query also the
gather and sort of its scalars), B2 (G2) and L.  Per chunk the tool records which Queue_Id each role ran on, and the time
from the end of the H role's last kernel to the end of the chunk.  The chunks between two steps' stage-0 commitments form
one proving round (one bench step); per round it reports:
  - proofs, wall time, ms per proof;
  - how many distinct queues a chunk's kernels used, and which roles of one chunk shared a queue (share of chunks);
  - the share of the round with no throughput kernel (accum0, NTT, digit sort, spmv, pointwise product) in flight;
  - the post-H tail of its chunks (median, mean, 90th percentile).
The first --warmup full rounds are the bench's warm-up steps and are left out of the summary.
"""
import argparse
import bisect
import collections
import csv
import json
import re
import statistics
import sys

ROLES = ("main", "B1", "B2", "L", "H")
BIG = ("k_msm_accum0", "k_ntt_pass4", "k_msm_hist", "k_msm_scatter", "k_spmv", "k_mul_pointwise")
FINISH_LAST = ("k_finish", "k_finish_c")


def base_name(name):
    m = re.match(r"(?:void )?hk::(\w+)(<.*)?", name)
    return m.group(1) if m else name


def is_g2(name):
    return "Fp2<" in name.split("(")[0]


def load(path):
    rows = list(csv.DictReader(open(path)))
    if not rows:
        sys.exit("empty trace")
    order = "Correlation_Id" if "Correlation_Id" in rows[0] else "Dispatch_Id"      # the host call's order
    ks = []
    for r in rows:
        name = r["Kernel_Name"]
        ks.append({"name": name, "base": base_name(name), "g2": is_g2(name), "t0": int(r["Start_Timestamp"]),
                   "t1": int(r["End_Timestamp"]), "queue": r.get("Queue_Id"), "stream": r.get("Stream_Id"),
                   "thread": r.get("Thread_Id"), "order": int(r[order]), "gy": int(r.get("Grid_Size_Y") or 1)})
    return ks


def chunks_of(ks):
    """Split each thread's dispatches into chunks and give every kernel of a chunk its role."""
    by_thread = collections.defaultdict(list)
    for k in ks:
        by_thread[k["thread"]].append(k)
    out, bad = [], 0
    for seq in by_thread.values():
        seq.sort(key=lambda k: k["order"])
        cur = None
        for k in seq:
            b = k["base"]
            if b == "k_prep_ext":
                if cur is not None:
                    bad += 1
                cur = {"kernels": [(k, "main")], "state": "start", "proofs": 0, "h_last": False}
                continue
            if cur is None:
                continue
            st = cur["state"]
            if st == "start":
                # the H chain (witness map first) is submitted before the queries, or after k_finish_ab
                cur["h_last"] = b == "k_msm_hist"
                st = cur["state"] = "zsort" if cur["h_last"] else "H"
            if st == "H":
                role = "H"
                if b == "k_msm_reduce_fused" and not k["g2"]:
                    cur["state"] = "zsort"
            elif st == "fin" and cur["h_last"] and b not in ("k_finish", "k_finish_ab", "k_finish_c"):
                role = "H"
            elif st == "zsort":
                role = "main"
                if b == "k_msm_scatter":
                    cur["state"] = "after_z"
            elif st in ("after_z", "bsort") and (b == "k_gather" or st == "bsort"):
                role = "B1"                      # a compact B query: its own gather and digit sort
                cur["state"] = "B2" if b == "k_msm_scatter" else "bsort"
            else:
                if st == "after_z":
                    st = cur["state"] = "B2"
                role = {"B2": "B2", "B1": "B1", "L": "L", "A": "main", "fin": "main"}[st]
                if b == "k_msm_reduce_fused":
                    cur["state"] = {"B2": "B1", "B1": "L", "L": "A", "A": "fin"}.get(st, st)
                if b in ("k_finish", "k_finish_ab"):
                    cur["proofs"] = k["gy"]
            cur["kernels"].append((k, role))
            if b in FINISH_LAST:
                if cur["state"] == "fin" and cur["proofs"]:
                    out.append(cur)
                else:
                    bad += 1
                cur = None
    for c in out:
        ker = c["kernels"]
        c["t0"] = min(k["t0"] for k, _ in ker)
        c["t1"] = max(k["t1"] for k, _ in ker)
        c["h_end"] = max(k["t1"] for k, r in ker if r == "H")
        c["queues"] = {r: sorted({k["queue"] for k, rr in ker if rr == r}) for r in ROLES}
        c["streams"] = {r: sorted({k["stream"] for k, rr in ker if rr == r}) for r in ROLES}
    return sorted(out, key=lambda c: c["t0"]), bad


def rounds_of(ks, chunks):
    """Group the chunks by bench step: every step opens with its stage-0 commitments (hk_commit_batch, whose
    k_points_mul_split launches run before any proof of the step), so the chunks between two such launches form a step's
    proving round."""
    marks = sorted(k["t0"] for k in ks if k["base"] == "k_points_mul_split")
    rounds = collections.OrderedDict()
    for c in chunks:
        rounds.setdefault(bisect.bisect_left(marks, c["t0"]), []).append(c)
    return [{"chunks": ch, "t0": min(c["t0"] for c in ch), "t1": max(c["t1"] for c in ch)} for ch in rounds.values()]


def idle_share(ks, t0, t1):
    """share of [t0, t1] with no throughput kernel in flight"""
    iv = sorted((max(k["t0"], t0), min(k["t1"], t1)) for k in ks
                if k["base"] in BIG and k["t1"] > t0 and k["t0"] < t1)
    busy, cs, ce = 0, None, None
    for s, e in iv:
        if cs is None or s > ce:
            if cs is not None:
                busy += ce - cs
            cs, ce = s, e
        else:
            ce = max(ce, e)
    if cs is not None:
        busy += ce - cs
    return 1.0 - busy / (t1 - t0) if t1 > t0 else 0.0


def shared_pairs(c):
    pairs = []
    for i, a in enumerate(ROLES):
        for b in ROLES[i + 1:]:
            if set(c["queues"][a]) & set(c["queues"][b]):
                pairs.append(a + "+" + b)
    return pairs


def summarise(ks, rnd):
    ch = rnd["chunks"]
    n = sum(c["proofs"] for c in ch)
    wall = (rnd["t1"] - rnd["t0"]) / 1e6
    tails = [(c["t1"] - c["h_end"]) / 1e6 for c in ch]
    nq = collections.Counter(len(set(q for r in ROLES for q in c["queues"][r])) for c in ch)
    pairs = collections.Counter(p for c in ch for p in shared_pairs(c))
    return {
        "proofs": n, "chunks": len(ch), "proofs_per_chunk": round(n / len(ch), 2), "wall_ms": round(wall, 2),
        "ms_per_proof": round(wall / n, 3),
        "queues_per_chunk": {str(k): v for k, v in sorted(nq.items())},
        "roles_sharing_a_queue_share_of_chunks": {p: round(v / len(ch), 2) for p, v in pairs.most_common()},
        "no_throughput_kernel_share": round(idle_share(ks, rnd["t0"], rnd["t1"]), 4),
        "post_h_tail_ms": {"median": round(statistics.median(tails), 3), "mean": round(statistics.mean(tails), 3),
                           "p90": round(sorted(tails)[int(0.9 * (len(tails) - 1))], 3)},
        "chunk_latency_ms_mean": round(statistics.mean((c["t1"] - c["t0"]) / 1e6 for c in ch), 3),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace")
    ap.add_argument("--warmup", type=int, default=1, help="full rounds to leave out (bench.py --warmup)")
    ap.add_argument("--json", default=None, help="also write the summary here")
    a = ap.parse_args()
    ks = load(a.trace)
    chunks, bad = chunks_of(ks)
    if not chunks:
        sys.exit("no prove_batch chunk found in the trace")
    rounds = rounds_of(ks, chunks)
    full = max(sum(c["proofs"] for c in r["chunks"]) for r in rounds)
    # the bench's steps (the post-timing single proofs form rounds of their own); a chunk the parser could not follow
    # leaves its step a few proofs short
    steps = [r for r in rounds if 2 * sum(c["proofs"] for c in r["chunks"]) >= full][a.warmup:]
    # which queues each role used over the timed steps (a role of a prove lane should keep one queue)
    roles_q = {r: collections.Counter(q for s in steps for c in s["chunks"] for q in c["queues"][r]) for r in ROLES}
    out = {"trace": a.trace, "chunks_parsed": len(chunks), "chunks_unparsed": bad, "rounds": len(rounds),
           "proofs_per_step": full, "timed_steps": [summarise(ks, s) for s in steps],
           "queue_ids_per_role_timed": {r: dict(v) for r, v in roles_q.items()},
           "distinct_queue_ids_timed": sorted({q for v in roles_q.values() for q in v})}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.json:
        open(a.json, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
