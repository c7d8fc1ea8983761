#!/usr/bin/env python3
"""Generates tests/golden/portal_layout.json: the column layout, the matrices and the host witnesses of the four portal jobs
(big-merkle, VM, partitioned R1CS, VKD), pinned as attribute values and SHA-256 digests.

hk_stage1_witness and hk_ram_stage1_witness write the portal and membership columns by position, so the column order of those
blocks is a contract with csrc/stage1.cuh and csrc/ram_witness.cuh.  This record is what holds a change of the Python side
to it: tests/test_portal_layout_cpu.py recomputes `record()` and compares it with the committed file entry by entry.

    python tests/golden/gen_portal_layout.py        # rewrites portal_layout.json next to this script

Per curve and job: every proving-key class (the attributes below that it has, a digest of `csr(fc)`, for the big-merkle classes
a digest of `tape.word_program(n_v)`) and every subcircuit (digests of `job.assignment_bytes(idx)` and `job.stage0_ints(idx)`).
The big-merkle job is (4, 1, 3): a parent reads two portals and sets one, so `ShaMerkleJob` takes no fewer than 3; the four
kinds are recorded once more as lone classes at n_portals = 2, depth = 2.
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from hekaton_system_amd.sha_circuit import ShaMerkleJob, ShaMerkleSubcircuit      # noqa: E402
from tests import r1cs_job_fixtures, vkd_fixtures, vm_cases                         # noqa: E402

CURVES = ("bn254", "bls12_381")
SHA_CHAL = (0x1234567, 0x7654321)
OUT = os.path.join(HERE, "portal_layout.json")
# plain values, recorded as they are
ATTRS = ("np_", "n0", "n_c", "n_wit", "n_v", "N_INST", "pos_col0", "pos_cols", "col0", "body_col0", "dummy_col0",
         "sha_root_col", "device_cols", "blocks", "cols", "pair_rows")


def _sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, (bytes, bytearray)) else memoryview(p).cast("B"))
    return h.hexdigest()


def _plain(v):
    """tuples -> lists, numpy ints -> ints: what json.load gives back."""
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return int(v)


def class_record(circ, word_program=False):
    out = {a: _plain(getattr(circ, a)) for a in ATTRS if hasattr(circ, a)}
    # the object-valued attributes: what identifies them
    out["tape"] = {"n_inst": circ.tape.n_inst, "n_rows": circ.tape.n_rows, "n_wit": circ.tape.n_wit}
    out["fc"] = {"nb": int(circ.fc.nb), "r_is_curve": circ.fc.r == circ.r}
    for name in ("leaf_cfg", "node_cfg"):
        cfg = getattr(circ, name)
        out[name] = {"p_is_r": cfg.p == circ.r, "t": cfg.t, "rate": cfg.rate, "alpha": cfg.alpha, "rf": cfg.rf, "rp": cfg.rp}
    out["csr"] = _sha(*[np_arr for m in circ.csr(circ.fc) for np_arr in (m[0], m[1], m[2])])
    if word_program:
        out["word_program"] = _sha(*circ.tape.word_program(circ.n_v))
    return out


def job_record(job, word_program=False):
    classes, subs = {}, []
    for idx in range(job.n):
        key = repr(job.class_of(idx))
        if key not in classes:
            classes[key] = class_record(job.make_class(idx), word_program)
        subs.append({"class": key, "assignment": _sha(job.assignment_bytes(idx).tobytes()),
                     "stage0": _sha(repr([int(x) for x in job.stage0_ints(idx)]).encode())})
    return {"classes": classes, "subcircuits": subs}


class _ShaJob:
    """`ShaMerkleJob` under the interface the other three jobs share (it has no `assignment_bytes(idx)` of its own)."""

    def __init__(self, job):
        self.job, self.n, self.class_of, self.stage0_ints = job, job.n, job.class_of, job.stage0_ints
        self._classes = {}

    def make_class(self, idx):
        key = self.job.class_of(idx)
        if key not in self._classes:
            self._classes[key] = self.job.make_class(idx)
        return self._classes[key]

    def assignment_bytes(self, idx):
        return self.make_class(idx).assignment_bytes(self.job.inputs(idx))[0]


def curve_record(curve):
    rnd = random.Random(0x504F5254)
    leaves = [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(2)]
    jobs = {"big-merkle": job_record(_ShaJob(ShaMerkleJob(curve, 4, 1, 3, leaves, *SHA_CHAL)), word_program=True)}
    jobs["big-merkle kinds"] = {"classes": {
        kind: class_record(ShaMerkleSubcircuit(curve, kind, 1, 2, depth=2), word_program=True)
        for kind in ("leaf", "parent", "root", "padding")}, "subcircuits": []}
    jobs["vm"] = job_record(vm_cases.vm_job(curve, 2, 1))
    for name in r1cs_job_fixtures.JOBS:
        jobs["r1cs " + name] = job_record(r1cs_job_fixtures.make_job(curve, name))
    small = vkd_fixtures.job_small.__wrapped__(curve)              # a copy of its own: the cached fixture is never changed
    small.set_challenges(*vkd_fixtures.CHAL)
    jobs["vkd small"] = job_record(small)
    jobs["vkd a"] = job_record(vkd_fixtures.job_a(curve))
    return jobs


def record():
    return {curve: curve_record(curve) for curve in CURVES}


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)
