"""CPU: the ABI surface of hk_stage1_witness without a device - the symbol is declared, listed and exported;
Context.stage1_witness fills hk_stage1_desc as include/hekaton.h lays it out (a stub library records it); the portal block the
call writes (10 k + 4 columns from N_INST, then the membership block at pos_col0) is column for column what
sha_circuit.full_values fills for a built ShaMerkleSubcircuit."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.poseidon import device_params
from hekaton_system_amd.sha_circuit import ShaMerkleJob, ShaMerkleSubcircuit, full_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_listed_exported():
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    declared = set(re.findall(r"\b(hk_[a-z0-9_]+)\s*\(", hdr))
    assert "hk_stage1_witness" in declared and "hk_stage1_witness" in capi.EXPORTS
    assert "hk_stage1_desc" in hdr
    if os.path.exists(capi.LIB_PATH):
        getattr(capi.load(), "hk_stage1_witness")


def test_struct_layout_follows_the_header():
    d = capi.hk_stage1_desc
    names = [f[0] for f in d._fields_]
    assert names == ["n_sub", "n_portals", "depth", "offsets", "time_entries_mont", "addr_entries_mont", "challenges_mont",
                     "evals_mont", "leaves_mont", "siblings_mont", "root_mont", "consts_mont", "n_consts", "leaf_hash",
                     "node_hash", "inst_col0", "col0", "pos_col0"]
    # the header's field order, name for name
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    body = hdr[hdr.rindex("typedef struct {", 0, hdr.index("} hk_stage1_desc;")):hdr.index("} hk_stage1_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == names
    assert (d.n_sub.offset, d.n_portals.offset, d.depth.offset, d.offsets.offset) == (0, 4, 8, 16)
    assert (d.consts_mont.offset, d.n_consts.offset, d.leaf_hash.offset, d.inst_col0.offset, d.pos_col0.offset) == \
           (80, 88, 96, 112, 120)
    assert C.sizeof(d) == 128


class _StubLib:
    """Stands in for libhekaton.so under a capi.Context: copies what hk_stage1_witness is handed and returns `status`."""

    def __init__(self, status=capi.HK_OK):
        self.status, self.seen = status, None

    def hk_stage1_witness(self, handle, desc, sub_index, batch, n_v, z_out):
        d = desc._obj
        n, depth = d.n_sub, d.depth
        off = list(np.ctypeslib.as_array(C.cast(d.offsets, C.POINTER(C.c_uint32)), (n + 1,)))
        grab = lambda p, count: bytes(C.string_at(p, count * 32)) if p else None
        self.seen = dict(handle=handle, n_sub=n, n_portals=d.n_portals, depth=depth, offsets=off,
                         time=grab(d.time_entries_mont, off[-1] * 2), addr=grab(d.addr_entries_mont, off[-1] * 2),
                         chal=grab(d.challenges_mont, 2), evals=grab(d.evals_mont, 2 * n), leaves=grab(d.leaves_mont, 4 * n),
                         siblings=grab(d.siblings_mont, n * depth), root=grab(d.root_mont, 1),
                         consts=grab(d.consts_mont, d.n_consts), n_consts=d.n_consts,
                         leaf=tuple(getattr(d.leaf_hash.contents, f[0]) for f in capi.hk_poseidon_desc._fields_),
                         node=tuple(getattr(d.node_hash.contents, f[0]) for f in capi.hk_poseidon_desc._fields_),
                         layout=(d.inst_col0, d.col0, d.pos_col0),
                         sub_index=list(np.ctypeslib.as_array(C.cast(sub_index, C.POINTER(C.c_uint32)), (batch,))) if batch else [],
                         batch=batch, n_v=n_v, z_out=z_out)
        return self.status


def _stub_context(curve, lib):
    ctx = capi.Context.__new__(capi.Context)
    ctx.lib, ctx.curve, ctx.handle, ctx.fr_bytes = lib, curve, "the-handle", 32
    return ctx


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_context_stage1_witness_marshals_its_arguments(curve):
    fc = FrCodec(curve)
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(7)
    params = device_params(curve, fc)
    n, k, depth = 8, 3, 3
    offsets = [k * i for i in range(n + 1)]
    rand = lambda count: fc.enc([rnd.randrange(r) for _ in range(count)])
    time_b, addr_b = rand(2 * k * n), rand(2 * k * n)
    outs = (rand(2 * n), rand(4 * n), rand(2 * n - 1), rand(n * depth), rand(1))
    chal = [rnd.randrange(r), rnd.randrange(r)]
    lib = _StubLib()
    z = 0x7000_0000_1000
    got = _stub_context(curve, lib).stage1_witness(params, k, offsets, time_b, addr_b, chal, outs, [5, 0, 7, 2, 2], 4321,
                                                   (1, 4, 38), z)
    s = lib.seen
    assert got == z and s["z_out"] == z and s["handle"] == "the-handle"
    assert (s["n_sub"], s["n_portals"], s["depth"], s["offsets"]) == (n, k, depth, offsets)
    assert (s["sub_index"], s["batch"], s["n_v"], s["layout"]) == ([5, 0, 7, 2, 2], 5, 4321, (1, 4, 38))
    assert s["time"] == time_b.tobytes() and s["addr"] == addr_b.tobytes()
    assert s["chal"] == fc.enc(chal).tobytes()                             # ints are encoded: entry_chal, tr_chal
    assert (s["evals"], s["leaves"], s["siblings"], s["root"]) == tuple(outs[j].tobytes() for j in (0, 1, 3, 4))   # nodes: unused
    assert s["consts"] == params[0].tobytes() and s["n_consts"] == params[1]
    assert (s["leaf"], s["node"]) == (params[2], params[3])
    # challenges already in Montgomery bytes pass through as they are
    lib2 = _StubLib()
    _stub_context(curve, lib2).stage1_witness(params, k, np.array(offsets, np.uint32), time_b, addr_b, fc.enc(chal), outs,
                                              np.array([1], np.uint32), 4321, (1, 4, 38), z)
    assert lib2.seen["chal"] == s["chal"] and lib2.seen["sub_index"] == [1]
    # a refusal surfaces as HekatonError with the library's status
    with pytest.raises(capi.HekatonError) as e:
        _stub_context(curve, _StubLib(capi.HK_ERR_ARG)).stage1_witness(params, k, offsets, time_b, addr_b, chal, outs, [0], 4321,
                                                                       (1, 4, 38), z)
    assert e.value.status == capi.HK_ERR_ARG


@pytest.mark.parametrize("kind,first,last,idx", [("leaf", True, False, 0), ("parent", False, False, 4), ("root", False, False, 6),
                                                 ("padding", False, True, 7)])
def test_portal_block_is_full_values_columns(kind, first, last, idx):
    """The layout hk_stage1_witness writes - instance at 1 .. 3, 10 k + 4 portal columns from N_INST in the documented order,
    the membership block at pos_col0 - against the columns and values full_values gives for a built class."""
    curve, k = "bn254", 4
    rnd = random.Random(11)
    job = ShaMerkleJob(curve, 8, 1, k, [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(4)])
    r = job.r
    job.set_challenges(rnd.randrange(r), rnd.randrange(r))
    circ = ShaMerkleSubcircuit(curve, kind, 1, k, first=first, last=last, depth=3)
    w = job.inputs(idx)
    cols, vals = full_values(circ, [w])
    cols = cols.tolist()
    if kind == "root":                                             # the one value that stays with hk_assignment_scatter
        assert cols[-1] == circ.sha_root_col and not (circ.N_INST <= circ.sha_root_col < circ.pos_col0 + circ.pos_cols)
        cols = cols[:-1]
    col0 = circ.N_INST
    assert cols == [1, 2, 3] + list(range(col0, col0 + 10 * k + 4))
    assert col0 + 10 * k + 4 == circ.pos_col0                      # the membership block follows at once
    # the documented order, value for value
    ech, tr = job.entry_chal, job.tr_chal
    want = [ech, tr, job.root]
    want += [x for e in w["time"] for x in e] + [x for e in w["addr"] for x in e]
    for key, e0 in (("time", w["time_eval0"]), ("addr", w["addr_eval0"])):
        cur = e0
        want.append(cur)
        for a, v in w[key]:
            e = (v + ech * a) % r
            cur = cur * ((tr - e) % r) % r
            want += [e, cur]
    want += list(w["prev"])
    chain = [w["prev"]] + list(w["addr"])
    for (a0, _), (a1, _) in zip(chain, chain[1:]):
        d = (a1 - a0) % r
        want += [pow(d, -1, r) if d else 0, 0 if d else 1]
    assert len(want) == 3 + 10 * k + 4
    assert circ.fc.dec(vals[0])[:len(want)] == [x % r for x in want]
