"""GPU: hk_vkd_tree (csrc/vkd_tree.cuh) against its host mirror `vkd_circuit.directory_paths`, byte for
byte: siblings, roots and status of every case of tests/vkd_tree_cases.py; the 64-event case with device operands, device
outputs and no status; 2 049 events (more than one tile of the sort) checked link by link; `VkdJob.from_directory` against the
host job of fixture B; every refusal with its outputs untouched and the lane usable afterwards."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import FrCodec
from hekaton_system_amd.poseidon import device_params
from hekaton_system_amd.vkd_circuit import (Append, SparseTree, Update, VkdJob, compute_root, concat, get_index, hash_leaf,
                                            leaves_table)
from tests import vkd_tree_cases as vc
from tests.vkd_fixtures import DEPTH, SPLIT, job_b

pytestmark = pytest.mark.gpu
PATTERN = 0xA5


def _ctx(cname, ctx_bn254, ctx_bls):
    return ctx_bn254 if cname == "bn254" else ctx_bls


@functools.lru_cache(maxsize=None)
def _params(cname):
    return device_params(cname, FrCodec(cname))


def _inputs(depth, leaves0, changes):
    return (depth, np.frombuffer(b"".join(leaves0), np.uint8), np.array([u.kind for u in changes], np.uint32),
            leaves_table(changes))


def _want(cname, which):
    initial, final, paths, status = vc.mirror(cname, which)
    fc = FrCodec(cname)
    return fc.enc([x for p in paths for x in p]).tobytes(), fc.enc([initial, final]).tobytes(), bytes(status)


@pytest.mark.parametrize("which", vc.ALL_CASES)
@pytest.mark.parametrize("cname", vc.CURVES)
def test_case_equals_mirror(cname, which, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    sib, roots, status = ctx.vkd_tree(*_inputs(*vc.case(cname, which)), _params(cname))
    want = _want(cname, which)
    assert roots.tobytes() == want[1]
    assert status.tobytes() == want[2]
    assert sib.tobytes() == want[0]


@pytest.mark.parametrize("cname", vc.CURVES)
def test_residency_and_null_status(cname, ctx_bn254, ctx_bls):
    """Case g at 64 events: every input a DeviceBuffer; device outputs; no status.  All as the host-pointer run."""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    depth, leaves0, kinds, leaves = _inputs(*vc.case(cname, "g64"))
    consts, n_consts, ld, nd = _params(cname)
    want = _want(cname, "g64")
    bufs = [capi.DeviceBuffer.from_host(ctx, x) for x in (leaves0, leaves, consts)]
    try:
        sib, roots, status = ctx.vkd_tree(depth, bufs[0], kinds, bufs[1], (bufs[2], n_consts, ld, nd))
        assert (sib.tobytes(), roots.tobytes(), status.tobytes()) == want
        outs = ctx.vkd_tree(depth, leaves0, kinds, leaves, _params(cname), device_out=True)
        try:
            assert tuple(x.to_host()[:len(w)].tobytes() for x, w in zip(outs, want)) == want
        finally:
            for x in outs:
                x.free()
        fr = ctx.fr_bytes
        out = (np.full(len(want[0]), PATTERN, np.uint8), np.full(2 * fr, PATTERN, np.uint8), None)
        ctx.vkd_tree(depth, leaves0, kinds, leaves, _params(cname), out=out)
        assert (out[0].tobytes(), out[1].tobytes()) == want[:2]
    finally:
        for b in bufs:
            b.free()


@functools.lru_cache(maxsize=None)
def _long_batch(cname):
    """2 049 changes over 40 users on an empty directory, the appends repeated now and then: (changes, the leaf each change
    finds at its index or None, the status the host dict predicts)."""
    rng = random.Random(7)
    users = [vc.name(100 + i) for i in range(40)]
    assert len({get_index(cname, u, vc.DEPTH) for u in users}) == 40
    held, changes, before, status = {}, [], [], []
    for k in range(2049):
        u = users[k] if k < 40 and k % 2 == 0 else users[rng.randrange(40)]
        cur = held.get(u)
        before.append(None if cur is None else concat(u, cur[1], cur[0]))
        if cur is None or rng.randrange(16) == 0:
            changes.append(Append(u, vc.key(k)))
            status.append(0 if cur is None else 1)
            held[u] = (0, vc.key(k))
        else:
            changes.append(Update(u, cur[0], cur[1], vc.key(k)))
            status.append(0)
            held[u] = ((cur[0] + 1) % 65535, vc.key(k))
    assert 1 in status and 0 in status
    return changes, before, status


@pytest.mark.parametrize("cname", vc.CURVES)
def test_long_batch_links(cname, ctx_bn254, ctx_bls):
    """More events than one tile of the sort: the root every path leads to from what the index held is the root the change
    before it left."""
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    changes, before, want_status = _long_batch(cname)
    U, depth, fc = len(changes), vc.DEPTH, FrCodec(cname)
    assert U > 2048
    sib, roots, status = ctx.vkd_tree(*_inputs(depth, [], changes), _params(cname))
    assert status.tobytes() == bytes(want_status)
    sib = fc.dec(sib)
    roots = fc.dec(roots)
    path = lambda u: sib[u * depth:(u + 1) * depth]
    index = lambda u: get_index(cname, changes[u].username, depth)
    empty = SparseTree(cname, depth)
    assert roots[0] == empty.root

    @functools.lru_cache(maxsize=None)
    def after(u):
        return compute_root(cname, hash_leaf(cname, changes[u].leaf_new), path(u), index(u))

    step = (2040 - 8) // 17
    for u in list(range(8)) + list(range(2040, 2049)) + [8 + step * (k + 1) for k in range(16)]:
        old = empty.null_leaf if before[u] is None else hash_leaf(cname, before[u])
        assert compute_root(cname, old, path(u), index(u)) == (after(u - 1) if u else empty.root), u
    assert roots[1] == after(U - 1)


@pytest.mark.parametrize("cname", vc.CURVES)
def test_from_directory_equals_host_job(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    host = job_b(cname)
    _, leaves0, changes = vc.case(cname, "b")
    assert all(u.path is None for u in changes)
    job = VkdJob.from_directory(ctx, cname, leaves0, changes, depth=DEPTH, split=SPLIT)
    try:
        assert (job.initial_root, job.final_root) == (host.initial_root, host.final_root)
        assert bytes(job.status) == bytes(3)
        assert job.tables()["siblings"] is job.siblings and isinstance(job.siblings, capi.DeviceBuffer)
        assert job.dev0.values.to_host().tobytes() == host.values_bytes().tobytes()
        time_bytes = host.flat("time").tobytes()
        assert job.dev0.traces[0].to_host()[:len(time_bytes)].tobytes() == time_bytes
    finally:
        job.free()
    assert job.siblings is None


def _refusals(cname):
    """(name, what to change of a good call's arguments)."""
    return [("leaves0 NULL", dict(leaves0=None)), ("kinds NULL", dict(kinds=None)), ("leaves NULL", dict(leaves=None)),
            ("consts NULL", dict(consts=None)), ("leaf_hash NULL", dict(leaf_hash=None)), ("node_hash NULL", dict(node_hash=None)),
            ("siblings NULL", dict(sib=None)), ("roots NULL", dict(roots=None)),
            ("depth 0", dict(depth=0)), ("depth 8", dict(depth=8)), ("depth 20", dict(depth=20)), ("depth 264", dict(depth=264)),
            ("U 0", dict(n_updates=0)), ("U above 2^20", dict(n_updates=(1 << 20) + 1)),
            ("M + U above 2^22", dict(n_leaves0=(1 << 22))), ("a kind of 2", dict(bad_kind=True)),
            ("descriptors swapped", dict(swap=True)), ("constants too short", dict(n_consts=8)),
            ("status inside leaves", dict(status="leaves")), ("roots inside siblings", dict(roots="sib")),
            ("siblings over the constants", dict(sib="consts"))]


@pytest.mark.parametrize("cname", vc.CURVES)
def test_refusals_touch_nothing(cname, ctx_bn254, ctx_bls):
    ctx = _ctx(cname, ctx_bn254, ctx_bls)
    depth, leaves0, kinds, leaves = _inputs(*vc.case(cname, "f"))
    consts, n_consts, ld, nd = _params(cname)
    consts = np.ascontiguousarray(consts, dtype=np.uint8)
    want = _want(cname, "f")
    fr, U = ctx.fr_bytes, kinds.size
    addr = lambda x: None if x is None else x.ctypes.data
    for what, change in _refusals(cname):
        a, b = capi.hk_poseidon_desc(*(nd if change.get("swap") else ld)), capi.hk_poseidon_desc(*(ld if change.get("swap") else nd))
        k = kinds.copy()
        if change.get("bad_kind"):
            k[1] = 2
        leaves_in = leaves.copy()
        outs = dict(sib=np.full(U * depth * fr, PATTERN, np.uint8), roots=np.full(2 * fr, PATTERN, np.uint8),
                    status=np.full(U, PATTERN, np.uint8))
        arg = dict(leaves0=leaves0, kinds=k, leaves=leaves_in, consts=consts, leaf_hash=C.pointer(a), node_hash=C.pointer(b))
        ptrs = {n: addr(v) if isinstance(v, np.ndarray) else v for n, v in {**arg, **outs}.items()}
        inside = dict(leaves=leaves_in.ctypes.data + 66, sib=outs["sib"].ctypes.data + fr, consts=consts.ctypes.data)
        for n in ("leaves0", "kinds", "leaves", "consts", "leaf_hash", "node_hash", "sib", "roots", "status"):
            if n in change:
                ptrs[n] = None if change[n] is None else inside[change[n]]
        d = capi.hk_vkd_tree_desc(change.get("depth", depth), change.get("n_leaves0", leaves0.size // 66), ptrs["leaves0"],
                                  change.get("n_updates", U), ptrs["kinds"], ptrs["leaves"], ptrs["consts"],
                                  change.get("n_consts", n_consts), ptrs["leaf_hash"], ptrs["node_hash"])
        keep_consts, keep_leaves = consts.copy(), leaves_in.copy()
        st = ctx.lib.hk_vkd_tree(ctx.handle, C.byref(d), ptrs["sib"], ptrs["roots"], ptrs["status"])
        assert st in (capi.HK_ERR_ARG, capi.HK_ERR_LEN), what
        assert all((o == PATTERN).all() for o in outs.values()), what
        assert (consts == keep_consts).all() and (leaves_in == keep_leaves).all(), what
    got = ctx.vkd_tree(depth, leaves0, kinds, leaves, _params(cname))
    assert tuple(x.tobytes() for x in got) == want
