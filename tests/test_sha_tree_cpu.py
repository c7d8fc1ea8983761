"""CPU: hk_sha_tree / hk_sha_tree_inputs without a device - the symbols are declared, listed and exported; Context.sha_tree
and Context.sha_tree_inputs hand the library what include/hekaton.h says (a stub library records it); csrc/sha256.cuh,
compiled for the host with g++, equals hashlib on the three message shapes the job has, iterated, and its digest -> field
value equals node_hash_field in Montgomery form on both curves; the round constants are the cube roots FIPS 180-4 names;
ShaMerkleJob without a context builds what it built before (values pinned from the commit before hk_sha_tree)."""
import ctypes as C
import hashlib
import os
import random
import re

import numpy as np
import pytest

from hekaton_system_amd import capi, sha_circuit
from hekaton_system_amd.cp_groth16 import FrCodec
from hekaton_system_amd.sha_circuit import INNER_HASH_SIZE, ShaMerkleJob, iterated_sha256, node_hash_field

from tests import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hk_sha_tree", "hk_sha_tree_inputs")


def test_symbols_declared_listed_exported():
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    declared = set(re.findall(r"\b(hk_[a-z0-9_]+)\s*\(", hdr))
    for sym in NEW:
        assert sym in declared and sym in capi.EXPORTS
    assert "hk_sha_tree_out" in hdr
    if os.path.exists(capi.LIB_PATH):
        lib = capi.load()
        for sym in NEW:
            getattr(lib, sym)


def _val(p):
    return p.value if isinstance(p, C.c_void_p) else p


class _StubLib:
    """Stands in for libhekaton.so under a capi.Context: records what the two calls are handed, writes a pattern to every
    output and returns `status`."""

    def __init__(self, status=capi.HK_OK):
        self.status, self.seen = status, None

    def hk_sha_tree(self, handle, leaves, n_sub, ns, n_portals, out):
        o = out._obj
        self.seen = dict(handle=handle, leaves=bytes(C.string_at(_val(leaves), n_sub // 2 * 64)), n_sub=n_sub, ns=ns,
                         n_portals=n_portals, outs=(o.digests_out, o.time_entries_mont_out, o.sha_root_mont_out))
        for p, nbytes, pat in zip(self.seen["outs"], (32 * n_sub, 64 * n_sub * n_portals, 32), (0x31, 0x32, 0x33)):
            C.memset(p, pat, nbytes)
        return self.status

    def hk_sha_tree_inputs(self, handle, leaves, digests, n_sub, n_inputs, sub_index, batch, out):
        sub = list(np.ctypeslib.as_array(C.cast(sub_index, C.POINTER(C.c_uint32)), (batch,))) if sub_index else None
        self.seen = dict(handle=handle, leaves=_val(leaves), digests=_val(digests), n_sub=n_sub, n_inputs=n_inputs, sub_index=sub,
                         batch=batch, out=_val(out))
        if batch:
            C.memset(_val(out), 0x34, 4 * batch * n_inputs)
        return self.status


def _stub_context(curve, lib):
    ctx = capi.Context.__new__(capi.Context)
    ctx.lib, ctx.curve, ctx.handle, ctx.fr_bytes = lib, curve, "the-handle", 32
    return ctx


def test_context_sha_tree_marshals_its_arguments():
    rnd = random.Random(3)
    leaves = [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(4)]
    for src in (leaves, np.frombuffer(b"".join(leaves), np.uint8)):     # a list of bytes, or the array of them
        lib = _StubLib()
        digests, time_e, root = _stub_context("bn254", lib).sha_tree(src, 8, 38, 5)
        s = lib.seen
        assert (s["handle"], s["leaves"], s["n_sub"], s["ns"], s["n_portals"]) == ("the-handle", b"".join(leaves), 8, 38, 5)
        assert s["outs"] == (digests.ctypes.data, time_e.ctypes.data, root.ctypes.data)
        assert (digests.size, time_e.size, root.size) == (8 * 32, 8 * 5 * 2 * 32, 32)
        assert (digests == 0x31).all() and (time_e == 0x32).all() and (root == 0x33).all()
    with pytest.raises(capi.HekatonError) as e:
        _stub_context("bn254", _StubLib(capi.HK_ERR_ARG)).sha_tree(leaves, 8, 1, 4)
    assert e.value.status == capi.HK_ERR_ARG


def test_context_sha_tree_inputs_marshals_its_arguments():
    leaves = np.arange(4 * 64, dtype=np.uint8)
    digests = np.arange(8 * 32, dtype=np.uint8)
    lib = _StubLib()
    ctx = _stub_context("bls12_381", lib)
    out = ctx.sha_tree_inputs(leaves, None, 8, 16, [7, 0, 0])
    s = lib.seen
    assert (s["handle"], s["leaves"], s["digests"]) == ("the-handle", leaves.ctypes.data, None)
    assert (s["n_sub"], s["n_inputs"], s["sub_index"], s["batch"]) == (8, 16, [7, 0, 0], 3)
    assert out.dtype == np.uint32 and out.shape == (3, 16) and s["out"] == out.ctypes.data and (out == 0x34343434).all()
    out = ctx.sha_tree_inputs(None, digests, 8, 54, [6, 4])
    s = lib.seen
    assert (s["leaves"], s["digests"], s["n_inputs"], s["sub_index"]) == (None, digests.ctypes.data, 54, [6, 4]) and out.shape == (2, 54)
    out = ctx.sha_tree_inputs(leaves, digests, 8, 54, [])
    assert (lib.seen["sub_index"], lib.seen["batch"]) == (None, 0) and out.shape == (0, 54)
    with pytest.raises(capi.HekatonError):
        _stub_context("bn254", _StubLib(capi.HK_ERR_ARG)).sha_tree_inputs(leaves, None, 8, 16, [1])


# ---- csrc/sha256.cuh on the host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim") / "sha256_shim.so")
    host_build.build("sha256_shim.cpp", out, "-O1", *host_build.SHARED)
    return host_build.load(out)


def _messages(nbytes, seed):
    rnd = random.Random(seed)
    edge = [bytes(nbytes), b"\xff" * nbytes, b"\x80" + bytes(nbytes - 1), bytes(nbytes - 1) + b"\x01"]
    return edge + [bytes(rnd.randrange(256) for _ in range(nbytes)) for _ in range(12)]


@pytest.mark.parametrize("ns", [1, 2, 3, 40])
def test_three_message_shapes_equal_hashlib(shim, ns):
    out = C.create_string_buffer(32)
    for msg in _messages(64, 64 + ns):                                 # a leaf: two blocks
        shim.shim_sha_iter64(msg, ns, out)
        assert out.raw == iterated_sha256(msg, ns)
    for dg in _messages(32, 32 + ns):                                  # a digest: one block
        shim.shim_sha_iter32(dg, ns, out)
        assert out.raw == iterated_sha256(dg, ns)
    for pair in _messages(64, 54 + ns):                                # two child digests, 27 bytes of each taken
        l, r = pair[:32], pair[32:]
        shim.shim_sha_iter54(l, r, ns, out)
        assert out.raw == iterated_sha256(l[:INNER_HASH_SIZE] + r[:INNER_HASH_SIZE], ns)
    # the bytes past the 27th of a child do not matter
    l, r = bytes(range(32)), bytes(range(100, 132))
    shim.shim_sha_iter54(l, r, ns, out)
    a = out.raw
    shim.shim_sha_iter54(l[:27] + b"\xaa" * 5, r[:27] + b"\x55" * 5, ns, out)
    assert out.raw == a


def test_one_compression_of_the_empty_message(shim):
    """The padded empty message is one block; its digest is the best-known SHA-256 value."""
    k, iv = np.zeros(64, np.uint32), np.zeros(8, np.uint32)
    shim.shim_sha_consts(k.ctypes.data_as(C.c_void_p), iv.ctypes.data_as(C.c_void_p))
    state = iv.copy()
    shim.shim_sha_compress(state.ctypes.data_as(C.c_void_p), b"\x80" + bytes(63))
    assert b"".join(int(x).to_bytes(4, "big") for x in state) == hashlib.sha256(b"").digest()


def _primes(n):
    p, k = [], 2
    while len(p) < n:
        if all(k % q for q in p):
            p.append(k)
        k += 1
    return p


def _iroot(x, e):
    lo, hi = 0, 1 << (x.bit_length() // e + 1)
    while lo < hi:
        m = (lo + hi + 1) // 2
        if m ** e <= x:
            lo = m
        else:
            hi = m - 1
    return lo


def test_round_constants_are_the_roots_of_the_primes(shim):
    k, iv = np.zeros(64, np.uint32), np.zeros(8, np.uint32)
    shim.shim_sha_consts(k.ctypes.data_as(C.c_void_p), iv.ctypes.data_as(C.c_void_p))
    ps = _primes(64)
    assert [int(x) for x in k] == [_iroot(p << 96, 3) & 0xffffffff for p in ps]          # floor(frac(cbrt p) 2^32)
    assert [int(x) for x in iv] == [_iroot(p << 64, 2) & 0xffffffff for p in ps[:8]]     # floor(frac(sqrt p) 2^32)


@pytest.mark.parametrize("cid,curve", [(0, "bn254"), (1, "bls12_381")])
def test_digest_field_value_equals_node_hash_field(shim, cid, curve):
    fc = FrCodec(curve)
    for dg in _messages(32, 7 + cid):
        out = np.zeros(8, np.uint32)
        shim.shim_sha_digest_field(cid, dg, out.ctypes.data_as(C.c_void_p))
        assert out.tobytes() == fc.enc([node_hash_field(dg)]).tobytes()
    assert node_hash_field(b"\xff" * 32) == (1 << 216) - 1 < fc.r                        # the largest value there is


# ---- the host job is the code it was ---------------------------------------------------------------------------------------
def test_job_without_a_context_builds_what_it_built_before():
    """Values of the (bn254, 8, 1, 4) job computed with the commit before this feature."""
    rnd = random.Random(21)
    job = ShaMerkleJob("bn254", 8, 1, 4, [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(4)])
    assert job.digest[0].hex() == "26d66010caaa14393ca638a4c35d732ddd1bd29eb6da3b9ab7449f4961938efc"
    assert job.digest[6].hex() == "bf49e0863158a70adb2bdaf19c36c23413ecb68720c1e3840610e459c28406ad"
    assert job.digest[7].hex() == "f5a5fd42d16a20302798ef6ed309979b43003d2320d9f0e8ea9831a92759fb4b"
    assert job.sha_root == 93819511697072420777861259407370981754138601518112421343741888959
    assert job.time[4] == [(1, 65519230431947047660850055369347630963832479036608586607329596966),
                           (2, 51485318510986459836853177969984055706383703476221762699765085242), (0, 0),
                           (5, 64858470012850264311603429047433033171526839503633365662384868335)]
    assert job.addr[7][-1] == (6, 95167333828168491454107802567403301527024606970488042966304015910)
    whole = hashlib.sha256(repr((job.time, job.addr, [d.hex() for d in job.digest])).encode()).hexdigest()
    assert whole == "565afa2c7d5326af041300de56adb11822f0ebd0c51b3c747590c75d4d70327d"
    assert job.root is None and job.entry_chal is None and job.depth == 3 and not hasattr(job, "tree")
    assert job.kind == ["leaf"] * 4 + ["parent"] * 2 + ["root", "padding"]
    assert job.children == {4: (0, 1), 5: (2, 3), 6: (4, 5)}


class _FakeBuffer:
    made = []

    def __init__(self, *a):
        self.data, self.freed = a[-1], False
        self.nbytes = a[-1] if isinstance(a[-1], int) else len(a[-1])
        _FakeBuffer.made.append(self)

    @classmethod
    def from_host(cls, ctx, arr):
        return cls(np.asarray(arr).tobytes())

    def free(self):
        self.freed = True


class _TreeCtx:
    fr_bytes = 32

    def __init__(self):
        self.curve, self.trees, self.inputs, self.sorts = "bn254", [], [], []

    def sha_tree(self, leaves, n_sub, ns, n_portals, device_out=False):
        self.trees.append((leaves, n_sub, ns, n_portals, device_out))
        return tuple(_FakeBuffer(x) for x in (b"digests", b"time", b"root"))

    def sha_tree_inputs(self, leaves, digests, n_sub, n_inputs, sub_index, device_out=False):
        self.inputs.append((leaves, digests, n_sub, n_inputs, list(sub_index), device_out))
        return _FakeBuffer(b"inputs")

    def trace_sort(self, k, time_b, n_entries=None, device_out=False, want_perm=False):
        self.sorts.append((k, time_b, n_entries, device_out))
        return _FakeBuffer(b"sorted")


def test_on_device_job_never_builds_the_host_traces(monkeypatch):
    monkeypatch.setattr(capi, "DeviceBuffer", _FakeBuffer)
    _FakeBuffer.made = []
    rnd = random.Random(5)
    leaves = [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(4)]
    host = ShaMerkleJob("bn254", 8, 2, 4, leaves)
    ctx = _TreeCtx()
    job = ShaMerkleJob.on_device(ctx, "bn254", 8, 2, 4, leaves)
    assert (job.kind, job.children, job.depth) == (host.kind, host.children, host.depth)
    assert [job.class_of(i) for i in range(8)] == [host.class_of(i) for i in range(8)]
    assert job.make_class(6).kind == "root" and job.make_class(6).n_v == host.make_class(6).n_v
    for name in ("time", "addr", "digest"):
        assert not hasattr(job, name)
    (src, n_sub, ns, k, dev), = ctx.trees
    assert src is job.tree.leaves and src.data == b"".join(leaves) and (n_sub, ns, k, dev) == (8, 2, 4, True)
    assert (job.tree.digests.data, job.tree.time.data, job.tree.sha_root.data) == (b"digests", b"time", b"root")
    # the challenges are only recorded: no evaluations, no execution tree
    job.set_challenges(5, 7, ctx)
    assert (job.entry_chal, job.tr_chal, job.root) == (5, 7, None) and not hasattr(job, "time_eval0")
    assert isinstance(job.tree, sha_circuit.TreeDevice)
    # inputs: the kind picks n_inputs
    job.tree.inputs(job.make_class(0), [0, 3])
    job.tree.inputs(job.make_class(7), [7])
    job.tree.inputs(job.make_class(4), [5, 4])
    job.tree.inputs(job.make_class(6), [6])
    assert [(a[3], a[4], a[5]) for a in ctx.inputs] == [(16, [0, 3], True), (16, [7], True), (54, [5, 4], True), (54, [6], True)]
    assert all(a[0] is job.tree.leaves and a[1] is job.tree.digests and a[2] == 8 for a in ctx.inputs)
    # stage 0 adopts the tree's trace: nothing encoded, nothing uploaded, and its free() leaves the trace alone
    n_made = len(_FakeBuffer.made)
    dev0 = job.stage0_device(ctx)
    assert dev0.traces[0] is job.tree.time and dev0.traces[1].data == b"sorted" and len(_FakeBuffer.made) == n_made + 1
    assert ctx.sorts == [(2, job.tree.time, 32, True)]
    time_buf = job.tree.time
    dev0.free()
    assert not time_buf.freed
    job.free()
    assert time_buf.freed and job.tree.leaves is None
