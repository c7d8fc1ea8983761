"""GPU: hk_trace_sort and hk_stage0_witness (csrc/trace_sort.cuh) against the pinned host mirror, byte for byte.  The checker
is always transcript.sort_subtraces_by_addr + transcript.flatten_subtraces (for the job: ShaMerkleJob's own host `addr` and
`stage0_ints`), never the device.  Every case with `perm` also checks that perm is a permutation, that sorted entry j is time
entry perm[j], and that perm increases within each run of equal keys.  Values are random Fr, 0 and r - 1 among them, and no
two entries share one: a stability error shows in the bytes.

Sizes: 1, 2, the wave edge 63 / 64 / 65, both sides of every power of two from 2^8 to 2^13 (the one-workgroup limit and a
ragged last tile whatever the tile), and 100 003 (49 tiles, the last one ragged).  Each host reference is computed once per
session (functools.lru_cache) and never modified."""
import ctypes as C
import random
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from hekaton_system_amd import capi, transcript
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec
from hekaton_system_amd.sha_circuit import ShaMerkleJob, Stage1Device
from hekaton_system_amd.transcript import RAM, ROM, RamTranscriptEntry, RomTranscriptEntry

pytestmark = pytest.mark.gpu

U64, U32 = (1 << 64) - 1, (1 << 32) - 1
BASE = 0x6a09e667f3bcc908                                          # the key whose single bytes the `byte` families vary
SIZES = [1, 2, 63, 64, 65] + [(1 << k) + d for k in range(8, 14) for d in (-1, 0, 1)] + [100003]
FAMILY_SIZES = [65, 4097, 100003]


def _ctx(curve, ctx_bn254, ctx_bls):
    return ctx_bn254 if curve == "bn254" else ctx_bls


def _pattern(nbytes, seed=0):
    return ((np.arange(nbytes, dtype=np.uint64) * 131 + 89 + seed) % 251).astype(np.uint8)


def _pool(rnd, size, top):
    return [0, top] + [rnd.randrange(top + 1) for _ in range(max(size, 2) - 2)]


def _rom_keys(family, n, rnd):
    if family == "equal":
        return [0xdeadbeef] * n
    if family == "two90":                                          # the placeholder-heavy shape of real traces
        return [0 if rnd.random() < 0.9 else 77 for _ in range(n)]
    if family in ("pool", "sorted", "reverse"):
        pool = _pool(rnd, n // 4, U64)
        keys = [rnd.choice(pool) for _ in range(n)]
        if n >= 2:
            keys[0], keys[-1] = U64, 0
        return keys if family == "pool" else sorted(keys, reverse=family == "reverse")
    if family.startswith("byte"):
        b = int(family[4:])
        return [(BASE & ~(0xff << (8 * b))) | (rnd.randrange(256) << (8 * b)) for _ in range(n)]
    raise KeyError(family)


def _ram_keys(family, n, rnd):
    if family == "six":
        ts = _pool(rnd, 9, U32)
        return [(rnd.choice([0, 1, 2, 1 << 32, U64 - 1, U64]), rnd.choice(ts)) for _ in range(n)]
    if family == "equal":
        return [(5, 1 << 31)] * n
    if family.startswith("ts"):
        b = int(family[2:])
        return [(BASE, (0x9e3779b9 & ~(0xff << (8 * b))) | (rnd.randrange(256) << (8 * b))) for _ in range(n)]
    if family == "addr_decides":                                   # (2, 0) comes first in time and last in address order
        return [(2, 0), (1, U32)] + [(rnd.choice([1, 2]), rnd.choice([0, U32])) for _ in range(n - 2)]
    raise KeyError(family)


@lru_cache(maxsize=None)
def _case(curve, mem, family, n):
    """One flattened time-ordered trace with what the host mirror makes of it: time_b, want_b (Montgomery bytes), the keys
    in sorted order."""
    r = CURVE_PARAMS[curve]["r"]
    fc = FrCodec(curve)
    rnd = random.Random("%s %s %s %d" % (curve, mem, family, n))
    vals = [rnd.randrange(r) for _ in range(n)]
    vals[rnd.randrange(n)] = 0
    if n > 1:
        vals[(vals.index(0) + 1 + rnd.randrange(n - 1)) % n] = r - 1
    assert len(set(vals)) == n
    if mem == ROM:
        entries = [RomTranscriptEntry(a, v) for a, v in zip(_rom_keys(family, n, rnd), vals)]
    else:
        entries = [RamTranscriptEntry(a, v, t, bool(rnd.randrange(2))) for (a, t), v in zip(_ram_keys(family, n, rnd), vals)]
    _, time_b = transcript.flatten_subtraces(fc, [entries])
    srt = transcript.sort_subtraces_by_addr([entries])
    _, want_b = transcript.flatten_subtraces(fc, srt)
    time_b.setflags(write=False)
    want_b.setflags(write=False)
    return SimpleNamespace(n=n, k=2 if mem == ROM else 4, time_b=time_b, want_b=want_b, keys=[e.sort_key() for e in srt[0]],
                           entries=entries, sorted=srt[0])


def _check_perm(case, got_b, perm):
    n, row = case.n, case.k * 32
    perm = np.asarray(perm)
    assert perm.dtype == np.uint32 and perm.size == n
    assert (np.sort(perm) == np.arange(n, dtype=np.uint32)).all()                          # a permutation
    assert (np.asarray(got_b).reshape(n, row) == case.time_b.reshape(n, row)[perm]).all()   # sorted entry j = time entry perm[j]
    same = np.array([a == b for a, b in zip(case.keys, case.keys[1:])], dtype=bool)
    assert (perm[1:][same] > perm[:-1][same]).all()                # equal keys keep their time order


def _run(ctx, case, dev_in=False, dev_out=False):
    """One trace_sort with perm over the given residency; returns (entries bytes, perm) on the host."""
    src = capi.DeviceBuffer.from_host(ctx, case.time_b) if dev_in else case.time_b
    out, perm = ctx.trace_sort(case.k, src, case.n, device_out=dev_out, want_perm=True)
    if dev_in:
        src.free()
    if dev_out:
        assert isinstance(out, capi.DeviceBuffer) and isinstance(perm, capi.DeviceBuffer)
        got, p = out.to_host()[:case.n * case.k * 32], perm.to_host()[:4 * case.n].view(np.uint32)
        out.free()
        perm.free()
        return got, p
    return out, perm


def _check(ctx, case, **kw):
    got, perm = _run(ctx, case, **kw)
    if not (got == case.want_b).all():
        bad = np.flatnonzero((got != case.want_b).reshape(case.n, -1).any(axis=1))
        raise AssertionError("first differing entry %d, %d of %d differ" % (bad[0], bad.size, case.n))
    _check_perm(case, got, perm)
    return got, perm


# ---- 1. sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_rom_sizes_bn254(n, ctx_bn254):
    _check(ctx_bn254, _case("bn254", ROM, "pool", n))


@pytest.mark.parametrize("n", [65, 4097, 100003])
def test_rom_sizes_bls(n, ctx_bls):
    _check(ctx_bls, _case("bls12_381", ROM, "pool", n))


@pytest.mark.parametrize("n", [65, 4097])
def test_ram_sizes_bls(n, ctx_bls):
    _check(ctx_bls, _case("bls12_381", RAM, "six", n))


# ---- 2. key families ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FAMILY_SIZES)
@pytest.mark.parametrize("family", ["equal", "two90", "sorted", "reverse"] + ["byte%d" % b for b in range(8)])
def test_rom_key_families(family, n, ctx_bn254):
    case = _case("bn254", ROM, family, n)
    if family == "reverse":
        assert len(set(case.keys)) < n                             # with duplicates
    _, perm = _check(ctx_bn254, case)
    if family == "equal":
        assert (perm == np.arange(n)).all()                        # no digit varies: every pass is skipped
    if family == "sorted":
        assert (perm == np.arange(n)).all()
    if family.startswith("byte"):
        b = int(family[4:])
        assert {k ^ case.keys[0] for k in case.keys} - {0} and all((k ^ BASE) & ~(0xff << (8 * b)) == 0 for k in case.keys)


@pytest.mark.parametrize("n", [65, 4097])
@pytest.mark.parametrize("family", ["six", "equal", "addr_decides"] + ["ts%d" % b for b in range(4)])
def test_ram_key_families(family, n, ctx_bn254):
    case = _case("bn254", RAM, family, n)
    _, perm = _check(ctx_bn254, case)
    if family == "six":
        ts = {t for _a, t in case.keys}
        assert 0 in ts and U32 in ts and {a for a, _t in case.keys} == {0, 1, 2, 1 << 32, U64 - 1, U64}
    if family == "equal":                                          # equal (addr, timestamp), differing is_read and val
        assert (perm == np.arange(n)).all() and len({e.read for e in case.entries}) == 2
    if family == "addr_decides":                                   # (1, 2^32 - 1) before (2, 0): the address decides
        assert case.keys.index((1, U32)) < case.keys.index((2, 0))
        assert int(np.flatnonzero(perm == 1)[0]) < int(np.flatnonzero(perm == 0)[0])


# ---- 3. residency ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev_in,dev_out", [(False, False), (True, True), (False, True), (True, False)])
def test_residency(dev_in, dev_out, ctx_bn254):
    _check(ctx_bn254, _case("bn254", ROM, "pool", 4097), dev_in=dev_in, dev_out=dev_out)
    _check(ctx_bn254, _case("bn254", RAM, "six", 4097), dev_in=dev_in, dev_out=dev_out)


def test_without_perm_and_through_the_transcript_wrapper(ctx_bn254):
    case = _case("bn254", ROM, "two90", 4097)
    assert (ctx_bn254.trace_sort(2, case.time_b) == case.want_b).all()
    for mem, fam in ((ROM, "pool"), (RAM, "six")):
        case = _case("bn254", mem, fam, 257)
        st = [case.entries[:0], case.entries[:100], [], case.entries[100:]]
        assert transcript.sort_subtraces_by_addr_device(ctx_bn254, st) == transcript.sort_subtraces_by_addr(st)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------
def test_three_runs_are_identical(ctx_bn254):
    case = _case("bn254", ROM, "two90", 100003)
    runs = [_run(ctx_bn254, case) for _ in range(3)]
    for got, perm in runs:
        assert (got == case.want_b).all()
        assert (got == runs[0][0]).all() and (perm == runs[0][1]).all()
    _check_perm(case, *runs[0])


# ---- 5. the job's chain ----------------------------------------------------------------------------------------------------
def test_sha_merkle_job_chain(ctx_bn254):
    ctx, curve = ctx_bn254, "bn254"
    fc = FrCodec(curve)
    r = CURVE_PARAMS[curve]["r"]
    rnd = random.Random(41)
    job = ShaMerkleJob(curve, 64, 1, 4, [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(32)])
    flat = lambda tr: fc.enc([x for ops in tr for e in ops for x in e])
    dev0 = job.stage0_device(ctx)
    assert list(dev0.offsets) == [4 * i for i in range(65)]
    assert (dev0.traces[0].to_host() == flat(job.time)).all()
    assert (dev0.traces[1].to_host() == flat(job.addr)).all()      # the device-sorted trace = the host-sorted one
    # stage-0 rows: scrambled with a repeat, a batch of one, every subcircuit
    for members in ([37, 0, 63, 5, 37, 12], [63], list(range(64))):
        w = dev0.rows(members)
        got = w.to_host().reshape(len(members), -1)
        w.free()
        assert got.shape[1] == 16 * 32
        for b, i in enumerate(members):
            assert (got[b] == fc.enc(job.stage0_ints(i))).all(), (members, b)
    # exec_tree and the stage-1 columns over the adopted traces = over the host-sorted upload
    job.set_challenges(rnd.randrange(r), rnd.randrange(r), ctx=ctx)
    ref = Stage1Device(job, ctx)
    dev = job.stage1_device(ctx, traces=dev0.traces)
    assert dev.traces[0] is dev0.traces[0] and dev.traces[1] is dev0.traces[1]
    assert dev.root == ref.root == job.root
    for a, b in zip(dev.outs, ref.outs):
        assert (a.to_host() == b.to_host()).all()
    classes = {}
    for i in range(job.n):
        classes.setdefault(job.class_of(i), []).append(i)
    assert len(classes) == 5
    for key, members in classes.items():
        members = members[:3] + members[-1:]
        circ = job.make_class(members[0])
        prefill = _pattern(len(members) * circ.n_v * 32, seed=len(members))
        zs = [capi.DeviceBuffer.from_host(ctx, prefill) for _ in range(2)]
        dev.fill(circ, members, zs[0])
        ref.fill(circ, members, zs[1])
        got, want = zs[0].to_host(), zs[1].to_host()
        for z in zs:
            z.free()
        assert (got == want).all(), key
        assert not (got == prefill).all()
    dev.free()
    ref.free()
    assert dev0.traces[0].ptr and dev0.traces[1].ptr               # adopted buffers stay their owner's
    dev0.free()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def _raw_sort(ctx, k, src, n, out, perm):
    p = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
    return ctx.lib.hk_trace_sort(ctx.handle, k, p(src), n, p(out), p(perm))


@pytest.mark.parametrize("n", [65, 4097])
def test_trace_sort_refusals_leave_the_outputs_untouched(n, ctx_bn254):
    ctx, curve = ctx_bn254, "bn254"
    fc = FrCodec(curve)
    r = CURVE_PARAMS[curve]["r"]
    rom, ram = _case(curve, ROM, "pool", n), _case(curve, RAM, "six", n)
    out_fill, perm_fill = _pattern(n * 128, seed=3), _pattern(4 * n, seed=4).view(np.uint32)
    out, perm = out_fill.copy(), perm_fill.copy()

    def with_field(case, entry, field, value):
        b = case.time_b.copy()
        at = (entry * case.k + field) * 32
        b[at:at + 32] = fc.enc([value])
        return b

    refused = {
        "addr 2^64": _raw_sort(ctx, 2, with_field(rom, n // 2, 0, 1 << 64), n, out, perm),
        "addr 2^64 in the last entry": _raw_sort(ctx, 2, with_field(rom, n - 1, 0, 1 << 64), n, out, perm),
        "addr r - 1": _raw_sort(ctx, 2, with_field(rom, 0, 0, r - 1), n, out, perm),
        "ram addr 2^64": _raw_sort(ctx, 4, with_field(ram, n - 1, 0, 1 << 64), n, out, perm),
        "ram timestamp 2^32": _raw_sort(ctx, 4, with_field(ram, n // 3, 2, 1 << 32), n, out, perm),
        "entry_fields 3": _raw_sort(ctx, 3, rom.time_b, n, out, perm),
        "entry_fields 0": _raw_sort(ctx, 0, rom.time_b, n, out, perm),
        "NULL output": _raw_sort(ctx, 2, rom.time_b, n, None, perm),
        "NULL input": _raw_sort(ctx, 2, None, n, out, perm),
        "n 2^31": _raw_sort(ctx, 2, rom.time_b, 1 << 31, out, perm),
    }
    # output ranges on the input: the same array, a range that starts inside it, one that ends inside it, perm inside it
    buf = np.concatenate([rom.time_b, rom.time_b])
    keep = buf.copy()
    at = buf.ctypes.data
    refused.update({
        "out = in": _raw_sort(ctx, 2, at, n, at, perm),
        "out starts in in": _raw_sort(ctx, 2, at, n, at + 64 * n - 32, perm),
        "out ends in in": _raw_sort(ctx, 2, at + 64 * n - 32, n, at, perm),
        "perm in in": _raw_sort(ctx, 2, at, n, out, at + 64),
    })
    assert refused == {name: capi.HK_ERR_ARG for name in refused}
    assert (out == out_fill).all() and (perm == perm_fill).all() and (buf == keep).all()
    # the largest values that fit are fine: addr 2^64 - 1 and timestamp 2^32 - 1 (both in the `six` family), and a wide val
    assert (U64, U32) in ram.keys or U64 in {a for a, _ in ram.keys}
    assert _raw_sort(ctx, 4, with_field(ram, 0, 1, r - 1), n, out, perm) == capi.HK_OK
    # nothing to sort
    assert _raw_sort(ctx, 2, None, 0, None, None) == capi.HK_OK
    assert _raw_sort(ctx, 4, rom.time_b, 0, out, perm) == capi.HK_OK
    # the same context still works, out just behind in
    assert _raw_sort(ctx, 2, at, n, at + 64 * n, None) == capi.HK_OK
    assert (buf[:64 * n] == rom.time_b).all() and (buf[64 * n:] == rom.want_b).all()


def test_stage0_witness_refusals_leave_w_out_untouched(ctx_bn254):
    ctx = ctx_bn254
    case = _case("bn254", ROM, "pool", 65)
    time_b, addr_b = case.time_b[:64 * 64], case.want_b[:64 * 64]   # 16 subcircuits of 4 entries (any two traces will do)
    offsets = np.arange(17, dtype=np.uint32) * 4
    uneven = offsets.copy()
    uneven[3] -= 1                                                 # subcircuit 2 owns 3 entries, subcircuit 3 owns 5
    prefill = _pattern(3 * 16 * 32, seed=9)
    w = capi.DeviceBuffer.from_host(ctx, prefill)
    host_w = prefill.copy()

    def call(off=offsets, n_sub=16, k=4, rows=(1, 15, 1), null=None, batch=None, w_ptr=None):
        off = np.ascontiguousarray(off, dtype=np.uint32)
        sub = np.array(rows, np.uint32)
        a = dict(offsets=off.ctypes.data, time=time_b.ctypes.data, addr=addr_b.ctypes.data, sub=sub.ctypes.data,
                 w=w.ptr if w_ptr is None else w_ptr)
        if null:
            a[null] = None
        return ctx.lib.hk_stage0_witness(ctx.handle, a["offsets"], n_sub, k, a["time"], a["addr"], a["sub"],
                                         len(rows) if batch is None else batch, a["w"])

    refused = {name: call(null=name) for name in ("offsets", "time", "addr", "sub", "w")}
    refused.update({
        "n_portals 0": call(k=0),
        "offsets[0] 1": call(off=[1] + list(offsets[1:])),
        "decreasing offsets": call(off=[0, 4, 8, 7] + list(offsets[4:])),
        "sub_index 16": call(rows=(1, 16, 2)),
        "3 entries": call(off=uneven, rows=(1, 2)),
        "5 entries": call(off=uneven, rows=(3,)),
        "another k": call(k=3),
        "w_out on the host": call(w_ptr=host_w.ctypes.data),
    })
    assert refused == {name: capi.HK_ERR_ARG for name in refused}
    assert call(batch=0) == capi.HK_OK and call(rows=(), batch=0, null="sub") == capi.HK_OK
    assert (w.to_host() == prefill).all() and (host_w == prefill).all()
    # the same context still works; uneven offsets are fine for the subcircuits that own k entries
    assert call() == capi.HK_OK and call(off=uneven, rows=(0, 15, 5)) == capi.HK_OK
    got = w.to_host().reshape(3, 2, 4 * 64)
    w.free()
    for b, i in enumerate((0, 15, 5)):
        assert (got[b, 0] == time_b[i * 256:(i + 1) * 256]).all() and (got[b, 1] == addr_b[i * 256:(i + 1) * 256]).all()
