"""CPU: the RAM portal subcircuit and the VM job (hekaton_system_amd/vm_circuit.py): the trace is the reference's
(`get_portal_subtraces`, vm/vm_constraints.rs:29-85), the host witness satisfies the R1CS the same program builds, and the
gadget is a check - each single tampering of an otherwise honest job fails in the block that states the violated rule."""
import random

import pytest

from hekaton_system_amd.cp_groth16 import r1cs_bad_rows
from hekaton_system_amd.transcript import RamTranscriptEntry, sort_subtraces_by_addr
from hekaton_system_amd.vm_circuit import ENTRY_COLS, RamSubcircuit, VmJob, vm_subtraces
from tests.vm_cases import CHAL, T0S, TAMPERINGS, bad_rows, random_ram_job, vm_job

CURVES = ("bn254", "bls12_381")
SHAPES = ((1, 1), (2, 1), (3, 2))


# ---- the trace ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,ops", SHAPES)
@pytest.mark.parametrize("t0", T0S)
def test_trace_is_the_reference_vm_pattern(log_n, ops, t0):
    rnd = random.Random(5)
    values = [rnd.randrange(1, 1 << 60) for _ in range(10000)]
    assert len(set(values)) == len(values)
    st = vm_subtraces(log_n, ops, values=values, t0=t0)
    assert [len(s) for s in st] == [16 + 3 * ops] + [32 + 3 * ops] * ((1 << log_n) - 1)
    flat = [e for s in st for e in s]
    assert [e.i for e in flat] == list(range(t0, t0 + len(flat)))
    assert {e.addr for e in flat} == set(range(1, 17))
    assert [e.addr for e in st[0][:16]] == list(range(1, 17)) and not any(e.read for e in st[0][:16])
    # `register 1` is the second register set: address 2; its operation is set, get, get
    assert [(e.addr, e.read) for e in st[0][16:19]] == [(2, False), (2, True), (2, True)]
    assert [(e.addr, e.read) for e in st[1][:16]] == [(a, True) for a in range(1, 17)]
    assert [(e.addr, e.read) for e in st[1][-16:]] == [(a, False) for a in range(1, 17)]
    # a get returns the last set; every set takes the next value
    mem, it = {}, iter(values)
    for e in flat:
        if not e.read:
            mem[e.addr] = next(it)
        assert e.val == mem[e.addr]
    # the address order steps by 0 or 1 everywhere, from the padding entry's address 0
    srt = [e for s in sort_subtraces_by_addr(st) for e in s]
    assert all(b.addr - a.addr in (0, 1) for a, b in zip([RamTranscriptEntry.padding()] + srt, srt))
    assert all(a.i < b.i for a, b in zip(srt, srt[1:]) if a.addr == b.addr)


def test_default_values_are_the_reference_ones():
    assert {e.val for s in vm_subtraces(2, 1) for e in s} == {1}
    assert vm_subtraces(1, 0)[0][0] == RamTranscriptEntry(1, 1, 0, False)


def test_three_classes():
    job = VmJob("bn254", 2, 1, 4)
    assert [job.class_of(i) for i in range(4)] == [(19, True, False), (35, False, False), (35, False, False), (35, False, True)]
    first, mid, last = job.make_class(0), job.make_class(1), job.make_class(3)
    assert job.make_class(2) is mid and mid is not last
    assert last.n_c == mid.n_c + 1 and last.n_v == mid.n_v                 # the `last` row
    for c in (first, mid, last):
        k = c.np_
        assert c.N_INST == 6 and c.n0 == 70 * k and c.col0 == 6 + 70 * k and c.pos_col0 == c.col0 + 43 * k + 37
        assert c.dummy_products == 2 and c.n_v == c.dummy_col0 + 6
        assert c.n_c + c.N_INST <= 1 << 14
        z = c.template_ints()
        assert z[0] == 1 and z[c.dummy_col0:] == [12, 12, 144] * 2 and not any(z[1:c.dummy_col0])


# ---- the honest witness ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n,ops", SHAPES)
@pytest.mark.parametrize("t0", T0S)
def test_honest_witness_satisfies_every_class(curve, log_n, ops, t0):
    job = vm_job(curve, log_n, ops, t0=t0)
    assert job.time_eval0[-1] == job.addr_eval0[-1]
    for idx in range(job.n):
        circ = job.make_class(idx)
        z = job.assignment_ints(idx)
        assert len(z) == circ.n_v
        assert r1cs_bad_rows(*circ.rows(), z, circ.r) == []
        # the stage-0 columns are exactly the first 70 k witnesses
        assert z[circ.N_INST:circ.N_INST + 2 * ENTRY_COLS * circ.np_] == job.stage0_ints(idx)
        assert z[:6] == [1] + list(CHAL) + [job.root]
        assert (job.make_class(idx).fc.dec(job.assignment_bytes(idx)) == z)


def test_matrices_and_rows_agree():
    """The CSR export keygen reads holds the rows the tests evaluate."""
    circ = RamSubcircuit("bn254", 3, first=True, last=False, depth=1, dummy_products=1)
    A, B, C = circ.rows()
    for rows, (rp, col, val) in zip((A, B, C), circ.csr(circ.fc)):
        vals = circ.fc.dec(val)
        assert len(rp) == circ.n_c + 1
        for i in (0, 5, circ.n_c // 2, circ.n_c - 1):
            got = sorted((int(col[k]), vals[k]) for k in range(int(rp[i]), int(rp[i + 1])))
            assert got == sorted((c, v % circ.r) for v, c in rows[i])


# ---- the gadget is a check ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tamper", TAMPERINGS, ids=lambda f: f.__name__)
def test_a_single_tampering_fails_in_the_block_of_its_rule(tamper):
    job = vm_job("bn254", 2, 1, chal=None)
    sub, block, pair, rule = tamper(job)
    job.set_challenges(CHAL)
    circ = job.make_class(sub)
    bad = bad_rows(job, sub)
    assert len(bad) >= 1
    lo, hi = circ.blocks[block]
    assert lo <= bad[0] < hi and circ.block_of(bad[0]) == block
    if block == "pairs":
        assert circ.pair_rule_of(bad[0]) == (pair, rule)
    if block == "last":                    # the permutation check is the last subcircuit's alone
        assert sub == job.n - 1 and bad == [lo]
        assert all(bad_rows(job, i) == [] for i in range(job.n - 1))


def test_subcircuit_0_pins_the_previous_entry_and_the_start_evaluations():
    job = vm_job("bn254", 2, 1)
    circ = job.make_class(0)
    for prev in (RamTranscriptEntry(0, 5, 0, False), RamTranscriptEntry(1, 0, 0, False), RamTranscriptEntry(0, 0, 1 << 31, False),
                 RamTranscriptEntry(0, 0, 0, True)):
        bad = bad_rows(job, 0, prev=prev)
        assert bad and circ.block_of(bad[0]) == "prev"
    bad = bad_rows(job, 0, time_eval0=2)
    assert bad and circ.block_of(bad[0]) == "time_chain" and bad[0] == circ.blocks["time_chain"][0]
    bad = bad_rows(job, 0, addr_eval0=2)
    assert bad and circ.block_of(bad[0]) == "addr_chain" and bad[0] == circ.blocks["addr_chain"][0]
    # a later subcircuit takes both from the previous leaf: no such rows
    assert job.make_class(1).blocks["prev"][1] - job.make_class(1).blocks["prev"][0] == 33      # booleanity only


def test_delta_bits_are_free_when_the_address_changes():
    """Tampering 8 is NOT a failure: the comparator's row is `same * (...) = 0`, so with same = 0 its 32 delta columns are
    constrained to be bits and nothing else (the device writes zeros there)."""
    job = vm_job("bn254", 2, 1)
    idx = 1
    circ = job.make_class(idx)
    z = job.assignment_ints(idx)
    k = circ.np_
    pair0 = circ.col0 + 37 + 8 * k
    j = next(j for j in range(k) if z[pair0 + 35 * j + 1] == 0)             # a pair with same = 0
    assert z[pair0 + 35 * j + 3:pair0 + 35 * j + 35] == [0] * 32
    for b in (0, 17, 31):
        z2 = list(z)
        z2[pair0 + 35 * j + 3 + b] = 1
        assert r1cs_bad_rows(*circ.rows(), z2, circ.r) == []
    z2 = list(z)
    z2[pair0 + 35 * j + 3] = 2                                             # ... but it must be a bit
    bad = r1cs_bad_rows(*circ.rows(), z2, circ.r)
    assert len(bad) == 1 and circ.pair_rule_of(bad[0]) == (j, "delta_boolean")


# ---- random RAM programs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_random_ram_programs_satisfy_the_circuit(seed):
    job = random_ram_job("bn254", seed)
    assert len({e.addr for st in job.time for e in st}) <= 5
    for idx in range(job.n):
        assert bad_rows(job, idx) == []


def test_random_programs_reach_every_position():
    """Over the 20 programs, every pair position of a subtrace (pair 0 included) sees a same-address read, a same-address
    write and a step to the next address."""
    seen = {}
    for seed in range(20):
        job = random_ram_job("bn254", seed, chal=None)
        flat = [RamTranscriptEntry.padding()] + [e for st in job.addr for e in st]
        k = len(job.addr[0])
        for n in range(1, len(flat)):
            p, e = flat[n - 1], flat[n]
            kind = "step" if e.addr != p.addr else ("read" if e.read else "write")
            seen.setdefault((n - 1) % k, set()).add(kind)
    assert all(seen[j] == {"step", "read", "write"} for j in range(k))
