"""Shared by tests/test_vm_circuit_cpu.py and the RAM GPU tests: seeded VM jobs, the single tamperings of an otherwise
honest job and which rule each one breaks, and seeded random RAM programs.  Not a test module."""
import dataclasses
import random

from hekaton_system_amd.cp_groth16 import r1cs_bad_rows
from hekaton_system_amd.transcript import RamTranscriptEntry
from hekaton_system_amd.vm_circuit import RamJob, VmJob

CHAL = (0x1234567, 0x7654321, 0xabcdef1, 0x1fedcba)
T0S = (0, (1 << 16) - 5, (1 << 32) - 400)


def distinct_values(seed, r):
    rnd = random.Random(seed)
    while True:
        yield rnd.randrange(2, r)


def vm_job(curve, log_n_sub, ops, dummy=4, t0=0, seed=7, chal=CHAL):
    from hekaton_system_amd.cp_groth16 import CURVE_PARAMS
    job = VmJob(curve, log_n_sub, ops, dummy, values=distinct_values(seed, CURVE_PARAMS[curve]["r"]), t0=t0)
    if chal is not None:
        job.set_challenges(chal)
    return job


def bad_rows(job, idx, **override):
    circ = job.make_class(idx)
    return r1cs_bad_rows(*circ.rows(), job.assignment_ints(idx, **override), circ.r)


def _time_pos(job, e):
    """(subcircuit, position) of the time-ordered copy of the entry e (timestamps are unique in an honest job)."""
    for s, st in enumerate(job.time):
        for j, x in enumerate(st):
            if x.i == e.i:
                return s, j
    raise KeyError(e)


def _set_both(job, s, j, **changes):
    """Replace fields of address-ordered entry (s, j) and of its time-ordered copy: the orders stay a permutation."""
    e = job.addr[s][j]
    ts, tj = _time_pos(job, e)
    job.addr[s][j] = dataclasses.replace(e, **changes)
    job.time[ts][tj] = dataclasses.replace(job.time[ts][tj], **changes)


def _find_addr(job, pred, s_min=0):
    """The first address-ordered (s, j) with pred(previous entry or None, entry, next entry or None)."""
    flat = [(s, j) for s in range(job.n) for j in range(len(job.addr[s]))]
    for n, (s, j) in enumerate(flat):
        if s < s_min:
            continue
        prev = job.addr[flat[n - 1][0]][flat[n - 1][1]] if n else None
        nxt = job.addr[flat[n + 1][0]][flat[n + 1][1]] if n + 1 < len(flat) else None
        if pred(prev, job.addr[s][j], nxt):
            return s, j
    raise LookupError


# Each tampering edits job.time / job.addr in place (before set_challenges) and returns (subcircuit, block, pair, rule):
# the subcircuit whose FIRST failing row must lie in `block` - for the `pairs` block in pair `pair` under rule `rule`.
def tamper_read_value(job):
    """1: a read returns a value other than the last write."""
    s, j = _find_addr(job, lambda p, e, n: e.read and p is not None and p.addr == e.addr, s_min=1)
    _set_both(job, s, j, val=(job.addr[s][j].val + 1) % job.r)
    return s, "pairs", j, "read_value"


def tamper_first_read(job):
    """2: the first access of an address turned into a read."""
    s, j = _find_addr(job, lambda p, e, n: p is not None and p.addr != e.addr and e.addr >= 3)
    _set_both(job, s, j, read=True)
    return s, "pairs", j, "first_write"


def tamper_addr_plus_2(job):
    """3: one address raised by 2."""
    s, j = _find_addr(job, lambda p, e, n: p is not None and p.addr == e.addr and e.addr >= 3)
    _set_both(job, s, j, addr=job.addr[s][j].addr + 2)
    return s, "pairs", j, "step"


def tamper_swap(job):
    """4a: two same-address entries swapped in the address order (the timestamp does not increase)."""
    s, j = _find_addr(job, lambda p, e, n: n is not None and e.read and n.read and e.addr == n.addr and e.val == n.val)
    assert j + 1 < len(job.addr[s])
    job.addr[s][j], job.addr[s][j + 1] = job.addr[s][j + 1], job.addr[s][j]
    return s, "pairs", j + 1, "timestamp"


def tamper_equal_ts(job):
    """4b: two same-address entries with equal timestamps."""
    s, j = _find_addr(job, lambda p, e, n: n is not None and e.read and n.read and e.addr == n.addr and e.val == n.val)
    assert j + 1 < len(job.addr[s])
    job.addr[s][j + 1] = dataclasses.replace(job.addr[s][j + 1], i=job.addr[s][j].i)
    return s, "pairs", j + 1, "timestamp"


def tamper_time_repeat(job):
    """5: a time-ordered timestamp repeated."""
    s, j = 1, 3
    job.time[s][j] = dataclasses.replace(job.time[s][j], i=job.time[s][j - 1].i)
    return s, "time_order", None, None


def tamper_no_permutation(job):
    """6: one address-ordered entry replaced so that the orders are no permutation: the last entry of the address order (a
    write nothing reads) gets another value.  Every rule of every pair still holds; only the final evaluations differ."""
    s, j = job.n - 1, len(job.addr[-1]) - 1
    assert not job.addr[s][j].read
    job.addr[s][j] = dataclasses.replace(job.addr[s][j], val=(job.addr[s][j].val + 1) % job.r)
    return s, "last", None, None


TAMPERINGS = [tamper_read_value, tamper_first_read, tamper_addr_plus_2, tamper_swap, tamper_equal_ts, tamper_time_repeat,
              tamper_no_permutation]


def random_ram_job(curve, seed, n_sub=4, k=6, chal=CHAL):
    """A seeded random RAM program over <= 5 addresses 1 .. a (each first written, then read or written at random), cut into
    n_sub subtraces of k entries."""
    rnd = random.Random(seed)
    n_addr = rnd.randrange(1, 6)
    mem, trace = {}, []
    for t in range(n_sub * k):
        fresh = [a for a in range(1, n_addr + 1) if a not in mem]
        if fresh and (not mem or rnd.random() < 0.3):
            a, write = fresh[0], True
        else:
            a, write = rnd.choice(sorted(mem)), rnd.random() < 0.5
        if write:
            mem[a] = rnd.randrange(1 << 64)
        trace.append(RamTranscriptEntry(a, mem[a], t, not write))
    job = RamJob(curve, [trace[i * k:(i + 1) * k] for i in range(n_sub)])
    if chal is not None:
        job.set_challenges(chal)
    return job
