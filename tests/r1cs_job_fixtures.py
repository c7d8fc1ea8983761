"""Shared by tests/test_r1cs_job_cpu.py and tests/test_r1cs_job_gpu.py: partitioned circom circuits built in Python - nothing
is downloaded and the reference tree holds no such files - and the three jobs the tests run.  Not a test module.

A partition is a multiply-and-add chain over its non-borrowed wires 1 .. u + n_owned - 1 (wire order: the constant, the own
wires, the owned ones, the borrowed ones).  Wires 1 and 2 are free inputs; every later wire w is defined by one constraint:

    w % 16 == 5     (x[w-1] + 3 ONE) (x[2] + 2 ONE) = x[w]                         a product, a term on wire 0 in A and in B
    a borrowed wire b still unused:  (x[w-1] + b + 5 ONE) ONE = x[w]                three terms in A
    w % 2 == 0      (2 x[w-1] + x[1] + 7 ONE) ONE = x[w] + x[w-1] + x[1]           three terms in A and in C:  x[w] = x[w-1] + 7
    otherwise       (x[w-1] + x[1] + 7 ONE) ONE = x[w]

so the owned wires, the last of the chain, depend on every free and every borrowed wire.  Every coefficient is a small positive
integer and every value stays below 2^200 (asserted), so the constraints hold over the integers and with them in the scalar
field of either curve: one set of files serves BN254 and BLS12-381.  Every partition goes through `R1CSFile.write` / `.new`,
`write_witness` / `read_witness` and `write_meta` / `read_meta` on its way into a `Partition`."""
import functools
import random

from hekaton_system_amd import circom
from hekaton_system_amd.r1cs_circuit import Partition, PartitionedR1csJob, read_meta, write_meta

CHAL = (0x1234567, 0x7654321)


class Chain:
    """The shape of one partition: n_wires, the ids it owns and the ids it borrows."""

    def __init__(self, n_wires, owned=(), borrowed=()):
        self.n_wires, self.owned, self.borrowed = n_wires, list(owned), list(borrowed)
        self.u = n_wires - len(self.owned) - len(self.borrowed)
        self.last = self.u + len(self.owned) - 1                       # the last non-borrowed wire
        assert self.last >= 2 + len(self.borrowed), "the chain needs a defined wire per borrowed one"
        self.steps = []                                                # (wire, kind, borrowed wire or None)
        pending = list(range(self.last + 1, n_wires))
        for w in range(3, self.last + 1):
            if w % 16 == 5:
                self.steps.append((w, "mul", None))
            elif pending:
                self.steps.append((w, "borrow", pending.pop(0)))
            else:
                self.steps.append((w, "sum3" if w % 2 == 0 else "sum", None))
        assert not pending

    def constraints(self):
        out = []
        for w, kind, b in self.steps:
            if kind == "mul":
                out.append(([(w - 1, 1), (0, 3)], [(2, 1), (0, 2)], [(w, 1)]))
            elif kind == "borrow":
                out.append(([(w - 1, 1), (b, 1), (0, 5)], [(0, 1)], [(w, 1)]))
            elif kind == "sum3":
                out.append(([(w - 1, 2), (1, 1), (0, 7)], [(0, 1)], [(w, 1), (w - 1, 1), (1, 1)]))
            else:
                out.append(([(w - 1, 1), (1, 1), (0, 7)], [(0, 1)], [(w, 1)]))
        return out

    def r1cs(self):
        cons = self.constraints()
        hdr = circom.Header(32, circom.BN254_R_LE, self.n_wires, 0, 0, self.n_wires - 1, self.n_wires, len(cons))
        return circom.R1CSFile(1, hdr, cons, wire_mapping=list(range(self.n_wires)))

    def solve(self, seed, shared):
        """The witness: wires 1 and 2 drawn from `seed`, the borrowed wires read from `shared` (id -> value), the rest
        computed.  Adds its own owned wires to `shared`."""
        rnd = random.Random(seed)
        x = [0] * self.n_wires
        x[0], x[1], x[2] = 1, rnd.randrange(1, 1000), rnd.randrange(1, 4)
        for j, vid in enumerate(self.borrowed):
            x[self.last + 1 + j] = shared[vid]
        for w, kind, b in self.steps:
            if kind == "mul":
                x[w] = (x[w - 1] + 3) * (x[2] + 2)
            elif kind == "borrow":
                x[w] = x[w - 1] + x[b] + 5
            elif kind == "sum3":
                x[w] = x[w - 1] + 7
            else:
                x[w] = x[w - 1] + x[1] + 7
        assert max(x) < 1 << 200
        for i, vid in enumerate(self.owned):
            shared[vid] = x[self.u + i]
        return x


def partition_files(chain, witness):
    """(r1cs bytes, json text, meta text): the three files of one partition."""
    return chain.r1cs().write(), circom.write_witness(witness), write_meta(chain.owned, chain.borrowed)


def make_partition(chain, witness):
    r1cs_b, json_t, meta_t = partition_files(chain, witness)
    owned, borrowed = read_meta(meta_t)
    return Partition(circom.R1CSFile.new(r1cs_b), circom.read_witness(json_t), owned, borrowed)


# the three jobs: name -> (chains, n_txs, distinct witnesses per transaction)
JOBS = {
    # no owned wire: every subcircuit's only entry is the dummy `set`
    "p1t2": ([Chain(6)], 2, False),
    "p2t1": ([Chain(9, owned=[1]), Chain(8, borrowed=[1])], 1, False),
    # portal counts 1, 2, 4, 5; bodies of 66 and 128 columns; id 10 is borrowed by three partitions, from the non-adjacent
    # partition 0 among them; nobody borrows id 40
    "p4t4": ([Chain(67, owned=[10]), Chain(130, owned=[20], borrowed=[10]), Chain(24, owned=[30, 31], borrowed=[10, 20]),
              Chain(21, owned=[40], borrowed=[31, 10, 20, 30])], 4, True),
}


def solve_tx(chains, seed):
    shared = {}
    return [c.solve(seed * 100 + p, shared) for p, c in enumerate(chains)]


@functools.lru_cache(maxsize=None)
def job_parts(name):
    """(partitions, witnesses or None) of a job: built once, never changed."""
    chains, n_txs, distinct = JOBS[name]
    parts = [make_partition(c, w) for c, w in zip(chains, solve_tx(chains, 1))]
    return parts, ([solve_tx(chains, 1 + g) for g in range(n_txs)] if distinct else None)


def make_job(curve, name, chal=CHAL, witnesses="default"):
    chains, n_txs, _ = JOBS[name]
    parts, wits = job_parts(name)
    job = PartitionedR1csJob(curve, parts, n_txs, witnesses=wits if witnesses == "default" else witnesses)
    if chal is not None:
        job.set_challenges(chal)
    return job


def circom_bad_rows(part, wires, r):
    """The imported constraints evaluated directly on a circom witness: the indices of those that fail."""
    dot = lambda terms: sum(c * wires[i] for i, c in terms) % r
    return [k for k, (a, b, c) in enumerate(part.r1cs.constraints) if dot(a) * dot(b) % r != dot(c)]


def tampered(cname, sub, wire, delta=1):
    """The (4, 4) job with one wire of subcircuit `sub`'s witness changed: (job, honest job)."""
    _parts, wits = job_parts("p4t4")
    wits = [[list(w) for w in tx] for tx in wits]
    g, p = divmod(sub, 4)
    wits[g][p][wire] += delta
    return make_job(cname, "p4t4", witnesses=wits), make_job(cname, "p4t4")


def owner_tampering(cname):
    """Subcircuit 5 = partition 1 of transaction 1 owns id 20 (its wire 128), which partitions 2 and 3 borrow."""
    return tampered(cname, 5, 128)
