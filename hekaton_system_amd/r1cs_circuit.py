"""The partitioned R1CS job: circom subcircuits joined by ROM portals.

The reference's fourth `CircuitWithPortals` (distributed-prover/src/partitioned_r1cs_circuit.rs, behind `setup-r1cs` of
mpi-snark/src/bin/node.rs) proves a circuit of the user's own: a circom R1CS cut into P partitions `<path>.<p>.r1cs` /
`.json` / `.meta` that exchange their shared wires through ROM portals, repeated over T transactions.  Subcircuit i is
partition i % P of transaction g = i // P (:124-126).  A partition's wires are, in order (:127-149): wire 0 the constant 1,
wires 1 .. u - 1 its own (u = n_wires - n_owned - n_borrowed), then its owned portal wires - each `set` under the name
"var{g}_{id}" - then its borrowed ones - each what `get` of that name returns.  With P = 1 every subcircuit also sets
"dummy{i}" to the constant 0 (:168-170).  `SetupRomPortalManager` (portal_manager/rom_portal_manager.rs:34-117) hands out
addresses from 1 in the order of the `set`s, so with O `set`s per transaction

    addr = 1 + g O + rank          rank: the wire's position among the `set`s of its transaction

The SEMANTICS above are the reference's and tests/test_r1cs_job_cpu.py pins them against a name-keyed restatement of the
portal manager.  The constraint LAYOUT is this build's own, as for every gadget set here: `R1csSubcircuit`
is a `portal_circuit.PortalSubcircuit`: the stage-0 block, the ROM portal block and the membership block are the base's
(`rom_portal_block`, `rom_membership_block`; k = n_owned + n_borrowed, + 1 for the dummy), which hk_stage0_witness and
hk_stage1_witness write, and after them the BODY:

    body            (u - 1) + n_owned columns: wires 1 .. u + n_owned - 1 in wire order (hk_r1cs_job_witness writes them)
    rows            one per owned wire: wire = the `val` column of its time-ordered entry (`pm.set` -> `enforce_equal`,
                    rom_portal_manager.rs:177-181); the dummy's: its `val` column = 0; then one per imported constraint, terms
                    remapped, terms on wire 0 folded into ONE with their coefficient (`make_lc`, :151-159)

Borrowed wire j IS the `val` column of time-ordered entry n_owned + j and has no column of its own.  Time order inside a
subcircuit: every owned `set`, every borrowed `get`, the dummy `set`.
"""
import functools
import re

import numpy as np

from .circom import R1CSFile, read_witness
from . import capi
from .cp_groth16 import FrCodec
from .portal_circuit import ONE, PortalJob, PortalStage0Device, PortalStage1Device, PortalSubcircuit
from .transcript import RomTranscriptEntry

SRC_ZERO = 0xFFFFFFFF                                  # include/hekaton.h HK_R1CS_SRC_ZERO
_USIZE = re.compile(r"\+?[0-9]+\Z")


def _lines(text):
    """`BufRead::lines`: split on "\\n", one trailing "\\r" dropped, no empty last line after a final newline."""
    out = text.split("\n")
    if out and out[-1] == "":
        out.pop()
    return [l[:-1] if l.endswith("\r") else l for l in out]


def read_meta(text):
    """A `.meta` file as partitioned_r1cs_circuit.rs:77-90 reads it: the first line is split on single spaces and the tokens
    that do not parse as unsigned integers are dropped; integer [1] is the number of owned portals; every later line is one
    variable id, the first n_owned of them owned, the rest borrowed.  Returns (owned, borrowed).  ValueError where the
    reference panics: no first line, fewer than two integers on it, a later line that is no integer, fewer ids than owned."""
    lines = _lines(text)
    if not lines:
        raise ValueError(".meta: no first line")
    ints = [int(tok) for tok in lines[0].split(" ") if _USIZE.match(tok) and int(tok) < 1 << 64]
    if len(ints) < 2:
        raise ValueError(".meta: the first line holds %d integers, the owned count is the second" % len(ints))
    ids = []
    for l in lines[1:]:
        if not _USIZE.match(l) or int(l) >= 1 << 64:
            raise ValueError(".meta: %r is no variable id" % l)
        ids.append(int(l))
    if ints[1] > len(ids):
        raise ValueError(".meta: %d owned portals, %d ids" % (ints[1], len(ids)))
    return ids[:ints[1]], ids[ints[1]:]


def write_meta(owned, borrowed):
    """The text `read_meta` reads back.  The reference only ever reads integer [1] of the first line; what stands in [0] and
    [2] is THIS PROJECT'S choice: the number of shared wires and the number of borrowed ones."""
    return "\n".join(["%d %d %d" % (len(owned) + len(borrowed), len(owned), len(borrowed))]
                     + ["%d" % v for v in list(owned) + list(borrowed)]) + "\n"


class Partition:
    """One partition: its `circom.R1CSFile`, its witness (one int per wire) and its (owned, borrowed) variable ids."""

    def __init__(self, r1cs, witness, owned, borrowed):
        self.r1cs, self.witness, self.owned, self.borrowed = r1cs, [int(v) for v in witness], list(owned), list(borrowed)
        self.n_wires = r1cs.header.n_wires
        self.n_owned, self.n_borrowed = len(self.owned), len(self.borrowed)
        if self.n_wires < 1 + self.n_owned + self.n_borrowed:
            raise ValueError("%d wires cannot hold the constant, %d owned and %d borrowed portals"
                             % (self.n_wires, self.n_owned, self.n_borrowed))
        if len(self.witness) != self.n_wires:
            raise ValueError("a witness of %d values for %d wires" % (len(self.witness), self.n_wires))
        self.u = self.n_wires - self.n_owned - self.n_borrowed
        self.body_len = self.u - 1 + self.n_owned

    @classmethod
    def load(cls, file_path, p):
        """`<file_path>.<p>.r1cs`, `.json` and `.meta`, as `PartitionedR1CSCircuit::new` opens them (:66-92)."""
        with open("%s.%d.r1cs" % (file_path, p), "rb") as f:
            r1cs = R1CSFile.new(f.read())
        with open("%s.%d.json" % (file_path, p)) as f:
            witness = read_witness(f.read())
        with open("%s.%d.meta" % (file_path, p)) as f:
            owned, borrowed = read_meta(f.read())
        return cls(r1cs, witness, owned, borrowed)

    def with_witness(self, witness):
        return Partition(self.r1cs, witness, self.owned, self.borrowed)


class R1csSubcircuit(PortalSubcircuit):
    """One proving-key class of a partitioned R1CS job: the partition `part` as the `first` (evals pinned to 1, previous
    entry pinned to padding), the `last` (time eval == addr eval) or a middle subcircuit; depth = log2(number of
    subcircuits); dummy: the job has a single partition, so the subcircuit also sets the dummy wire.  Only the partition's
    shape and constraints enter the class - never its witness."""

    def __init__(self, curve, part, first=False, last=False, depth=1, dummy=False):
        self.part, self.first, self.last, self.depth, self.dummy = part, first, last, depth, bool(dummy)
        self.np_ = part.n_owned + part.n_borrowed + int(self.dummy)
        if self.np_ == 0:
            raise ValueError("a partition without a portal has no last entry for its execution leaf")
        assert depth >= 1
        self.blocks = {}
        self._build(curve, 4 * self.np_)

    # ---- the program: identical in BUILD and EVAL --------------------------------------------------------
    def _program(self, t, inp):
        """inp (EVAL): dict of per-batch lists, see `_batch_inputs`."""
        ev = not t.build
        r, k, ni, part = self.r, self.np_, self.N_INST, self.part
        col = lambda vals: t.alloc_full(vals if ev else None)
        block = self._block_recorder(t)
        portal = self.rom_portal_block(t, inp)
        block("portal")
        self.rom_membership_block(t, inp, portal)
        block("membership")
        time_e = portal[0]
        # ---- the body: wires 1 .. u + n_owned - 1 in wire order
        self.body_col0 = ni + t.n_wit
        wire_col = [ONE] + [col(ev and [w[x] % r for w in inp["wires"]]) for x in range(1, part.u + part.n_owned)]
        wire_col += [time_e[part.n_owned + j][1] for j in range(part.n_borrowed)]        # what `pm.get` returns
        assert ni + t.n_wit == self.body_col0 + part.body_len and len(wire_col) == part.n_wires
        for i in range(part.n_owned):                                                    # `pm.set`: enforce_equal
            t.big_row([(1, wire_col[part.u + i])], [(1, ONE)], [(1, time_e[i][1])])
        block("owned")
        if self.dummy:                                                                   # the constant 0 == the trace's value
            t.big_row([(1, time_e[k - 1][1])], [(1, ONE)], [])
        block("dummy")
        lc = lambda terms: [(coeff % r, wire_col[idx]) for idx, coeff in terms]           # wire 0: coefficient on ONE
        for a, b, c in part.r1cs.constraints:
            t.big_row(lc(a), lc(b), lc(c))
        block("constraints")

    def _batch_inputs(self, inputs):
        """inputs: per-subcircuit dicts (`PartitionedR1csJob.inputs`): what `rom_inputs` takes, and wires (the subcircuit's
        witness, one int per wire; the borrowed wires' values are not read)."""
        inp = super()._batch_inputs(inputs)
        inp["wires"] = [i["wires"] for i in inputs]
        return inp


@functools.lru_cache(maxsize=None)
def r1cs_class(curve, part, first, last, depth, dummy):
    """The class's `R1csSubcircuit`, built once per process and partition object (nothing changes in it after BUILD)."""
    return R1csSubcircuit(curve, part, first=first, last=last, depth=depth, dummy=dummy)


# ---------------------------------------------------------------------------------------------------------------------
class PartitionedR1csJob(PortalJob):
    """A whole partitioned R1CS job: N = P T subcircuits, subcircuit i = partition i % P of transaction i // P; the
    addresses `SetupRomPortalManager` hands out, the time-ordered trace (`get_portal_subtraces`, :182-220), its address
    order and - once the round's challenges are in - the running evaluations, the execution tree and every subcircuit's
    inputs.  witnesses: None - every transaction uses the partitions' own witnesses, as the reference (:104, 124) - or
    witnesses[g][p], one list of ints per wire, so that transactions differ.  A borrower's own value for a borrowed wire is
    never read: the trace carries the owner's.  ValueError: N no power of two >= 2 (hk_exec_tree's domain); a partition
    without any portal; an id owned twice in a transaction (the reference: "cannot set portal wire more than once"); a
    borrowed id that neither an earlier partition nor the borrower itself owns ("cannot get portal wire" - the reference's
    `get`s come after the subcircuit's own `set`s, so it finds those too)."""

    def __init__(self, curve, partitions, n_txs, witnesses=None):
        P, T = len(partitions), int(n_txs)
        n = P * T
        if n < 2 or n & (n - 1):
            raise ValueError("%d partitions x %d transactions = %d subcircuits: not a power of two >= 2" % (P, T, n))
        self._set_shape(curve, n)
        self.parts, self.P, self.T = list(partitions), P, T
        self.dummy = P == 1
        # one transaction's witness block: the P witnesses back to back
        self.wit_offsets = np.zeros(P + 1, np.uint32)
        self.wit_offsets[1:] = np.cumsum([p.n_wires for p in self.parts])
        self.tx_len = int(self.wit_offsets[-1])
        # the `set`s of a transaction in order, and per partition its slots in time order as (rank, src)
        owner, self.slots = {}, []
        for p, part in enumerate(self.parts):
            if part.n_owned + part.n_borrowed + int(self.dummy) == 0:
                raise ValueError("partition %d has no portal: no last entry for its execution leaf" % p)
            for i, vid in enumerate(part.owned):
                if vid in owner:
                    raise ValueError("cannot set portal wire more than once; wire 'var_%d' (partition %d)" % (vid, p))
                owner[vid] = (len(owner), int(self.wit_offsets[p]) + part.u + i)
            sl = [owner[vid] for vid in part.owned]
            for vid in part.borrowed:
                if vid not in owner:
                    raise ValueError("cannot get portal wire 'var_%d' (partition %d)" % (vid, p))
                sl.append(owner[vid])
            if self.dummy:
                sl.append((part.n_owned, SRC_ZERO))
            self.slots.append(sl)
        self.sets_per_tx = len(owner) + int(self.dummy)
        if witnesses is None:
            self.wit_blocks, self.tx_stride = [[v % self.r for part in self.parts for v in part.witness]], 0
        else:
            if len(witnesses) != T or any(len(w) != P for w in witnesses):
                raise ValueError("witnesses is witnesses[transaction][partition]")
            for w in witnesses:
                if [len(x) for x in w] != [p.n_wires for p in self.parts]:
                    raise ValueError("a witness holds one value per wire of its partition")
            self.wit_blocks, self.tx_stride = [[int(v) % self.r for x in w for v in x] for w in witnesses], self.tx_len
        time = []
        for i in range(n):
            g, blk = i // P, self.wit_blocks[i // P if self.tx_stride else 0]
            time.append([RomTranscriptEntry(1 + g * self.sets_per_tx + rank, 0 if src == SRC_ZERO else blk[src])
                         for rank, src in self.slots[i % P]])
        self._set_traces(time)

    @classmethod
    def load(cls, curve, file_path, n_partitions, n_txs):
        """The job of `PartitionedR1CSCircuitParams { num_subcircuits, num_txs, file_path }`."""
        return cls(curve, [Partition.load(file_path, p) for p in range(n_partitions)], n_txs)

    def wires(self, idx):
        """The witness of subcircuit idx, one int per wire."""
        p, blk = idx % self.P, self.wit_blocks[idx // self.P if self.tx_stride else 0]
        return blk[int(self.wit_offsets[p]):int(self.wit_offsets[p + 1])]

    def class_of(self, idx):
        """(partition, first, last): the proving-key class a subcircuit needs."""
        return idx % self.P, idx == 0, idx == self.n - 1

    def make_class(self, idx):
        p, first, last = self.class_of(idx)
        return r1cs_class(self.curve, self.parts[p], first, last, self.depth, self.dummy)

    def inputs(self, idx):
        """The common inputs (`PortalJob.inputs`), and the subcircuit's witness."""
        return dict(super().inputs(idx), wires=self.wires(idx))

    def witness_bytes(self):
        """Montgomery bytes of the witness blocks, one per transaction (or the one every transaction shares): what
        hk_r1cs_job_trace / hk_r1cs_job_witness read as `witness_mont`."""
        return FrCodec(self.curve).enc([v for blk in self.wit_blocks for v in blk])

    def tables(self):
        """The job as hk_r1cs_job_desc states it (`Context.r1cs_job_trace` / `r1cs_job_witness` take this dict)."""
        so = np.zeros(self.P + 1, np.uint32)
        so[1:] = np.cumsum([len(sl) for sl in self.slots])
        flat = [x for sl in self.slots for x in sl]
        return dict(n_parts=self.P, n_txs=self.T, slot_offsets=so, slot_rank=np.array([x[0] for x in flat], np.uint32),
                    slot_src=np.array([x[1] for x in flat], np.uint32), sets_per_tx=self.sets_per_tx, tx_len=self.tx_len,
                    tx_stride=self.tx_stride, wit_offsets=self.wit_offsets.copy(),
                    body_len=np.array([p.body_len for p in self.parts], np.uint32))

    def stage0_device(self, ctx):
        """The job's stage-0 side on the device: the witness blocks uploaded once, the time-ordered trace gathered from
        them (hk_r1cs_job_trace), the address-ordered one sorted from it (hk_trace_sort).  Returns an `R1csStage0Device`."""
        return R1csStage0Device(self, ctx)

    def stage1_device(self, ctx, dev0=None):
        """The job's stage-1 witness on the device: hk_exec_tree over the two traces, then per class hk_r1cs_job_witness +
        hk_stage1_witness.  Needs `chal` (set_challenges, or assign it).  dev0: the `stage0_device(ctx)` whose witness and
        traces to read instead of uploading and gathering again.  Returns an `R1csStage1Device`."""
        assert self.chal is not None, "stage1_device needs the round's challenges"
        return R1csStage1Device(self, ctx, dev0=dev0)


class R1csStage0Device(PortalStage0Device):
    """`witness` (the job's witness blocks, uploaded once), `traces = [time, addr]` - the time-ordered one gathered from the
    witness (hk_r1cs_job_trace) - and `tables` = `job.tables()`."""

    def _time_trace(self):
        self.tables = self.job.tables()
        self.witness = self._own(capi.DeviceBuffer.from_host(self.ctx, self.job.witness_bytes()))
        return self._own(self.ctx.r1cs_job_trace(self.tables, self.witness, device_out=True))


class R1csStage1Device(PortalStage1Device):
    """The job's witness, traces and hk_exec_tree's outputs as DeviceBuffers; `fill(circ, members, z)` writes whole
    assignment rows of one class from them (hk_r1cs_job_witness + hk_stage1_witness) and `check(pk, z, members)` tests them
    where they lie (hk_pk_r1cs_check).  dev0: the `R1csStage0Device` to read instead of making one here."""

    def __init__(self, job, ctx, dev0=None):
        super().__init__(job, ctx, job.chal, dev0=dev0)

    def _traces(self, dev0=None):
        self.dev0 = dev0 if dev0 is not None else self._own(R1csStage0Device(self.job, self.ctx))
        return self.dev0.traces

    def fill(self, circ, members, z):
        """Row b of the DeviceBuffer z (len(members) x circ.n_v Fr) <- the assignment of subcircuit members[b], all of class
        `circ`: every column of the row is written by one of the two calls."""
        members = np.ascontiguousarray(members, dtype=np.uint32)
        self.ctx.r1cs_job_witness(self.dev0.tables, self.dev0.witness, members, circ.n_v, circ.body_col0, z)
        self._stage1_witness(circ, members, z)
        return z
