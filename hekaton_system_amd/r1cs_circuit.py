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
is its own class on `sha_circuit.Tape`, with the stage-0 block, the ROM portal block and the membership block in the columns
and order of `ShaMerkleSubcircuit._program` (k = n_owned + n_borrowed, + 1 for the dummy), so hk_stage0_witness and
hk_stage1_witness write them unchanged, and after them the BODY:

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
from .cp_groth16 import CURVE_PARAMS, FrCodec, MultiStageConstraintSynthesizer
from .sha_circuit import ONE, ShaMerkleSubcircuit, Stage1Device, Tape, poseidon_path_trace
from .transcript import ROM, RomTranscriptEntry, RunningEvaluation, running_evaluations, sort_subtraces_by_addr

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


class R1csSubcircuit(MultiStageConstraintSynthesizer):
    """One proving-key class of a partitioned R1CS job: the partition `part` as the `first` (evals pinned to 1, previous
    entry pinned to padding), the `last` (time eval == addr eval) or a middle subcircuit; depth = log2(number of
    subcircuits); dummy: the job has a single partition, so the subcircuit also sets the dummy wire.  Only the partition's
    shape and constraints enter the class - never its witness."""
    N_INST = 4                                         # ONE, entry_chal, tr_chal, root
    # the Poseidon gadget, the CSR export and the QAP evaluation are the big-merkle class's, unchanged
    _poseidon_crh = ShaMerkleSubcircuit._poseidon_crh
    _poseidon_permute = ShaMerkleSubcircuit._poseidon_permute
    csr = ShaMerkleSubcircuit.csr
    qap_evaluate = ShaMerkleSubcircuit.qap_evaluate
    total_num_stages = ShaMerkleSubcircuit.total_num_stages

    def __init__(self, curve, part, first=False, last=False, depth=1, dummy=False):
        self.curve, self.part, self.first, self.last, self.depth, self.dummy = curve, part, first, last, depth, bool(dummy)
        self.np_ = part.n_owned + part.n_borrowed + int(self.dummy)
        if self.np_ == 0:
            raise ValueError("a partition without a portal has no last entry for its execution leaf")
        assert depth >= 1
        from .poseidon import merkle_params
        self.leaf_cfg, self.node_cfg = merkle_params(curve)
        self.r = CURVE_PARAMS[curve]["r"]
        self.fc = FrCodec(curve)
        self.n0 = 4 * self.np_
        self.blocks = {}
        t = Tape(self.N_INST)
        self._program(t, None)
        self.tape = t
        self.n_c, self.n_wit, self.n_v = t.n_rows, t.n_wit, self.N_INST + t.n_wit
        self._csr = None

    # ---- the program: identical in BUILD and EVAL --------------------------------------------------------
    def _program(self, t, inp):
        """inp (EVAL): dict of per-batch lists, see `witness_batch`."""
        ev = not t.build
        B, r, k, ni, part = t.batch, self.r, self.np_, self.N_INST, self.part
        ENTRY, TR, ROOT = 1, 2, 3
        neg = r - 1
        col = lambda vals: t.alloc_full(vals if ev else None)
        start = [0]

        def block(name):
            if t.build:
                self.blocks[name] = (start[0], t.n_rows)
            start[0] = t.n_rows

        # ---- stage 0: (addr, val) of every time-ordered, then of every address-ordered entry
        time_e = [(col(ev and inp["time"][j][0]), col(ev and inp["time"][j][1])) for j in range(k)]
        addr_e = [(col(ev and inp["addr"][j][0]), col(ev and inp["addr"][j][1])) for j in range(k)]
        assert t.n_wit == self.n0

        # ---- stage 1, the ROM portal block: `ShaMerkleSubcircuit._program`'s columns and rows
        def running(entries, start_vals, key):
            ev_col, cur = col(start_vals), start_vals
            if self.first:
                t.big_row([(1, ev_col)], [(1, ONE)], [(1, ONE)])
            for j, (a_col, v_col) in enumerate(entries):
                if ev:
                    ech, tr = inp["entry_chal"], inp["tr_chal"]
                    e_vals = [(v + ech * a) % r for a, v in zip(inp[key][j][0], inp[key][j][1])]
                    nxt = [c * ((tr - e) % r) % r for c, e in zip(cur, e_vals)]
                else:
                    e_vals = nxt = None
                e_col, n_col = col(e_vals), col(nxt)
                t.big_row([(1, ENTRY)], [(1, a_col)], [(1, e_col), (neg, v_col)])
                t.big_row([(1, ev_col)], [(1, TR), (neg, e_col)], [(1, n_col)])
                ev_col, cur = n_col, nxt
            return ev_col, cur
        t_final, t_vals = running(time_e, inp["time_eval0"] if ev else None, "time")
        a_final, a_vals = running(addr_e, inp["addr_eval0"] if ev else None, "addr")
        if self.last:
            t.big_row([(1, t_final), (neg, a_final)], [(1, ONE)], [])
        prev = (col(ev and inp["prev"][0]), col(ev and inp["prev"][1]))
        if self.first:
            t.big_row([(1, prev[0])], [(1, ONE)], [])
        chain = [prev] + addr_e
        for j in range(1, len(chain)):
            (a0, v0), (a1, v1) = chain[j - 1], chain[j]
            if ev:
                prev_a = inp["prev"][0] if j == 1 else inp["addr"][j - 2][0]
                d = [(x - y) % r for x, y in zip(inp["addr"][j - 1][0], prev_a)]
                inv = [pow(x, -1, r) if x else 0 for x in d]
                same = [0 if x else 1 for x in d]
            else:
                inv = same = None
            inv_c, same_c = col(inv), col(same)
            t.big_row([(1, a1), (neg, a0)], [(1, inv_c)], [(1, ONE), (neg, same_c)])
            t.big_row([(1, same_c)], [(1, a1), (neg, a0)], [])
            t.big_row([(1, ONE), (neg, same_c)], [(1, a1), (neg, a0), (neg, ONE)], [])
            t.big_row([(1, same_c)], [(1, v1), (neg, v0)], [])
        assert ni + t.n_wit == ni + 10 * k + 4
        block("portal")
        # ---- the subcircuit's own execution leaf is in the tree (subcircuit_circuit.rs:233-252)
        self.pos_col0 = ni + t.n_wit
        leaf_lcs = [[(1, t_final)], [(1, a_final)], [(1, addr_e[-1][0])], [(1, addr_e[-1][1])]]
        if ev:
            traces = [poseidon_path_trace(self.leaf_cfg, self.node_cfg,
                                          [t_vals[b], a_vals[b], inp["addr"][-1][0][b], inp["addr"][-1][1][b]],
                                          inp["path_sib"][b], inp["path_idx"][b]) for b in range(B)]
            it = iter(zip(*traces))
        nxt = (lambda: t.alloc_full(list(next(it)))) if ev else (lambda: t.alloc_full(None))
        cur = self._poseidon_crh(t, self.leaf_cfg, leaf_lcs, nxt)
        for _lvl in range(self.depth):
            bit, sib, left = nxt(), nxt(), nxt()
            t.big_row([(1, bit)], [(1, ONE), (neg, bit)], [])
            t.big_row([(1, bit)], [(1, sib), (neg, cur)], [(1, left), (neg, cur)])
            cur = self._poseidon_crh(t, self.node_cfg, [[(1, left)], [(1, sib), (1, cur), (neg, left)]], nxt)
        t.big_row([(1, cur), (neg, ROOT)], [(1, ONE)], [])
        self.pos_cols = ni + t.n_wit - self.pos_col0
        block("membership")
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

    # ---- what the tests and the host mirror of hk_r1cs_check read ------------------------------------------
    def rows(self):
        """(A, B, C) as ark-style rows [(coeff, col)] - what cp_groth16.r1cs_bad_rows takes."""
        big = self.tape.big
        assert [e[0] for e in big] == list(range(self.n_c))
        return [e[1] for e in big], [e[2] for e in big], [e[3] for e in big]

    def block_of(self, row):
        for name, (lo, hi) in self.blocks.items():
            if lo <= row < hi:
                return name
        raise IndexError(row)

    # ---- MultiStageConstraintSynthesizer -------------------------------------------------------------------
    def generate_constraints(self, stage, cs):
        z = [1] + [0] * (self.n_v - 1)                     # setup mode: only the counts matter
        ni = self.N_INST
        cs.initialize_stage()
        if stage == 0:
            cs.witness_assignment.extend(z[ni:ni + self.n0])
        else:
            cs.instance_assignment.extend(z[1:ni])
            cs.witness_assignment.extend(z[ni + self.n0:])
            cs._n_constraints += self.n_c
        cs.finalize_stage()

    # ---- witness generation --------------------------------------------------------------------------------
    def witness_batch(self, inputs):
        """inputs: per-subcircuit dicts (`PartitionedR1csJob.inputs`): entry_chal, tr_chal, root, time / addr (k (addr, val)
        pairs each), prev (a pair), time_eval0, addr_eval0, path (siblings, index), wires (the subcircuit's witness, one int
        per wire; the borrowed wires' values are not read).  Returns the full assignments as lists of ints."""
        B, k, r = len(inputs), self.np_, self.r
        assert all(i["entry_chal"] == inputs[0]["entry_chal"] and i["tr_chal"] == inputs[0]["tr_chal"] for i in inputs)
        inp = dict(entry_chal=inputs[0]["entry_chal"] % r, tr_chal=inputs[0]["tr_chal"] % r)
        for key in ("time", "addr"):
            assert all(len(i[key]) == k for i in inputs)
            inp[key] = [([i[key][j][0] % r for i in inputs], [i[key][j][1] % r for i in inputs]) for j in range(k)]
        inp["prev"] = ([i["prev"][0] % r for i in inputs], [i["prev"][1] % r for i in inputs])
        inp["time_eval0"] = [i["time_eval0"] for i in inputs]
        inp["addr_eval0"] = [i["addr_eval0"] for i in inputs]
        inp["path_sib"] = [i["path"][0] for i in inputs]
        inp["path_idx"] = [i["path"][1] for i in inputs]
        inp["wires"] = [i["wires"] for i in inputs]
        t = Tape(self.N_INST, batch=B)
        self._program(t, inp)
        assert t.n_wit == self.n_wit
        out = []
        for b in range(B):
            z = [0] * self.n_v
            z[:self.N_INST] = [1, inp["entry_chal"], inp["tr_chal"], inputs[b]["root"] % r]
            for c, vals in t.full_records:
                z[c] = int(vals[b]) % r
            out.append(z)
        return out

    def assignment_ints(self, inputs):
        return self.witness_batch(inputs if isinstance(inputs, list) else [inputs])

    def assignment_bytes(self, inputs):
        """Montgomery bytes of the full assignments, (batch, n_v * 32)."""
        return np.stack([self.fc.enc(z) for z in self.assignment_ints(inputs)])

    def stage0_witness_bytes(self, inputs):
        """Montgomery bytes of the stage-0 witnesses (what the class's stage-0 commitment is over), (batch, n0 * 32)."""
        return np.stack([self.fc.enc(z[self.N_INST:self.N_INST + self.n0]) for z in self.assignment_ints(inputs)])


@functools.lru_cache(maxsize=None)
def r1cs_class(curve, part, first, last, depth, dummy):
    """The class's `R1csSubcircuit`, built once per process and partition object (nothing changes in it after BUILD)."""
    return R1csSubcircuit(curve, part, first=first, last=last, depth=depth, dummy=dummy)


# ---------------------------------------------------------------------------------------------------------------------
class PartitionedR1csJob:
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
        self.curve, self.parts, self.P, self.T, self.n, self.depth = curve, list(partitions), P, T, n, n.bit_length() - 1
        self.r = CURVE_PARAMS[curve]["r"]
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
        self.time = []
        for i in range(n):
            g, blk = i // P, self.wit_blocks[i // P if self.tx_stride else 0]
            self.time.append([RomTranscriptEntry(1 + g * self.sets_per_tx + rank, 0 if src == SRC_ZERO else blk[src])
                              for rank, src in self.slots[i % P]])
        self.addr = sort_subtraces_by_addr(self.time)
        self.offsets = np.zeros(n + 1, np.uint32)
        self.offsets[1:] = np.cumsum([len(st) for st in self.time])
        self.chal = self.entry_chal = self.tr_chal = self.root = self.tree = None

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

    def stage0_ints(self, idx):
        """The subcircuit's stage-0 witness: (addr, val) of its time-ordered then of its address-ordered entries."""
        return [x % self.r for e in self.time[idx] + self.addr[idx] for x in (e.addr, e.val)]

    def set_challenges(self, chals, tr_chal=None, ctx=None):
        """chals: (entry_chal, tr_chal) - or entry_chal with tr_chal beside it - or the super commitment they are hashed from
        (`RunningEvaluation.new(ROM, ...)`).  Running evaluations after every subcircuit and the execution tree
        (coordinator.rs:125-174); with ctx (a capi.Context of the job's curve) from one hk_exec_tree call."""
        from .poseidon import ExecTree
        r = self.r
        com = chals if isinstance(chals, (bytes, bytearray)) or hasattr(chals, "serialize_uncompressed") else None
        if com is not None:
            chals = RunningEvaluation.new(ROM, com, r).challenges
        elif tr_chal is not None:
            chals = (chals, tr_chal)
        self.chal = tuple(c % r for c in chals)
        assert len(self.chal) == 2
        self.entry_chal, self.tr_chal = self.chal
        if ctx is not None:
            from .transcript import exec_tree_device
            leaves, self.tree = exec_tree_device(ctx, ROM, self.chal, self.time, self.addr)
        elif com is not None:
            leaves = running_evaluations(ROM, com, r, self.time, self.addr)
        else:
            run, last, leaves = RunningEvaluation(ROM, r, self.chal), RomTranscriptEntry.padding(), []
            for ts, as_ in zip(self.time, self.addr):          # `transcript.running_evaluations` from given challenges
                for te, ae in zip(ts, as_):
                    run.update_time_ordered(te)
                    run.update_addr_ordered(ae)
                    last = ae
                leaves.append((run.copy(), last))
        if ctx is None:
            self.tree = ExecTree(self.curve, [[e.time_ordered_eval, e.addr_ordered_eval, last.addr % r, last.val % r]
                                              for e, last in leaves])
        self.time_eval0 = [1] + [e.time_ordered_eval for e, _ in leaves]
        self.addr_eval0 = [1] + [e.addr_ordered_eval for e, _ in leaves]
        self.root = self.tree.root

    def inputs(self, idx):
        """What the subcircuit's Stage1Request carries (coordinator.rs:569-604), and its witness."""
        pair = lambda e: (e.addr, e.val)
        return dict(entry_chal=self.entry_chal, tr_chal=self.tr_chal, root=self.root, time=[pair(e) for e in self.time[idx]],
                    addr=[pair(e) for e in self.addr[idx]], prev=pair(self.addr[idx - 1][-1]) if idx else (0, 0),
                    time_eval0=self.time_eval0[idx], addr_eval0=self.addr_eval0[idx], path=self.tree.path(idx),
                    wires=self.wires(idx))

    def assignment_ints(self, idx, **override):
        """The subcircuit's full assignment (the host witness); override: inputs to replace (tests)."""
        w = self.inputs(idx)
        w.update(override)
        return self.make_class(idx).assignment_ints(w)[0]

    def assignment_bytes(self, idx):
        return self.make_class(idx).fc.enc(self.assignment_ints(idx))

    def flat(self, which):
        """Montgomery bytes of one flattened trace, (addr, val) per entry: hk_trace_sort's / hk_exec_tree's layout."""
        tr = self.time if which == "time" else self.addr
        return FrCodec(self.curve).enc([x % self.r for st in tr for e in st for x in (e.addr, e.val)])

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


class R1csStage0Device:
    """`witness` (the job's witness blocks), `traces = [time, addr]` as DeviceBuffers, `tables` = `job.tables()`; `rows(members)`
    cuts the stage-0 witnesses of subcircuits of ONE class out of the traces (hk_stage0_witness)."""

    def __init__(self, job, ctx):
        from .capi import DeviceBuffer
        self.job, self.ctx, self.tables, self.traces = job, ctx, job.tables(), []
        self.witness = DeviceBuffer.from_host(ctx, job.witness_bytes())
        try:
            self.traces.append(ctx.r1cs_job_trace(self.tables, self.witness, device_out=True))
            self.traces.append(ctx.trace_sort(2, self.traces[0], int(job.offsets[-1]), device_out=True))
        except Exception:
            self.free()
            raise

    def rows(self, members):
        """DeviceBuffer of len(members) x 4 k Fr: row b = `job.stage0_ints(members[b])`.  The caller frees it."""
        from .capi import DeviceBuffer
        members = np.ascontiguousarray(members, dtype=np.uint32)
        k = len(self.job.time[int(members[0])]) if members.size else 1
        w = DeviceBuffer(self.ctx, max(members.size * 4 * k * self.ctx.fr_bytes, 1))
        try:
            self.ctx.stage0_witness(self.job.offsets, k, self.traces[0], self.traces[1], members, w)
        except Exception:
            w.free()
            raise
        return w

    def free(self):
        for x in self.traces + [self.witness]:
            if x is not None:
                x.free()
        self.traces, self.witness = [], None


class R1csStage1Device:
    """The job's witness, traces and hk_exec_tree's outputs as DeviceBuffers; `fill(circ, members, z)` writes whole
    assignment rows of one class from them (hk_r1cs_job_witness + hk_stage1_witness) and `check(pk, z, members)` tests them
    where they lie (hk_pk_r1cs_check).  `root` is the one value read back."""
    check = Stage1Device.check

    def __init__(self, job, ctx, dev0=None):
        from .capi import DeviceBuffer
        from .poseidon import device_params
        fc = FrCodec(job.curve)
        self.job, self.ctx, self._own0, self.outs, self.params = job, ctx, None, (), None
        try:
            if dev0 is None:
                dev0 = self._own0 = R1csStage0Device(job, ctx)
            self.dev0 = dev0
            consts, n_consts, ld, nd = device_params(job.curve, fc)
            self.params = (DeviceBuffer.from_host(ctx, consts), n_consts, ld, nd)
            self.challenges = fc.enc(list(job.chal))
            self.outs = ctx.exec_tree(self.params, 2, job.offsets, dev0.traces[0], dev0.traces[1], self.challenges,
                                      device_out=True)
        except Exception:
            self.free()
            raise
        self.root = fc.dec(self.outs[4].to_host())[0]

    def fill(self, circ, members, z):
        """Row b of the DeviceBuffer z (len(members) x circ.n_v Fr) <- the assignment of subcircuit members[b], all of class
        `circ`: every column of the row is written by one of the two calls."""
        members = np.ascontiguousarray(members, dtype=np.uint32)
        d = self.dev0
        self.ctx.r1cs_job_witness(d.tables, d.witness, members, circ.n_v, circ.body_col0, z)
        self.ctx.stage1_witness(self.params, circ.np_, self.job.offsets, d.traces[0], d.traces[1], self.challenges, self.outs,
                                members, circ.n_v, (1, circ.N_INST, circ.pos_col0), z)
        return z

    def free(self):
        for x in ([self.params[0]] if self.params else []) + list(self.outs):
            x.free()
        if self._own0 is not None:
            self._own0.free()
            self._own0 = None
        self.outs, self.params = (), None
