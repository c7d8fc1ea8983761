"""The RAM portal subcircuit and the reference's virtual-machine job on it.

The reference's third circuit family (distributed-prover/src/vm/, `MEM_TYPE = Ram`) reads and WRITES its portal memory: an
entry is (addr, val, timestamp, read) (transcript/ram_transcript.rs:260-390), the address order is sorted by (addr,
timestamp), and the prover-side portal manager (portal_manager/ram_portal_manager.rs:150-230) checks, over consecutive
address-ordered entries: same address or exactly one larger; one larger -> a write; same address and read -> same value; same
address -> larger timestamp; and over consecutive time-ordered entries: next timestamp = this one + 1.  The gadget crates
(ark-r1cs-std `UInt32`, `FpVar`) are third-party and absent, so the constraint LAYOUT is this build's own (parity unpinned,
DESIGN section 3); the FUNCTION is pinned by tests/test_vm_circuit_cpu.py.

One program, two interpreters, on `sha_circuit.Tape` as `ShaMerkleSubcircuit._program`: BUILD records the rows, EVAL emits
the assignment.  Instance: ONE, entry_chal_1..3, tr_chal, root (N_INST = 6).  An ENTRY takes 35 columns: val, addr,
timestamp bit 0 .. 31 (little-endian), read.  With k entries per order, the witness columns in order (the device calls
hk_ram_stage0_witness / hk_ram_stage1_witness write the same order; csrc/ram_witness.cuh restates it):

    stage 0          70 k            the k time-ordered entries, then the k address-ordered ones; timestamp and read bits boolean
    stage 1, portal block  43 k + 37
        35                            the previous leaf's last address-ordered entry (zero when `first`)
        1 + 4 k                       time chain: the start evaluation (1 when `first`), then per entry p1 = c1 addr, p2 = c2 ts,
                                      e = val + p1 + p2 + c3 read, cur <- cur (tr_chal - e); ts = the combination of its bit columns
        1 + 4 k                       address chain, the same
        35 k                          per consecutive pair of [previous] + address-ordered entries, d = addr' - addr:
                                      inv, same, sr, delta_0 .. delta_31
    stage 1, membership block         Poseidon CRH over the six leaf fields, then the path (sha_circuit.poseidon_path_trace)
    stage 1, dummy products  3 n      (12, 12, 144) triples, one row each: the VM's `dummy_constraint_num / 2` products

e needs three products of a challenge and a witness, and one R1CS row holds one: p1 and p2 carry the other two.

`RamSubcircuit.blocks` names the row range of every rule (recorded at BUILD) - the tests assert which one a tampering breaks.
"""
import functools

import numpy as np

from .cp_groth16 import CURVE_PARAMS, FrCodec, MultiStageConstraintSynthesizer
from .sha_circuit import ONE, ShaMerkleSubcircuit, Tape, poseidon_path_trace
from .transcript import RAM, RamTranscriptEntry, RunningEvaluation, sort_subtraces_by_addr

REGISTER_NUM = 16                  # vm/mod.rs
ENTRY_COLS = 35                    # val, addr, 32 timestamp bits, read


def vm_subtraces(log_n_sub, ops_per_chunk, values=None, t0=0):
    """`VirtualMachine::get_portal_subtraces` (vm/vm_constraints.rs:29-85): the time-ordered subtraces as lists of
    `RamTranscriptEntry`.  Subcircuit 0 sets the 16 registers, then per operation `set register 1; get; get`; every later
    one gets the 16, runs the same operations, then sets the 16.  `register i` gets address 1 + i (addresses are handed out
    from 1 in order of first use), one global timestamp counts every access from t0.  values: an iterator (or list) of what
    each `set` writes, in order (default: 1 every time, as the reference); a `get` returns the last value set."""
    vals = iter(values) if values is not None else None
    mem, clock, out = {}, [t0], []

    def access(reg, write):
        if write:
            mem[reg] = next(vals) if vals is not None else 1
        e = RamTranscriptEntry(1 + reg, mem[reg], clock[0], not write)
        clock[0] += 1
        return e
    for idx in range(1 << log_n_sub):
        st = []
        st += [access(i, idx == 0) for i in range(REGISTER_NUM)]
        for _ in range(ops_per_chunk):
            st += [access(1, True), access(1, False), access(1, False)]
        if idx:
            st += [access(i, True) for i in range(REGISTER_NUM)]
        out.append(st)
    return out


class _Entry:
    """The 35 columns of one allocated entry and, in EVAL mode, the entries they hold over the batch."""
    __slots__ = ("val", "addr", "bits", "read", "es")

    def __init__(self, val, addr, bits, read, es):
        self.val, self.addr, self.bits, self.read, self.es = val, addr, bits, read, es

    def ts(self, sign=1):
        return [(sign * (1 << j), c) for j, c in enumerate(self.bits)]


class RamSubcircuit(MultiStageConstraintSynthesizer):
    """One proving-key class of a RAM job: a subcircuit that owns `n_portals` entries in each order.  `first` marks
    subcircuit 0 (evals pinned to 1, previous entry pinned to padding), `last` the final one (time eval == addr eval);
    depth = log2(number of subcircuits); dummy_products: the (12, 12, 144) triples after the membership block."""
    N_INST = 6
    # the Poseidon gadget, the CSR export and the QAP evaluation are the big-merkle class's, unchanged
    _poseidon_crh = ShaMerkleSubcircuit._poseidon_crh
    _poseidon_permute = ShaMerkleSubcircuit._poseidon_permute
    csr = ShaMerkleSubcircuit.csr
    qap_evaluate = ShaMerkleSubcircuit.qap_evaluate
    total_num_stages = ShaMerkleSubcircuit.total_num_stages

    def __init__(self, curve, n_portals, first=False, last=False, depth=3, dummy_products=0):
        assert n_portals >= 1 and depth >= 1
        self.curve, self.np_, self.first, self.last, self.depth = curve, n_portals, first, last, depth
        self.dummy_products = dummy_products
        from .poseidon import merkle_params
        self.leaf_cfg, self.node_cfg = merkle_params(curve)
        self.r = CURVE_PARAMS[curve]["r"]
        self.fc = FrCodec(curve)
        self.n0 = 2 * ENTRY_COLS * n_portals
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
        B, r, k, ni = t.batch, self.r, self.np_, self.N_INST
        C1, C2, C3, TR, ROOT = 1, 2, 3, 4, 5
        neg = r - 1
        col = lambda vals: t.alloc_full(vals if ev else None)
        start = [0]

        def block(name):
            if t.build:
                self.blocks[name] = (start[0], t.n_rows)
            start[0] = t.n_rows

        def entry(es):
            val = col(ev and [e.val % r for e in es])
            addr = col(ev and [e.addr % r for e in es])
            bits = [col(ev and [(e.i >> j) & 1 for e in es]) for j in range(32)]
            read = col(ev and [int(e.read) % r for e in es])
            return _Entry(val, addr, bits, read, es)

        def boolean(e):
            for c in e.bits + [e.read]:
                t.big_row([(1, c)], [(1, ONE), (neg, c)], [])

        # ---- stage 0
        time_e = [entry(inp["time"][j] if ev else None) for j in range(k)]
        addr_e = [entry(inp["addr"][j] if ev else None) for j in range(k)]
        assert t.n_wit == self.n0
        for e in time_e + addr_e:
            boolean(e)
        block("stage0_boolean")
        # ---- stage 1: the previous leaf's last address-ordered entry (subcircuit_circuit.rs:167, 199-216)
        self.col0 = ni + t.n_wit
        prev = entry(inp["prev"] if ev else None)
        if self.first:
            for c in [prev.val, prev.addr] + prev.bits + [prev.read]:
                t.big_row([(1, c)], [(1, ONE)], [])
        else:
            boolean(prev)
        block("prev")

        # running evaluations (ram_transcript.rs:101-135): eval' = eval (tr_chal - (val + c1 addr + c2 ts + c3 read))
        def running(entries, start_vals):
            cur_col, cur = col(start_vals), start_vals
            if self.first:
                t.big_row([(1, cur_col)], [(1, ONE)], [(1, ONE)])
            for e in entries:
                if ev:
                    c1, c2, c3, tr = inp["chal"]
                    p1 = [c1 * (x.addr % r) % r for x in e.es]
                    p2 = [c2 * (x.i % r) % r for x in e.es]
                    ev_ = [(x.val + a + b + c3 * int(x.read)) % r for x, a, b in zip(e.es, p1, p2)]
                    cur = [c * ((tr - x) % r) % r for c, x in zip(cur, ev_)]
                else:
                    p1 = p2 = ev_ = None
                p1_c, p2_c, e_c, n_c = col(p1), col(p2), col(ev_), col(cur)
                t.big_row([(1, C1)], [(1, e.addr)], [(1, p1_c)])
                t.big_row([(1, C2)], e.ts(), [(1, p2_c)])
                t.big_row([(1, C3)], [(1, e.read)], [(1, e_c), (neg, e.val), (neg, p1_c), (neg, p2_c)])
                t.big_row([(1, cur_col)], [(1, TR), (neg, e_c)], [(1, n_c)])
                cur_col = n_c
            return cur_col, cur
        t_final, t_vals = running(time_e, inp["time_eval0"] if ev else None)
        block("time_chain")
        a_final, a_vals = running(addr_e, inp["addr_eval0"] if ev else None)
        block("addr_chain")
        # the address order (ram_portal_manager.rs:170-215), every consecutive pair of [previous] + slice - pair 0 joins
        # the previous subcircuit's last entry to this one's first, which the reference's `get` never looks at
        chain = [prev] + addr_e
        for j in range(k):
            p, q = chain[j], chain[j + 1]
            if ev:
                d = [(y.addr - x.addr) % r for x, y in zip(p.es, q.es)]
                same = [0 if x else 1 for x in d]
                inv = [pow(x, -1, r) if x else 0 for x in d]
                sr = [s * int(y.read) % r for s, y in zip(same, q.es)]
                delta = [((y.i - x.i - 1) & 0xffffffff) if s else 0 for s, x, y in zip(same, p.es, q.es)]
            else:
                inv = same = sr = delta = None
            inv_c, same_c, sr_c = col(inv), col(same), col(sr)
            dl = [col(ev and [(x >> b) & 1 for x in delta]) for b in range(32)]
            d_lc = [(1, q.addr), (neg, p.addr)]
            not_same = [(1, ONE), (neg, same_c)]
            t.big_row(d_lc, [(1, inv_c)], not_same)                              # same = [d == 0] ...
            t.big_row([(1, same_c)], d_lc, [])
            t.big_row(not_same, d_lc + [(neg, ONE)], [])                         # another address: exactly one larger
            t.big_row(not_same, [(1, q.read)], [])                               # ... and its first access is a write
            t.big_row([(1, same_c)], [(1, q.read)], [(1, sr_c)])
            t.big_row([(1, sr_c)], [(1, q.val), (neg, p.val)], [])               # a read returns the last value
            for c in dl:
                t.big_row([(1, c)], [(1, ONE), (neg, c)], [])
            # the same address: a larger timestamp, ts' - ts - 1 = sum 2^b delta_b in [0, 2^32)
            t.big_row([(1, same_c)], q.ts() + p.ts(-1 % r) + [(neg, ONE)] + [(-(1 << b) % r, c) for b, c in enumerate(dl)], [])
        block("pairs")
        self.pair_rows = 7 + 32
        # the time order (ram_portal_manager.rs:217-227): next timestamp = this one + 1
        for j in range(1, k):
            t.big_row(time_e[j].ts() + time_e[j - 1].ts(-1 % r) + [(neg, ONE)], [(1, ONE)], [])
        block("time_order")
        if self.last:
            t.big_row([(1, t_final), (neg, a_final)], [(1, ONE)], [])
        block("last")
        assert ni + t.n_wit == self.col0 + 43 * k + 37
        # ---- the subcircuit's own execution leaf is in the tree (subcircuit_circuit.rs:233-260)
        self.pos_col0 = ni + t.n_wit
        le = addr_e[-1]
        leaf_lcs = [[(1, t_final)], [(1, a_final)], [(1, le.addr)], [(1, le.val)], le.ts(), [(1, le.read)]]
        if ev:
            traces = []
            for b in range(B):
                x = le.es[b]
                leaf = [t_vals[b], a_vals[b], x.addr % r, x.val % r, x.i % r, int(x.read) % r]
                traces.append(poseidon_path_trace(self.leaf_cfg, self.node_cfg, leaf, inp["path_sib"][b], inp["path_idx"][b]))
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
        # ---- the VM's dummy products (vm_constraints.rs:186-190): the same in every subcircuit of the class
        self.dummy_col0 = ni + t.n_wit
        for _ in range(self.dummy_products):
            a, b, c = col(ev and [12] * B), col(ev and [12] * B), col(ev and [144] * B)
            t.big_row([(1, a)], [(1, b)], [(1, c)])
        block("dummy")

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

    def pair_rule_of(self, row):
        """(pair j, rule) of a row of the `pairs` block: rule one of same, step, first_write, sr, read_value, delta_boolean,
        timestamp."""
        lo, hi = self.blocks["pairs"]
        assert lo <= row < hi
        j, q = divmod(row - lo, self.pair_rows)
        names = ["same", "same", "step", "first_write", "sr", "read_value"] + ["delta_boolean"] * 32 + ["timestamp"]
        return j, names[q]

    def template_ints(self):
        """The class's constant row: column 0 and the dummy products filled, every other column 0."""
        z = [0] * self.n_v
        z[ONE] = 1
        for j in range(self.dummy_products):
            z[self.dummy_col0 + 3 * j:self.dummy_col0 + 3 * j + 3] = [12, 12, 144]
        return z

    # ---- MultiStageConstraintSynthesizer -------------------------------------------------------------------
    def generate_constraints(self, stage, cs):
        z = self.template_ints()                           # setup mode: only the counts matter
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
        """inputs: per-subcircuit dicts (`RamJob.inputs`): chal (4 ints), root, time / addr (k entries each), prev (an entry),
        time_eval0, addr_eval0, path (siblings, index).  Returns the full assignments as lists of ints."""
        B, k = len(inputs), self.np_
        assert all(i["chal"] == inputs[0]["chal"] for i in inputs)
        inp = dict(chal=inputs[0]["chal"])
        for key in ("time", "addr"):
            assert all(len(i[key]) == k for i in inputs)
            inp[key] = [[i[key][j] for i in inputs] for j in range(k)]
        inp["prev"] = [i["prev"] for i in inputs]
        inp["time_eval0"] = [i["time_eval0"] for i in inputs]
        inp["addr_eval0"] = [i["addr_eval0"] for i in inputs]
        inp["path_sib"] = [i["path"][0] for i in inputs]
        inp["path_idx"] = [i["path"][1] for i in inputs]
        t = Tape(self.N_INST, batch=B)
        self._program(t, inp)
        assert t.n_wit == self.n_wit
        out = []
        for b in range(B):
            z = [0] * self.n_v
            z[:self.N_INST] = [1] + [c % self.r for c in inputs[b]["chal"]] + [inputs[b]["root"] % self.r]
            for c, vals in t.full_records:
                z[c] = int(vals[b]) % self.r
            out.append(z)
        return out

    def assignment_ints(self, inputs):
        return self.witness_batch(inputs if isinstance(inputs, list) else [inputs])

    def assignment_bytes(self, inputs):
        """Montgomery bytes of the full assignments, (batch, n_v * 32)."""
        zs = self.assignment_ints(inputs)
        return np.stack([self.fc.enc(z) for z in zs])


@functools.lru_cache(maxsize=None)
def ram_class(curve, n_portals, first, last, depth, dummy_products):
    """The class's `RamSubcircuit`, built once per process (nothing changes in it after BUILD)."""
    return RamSubcircuit(curve, n_portals, first=first, last=last, depth=depth, dummy_products=dummy_products)


# ---------------------------------------------------------------------------------------------------------------------
class RamJob:
    """A whole RAM job from its time-ordered subtraces (lists of `RamTranscriptEntry`): the address order
    (coordinator.rs:92-123), the slices each subcircuit commits to in stage 0, and - once the round's four challenges are
    in - the running evaluations, the execution tree and every subcircuit's inputs.  A class is (entries owned, first,
    last); `time` / `addr` may be edited in place before `set_challenges` (the tests tamper with them)."""

    def __init__(self, curve, time_subtraces, dummy_products=0):
        n = len(time_subtraces)
        assert n >= 2 and n & (n - 1) == 0 and all(len(st) for st in time_subtraces)
        self.curve, self.n, self.depth = curve, n, n.bit_length() - 1
        self.r = CURVE_PARAMS[curve]["r"]
        self.dummy_products = dummy_products
        self.time = [list(st) for st in time_subtraces]
        self.addr = sort_subtraces_by_addr(self.time)
        self.offsets = np.zeros(n + 1, np.uint32)
        self.offsets[1:] = np.cumsum([len(st) for st in self.time])
        self.chal = self.root = self.tree = None

    def class_of(self, idx):
        """(entries owned, first, last): the proving-key class a subcircuit needs."""
        return len(self.time[idx]), idx == 0, idx == self.n - 1

    def make_class(self, idx):
        k, first, last = self.class_of(idx)
        return ram_class(self.curve, k, first, last, self.depth, self.dummy_products)

    def stage0_ints(self, idx):
        """The subcircuit's stage-0 witness: 35 columns per entry, its time-ordered then its address-ordered entries."""
        out = []
        for e in self.time[idx] + self.addr[idx]:
            out += [e.val % self.r, e.addr % self.r] + [(e.i >> j) & 1 for j in range(32)] + [int(e.read) % self.r]
        return out

    def set_challenges(self, chals, ctx=None):
        """chals: (entry_chal_1, entry_chal_2, entry_chal_3, tr_chal), or the super commitment they are hashed from
        (`RunningEvaluation.new(RAM, ...)`).  Running evaluations after every subcircuit and the execution tree
        (coordinator.rs:125-174); with ctx (a capi.Context of the job's curve) from one hk_exec_tree call."""
        from .poseidon import ExecTree
        r = self.r
        if isinstance(chals, (bytes, bytearray)) or hasattr(chals, "serialize_uncompressed"):
            chals = RunningEvaluation.new(RAM, chals, r).challenges
        self.chal = tuple(c % r for c in chals)
        assert len(self.chal) == 4
        if ctx is not None:
            from .transcript import exec_tree_device
            leaves, self.tree = exec_tree_device(ctx, RAM, self.chal, self.time, self.addr)
            evs = [(e.time_ordered_eval, e.addr_ordered_eval) for e, _ in leaves]
        else:
            run = RunningEvaluation(RAM, r, self.chal)
            evs, fields, last = [], [], RamTranscriptEntry.padding()
            for ts, as_ in zip(self.time, self.addr):
                for te, ae in zip(ts, as_):
                    run.update_time_ordered(te)
                    run.update_addr_ordered(ae)
                    last = ae
                evs.append((run.time_ordered_eval, run.addr_ordered_eval))
                fields.append(list(evs[-1]) + [x % r for x in last.to_field_elements()])
            self.tree = ExecTree(self.curve, fields)
        self.time_eval0 = [1] + [e[0] for e in evs]
        self.addr_eval0 = [1] + [e[1] for e in evs]
        self.root = self.tree.root

    def inputs(self, idx):
        """What the subcircuit's Stage1Request carries (coordinator.rs:569-604)."""
        return dict(chal=self.chal, root=self.root, time=self.time[idx], addr=self.addr[idx],
                    prev=self.addr[idx - 1][-1] if idx else RamTranscriptEntry.padding(),
                    time_eval0=self.time_eval0[idx], addr_eval0=self.addr_eval0[idx], path=self.tree.path(idx))

    def assignment_ints(self, idx, **override):
        """The subcircuit's full assignment (the host witness); override: inputs to replace (tests)."""
        w = self.inputs(idx)
        w.update(override)
        return self.make_class(idx).assignment_ints(w)[0]

    def assignment_bytes(self, idx):
        return self.make_class(idx).fc.enc(self.assignment_ints(idx))

    def flat(self, which):
        """Montgomery bytes of one flattened trace, `to_field_elements()` order: hk_trace_sort's / hk_exec_tree's layout."""
        fc = FrCodec(self.curve)
        tr = self.time if which == "time" else self.addr
        return fc.enc([x % self.r for st in tr for e in st for x in e.to_field_elements()])

    def stage0_device(self, ctx):
        """The job's stage-0 side on the device: the time-ordered trace uploaded once, the address-ordered one made from it
        by hk_trace_sort.  Returns a `RamStage0Device`."""
        return RamStage0Device(self, ctx)

    def stage1_device(self, ctx, traces=None):
        """The job's challenge-dependent witness on the device: hk_trace_sort -> hk_exec_tree -> hk_ram_stage1_witness, all
        device-resident.  Needs `chal` (set_challenges, or assign it).  traces: `stage0_device(ctx).traces` to read instead
        of uploading and sorting again.  Returns a `RamStage1Device`."""
        assert self.chal is not None, "stage1_device needs the round's challenges"
        return RamStage1Device(self, ctx, traces=traces)


class VmJob(RamJob):
    """The reference's VM job (vm/vm.rs, vm/vm_constraints.rs; `use_merkle_memory = false`): 2^log_n_sub subcircuits over 16
    registers.  Three key classes - first (16 + 3 ops entries), middle and last (32 + 3 ops): the `last` row makes the last
    subcircuit's matrices differ from the middle ones', as in `ShaMerkleJob` (the reference has two classes because its
    last-subcircuit check lives outside `generate_constraints`)."""

    def __init__(self, curve, log_n_sub, ops_per_chunk, dummy_constraint_num, values=None, t0=0):
        self.log_n_sub, self.ops, self.dummy_constraint_num = log_n_sub, ops_per_chunk, dummy_constraint_num
        super().__init__(curve, vm_subtraces(log_n_sub, ops_per_chunk, values, t0),
                         dummy_products=ops_per_chunk * (dummy_constraint_num // 2))


class RamStage0Device:
    """`traces = [time, addr]` as DeviceBuffers (4 Fr per entry), the second sorted from the first on the device;
    `rows(members)` cuts the stage-0 witnesses of subcircuits of ONE class out of them (hk_ram_stage0_witness)."""

    def __init__(self, job, ctx):
        from .capi import DeviceBuffer
        self.job, self.ctx = job, ctx
        time = DeviceBuffer.from_host(ctx, job.flat("time"))
        self.traces = [time]
        try:
            self.traces.append(ctx.trace_sort(4, time, int(job.offsets[-1]), device_out=True))
        except Exception:
            self.free()
            raise

    def rows(self, members):
        """DeviceBuffer of len(members) x 70 k Fr: row b = `job.stage0_ints(members[b])`.  The caller frees it."""
        from .capi import DeviceBuffer
        members = np.ascontiguousarray(members, dtype=np.uint32)
        k = len(self.job.time[int(members[0])]) if members.size else 1
        w = DeviceBuffer(self.ctx, max(members.size * 2 * ENTRY_COLS * k * self.ctx.fr_bytes, 1))
        try:
            self.ctx.ram_stage0_witness(self.job.offsets, k, self.traces[0], self.traces[1], members, w)
        except Exception:
            w.free()
            raise
        return w

    def free(self):
        for x in self.traces:
            x.free()
        self.traces = []


class RamStage1Device:
    """The job's traces and hk_exec_tree's RAM outputs as DeviceBuffers; `fill(circ, members, z)` writes whole assignment
    rows of one class from them (hk_ram_stage1_witness).  `root` is the one value read back."""

    def __init__(self, job, ctx, traces=None):
        from .capi import DeviceBuffer
        from .poseidon import device_params
        fc = FrCodec(job.curve)
        self.job, self.ctx, self._dev0, self.outs, self.params = job, ctx, None, (), None
        try:
            if traces is None:
                self._dev0 = RamStage0Device(job, ctx)
                traces = self._dev0.traces
            self.traces = list(traces)
            consts, n_consts, ld, nd = device_params(job.curve, fc)
            self.params = (DeviceBuffer.from_host(ctx, consts), n_consts, ld, nd)
            self.challenges = fc.enc(list(job.chal))
            self.outs = ctx.exec_tree(self.params, 4, job.offsets, self.traces[0], self.traces[1], self.challenges,
                                      device_out=True)
        except Exception:
            self.free()
            raise
        self.root = fc.dec(self.outs[4].to_host())[0]
        self._templates = {}

    def fill(self, circ, members, z, template=True):
        """Row b of the DeviceBuffer z (len(members) x circ.n_v Fr) <- the assignment of subcircuit members[b], all of class
        `circ`.  template: start every row from the class's constant row (`circ.template_ints()`); False keeps the bytes
        of every column the call does not own."""
        from .capi import DeviceBuffer
        members = np.ascontiguousarray(members, dtype=np.uint32)
        tm = None
        if template:
            if circ not in self._templates:
                self._templates[circ] = DeviceBuffer.from_host(self.ctx, circ.fc.enc(circ.template_ints()))
            tm = self._templates[circ]
        self.ctx.ram_stage1_witness(self.params, circ.np_, self.job.offsets, self.traces[0], self.traces[1], self.challenges,
                                    self.outs, members, circ.n_v, (1, circ.N_INST, circ.col0, circ.pos_col0), z, template=tm)
        return z

    def free(self):
        for x in ([self.params[0]] if self.params else []) + list(self.outs) + list(getattr(self, "_templates", {}).values()):
            x.free()
        if self._dev0 is not None:
            self._dev0.free()
            self._dev0 = None
        self.traces, self.outs, self.params, self._templates = [], (), None, {}
