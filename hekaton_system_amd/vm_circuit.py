"""The RAM portal subcircuit and the reference's virtual-machine job on it.

The reference's third circuit family (distributed-prover/src/vm/, `MEM_TYPE = Ram`) reads and WRITES its portal memory: an
entry is (addr, val, timestamp, read) (transcript/ram_transcript.rs:260-390), the address order is sorted by (addr,
timestamp), and the prover-side portal manager (portal_manager/ram_portal_manager.rs:150-230) checks, over consecutive
address-ordered entries: same address or exactly one larger; one larger -> a write; same address and read -> same value; same
address -> larger timestamp; and over consecutive time-ordered entries: next timestamp = this one + 1.  The gadget crates
(ark-r1cs-std `UInt32`, `FpVar`) are third-party and absent, so the constraint LAYOUT is this build's own (parity unpinned,
DESIGN section 3); the FUNCTION is pinned by tests/test_vm_circuit_cpu.py.

`RamSubcircuit` is a `portal_circuit.PortalSubcircuit` (one program, two interpreters on `sha_circuit.Tape`: BUILD records the
rows, EVAL emits the assignment) with a portal block of its own and the base's membership block over six leaf fields.  Instance: ONE, entry_chal_1..3, tr_chal, root (N_INST = 6).  An ENTRY takes 35 columns: val, addr,
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
    stage 1, membership block         `PortalSubcircuit.membership_block` over the six leaf fields
    stage 1, dummy products  3 n      (12, 12, 144) triples, one row each: the VM's `dummy_constraint_num / 2` products

e needs three products of a challenge and a witness, and one R1CS row holds one: p1 and p2 carry the other two.

`RamSubcircuit.blocks` names the row range of every rule (recorded at BUILD) - the tests assert which one a tampering breaks.
"""
import functools

import numpy as np

from . import capi
from .portal_circuit import ONE, PortalJob, PortalStage0Device, PortalStage1Device, PortalSubcircuit
from .transcript import RAM, RamTranscriptEntry

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


class RamSubcircuit(PortalSubcircuit):
    """One proving-key class of a RAM job: a subcircuit that owns `n_portals` entries in each order.  `first` marks
    subcircuit 0 (evals pinned to 1, previous entry pinned to padding), `last` the final one (time eval == addr eval);
    depth = log2(number of subcircuits); dummy_products: the (12, 12, 144) triples after the membership block."""
    N_INST = 6                                         # ONE, entry_chal_1..3, tr_chal, root

    def __init__(self, curve, n_portals, first=False, last=False, depth=3, dummy_products=0):
        assert n_portals >= 1 and depth >= 1
        self.np_, self.first, self.last, self.depth = n_portals, first, last, depth
        self.dummy_products = dummy_products
        self.blocks = {}
        self._build(curve, 2 * ENTRY_COLS * n_portals)

    # ---- the program: identical in BUILD and EVAL --------------------------------------------------------
    def _program(self, t, inp):
        """inp (EVAL): dict of per-batch lists, see `witness_batch`."""
        ev = not t.build
        B, r, k, ni = t.batch, self.r, self.np_, self.N_INST
        C1, C2, C3, TR = 1, 2, 3, 4
        neg = r - 1
        col = lambda vals: t.alloc_full(vals if ev else None)
        block = self._block_recorder(t)

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
        le = addr_e[-1]
        leaf_lcs = [[(1, t_final)], [(1, a_final)], [(1, le.addr)], [(1, le.val)], le.ts(), [(1, le.read)]]
        self.membership_block(t, leaf_lcs, ev and [[te, ae, x.addr % r, x.val % r, x.i % r, int(x.read) % r]
                                                   for te, ae, x in zip(t_vals, a_vals, le.es)], inp)
        block("membership")
        # ---- the VM's dummy products (vm_constraints.rs:186-190): the same in every subcircuit of the class
        self.dummy_col0 = ni + t.n_wit
        for _ in range(self.dummy_products):
            a, b, c = col(ev and [12] * B), col(ev and [12] * B), col(ev and [144] * B)
            t.big_row([(1, a)], [(1, b)], [(1, c)])
        block("dummy")

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

    def _setup_assignment(self):
        return self.template_ints()                        # setup mode: only the counts matter

    # ---- witness generation --------------------------------------------------------------------------------
    def _batch_inputs(self, inputs):
        """inputs: per-subcircuit dicts (`RamJob.inputs`): chal (4 ints), root, time / addr (k entries each), prev (an entry),
        time_eval0, addr_eval0, path (siblings, index)."""
        k = self.np_
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
        return inp

    def _instance(self, w):
        return list(w["chal"]) + [w["root"]]


@functools.lru_cache(maxsize=None)
def ram_class(curve, n_portals, first, last, depth, dummy_products):
    """The class's `RamSubcircuit`, built once per process (nothing changes in it after BUILD)."""
    return RamSubcircuit(curve, n_portals, first=first, last=last, depth=depth, dummy_products=dummy_products)


# ---------------------------------------------------------------------------------------------------------------------
class RamJob(PortalJob):
    """A whole RAM job from its time-ordered subtraces (lists of `RamTranscriptEntry`): a `PortalJob` over four-field
    entries and four challenges.  A class is (entries owned, first, last)."""
    MEM, ENTRY = RAM, RamTranscriptEntry

    def __init__(self, curve, time_subtraces, dummy_products=0):
        n = len(time_subtraces)
        assert n >= 2 and n & (n - 1) == 0 and all(len(st) for st in time_subtraces)
        self._set_shape(curve, n)
        self.dummy_products = dummy_products
        self._set_traces(time_subtraces)

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

    def entry_input(self, e):
        return e                                           # `RamSubcircuit` reads the entries themselves

    def set_challenges(self, chals, ctx=None):
        """chals: (entry_chal_1, entry_chal_2, entry_chal_3, tr_chal), or the super commitment they are hashed from."""
        super().set_challenges(chals, ctx=ctx)

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


class RamStage0Device(PortalStage0Device):
    """`traces = [time, addr]` as DeviceBuffers (4 Fr per entry), the second sorted from the first on the device;
    `rows(members)`: 70 k Fr per subcircuit (hk_ram_stage0_witness)."""
    ENTRY_FR, ENTRY_COLS = 4, ENTRY_COLS

    def _cut(self, k, members, w):
        self.ctx.ram_stage0_witness(self.offsets, k, self.traces[0], self.traces[1], members, w)


class RamStage1Device(PortalStage1Device):
    """The job's traces and hk_exec_tree's RAM outputs as DeviceBuffers; `fill(circ, members, z)` writes whole assignment
    rows of one class from them (hk_ram_stage1_witness).  traces: a `RamStage0Device`'s, to read instead of uploading and
    sorting again."""
    ENTRY_FR = 4

    def __init__(self, job, ctx, traces=None):
        self._templates = {}                               # per class: its constant row on the device
        super().__init__(job, ctx, job.chal, traces=traces)

    def _traces(self, traces=None):
        return traces if traces is not None else self._own(RamStage0Device(self.job, self.ctx)).traces

    def fill(self, circ, members, z, template=True):
        """Row b of the DeviceBuffer z (len(members) x circ.n_v Fr) <- the assignment of subcircuit members[b], all of class
        `circ`.  template: start every row from the class's constant row (`circ.template_ints()`); False keeps the bytes
        of every column the call does not own."""
        members = np.ascontiguousarray(members, dtype=np.uint32)
        tm = None
        if template:
            if circ not in self._templates:
                self._templates[circ] = self._own(capi.DeviceBuffer.from_host(self.ctx, circ.fc.enc(circ.template_ints())))
            tm = self._templates[circ]
        self.ctx.ram_stage1_witness(self.params, circ.np_, self.offsets, self.traces[0], self.traces[1], self.challenges,
                                    self.outs, members, circ.n_v, (1, circ.N_INST, circ.col0, circ.pos_col0), z, template=tm)
        return z

    def free(self):
        super().free()
        self._templates = {}
