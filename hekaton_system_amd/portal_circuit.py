"""What the four portal jobs share: one subcircuit base, one job base, two device bases.

Every job here - big-merkle (sha_circuit.py), VM / RAM (vm_circuit.py), partitioned R1CS (r1cs_circuit.py), VKD
(vkd_circuit.py) - is N subcircuits that talk through portal memory, proved in two stages: stage 0 commits to a subcircuit's
slices of the time-ordered and the address-ordered trace, stage 1 - under the round's challenges - chains the running
evaluations of both slices, checks the address order and shows that the subcircuit's own execution leaf lies under the
public root.

The device fills these columns BY POSITION: hk_stage1_witness and hk_ram_stage1_witness are told `(1, N_INST, pos_col0)` and
write the portal block and the membership block in the order of `PortalSubcircuit.rom_portal_block` (csrc/stage1.cuh),
`RamSubcircuit._program` (csrc/ram_witness.cuh) and `PortalSubcircuit.membership_block`.  Each of these orders is written
down once, here or there; tests/test_portal_layout_cpu.py pins them.

A new job supplies: its body in `_program`, its leaf fields (ROM: `rom_membership_block` as it is), the layout of its
transcript entries (`PortalJob.ENTRY`) and where its time-ordered trace comes from (`PortalStage0Device._time_trace`).
"""
import numpy as np

from . import capi
from .cp_groth16 import CURVE_PARAMS, FrCodec, MultiStageConstraintSynthesizer, _batch_inverse
from .poseidon import ExecTree, device_params, merkle_params
from .transcript import ROM, RomTranscriptEntry, RunningEvaluation, exec_tree_device, sort_subtraces_by_addr

ONE = 0                       # column of the constant 1


def poseidon_path_trace(leaf_cfg, node_cfg, leaf, siblings, index):
    """Every witness of the membership block of one subcircuit, in allocation order (= what `k_poseidon_membership` writes):
    the leaf hash's permutation traces, then per level (bit, sibling, left, the two-to-one hash's trace).  The last
    value is the root the path leads to."""
    out = []
    cur = leaf_cfg.crh(leaf, out)
    for lvl, sib in enumerate(siblings):
        bit = (index >> lvl) & 1
        left, right = (sib, cur) if bit else (cur, sib)
        out += [bit, sib % leaf_cfg.p, left]
        cur = node_cfg.crh([left, right], out)
    return out


def poseidon_path_root(leaf_cfg, node_cfg, leaf, siblings, index):
    cur = leaf_cfg.crh(leaf)
    for lvl, sib in enumerate(siblings):
        cur = node_cfg.crh([sib, cur] if (index >> lvl) & 1 else [cur, sib])
    return cur


def rom_inputs(inputs, k, r=None):
    """The per-subcircuit input dicts of a ROM class, transposed for a batch: `time` / `addr` as k pairs ([addr per batch
    element], [val per batch element]), `prev` as one such pair, and time_eval0, addr_eval0, path_sib, path_idx as lists.
    r: reduce challenges, addresses and values mod r; None leaves every value as it came."""
    red = (lambda x: x % r) if r else (lambda x: x)
    assert all(i["entry_chal"] == inputs[0]["entry_chal"] and i["tr_chal"] == inputs[0]["tr_chal"] for i in inputs)
    inp = dict(entry_chal=red(inputs[0]["entry_chal"]), tr_chal=red(inputs[0]["tr_chal"]))
    for key in ("time", "addr"):
        assert all(len(i[key]) == k for i in inputs)
        inp[key] = [([red(i[key][j][0]) for i in inputs], [red(i[key][j][1]) for i in inputs]) for j in range(k)]
    inp["prev"] = ([red(i["prev"][0]) for i in inputs], [red(i["prev"][1]) for i in inputs])
    inp["time_eval0"] = [i["time_eval0"] for i in inputs]
    inp["addr_eval0"] = [i["addr_eval0"] for i in inputs]
    inp["path_sib"] = [i["path"][0] for i in inputs]
    inp["path_idx"] = [i["path"][1] for i in inputs]
    return inp


# ---------------------------------------------------------------------------------------------------------------------
class PortalSubcircuit(MultiStageConstraintSynthesizer):
    """One proving-key class of a portal job.  A subclass sets its own parameters (`np_`, `first`, `last`, `depth` among
    them), calls `_build(curve, n0)` and writes `_program(t, inp)`: one program, two interpreters (`sha_circuit.Tape`) -
    BUILD (inp None) records the R1CS rows, EVAL runs it over a batch and emits the assignment.  Instance: ONE, the
    challenges, the execution tree's root last."""
    N_INST = 4                                         # ONE, entry_chal, tr_chal, root
    block_ranges = False                               # `blocks`: name -> (lo, hi); True: name -> [(lo, hi), ...]

    def _tape(self, batch=0):
        from .sha_circuit import Tape                  # sha_circuit imports this module: the one import that has to wait
        return Tape(self.N_INST, batch=batch)

    def _build(self, curve, n0):
        """n0: the number of stage-0 witnesses.  Runs the program in BUILD mode: `tape`, `n_c`, `n_wit`, `n_v`."""
        self.curve, self.n0 = curve, n0
        self.leaf_cfg, self.node_cfg = merkle_params(curve)
        self.r = CURVE_PARAMS[curve]["r"]
        self.fc = FrCodec(curve)
        t = self._tape()
        self._program(t, None)
        self.tape = t
        self.n_c, self.n_wit, self.n_v = t.n_rows, t.n_wit, self.N_INST + t.n_wit
        self._csr = None

    # ---- the blocks every `_program` is made of ----------------------------------------------------------------
    def _block_recorder(self, t):
        """`block(name)`: at BUILD the rows since the last call are the block `name` of `self.blocks` - the tests assert
        which one a tampering breaks."""
        start = [0]

        def block(name):
            if t.build and self.block_ranges:
                if t.n_rows > start[0]:
                    self.blocks.setdefault(name, []).append((start[0], t.n_rows))
            elif t.build:
                self.blocks[name] = (start[0], t.n_rows)
            start[0] = t.n_rows
        return block

    def rom_portal_block(self, t, inp):
        """Stage 0 and the ROM portal block of a class with k = `np_` entries per order (csrc/stage1.cuh restates the
        columns).  inp (EVAL): `rom_inputs`' dict.
            stage 0           4 k      (addr, val) of the k time-ordered, then of the k address-ordered entries
            1 + 2 k                    time chain: the start evaluation (1 when `first`), then per entry e = val + entry_chal
                                       addr and cur <- cur (tr_chal - e)                     (rom_transcript.rs:77-107)
            1 + 2 k                    address chain, the same; when `last` the two final evaluations are equal
            2                          the previous leaf's last address-ordered entry, witnessed; padding - address 0 - in
                                       front of subcircuit 0 (subcircuit_circuit.rs:167, 199-216)
            2 k                        inv, same per consecutive pair of [previous] + address-ordered entries
        Returns (time_e, addr_e, t_final, a_final, t_vals, a_vals): the entries' (addr, val) columns, the columns of the two
        final evaluations and (EVAL) their values per batch element."""
        ev, r, k = not t.build, self.r, self.np_
        ENTRY, TR = 1, 2
        neg = r - 1
        col = lambda vals: t.alloc_full(vals if ev else None)
        time_e = [(col(ev and inp["time"][j][0]), col(ev and inp["time"][j][1])) for j in range(k)]
        addr_e = [(col(ev and inp["addr"][j][0]), col(ev and inp["addr"][j][1])) for j in range(k)]
        assert t.n_wit == self.n0

        def running(entries, start_vals, key):
            ev_col, cur = col(start_vals), start_vals
            if self.first:
                t.big_row([(1, ev_col)], [(1, ONE)], [(1, ONE)])                    # subcircuit 0: eval = 1
            for j, (a_col, v_col) in enumerate(entries):
                if ev:
                    ech, tr = inp["entry_chal"], inp["tr_chal"]
                    e_vals = [(int(v) + ech * int(a)) % r for a, v in zip(inp[key][j][0], inp[key][j][1])]
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
        # the address-step check of every consecutive pair of [previous entry] + slice (rom_portal_manager.rs:151-165):
        #   d = addr' - addr;  d * inv = 1 - same;  same * d = 0          (same = [d == 0], `is_eq`)
        #   (1 - same) * (d - 1) = 0                                     (not the same address -> exactly one larger)
        #   same * (val' - val) = 0                                      (`conditional_enforce_equal`)
        chain = [prev] + addr_e
        for j in range(1, len(chain)):
            (a0, v0), (a1, v1) = chain[j - 1], chain[j]
            if ev:
                prev_a = inp["prev"][0] if j == 1 else inp["addr"][j - 2][0]
                d = [(int(x) - int(y)) % r for x, y in zip(inp["addr"][j - 1][0], prev_a)]
                inv = [pow(x, -1, r) if x else 0 for x in d]
                same = [0 if x else 1 for x in d]
            else:
                inv = same = None
            inv_c, same_c = col(inv), col(same)
            t.big_row([(1, a1), (neg, a0)], [(1, inv_c)], [(1, ONE), (neg, same_c)])
            t.big_row([(1, same_c)], [(1, a1), (neg, a0)], [])
            t.big_row([(1, ONE), (neg, same_c)], [(1, a1), (neg, a0), (neg, ONE)], [])
            t.big_row([(1, same_c)], [(1, v1), (neg, v0)], [])
        assert t.n_wit == 10 * k + 4
        return time_e, addr_e, t_final, a_final, t_vals, a_vals

    def trace_columns(self, t, traces):
        """`nxt()`: the next full-width witness, holding the next value of a Poseidon trace; traces (EVAL): one list of
        values per batch element."""
        if t.build:
            return lambda: t.alloc_full(None)
        it = iter(zip(*traces))
        return lambda: t.alloc_full(list(next(it)))

    def membership_block(self, t, leaf_lcs, leaf_vals, inp):
        """The subcircuit's own execution leaf is in the tree (subcircuit_circuit.rs:233-260): the leaf CRH over the linear
        combinations `leaf_lcs`, `depth` levels of (bit, sibling, left, the node CRH) and the row that ties the result to
        the public root; the columns are `poseidon_path_trace`'s values in order.  leaf_vals (EVAL): the leaf's field
        values per batch element; inp: `path_sib`, `path_idx`.  Sets `pos_col0` and `pos_cols`."""
        ni, neg, ROOT = self.N_INST, self.r - 1, self.N_INST - 1
        self.pos_col0 = ni + t.n_wit
        nxt = self.trace_columns(t, t.build or [
            poseidon_path_trace(self.leaf_cfg, self.node_cfg, leaf, sib, idx)
            for leaf, sib, idx in zip(leaf_vals, inp["path_sib"], inp["path_idx"])])
        cur = self._poseidon_crh(t, self.leaf_cfg, leaf_lcs, nxt)
        for _lvl in range(self.depth):
            bit, sib, left = nxt(), nxt(), nxt()
            t.big_row([(1, bit)], [(1, ONE), (neg, bit)], [])                               # boolean
            t.big_row([(1, bit)], [(1, sib), (neg, cur)], [(1, left), (neg, cur)])          # left = bit ? sib : cur
            cur = self._poseidon_crh(t, self.node_cfg, [[(1, left)], [(1, sib), (1, cur), (neg, left)]], nxt)
        t.big_row([(1, cur), (neg, ROOT)], [(1, ONE)], [])                                  # the public root
        self.pos_cols = ni + t.n_wit - self.pos_col0

    def rom_membership_block(self, t, inp, portal):
        """`membership_block` over a ROM class's leaf: the two final evaluations and the last address-ordered entry.
        portal: what `rom_portal_block` returned."""
        _time_e, addr_e, t_final, a_final, t_vals, a_vals = portal
        r = self.r
        leaf_lcs = [[(1, t_final)], [(1, a_final)], [(1, addr_e[-1][0])], [(1, addr_e[-1][1])]]
        leaf_vals = t.build or [[te, ae, int(a) % r, int(v) % r]
                                for te, ae, a, v in zip(t_vals, a_vals, inp["addr"][-1][0], inp["addr"][-1][1])]
        self.membership_block(t, leaf_lcs, leaf_vals, inp)

    def _poseidon_crh(self, t, cfg, inputs, nxt):
        """`poseidon::constraints::CRHGadget::evaluate` with an own layout: inputs = linear combinations [(coef, col)];
        per round the S-box chain of every S-boxed element and the new state are witnesses (`nxt()` allocates the next
        one, in the order poseidon.PoseidonConfig.permute traces them); returns the digest's column."""
        tt = cfg.t
        state = [[] for _ in range(tt)]                      # linear combinations; [] = 0
        k = 0
        while True:
            blk = inputs[k:k + cfg.rate]
            for i, lc in enumerate(blk):
                state[1 + i] = state[1 + i] + lc
            k += len(blk)
            if k >= len(inputs):
                break
            state = self._poseidon_permute(t, cfg, state, nxt)
        state = self._poseidon_permute(t, cfg, state, nxt)
        return state[1][0][1]

    def _poseidon_permute(self, t, cfg, state, nxt):
        half = cfg.rf // 2
        for r in range(cfg.rf + cfg.rp):
            full = r < half or r >= half + cfg.rp
            y = [state[i] + [(cfg.ark[r][i], ONE)] for i in range(cfg.t)]
            for i in range(cfg.t if full else 1):
                u = y[i]
                prev_col = None
                n_chain = 3 if cfg.alpha == 5 else 5
                for step in range(n_chain):
                    c = nxt()
                    if step == 0:
                        t.big_row(u, u, [(1, c)])                                  # u^2
                    elif step < n_chain - 1:
                        t.big_row([(1, prev_col)], [(1, prev_col)], [(1, c)])      # squarings
                    else:
                        t.big_row([(1, prev_col)], u, [(1, c)])                    # x^(alpha-1) * u
                    prev_col = c
                y[i] = [(1, prev_col)]
            new = []
            for i in range(cfg.t):
                c = nxt()
                lc = [(cfg.mds[i][j] * coef % cfg.p, col) for j in range(cfg.t) for coef, col in y[j]]
                t.big_row(lc, [(1, ONE)], [(1, c)])
                new.append([(1, c)])
            state = new
        return state

    # ---- what the tests and the host mirror of hk_r1cs_check read ------------------------------------------
    def rows(self):
        """(A, B, C) as ark-style rows [(coeff, col)] - what cp_groth16.r1cs_bad_rows takes (a class whose rows are all
        `big_row`s: every one but the big-merkle classes)."""
        big = self.tape.big
        assert [e[0] for e in big] == list(range(self.n_c))
        return [e[1] for e in big], [e[2] for e in big], [e[3] for e in big]

    def block_of(self, row):
        for name, ranges in self.blocks.items():
            if any(lo <= row < hi for lo, hi in (ranges if self.block_ranges else [ranges])):
                return name
        raise IndexError(row)

    # ---- MultiStageConstraintSynthesizer -------------------------------------------------------------------
    def total_num_stages(self):
        return 2

    def _setup_assignment(self):
        """The assignment `generate_constraints` hands out; in setup mode only the counts matter."""
        return [1] + [0] * (self.n_v - 1)

    def generate_constraints(self, stage, cs):
        z = self._setup_assignment()
        ni = self.N_INST
        cs.initialize_stage()
        if stage == 0:
            cs.witness_assignment.extend(z[ni:ni + self.n0])
        else:
            cs.instance_assignment.extend(z[1:ni])
            cs.witness_assignment.extend(z[ni + self.n0:])
            cs._n_constraints += self.n_c
        cs.finalize_stage()

    def csr(self, fc):
        if self._csr is None:
            self._csr = self.tape.csr(fc)
        return tuple((rp, col, val) for rp, col, val, _vi, _tab in self._csr)

    def qap_evaluate(self, t_pt):
        """instance_map_with_evaluation over the tape's rows (generator.rs:75-76)."""
        p = CURVE_PARAMS[self.curve]
        r, ni, n_c = self.r, self.N_INST, self.n_c
        m, log_m = 1, 0
        while m < n_c + ni:
            m *= 2
            log_m += 1
        w = pow(pow(p["gen"], (r - 1) >> p["two_adicity"], r), 1 << (p["two_adicity"] - log_m), r)
        zt = (pow(t_pt, m, r) - 1) % r
        wi = [1] * m
        for i in range(1, m):
            wi[i] = wi[i - 1] * w % r
        den = _batch_inverse([m * (t_pt - x) % r for x in wi], r)
        u = [zt * x % r * d % r for x, d in zip(wi, den)]
        self.csr(self.fc)
        outs = []
        for (rp, col, _val, vidx, table) in self._csr:
            acc = [0] * self.n_v
            rp_l, col_l, vi_l = rp.tolist(), col.tolist(), vidx.tolist()
            for i in range(n_c):
                ui = u[i]
                for k in range(rp_l[i], rp_l[i + 1]):
                    acc[col_l[k]] += ui * table[vi_l[k]]
            outs.append([x % r for x in acc])
        a, b, c = outs
        for j in range(ni):
            a[j] = (a[j] + u[n_c + j]) % r
        return a, b, c, zt, m

    # ---- witness generation --------------------------------------------------------------------------------
    def _batch_inputs(self, inputs):
        """The per-subcircuit input dicts transposed into what `_program` reads in EVAL mode."""
        return rom_inputs(inputs, self.np_, self.r)

    def _instance(self, w):
        """Columns 1 .. N_INST - 1 of the subcircuit with the inputs w."""
        return [w["entry_chal"], w["tr_chal"], w["root"]]

    def _assignments(self, t, inputs):
        """The full assignments, as lists of ints, of a tape the program ran on in EVAL mode over `inputs`."""
        assert t.n_wit == self.n_wit
        out = []
        for b, w in enumerate(inputs):
            z = [0] * self.n_v
            z[:self.N_INST] = [1] + [x % self.r for x in self._instance(w)]
            for c, vals in t.full_records:
                z[c] = int(vals[b]) % self.r
            out.append(z)
        return out

    def witness_batch(self, inputs):
        """inputs: the per-subcircuit dicts the class's job hands out (`inputs(idx)`).  Runs the program in EVAL mode over
        the whole batch.  Returns the full assignments as lists of ints."""
        t = self._tape(batch=len(inputs))
        self._program(t, self._batch_inputs(inputs))
        return self._assignments(t, inputs)

    def assignment_ints(self, inputs):
        return self.witness_batch(inputs if isinstance(inputs, list) else [inputs])

    def assignment_bytes(self, inputs):
        """Montgomery bytes of the full assignments, (batch, n_v * 32)."""
        return np.stack([self.fc.enc(z) for z in self.assignment_ints(inputs)])

    def stage0_witness_bytes(self, inputs):
        """Montgomery bytes of the stage-0 witnesses (what the class's stage-0 commitment is over), (batch, n0 * 32)."""
        return np.stack([self.fc.enc(z[self.N_INST:self.N_INST + self.n0]) for z in self.assignment_ints(inputs)])


# ---------------------------------------------------------------------------------------------------------------------
class PortalJob:
    """A whole job from its time-ordered subtraces (lists of `ENTRY`): the address order (coordinator.rs:92-123), the slices
    each subcircuit commits to in stage 0 and - once the round's challenges are in - the running evaluations, the execution
    tree and every subcircuit's inputs.  A subclass states its memory type and entry class, and has `class_of(idx)` and
    `make_class(idx)`; `time` / `addr` may be edited in place before `set_challenges` (the tests tamper with them)."""
    MEM, ENTRY = ROM, RomTranscriptEntry               # the entry's `to_field_elements()` is the layout of the flat traces

    def _set_shape(self, curve, n):
        self.curve, self.n, self.depth = curve, n, n.bit_length() - 1
        self.r = CURVE_PARAMS[curve]["r"]
        self.chal = self.entry_chal = self.tr_chal = self.root = self.tree = None

    def _set_traces(self, time, lengths=None):
        """time: the time-ordered subtraces, or None (a job whose traces exist on the device only) with their lengths."""
        self.time = self.addr = None
        if time is not None:
            self.time = [list(st) for st in time]
            self.addr = sort_subtraces_by_addr(self.time)
        self.offsets = np.zeros(self.n + 1, np.uint32)
        self.offsets[1:] = np.cumsum([len(st) for st in self.time] if lengths is None else lengths)

    def entry_input(self, e):
        """A transcript entry as the class's `witness_batch` takes it: ROM, the pair (addr, val)."""
        return (e.addr, e.val)

    def stage0_ints(self, idx):
        """The subcircuit's stage-0 witness: the fields of its time-ordered then of its address-ordered entries."""
        return [x % self.r for e in self.time[idx] + self.addr[idx] for x in e.to_field_elements()]

    def _take_challenges(self, chals, tr_chal=None):
        """chals: the challenges in `RunningEvaluation.challenges` order - ROM: or entry_chal with tr_chal beside it - or
        the super commitment they are hashed from (`RunningEvaluation.new`)."""
        if isinstance(chals, (bytes, bytearray)) or hasattr(chals, "serialize_uncompressed"):
            chals = RunningEvaluation.new(self.MEM, chals, self.r).challenges
        elif tr_chal is not None:
            chals = (chals, tr_chal)
        self.chal = tuple(c % self.r for c in chals)
        assert len(self.chal) == (2 if self.MEM == ROM else 4)
        if self.MEM == ROM:
            self.entry_chal, self.tr_chal = self.chal

    def set_challenges(self, chals, tr_chal=None, ctx=None):
        """Running evaluations after every subcircuit and the execution tree (coordinator.rs:125-174); with ctx (a
        capi.Context of the job's curve) from one hk_exec_tree call.  chals, tr_chal: see `_take_challenges`."""
        self._take_challenges(chals, tr_chal)
        r = self.r
        if ctx is not None:
            leaves, self.tree = exec_tree_device(ctx, self.MEM, self.chal, self.time, self.addr)
        else:
            run, last, leaves = RunningEvaluation(self.MEM, r, self.chal), self.ENTRY.padding(), []
            for ts, as_ in zip(self.time, self.addr):          # `transcript.running_evaluations` from given challenges
                for te, ae in zip(ts, as_):
                    run.update_time_ordered(te)
                    run.update_addr_ordered(ae)
                    last = ae
                leaves.append((run.copy(), last))
            self.tree = ExecTree(self.curve, [[e.time_ordered_eval, e.addr_ordered_eval]
                                              + [x % r for x in last.to_field_elements()] for e, last in leaves])
        self.time_eval0 = [1] + [e.time_ordered_eval for e, _ in leaves]
        self.addr_eval0 = [1] + [e.addr_ordered_eval for e, _ in leaves]
        self.root = self.tree.root

    def inputs(self, idx):
        """What the subcircuit's Stage1Request carries (coordinator.rs:569-604): the challenges, the root, its two slices,
        the previous leaf (evals and last entry; padding before subcircuit 0) and the membership path of its own leaf."""
        w = dict(entry_chal=self.entry_chal, tr_chal=self.tr_chal) if self.MEM == ROM else dict(chal=self.chal)
        w.update(root=self.root, time=[self.entry_input(e) for e in self.time[idx]],
                 addr=[self.entry_input(e) for e in self.addr[idx]],
                 prev=self.entry_input(self.addr[idx - 1][-1] if idx else self.ENTRY.padding()),
                 time_eval0=self.time_eval0[idx], addr_eval0=self.addr_eval0[idx], path=self.tree.path(idx))
        return w

    def assignment_ints(self, idx, **override):
        """The subcircuit's full assignment (the host witness); override: inputs to replace (tests)."""
        w = self.inputs(idx)
        w.update(override)
        return self.make_class(idx).assignment_ints(w)[0]

    def assignment_bytes(self, idx):
        return self.make_class(idx).fc.enc(self.assignment_ints(idx))

    def flat(self, which):
        """Montgomery bytes of one flattened trace, `to_field_elements()` order: hk_trace_sort's / hk_exec_tree's layout."""
        tr = self.time if which == "time" else self.addr
        return FrCodec(self.curve).enc([x % self.r for st in tr for e in st for x in e.to_field_elements()])


# ---------------------------------------------------------------------------------------------------------------------
class PortalStage0Device:
    """A job's stage-0 side on the device: `traces = [time, addr]` as DeviceBuffers, the address-ordered one sorted from the
    time-ordered one by hk_trace_sort; `rows(members)` cuts the stage-0 witnesses of subcircuits of ONE class out of them
    for `ProvingKey.commit_batch`.  A subclass says where the time-ordered trace comes from (`_time_trace`).  `_owned` lists
    what this object allocated - `_own(x)` adds to it; `free()` releases exactly that, once, also after a failed constructor."""
    ENTRY_FR, ENTRY_COLS = 2, 2                        # Fr per entry of a trace; stage-0 columns per entry

    def __init__(self, job, ctx):
        self.job, self.ctx, self.offsets, self.traces, self._owned = job, ctx, job.offsets, [], []
        try:
            time = self._time_trace()
            self.traces = [time, self._own(ctx.trace_sort(self.ENTRY_FR, time, int(self.offsets[-1]), device_out=True))]
        except Exception:
            self.free()
            raise

    def _own(self, x):
        self._owned.append(x)
        return x

    def _time_trace(self):
        """The flattened time-ordered trace as a DeviceBuffer: the job's own, uploaded."""
        return self._own(capi.DeviceBuffer.from_host(self.ctx, self.job.flat("time")))

    def _cut(self, k, members, w):
        self.ctx.stage0_witness(self.offsets, k, self.traces[0], self.traces[1], members, w)

    def rows(self, members):
        """DeviceBuffer of len(members) x 2 ENTRY_COLS k Fr: row b = `job.stage0_ints(members[b])` in Montgomery form, k the
        number of entries the members' class owns.  The caller frees it."""
        members = np.ascontiguousarray(members, dtype=np.uint32)
        k = int(self.offsets[int(members[0]) + 1] - self.offsets[int(members[0])]) if members.size else 1
        w = capi.DeviceBuffer(self.ctx, max(members.size * 2 * self.ENTRY_COLS * k * self.ctx.fr_bytes, 1))
        try:
            self._cut(k, members, w)
        except Exception:
            w.free()
            raise
        return w

    def free(self):
        for x in self._owned:
            x.free()
        self._owned, self.traces = [], []


class R1csUnsatisfied(AssertionError):
    """An assignment on the device fails its class's R1CS (PortalStage1Device.check).  failures: [(subcircuit, n_bad,
    first_bad, [the first failing rows])] of every failing subcircuit of the call, in the order of `members`."""

    def __init__(self, failures):
        self.failures = failures
        self.subcircuit, self.n_bad, self.row, _ = failures[0]
        super().__init__("subcircuit %d: constraint %d is unsatisfied (%d failing rows in it; %d failing subcircuits in the call)"
                         % (self.subcircuit, self.row, self.n_bad, len(failures)))


class PortalStage1Device:
    """A job's challenge-dependent side on the device: the two traces, the Poseidon parameters, the encoded challenges and
    hk_exec_tree's outputs (evaluations, leaves, nodes, siblings, root) as DeviceBuffers, from which a subclass's `fill(circ,
    members, z)` writes assignment rows of one class without a host value in between.  `root` is the one value read back (an
    int).  A subclass says where the traces come from (`_traces(**source)`, the constructor's keywords).  Ownership as in
    `PortalStage0Device`; a stage-0 device made here is owned like a buffer."""
    ENTRY_FR = 2

    def __init__(self, job, ctx, chal, **source):
        fc = FrCodec(job.curve)
        self.job, self.ctx, self.offsets, self._owned = job, ctx, job.offsets, []
        self.traces, self.outs, self.params = [], (), None
        try:
            self.traces = list(self._traces(**source))
            self.params = self._params()
            self.challenges = fc.enc(list(chal))
            self.outs = ctx.exec_tree(self.params, self.ENTRY_FR, self.offsets, self.traces[0], self.traces[1], self.challenges,
                                      device_out=True)
            self._owned += self.outs
        except Exception:
            self.free()
            raise
        self.root = fc.dec(self.outs[4].to_host())[0]

    def _own(self, x):
        self._owned.append(x)
        return x

    def _params(self):
        consts, n_consts, ld, nd = device_params(self.job.curve, FrCodec(self.job.curve))
        return (self._own(capi.DeviceBuffer.from_host(self.ctx, consts)), n_consts, ld, nd)

    def _stage1_witness(self, circ, members, z):
        """hk_stage1_witness: the instance, the ROM portal block and the membership block of every row."""
        self.ctx.stage1_witness(self.params, circ.np_, self.offsets, self.traces[0], self.traces[1], self.challenges, self.outs,
                                members, circ.n_v, (1, circ.N_INST, circ.pos_col0), z)

    def check(self, pk, z, members, cap=8):
        """ark's `assert!(cs.is_satisfied())` on the filled rows (subcircuit_circuit.rs:311-399), where they lie: one
        hk_pk_r1cs_check over the DeviceBuffer z (row b = members[b]) against the matrices of the class's key `pk` (a
        capi.DevicePk, or anything with its r1cs_check).  Raises R1csUnsatisfied naming the first failing (subcircuit, row);
        its `failures` lists up to `cap` rows per failing subcircuit.  Nothing calls this unless asked to."""
        members = [int(i) for i in members]
        if not members:
            return
        res = pk.r1cs_check(z, batch=len(members), cap=cap)
        verdicts, rows = res if cap else (res, None)
        failures = [(i, n_bad, first, [] if rows is None else [int(x) for x in rows[b] if x != 0xffffffff])
                    for b, (i, (n_bad, first)) in enumerate(zip(members, verdicts)) if n_bad]
        if failures:
            raise R1csUnsatisfied(failures)

    def free(self):
        for x in self._owned:
            x.free()
        self._owned, self.traces, self.outs, self.params = [], [], (), None
