"""The verifiable key directory job: sparse-tree path subcircuits joined by ROM portals.

The reference's `VerifiableKeyDirectoryCircuit` (distributed-prover/src/vkd/*.rs) proves a batch of directory updates over
a depth-128 sparse Merkle tree whose statement is Poseidon through and through: a leaf `username || counter u16 LE || key`
(66 bytes) is hashed at rate 3 (`hash.rs:85-107`), two children at rate 2 (:54-83), every node is the first 27 bytes of
its digest (`INNER_HASH_SIZE`), and the index of a user is the low `depth` bits of `hash(username)`
(sparse_tree.rs:170-176).  An update is two `depth`-level paths - the old leaf (or the null leaf) up to the previous root,
the new leaf up to the next root - each cut into `split` segments of L = depth / split levels; the segments, the leaf
hashes, the index words and the roots talk through ROM portals (vkd.rs:362-617 `vkd_update_to_subcircuit`,
vkd_constraints.rs:70-193 `get_portal_subtraces`, :237-342 `generate_constraints`).

The SEMANTICS are the reference's; tests/test_vkd_circuit_cpu.py pins the trace against a name-keyed restatement of
`SetupRomPortalManager`.  The constraint LAYOUT is this build's own: `VkdSubcircuit` is its own class on
`sha_circuit.Tape` with the stage-0 block, the ROM portal block and the membership block in the columns and order of
`ShaMerkleSubcircuit._program`, then one body per primitive (the table in section 4o).  Three deliberate deviations:

  1. the truncation to 27 bytes is CONSTRAINED (`bits` / `canon` / `trunc`); hash.rs:146-151 re-witnesses it without a row;
  2. ONE bit convention: level l counts from the leaf and uses bit l of the index, bit 1 = the current node is the right
     child, segment s covers levels s L .. s L + L - 1 (the reference's native `to_bit_vector` and its circuit disagree);
  3. padding p sets the dummy "pad{p}" <- 0 under a row `val = 0` (the reference's padding subtrace is empty, but an
     execution leaf needs a last entry and hk_stage1_witness refuses k = 0).

A node is an int below 2^216 (its 27 bytes read little-endian) everywhere in this module.
"""
import functools

import numpy as np

from .cp_groth16 import CURVE_PARAMS, FrCodec, MultiStageConstraintSynthesizer
from .poseidon import merkle_params
from .sha_circuit import ONE, ShaMerkleSubcircuit, Stage1Device, Tape, poseidon_path_trace
from .transcript import ROM, RomTranscriptEntry, RunningEvaluation, running_evaluations, sort_subtraces_by_addr

INNER_HASH_SIZE = 27                                   # vkd/sparse_tree.rs:42
NODE_BITS = 8 * INNER_HASH_SIZE
NODE_MASK = (1 << NODE_BITS) - 1
LEAF_BYTES, NAME_BYTES = 66, 32
SRC_ZERO = 0xFFFFFFFF                                  # include/hekaton.h HK_VKD_SRC_ZERO
KIND_APPEND, KIND_UPDATE = 0, 1                        # include/hekaton.h HK_VKD_APPEND / HK_VKD_UPDATE
N_PADDINGS = 6
KINDS = ["padding", "write pp", "hash leaf, get index, compute path", "compute path", "compute path, equality",
         "equality, hash leaf, compute path", "equality"]              # hk_vkd_cols.kind = the index of the type string
PORTALS = {"padding": 1, "write pp": 3, "hash leaf": 1, "compute path": 3, "equality": 2}     # "get index": split


# ---- hashes (vkd/hash.rs, HASH_TYPE = Poseidon) ----------------------------------------------------------------------
def chunks(data):
    """`value.chunks(INNER_HASH_SIZE)`, each `from_le_bytes_mod_order` (27 bytes are below either r)."""
    return [int.from_bytes(data[i:i + INNER_HASH_SIZE], "little") for i in range(0, len(data), INNER_HASH_SIZE)]


def vkd_digest(curve, data, trace=None):
    """The canonical field element `hash` squeezes: the rate-3 CRH over the 27-byte chunks."""
    return merkle_params(curve)[0].crh(chunks(bytes(data)), trace)


def vkd_hash(curve, data):
    """`hash` (hash.rs:85-107): the 32 little-endian bytes of the digest."""
    return vkd_digest(curve, data).to_bytes(32, "little")


def hash_leaf(curve, data):
    """`hash_leaf` (:49-52): the first 27 bytes of `hash`, as a node."""
    return vkd_digest(curve, data) & NODE_MASK


def hash_inner_node(curve, left, right, trace=None):
    """`hash_inner_node` (:54-83): the first 27 bytes of the rate-2 CRH of the two nodes."""
    return merkle_params(curve)[1].crh([left, right], trace) & NODE_MASK


def get_index(curve, username, depth):
    """`SparseMerkleTree::get_index` of `hash(username)`: its first depth / 8 bytes, little-endian."""
    return vkd_digest(curve, username) & ((1 << depth) - 1)


def compute_root(curve, node, siblings, index, level0=0):
    """`MerkleTreePath::compute_root` from an inner node under this module's bit convention: siblings[j] joins at level
    level0 + j, on the left when bit level0 + j of the index is 1."""
    for j, sib in enumerate(siblings):
        node = hash_inner_node(curve, sib, node) if (index >> (level0 + j)) & 1 else hash_inner_node(curve, node, sib)
    return node


def concat(username, key, counter):
    """`concat` (vkd.rs:101-107): the 66-byte leaf."""
    username, key = bytes(username), bytes(key)
    assert len(username) == NAME_BYTES and len(key) == 32 and 0 <= counter < 1 << 16
    return username + int(counter).to_bytes(2, "little") + key


class SparseTree:
    """`SparseMerkleTree` (sparse_tree.rs:70-177), host only: it makes jobs and checks them.  A node is keyed (index, depth)
    with depth 0 the root; `sparse_initial_hashes[d]` is the empty subtree's node at depth d."""

    def __init__(self, curve, depth):
        h = [hash_leaf(curve, bytes(32))]
        for _ in range(depth):
            h.append(hash_inner_node(curve, h[-1], h[-1]))
        h.reverse()
        self.curve, self.depth, self.sparse_initial_hashes, self.tree, self.leaves, self.root = curve, depth, h, {}, {}, h[0]

    @property
    def null_leaf(self):
        return self.sparse_initial_hashes[self.depth]

    def lookup_internal_node(self, index, depth):
        return self.tree.get((index, depth), self.sparse_initial_hashes[depth])

    def insert(self, index, leaf):
        i = index
        self.leaves[index] = bytes(leaf)
        self.tree[(i, self.depth)] = hash_leaf(self.curve, leaf)
        for d in range(self.depth - 1, -1, -1):
            i >>= 1
            self.tree[(i, d)] = hash_inner_node(self.curve, self.lookup_internal_node(2 * i, d + 1),
                                                self.lookup_internal_node(2 * i + 1, d + 1))
        self.root = self.tree[(0, 0)]

    def lookup_path(self, index):
        """The siblings from the leaf's up to the root's child."""
        path, i = [], index
        for d in range(self.depth, 0, -1):
            path.append(self.lookup_internal_node(i ^ 1, d))
            i >>= 1
        return path


class Append:
    """`VkdAppend`: add (username, 0, key); path: the `depth` siblings of the user's (still empty) leaf."""
    kind = KIND_APPEND

    def __init__(self, username, key, path):
        self.username, self.key, self.path = bytes(username), bytes(key), [int(x) for x in path]
        self.leaf_old, self.leaf_new = None, concat(username, key, 0)


class Update:
    """`VkdUpdate`: (username, counter, key1) -> (username, counter + 1, key2); path: the siblings of the user's leaf."""
    kind = KIND_UPDATE

    def __init__(self, username, counter, key1, key2, path):
        self.username, self.counter, self.key1, self.key2 = bytes(username), int(counter), bytes(key1), bytes(key2)
        self.path = [int(x) for x in path]
        self.leaf_old, self.leaf_new = concat(username, key1, counter), concat(username, key2, counter + 1)


# ---- one proving-key class ---------------------------------------------------------------------------------------------
class VkdSubcircuit(MultiStageConstraintSynthesizer):
    """kind: the reference's `get_type()` string, its primitives in order; n_levels = L; `first` / `last` as in every class
    here; depth_exec = log2(number of subcircuits).  `blocks` maps a block's name to its row ranges."""
    N_INST = 4
    _poseidon_crh = ShaMerkleSubcircuit._poseidon_crh
    _poseidon_permute = ShaMerkleSubcircuit._poseidon_permute
    csr = ShaMerkleSubcircuit.csr
    qap_evaluate = ShaMerkleSubcircuit.qap_evaluate
    total_num_stages = ShaMerkleSubcircuit.total_num_stages

    def __init__(self, curve, kind, n_levels, split, first=False, last=False, depth_exec=4):
        self.curve, self.kind, self.L, self.split, self.first, self.last = curve, kind, int(n_levels), int(split), first, last
        self.depth = depth_exec
        self.prims = kind.split(", ")
        assert all(p in PORTALS or p == "get index" for p in self.prims) and depth_exec >= 1
        assert "get index" not in self.prims or self.prims[:2] == ["hash leaf", "get index"]
        self.np_ = sum(self.split if p == "get index" else PORTALS[p] for p in self.prims)
        self.leaf_cfg, self.node_cfg = merkle_params(curve)
        self.r = CURVE_PARAMS[curve]["r"]
        self.nbits = self.r.bit_length()
        self.fc = FrCodec(curve)
        self.n0 = 4 * self.np_
        self.blocks, self.cols = {}, {}
        t = Tape(self.N_INST)
        self._program(t, None)
        self.tape = t
        self.n_c, self.n_wit, self.n_v = t.n_rows, t.n_wit, self.N_INST + t.n_wit
        self._csr = None

    def _program(self, t, inp):
        ev = not t.build
        B, r, k, ni = t.batch, self.r, self.np_, self.N_INST
        ENTRY, TR, ROOT = 1, 2, 3
        neg = r - 1
        col = lambda vals: t.alloc_full(vals if ev else None)
        start = [0]

        def block(name):
            if t.build and t.n_rows > start[0]:
                self.blocks.setdefault(name, []).append((start[0], t.n_rows))
            start[0] = t.n_rows

        # ---- stage 0 and the ROM portal block: `R1csSubcircuit._program`'s, column for column
        time_e = [(col(ev and inp["time"][j][0]), col(ev and inp["time"][j][1])) for j in range(k)]
        addr_e = [(col(ev and inp["addr"][j][0]), col(ev and inp["addr"][j][1])) for j in range(k)]
        assert t.n_wit == self.n0

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
        # ---- the subcircuit's own execution leaf is in the tree
        self.pos_col0 = ni + t.n_wit

        def seq(traces):
            """Allocates the next witness of a Poseidon trace; traces: one list per batch element (EVAL)."""
            if not ev:
                return lambda: t.alloc_full(None)
            it = iter(zip(*traces))
            return lambda: t.alloc_full(list(next(it)))
        leaf_lcs = [[(1, t_final)], [(1, a_final)], [(1, addr_e[-1][0])], [(1, addr_e[-1][1])]]
        nxt = seq(ev and [poseidon_path_trace(self.leaf_cfg, self.node_cfg,
                                              [t_vals[b], a_vals[b], inp["addr"][-1][0][b], inp["addr"][-1][1][b]],
                                              inp["path_sib"][b], inp["path_idx"][b]) for b in range(B)])
        cur = self._poseidon_crh(t, self.leaf_cfg, leaf_lcs, nxt)
        for _lvl in range(self.depth):
            bit, sib, left = nxt(), nxt(), nxt()
            t.big_row([(1, bit)], [(1, ONE), (neg, bit)], [])
            t.big_row([(1, bit)], [(1, sib), (neg, cur)], [(1, left), (neg, cur)])
            cur = self._poseidon_crh(t, self.node_cfg, [[(1, left)], [(1, sib), (1, cur), (neg, left)]], nxt)
        t.big_row([(1, cur), (neg, ROOT)], [(1, ONE)], [])
        self.pos_cols = ni + t.n_wit - self.pos_col0
        block("membership")

        # ---- the body, one part per primitive ---------------------------------------------------------------------
        self.body_col0 = ni + t.n_wit

        def booleans(vals, n):
            """n boolean columns: bit i of vals[b]."""
            cols = [col(ev and [(v >> i) & 1 for v in vals]) for i in range(n)]
            for c in cols:
                t.big_row([(1, c)], [(1, ONE), (neg, c)], [])
            return cols

        def packed(cols):
            return [(1 << i, c) for i, c in enumerate(cols)]

        def digest_bits(d_col, d_vals):
            """The digest's nbits bits: boolean, summing to it (`bits`), and as a bit string at most r - 1 (`canon`):
            e = "every bit so far equals r - 1's", from the top; at a 1 of r - 1 e <- e AND bit (a column, but for the top
            bit, where e is the bit itself), at a 0 of r - 1 the row e * bit = 0."""
            bits = booleans(d_vals, self.nbits)
            t.big_row(packed(bits), [(1, ONE)], [(1, d_col)])
            block("bits")
            e, e_vals = bits[self.nbits - 1], ev and [(v >> (self.nbits - 1)) & 1 for v in d_vals]
            for i in range(self.nbits - 2, -1, -1):
                if (neg >> i) & 1:
                    e_vals = ev and [x & (v >> i) & 1 for x, v in zip(e_vals, d_vals)]
                    new = col(e_vals)
                    t.big_row([(1, e)], [(1, bits[i])], [(1, new)])
                    e = new
                else:
                    t.big_row([(1, e)], [(1, bits[i])], [])
            block("canon")
            return bits

        j, leaf_bits = 0, None
        for prim in self.prims:
            if prim == "padding":
                t.big_row([(1, time_e[j][1])], [(1, ONE)], [])
                block("pad")
            elif prim == "equality":
                t.big_row([(1, time_e[j][1]), (neg, time_e[j + 1][1])], [(1, ONE)], [])
                block("equal")
            elif prim == "hash leaf":
                self.cols["hash leaf"] = ni + t.n_wit
                leaves = ev and [bytes(x) for x in inp["leaf"]]
                assert not ev or all(len(x) == LEAF_BYTES for x in leaves)
                leaf_bits = booleans(ev and [int.from_bytes(x, "little") for x in leaves], 8 * LEAF_BYTES)
                block("bits")
                lcs = [packed(leaf_bits[c:c + NODE_BITS]) for c in range(0, 8 * LEAF_BYTES, NODE_BITS)]
                traces, d_vals = [], []
                for x in leaves or []:
                    traces.append([])
                    d_vals.append(vkd_digest(self.curve, x, traces[-1]))
                d_col = self._poseidon_crh(t, self.leaf_cfg, lcs, seq(traces))
                block("hash")
                bits = digest_bits(d_col, d_vals)
                t.big_row(packed(bits[:NODE_BITS]), [(1, ONE)], [(1, time_e[j][1])])
                block("trunc")
            elif prim == "get index":
                self.cols["get index"] = ni + t.n_wit
                name_bits = leaf_bits[:8 * NAME_BYTES]                      # our choice: the reference witnesses them twice
                lcs = [packed(name_bits[c:c + NODE_BITS]) for c in range(0, 8 * NAME_BYTES, NODE_BITS)]
                traces, d_vals = [], []
                for x in (ev and leaves) or []:
                    traces.append([])
                    d_vals.append(vkd_digest(self.curve, x[:NAME_BYTES], traces[-1]))
                d_col = self._poseidon_crh(t, self.leaf_cfg, lcs, seq(traces))
                block("hash")
                bits = digest_bits(d_col, d_vals)
                for s in range(self.split):
                    t.big_row(packed(bits[s * self.L:(s + 1) * self.L]), [(1, ONE)], [(1, time_e[j + s][1])])
                block("index")
            elif prim == "compute path":
                self.cols["compute path"] = ni + t.n_wit
                cur, word, out = time_e[j][1], time_e[j + 1][1], time_e[j + 2][1]
                cur_v, word_v = (inp["time"][j][1], inp["time"][j + 1][1]) if ev else (None, None)
                ib = booleans(word_v, self.L)
                t.big_row(packed(ib), [(1, ONE)], [(1, word)])
                block("index")
                for l in range(self.L):
                    if ev:
                        sib_v = [s[l] % r for s in inp["sibs"]]
                        bit_v = [(w >> l) & 1 for w in word_v]
                        left_v = [s if b else c for s, b, c in zip(sib_v, bit_v, cur_v)]
                        right_v = [c if b else s for s, b, c in zip(sib_v, bit_v, cur_v)]
                    else:
                        sib_v = left_v = None
                    sib, left = col(sib_v), col(left_v)
                    t.big_row([(1, ib[l])], [(1, sib), (neg, cur)], [(1, left), (neg, cur)])
                    block("select")
                    traces, d_vals = [], []
                    for b in range(B):
                        traces.append([])
                        d_vals.append(self.node_cfg.crh([left_v[b], right_v[b]], traces[-1]))
                    d_col = self._poseidon_crh(t, self.node_cfg, [[(1, left)], [(1, sib), (1, cur), (neg, left)]], seq(traces))
                    block("hash")
                    bits = digest_bits(d_col, d_vals)
                    cur_v = ev and [d & NODE_MASK for d in d_vals]
                    cur = out if l == self.L - 1 else col(cur_v)                # the last node IS the `val` of the `set`
                    t.big_row(packed(bits[:NODE_BITS]), [(1, ONE)], [(1, cur)])
                    block("trunc")
            j += self.split if prim == "get index" else PORTALS[prim]               # "write pp": no rows, as in the reference
        assert j == k
        self.body_cols = ni + t.n_wit - self.body_col0

    # ---- what the tests and the host mirror of hk_r1cs_check read ------------------------------------------
    def rows(self):
        big = self.tape.big
        assert [e[0] for e in big] == list(range(self.n_c))
        return [e[1] for e in big], [e[2] for e in big], [e[3] for e in big]

    @property
    def device_cols(self):
        """(kind, hash_col0, index_col0, path_col0): what hk_vkd_witness takes as `cols`."""
        return (KINDS.index(self.kind), self.cols.get("hash leaf", 0), self.cols.get("get index", 0),
                self.cols.get("compute path", 0))

    def block_of(self, row):
        for name, ranges in self.blocks.items():
            if any(lo <= row < hi for lo, hi in ranges):
                return name
        raise IndexError(row)

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

    def witness_batch(self, inputs):
        """inputs: per-subcircuit dicts (`VkdJob.inputs`): the keys every class here takes (entry_chal, tr_chal, root, time,
        addr, prev, time_eval0, addr_eval0, path) and the primitives' own: leaf (66 bytes; "hash leaf"), sibs (L nodes;
        "compute path").  What a path starts from and its index word are read from the time-ordered entries."""
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
        inp["leaf"] = [i.get("leaf") for i in inputs]
        inp["sibs"] = [i.get("sibs") for i in inputs]
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
        return np.stack([self.fc.enc(z) for z in self.assignment_ints(inputs)])

    def stage0_witness_bytes(self, inputs):
        return np.stack([self.fc.enc(z[self.N_INST:self.N_INST + self.n0]) for z in self.assignment_ints(inputs)])


@functools.lru_cache(maxsize=None)
def vkd_class(curve, kind, n_levels, split, first, last, depth_exec):
    return VkdSubcircuit(curve, kind, n_levels, split, first=first, last=last, depth_exec=depth_exec)


# ---------------------------------------------------------------------------------------------------------------------
class VkdJob:
    """A whole VKD job: N = 8 + 2 split U subcircuits over U updates (6 paddings, write-pp, 2 split per update, the final
    equality), the addresses `SetupRomPortalManager` hands out, the VALUE TABLE every traced value is read from, the
    time-ordered trace, its address order and - once the round's challenges are in - the running evaluations, the
    execution tree and every subcircuit's inputs.  The job never builds the sparse tree: every update carries its siblings.

    The value table (what hk_vkd_trace writes as `values_out`), V = 3 + U (2 + 3 split) nodes / words:
        0 initial root   1 final root   2 null leaf
        base(u) = 3 + u (2 + 3 split):  + 0 hash of leaf_old (0 for an append)   + 1 hash of leaf_new
                                        + 2 + s index word s of the update's user
                                        + 2 + split + p split + s the node after segment s of path p
    ValueError: N no power of two >= 16; depth no multiple of 8 split or L < 8; a path of another length than depth; a name
    set twice; a name read before it is set (where the reference panics)."""

    def __init__(self, curve, initial_root, final_root, updates, depth=128, split=4, host_values=True):
        self.curve, self.depth_tree, self.split, self.updates = curve, int(depth), int(split), list(updates)
        self.r = CURVE_PARAMS[curve]["r"]
        S, U = self.split, len(self.updates)
        if S < 2 or depth % (8 * S) or depth // S < 8:
            raise ValueError("depth %d over %d segments: L must be a multiple of 8, at least 8, and split >= 2" % (depth, S))
        self.L = L = depth // S
        n = 8 + 2 * S * U
        if n < 16 or n & (n - 1):
            raise ValueError("8 + 2 x %d x %d updates = %d subcircuits: not a power of two >= 16" % (S, U, n))
        if any(len(u.path) != depth for u in self.updates):
            raise ValueError("every update carries its %d siblings" % depth)
        self.n, self.depth = n, n.bit_length() - 1
        self.initial_root, self.final_root = int(initial_root) & NODE_MASK, int(final_root) & NODE_MASK
        self.null_leaf = hash_leaf(curve, bytes(32)) if host_values else None
        self.stride = 2 + 3 * S
        # ---- the value table
        vals = [self.initial_root, self.final_root, self.null_leaf]
        for u in self.updates if host_values else ():
            idx = get_index(curve, u.username, depth)
            h_old = hash_leaf(curve, u.leaf_old) if u.kind == KIND_UPDATE else 0
            h_new = hash_leaf(curve, u.leaf_new)
            vals += [h_old, h_new] + [(idx >> (s * L)) & ((1 << L) - 1) for s in range(S)]
            for node in (h_old if u.kind == KIND_UPDATE else self.null_leaf, h_new):
                for s in range(S):
                    node = compute_root(curve, node, u.path[s * L:(s + 1) * L], idx, s * L)
                    vals.append(node)
        self.values = vals if host_values else None      # None: `on_device` - hk_vkd_trace computes them, no hash runs here
        # ---- the subcircuits: their primitives, and the portal operations in time order
        self.prims, self.ops = [], []
        self._names, self._next = {}, 1
        for p in range(N_PADDINGS):
            self._sub([("padding", ("set", "pad%d" % p, SRC_ZERO))])
        self._sub([("write pp", ("set", "initial root", 0), ("set", "final root", 1), ("set", "null leaf", 2))])
        prev_root = "initial root"
        for ui, u in enumerate(self.updates):
            base = 3 + ui * self.stride
            hash_new = ("hash leaf", ("set", ("leaf hash", u.leaf_new), base + 1))
            node = lambda p, s: ("root", ui, p) if s == S - 1 else ("node", ui, p, s)

            def path(p, s, leaf_name):
                return ("compute path", ("get", node(p, s - 1) if s else leaf_name), ("get", ("index", s, u.username)),
                        ("set", node(p, s), base + 2 + S + p * S + s))
            equal = ("equality", ("get", ("root", ui, 0)), ("get", prev_root))
            if u.kind == KIND_APPEND:
                index = ("get index",) + tuple(("set", ("index", s, u.username), base + 2 + s) for s in range(S))
                self._sub([hash_new, index, path(0, 0, "null leaf")])
                for s in range(1, S - 1):
                    self._sub([path(0, s, "null leaf")])
                self._sub([path(0, S - 1, "null leaf"), equal])
                for s in range(S):
                    self._sub([path(1, s, ("leaf hash", u.leaf_new))])
            else:
                for s in range(S):
                    self._sub([path(0, s, ("leaf hash", u.leaf_old))])
                self._sub([equal, hash_new, path(1, 0, ("leaf hash", u.leaf_new))])
                for s in range(1, S):
                    self._sub([path(1, s, ("leaf hash", u.leaf_new))])
            prev_root = ("root", ui, 1)
        self._sub([("equality", ("get", "final root"), ("get", prev_root))])
        assert len(self.prims) == n
        del self._names, self._next
        self.types = [", ".join(p[0] for p in ps) for ps in self.prims]
        self.slot_addr = np.array([a for ops in self.ops for a, _ in ops], np.uint32)
        self.slot_src = np.array([s for ops in self.ops for _, s in ops], np.uint32)
        self.time = self.addr = None
        if host_values:
            self.time = [[RomTranscriptEntry(a, 0 if s == SRC_ZERO else vals[s]) for a, s in ops] for ops in self.ops]
            self.addr = sort_subtraces_by_addr(self.time)
        self.offsets = np.zeros(n + 1, np.uint32)
        self.offsets[1:] = np.cumsum([len(ops) for ops in self.ops])
        self.chal = self.entry_chal = self.tr_chal = self.root = self.tree = None

    def _sub(self, prims):
        """One subcircuit: its portal operations resolved as `SetupRomPortalManager` does (rom_portal_manager.rs:34-117)."""
        ops = []
        for prim in prims:
            for op in prim[1:]:
                name = op[1]
                if op[0] == "set":
                    if name in self._names:
                        raise ValueError("cannot set portal wire more than once; wire %r" % (name,))
                    self._names[name] = (self._next, op[2])
                    self._next += 1
                elif name not in self._names:
                    raise ValueError("cannot get portal wire %r: nothing in this batch set it" % (name,))
                ops.append(self._names[name])
        self.prims.append(prims)
        self.ops.append(ops)

    # ---- vkd.rs:122-275 -----------------------------------------------------------------------------------------------
    @classmethod
    def random(cls, curve, log_n, depth=128, split=4):
        """`VerifiableKeyDirectoryCircuit::random`: a tree holding the genesis user, one append of user [8; 32], then
        (N - 8) / (2 split) - 1 updates of that user, update i to the key [i % 256; 32]."""
        n = 1 << log_n
        if n < 16 or (n - 8) % (2 * split):
            raise ValueError("2^%d subcircuits hold no whole number of updates of %d subcircuits" % (log_n, 2 * split))
        tree = SparseTree(curve, depth)
        tree.insert(get_index(curve, bytes(32), depth), concat(bytes(32), bytes(32), 0))
        initial_root = tree.root
        username, key, counter = bytes([8]) * 32, bytes(32), 0
        index = get_index(curve, username, depth)
        updates = [Append(username, key, tree.lookup_path(index))]
        tree.insert(index, concat(username, key, 0))
        for i in range((n - 8) // (2 * split) - 1):
            key2 = bytes([i % 256]) * 32
            updates.append(Update(username, counter, key, key2, tree.lookup_path(index)))
            counter, key = counter + 1, key2
            tree.insert(index, concat(username, key, counter))
        return cls(curve, initial_root, tree.root, updates, depth=depth, split=split)

    @classmethod
    def on_device(cls, ctx, curve, initial_root, final_root, updates, depth=128, split=4):
        """A job whose value table and traces exist on the device only: names and addresses are resolved here, no hash runs
        on the host.  `job.dev0` is its `VkdStage0Device`; `set_challenges(..., ctx=ctx)` and `stage1_device(ctx)` go on from
        it.  `free()` releases it."""
        job = cls(curve, initial_root, final_root, updates, depth=depth, split=split, host_values=False)
        job.dev0 = VkdStage0Device(job, ctx)
        return job

    def free(self):
        for name in ("dev1", "dev0"):
            if getattr(self, name, None) is not None:
                getattr(self, name).free()
                setattr(self, name, None)

    def verify(self):
        """`verify` (vkd.rs:216-275) with pp = the null leaf: every path leads from the old leaf (or the null leaf) to the
        root so far, and the new leaves lead to the final root."""
        root, ok = self.initial_root, True
        for u in self.updates:
            idx = get_index(self.curve, u.username, self.depth_tree)
            old = hash_leaf(self.curve, u.leaf_old if u.kind == KIND_UPDATE else bytes(32))
            ok &= compute_root(self.curve, old, u.path, idx) == root
            root = compute_root(self.curve, hash_leaf(self.curve, u.leaf_new), u.path, idx)
        return ok and root == self.final_root

    # ---- classes --------------------------------------------------------------------------------------------------------
    def type_of(self, idx):
        """The reference's `SubCircuit::get_type()` string."""
        return self.types[idx]

    def class_of(self, idx):
        """(type, first, last): 8 classes where the reference has 7 - subcircuit 0 is a padding with `first`."""
        return self.types[idx], idx == 0, idx == self.n - 1

    def class_rep(self, idx):
        """`representative_subcircuit`: the first subcircuit of the same type (the last one for the final equality)."""
        t = self.types[idx]
        return self.n - 1 if t == "equality" else self.types.index(t)

    def classes(self):
        """{class: its members in order}."""
        out = {}
        for i in range(self.n):
            out.setdefault(self.class_of(i), []).append(i)
        return out

    def make_class(self, idx):
        kind, first, last = self.class_of(idx)
        return vkd_class(self.curve, kind, self.L, self.split, first, last, self.depth)

    # ---- the round --------------------------------------------------------------------------------------------------------
    def stage0_ints(self, idx):
        return [x % self.r for e in self.time[idx] + self.addr[idx] for x in (e.addr, e.val)]

    def set_challenges(self, chals, tr_chal=None, ctx=None):
        """As `PartitionedR1csJob.set_challenges`: (entry_chal, tr_chal), or the super commitment they are hashed from; with
        ctx the evaluations and the execution tree come from one hk_exec_tree call."""
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
        if ctx is not None and self.time is None:                 # an `on_device` job: hk_exec_tree over the device's traces
            self.dev1 = VkdStage1Device(self, ctx, dev0=self.dev0)
            self.root = self.dev1.root
            return
        if ctx is not None:
            from .transcript import exec_tree_device
            leaves, self.tree = exec_tree_device(ctx, ROM, self.chal, self.time, self.addr)
        elif com is not None:
            leaves = running_evaluations(ROM, com, r, self.time, self.addr)
        else:
            run, last, leaves = RunningEvaluation(ROM, r, self.chal), RomTranscriptEntry.padding(), []
            for ts, as_ in zip(self.time, self.addr):
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
        """What the subcircuit's Stage1Request carries, and its primitives' own witnesses."""
        pair = lambda e: (e.addr, e.val)
        w = dict(entry_chal=self.entry_chal, tr_chal=self.tr_chal, root=self.root, time=[pair(e) for e in self.time[idx]],
                 addr=[pair(e) for e in self.addr[idx]], prev=pair(self.addr[idx - 1][-1]) if idx else (0, 0),
                 time_eval0=self.time_eval0[idx], addr_eval0=self.addr_eval0[idx], path=self.tree.path(idx))
        for prim in self.prims[idx]:
            if prim[0] == "hash leaf":
                w["leaf"] = prim[1][1][1]
            elif prim[0] == "compute path":
                _, ui, _p, *s = prim[3][1]
                s = s[0] if s else self.split - 1
                w["sibs"] = self.updates[ui].path[s * self.L:(s + 1) * self.L]
        return w

    def assignment_ints(self, idx, **override):
        w = self.inputs(idx)
        w.update(override)
        return self.make_class(idx).assignment_ints(w)[0]

    def assignment_bytes(self, idx):
        return self.make_class(idx).fc.enc(self.assignment_ints(idx))

    def flat(self, which):
        """Montgomery bytes of one flattened trace, (addr, val) per entry: hk_trace_sort's / hk_exec_tree's layout."""
        tr = self.time if which == "time" else self.addr
        return FrCodec(self.curve).enc([x % self.r for st in tr for e in st for x in (e.addr, e.val)])

    def values_bytes(self):
        """Montgomery bytes of the value table: what hk_vkd_trace writes as `values_out`."""
        return FrCodec(self.curve).enc(self.values)

    def tables(self):
        """The job as hk_vkd_desc states it (`Context.vkd_trace` takes this dict)."""
        fc = FrCodec(self.curve)
        leaves = np.zeros((len(self.updates), 2, LEAF_BYTES), np.uint8)
        for i, u in enumerate(self.updates):
            if u.kind == KIND_UPDATE:
                leaves[i, 0] = np.frombuffer(u.leaf_old, np.uint8)
            leaves[i, 1] = np.frombuffer(u.leaf_new, np.uint8)
        return dict(depth=self.depth_tree, split=self.split, n_updates=len(self.updates),
                    kinds=np.array([u.kind for u in self.updates], np.uint32), leaves=leaves,
                    siblings=fc.enc([x for u in self.updates for x in u.path]),
                    roots=fc.enc([self.initial_root, self.final_root]), slot_addr=self.slot_addr.copy(),
                    slot_src=self.slot_src.copy())

    def stage0_device(self, ctx):
        """The job's stage-0 side on the device: value table and time-ordered trace from hk_vkd_trace, the address order
        from hk_trace_sort.  Returns a `VkdStage0Device`."""
        return VkdStage0Device(self, ctx)


    def stage1_device(self, ctx, dev0=None):
        """The job's stage-1 witness on the device: hk_exec_tree over the two traces, then per class hk_vkd_witness +
        hk_stage1_witness.  Needs `chal`.  dev0: the `stage0_device(ctx)` to read instead of running hk_vkd_trace again."""
        assert self.chal is not None, "stage1_device needs the round's challenges"
        return VkdStage1Device(self, ctx, dev0=dev0 if dev0 is not None else getattr(self, "dev0", None))


class VkdStage0Device:
    """`values` (the value table), `traces = [time, addr]` as DeviceBuffers; `rows(members)` cuts the stage-0 witnesses of
    subcircuits of ONE class out of the traces (hk_stage0_witness)."""

    def __init__(self, job, ctx):
        from .capi import DeviceBuffer
        from .poseidon import device_params
        self.job, self.ctx, self.traces, self.values, self.params = job, ctx, [], None, None
        try:
            consts, n_consts, ld, nd = device_params(job.curve, FrCodec(job.curve))
            self.params = (DeviceBuffer.from_host(ctx, consts), n_consts, ld, nd)
            self.values, time = ctx.vkd_trace(job.tables(), self.params, device_out=True)
            self.traces.append(time)
            self.traces.append(ctx.trace_sort(2, time, int(job.offsets[-1]), device_out=True))
        except Exception:
            self.free()
            raise

    def rows(self, members):
        """DeviceBuffer of len(members) x 4 k Fr: row b = `job.stage0_ints(members[b])`.  The caller frees it."""
        from .capi import DeviceBuffer
        members = np.ascontiguousarray(members, dtype=np.uint32)
        k = int(self.job.offsets[int(members[0]) + 1] - self.job.offsets[int(members[0])]) if members.size else 1
        w = DeviceBuffer(self.ctx, max(members.size * 4 * k * self.ctx.fr_bytes, 1))
        try:
            self.ctx.stage0_witness(self.job.offsets, k, self.traces[0], self.traces[1], members, w)
        except Exception:
            w.free()
            raise
        return w

    def free(self):
        for x in self.traces + [self.values] + ([self.params[0]] if self.params else []):
            if x is not None:
                x.free()
        self.traces, self.values, self.params = [], None, None


class VkdStage1Device:
    """The job's value table, traces and hk_exec_tree's outputs as DeviceBuffers; `fill(circ, members, z)` writes whole
    assignment rows of one class from them (hk_vkd_witness + hk_stage1_witness) and `check(pk, z, members)` tests them where
    they lie (hk_pk_r1cs_check).  `root` is the one value read back."""
    check = Stage1Device.check

    def __init__(self, job, ctx, dev0=None):
        fc = FrCodec(job.curve)
        self.job, self.ctx, self._own0, self.outs = job, ctx, None, ()
        try:
            if dev0 is None:
                dev0 = self._own0 = VkdStage0Device(job, ctx)
            self.dev0, self.params = dev0, dev0.params
            self.tables = job.tables()
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
        self.ctx.vkd_witness(self.tables, self.params, d.values, members, circ.n_v, circ.device_cols, z)
        self.ctx.stage1_witness(self.params, circ.np_, self.job.offsets, d.traces[0], d.traces[1], self.challenges, self.outs,
                                members, circ.n_v, (1, circ.N_INST, circ.pos_col0), z)
        return z

    def free(self):
        for x in self.outs:
            x.free()
        if self._own0 is not None:
            self._own0.free()
            self._own0 = None
        self.outs = ()
