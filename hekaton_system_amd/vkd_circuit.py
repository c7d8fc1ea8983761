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
`SetupRomPortalManager`.  The constraint LAYOUT is this build's own: `VkdSubcircuit` is a
`portal_circuit.PortalSubcircuit` - the stage-0 block, the ROM portal block and the membership block are the base's
(`rom_portal_block`, `rom_membership_block`) - then one body per primitive (the table in section 4o).  Three deliberate deviations:

  1. the truncation to 27 bytes is CONSTRAINED (`bits` / `canon` / `trunc`); hash.rs:146-151 re-witnesses it without a row;
  2. ONE bit convention: level l counts from the leaf and uses bit l of the index, bit 1 = the current node is the right
     child, segment s covers levels s L .. s L + L - 1 (the reference's native `to_bit_vector` and its circuit disagree);
  3. padding p sets the dummy "pad{p}" <- 0 under a row `val = 0` (the reference's padding subtrace is empty, but an
     execution leaf needs a last entry and hk_stage1_witness refuses k = 0).

A node is an int below 2^216 (its 27 bytes read little-endian) everywhere in this module.
"""
import functools

import numpy as np

from . import capi
from .cp_groth16 import CURVE_PARAMS, FrCodec
from .poseidon import device_params, merkle_params
from .portal_circuit import ONE, PortalJob, PortalStage0Device, PortalStage1Device, PortalSubcircuit
from .transcript import RomTranscriptEntry

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


ST_OK, ST_OCCUPIED, ST_ABSENT, ST_STALE = 0, 1, 2, 3    # include/hekaton.h HK_VKD_ST_*


class Append:
    """`VkdAppend`: add (username, 0, key); path: the `depth` siblings of the user's (still empty) leaf, or None when the
    job reads its siblings from the device (`VkdJob(siblings=...)`)."""
    kind = KIND_APPEND

    def __init__(self, username, key, path=None):
        self.username, self.key = bytes(username), bytes(key)
        self.path = None if path is None else [int(x) for x in path]
        self.leaf_old, self.leaf_new = None, concat(username, key, 0)


class Update:
    """`VkdUpdate`: (username, counter, key1) -> (username, counter + 1, key2); path: the siblings of the user's leaf, or
    None as for `Append`."""
    kind = KIND_UPDATE

    def __init__(self, username, counter, key1, key2, path=None):
        self.username, self.counter, self.key1, self.key2 = bytes(username), int(counter), bytes(key1), bytes(key2)
        self.path = None if path is None else [int(x) for x in path]
        self.leaf_old, self.leaf_new = concat(username, key1, counter), concat(username, key2, counter + 1)


def leaves_table(changes):
    """U x 2 x 66 bytes: (leaf_old - zeros for an append -, leaf_new) of every change: hk_vkd_desc.leaves."""
    leaves = np.zeros((len(changes), 2, LEAF_BYTES), np.uint8)
    for i, u in enumerate(changes):
        if u.kind == KIND_UPDATE:
            leaves[i, 0] = np.frombuffer(u.leaf_old, np.uint8)
        leaves[i, 1] = np.frombuffer(u.leaf_new, np.uint8)
    return leaves


def directory_paths(curve, depth, leaves0, changes):
    """The host mirror of hk_vkd_tree: a `SparseTree` that takes the directory's leaves `leaves0`
    (66 bytes each, a later one replacing an earlier one of the same index), then one change after the other.  Returns
    (initial_root, final_root, paths, status): paths[u] the `depth` siblings of change u's leaf right before it is applied,
    status[u] what the change met (ST_*): an append onto an occupied index, an update of an absent user or one whose leaf_old
    is not what the index holds.  The tree inserts whatever the status is, as the reference's does."""
    t = SparseTree(curve, depth)
    for leaf in leaves0:
        leaf = bytes(leaf)
        assert len(leaf) == LEAF_BYTES
        t.insert(get_index(curve, leaf[:NAME_BYTES], depth), leaf)
    initial, paths, status = t.root, [], []
    for u in changes:
        idx = get_index(curve, u.username, depth)
        held = t.leaves.get(idx)
        if u.kind == KIND_APPEND:
            status.append(ST_OK if held is None else ST_OCCUPIED)
        else:
            status.append(ST_ABSENT if held is None else ST_OK if held == u.leaf_old else ST_STALE)
        paths.append(t.lookup_path(idx))
        t.insert(idx, u.leaf_new)
    return initial, t.root, paths, status


# ---- one proving-key class ---------------------------------------------------------------------------------------------
class VkdSubcircuit(PortalSubcircuit):
    """kind: the reference's `get_type()` string, its primitives in order; n_levels = L; `first` / `last` as in every class
    here; depth_exec = log2(number of subcircuits).  `blocks` maps a block's name to its row ranges: a name recurs once per
    primitive and level."""
    block_ranges = True

    def __init__(self, curve, kind, n_levels, split, first=False, last=False, depth_exec=4):
        self.kind, self.L, self.split, self.first, self.last = kind, int(n_levels), int(split), first, last
        self.depth = depth_exec
        self.prims = kind.split(", ")
        assert all(p in PORTALS or p == "get index" for p in self.prims) and depth_exec >= 1
        assert "get index" not in self.prims or self.prims[:2] == ["hash leaf", "get index"]
        self.np_ = sum(self.split if p == "get index" else PORTALS[p] for p in self.prims)
        self.nbits = CURVE_PARAMS[curve]["r"].bit_length()
        self.blocks, self.cols = {}, {}
        self._build(curve, 4 * self.np_)

    def _program(self, t, inp):
        ev = not t.build
        B, r, k, ni = t.batch, self.r, self.np_, self.N_INST
        neg = r - 1
        col = lambda vals: t.alloc_full(vals if ev else None)
        seq = lambda traces: self.trace_columns(t, traces)
        block = self._block_recorder(t)
        portal = self.rom_portal_block(t, inp)
        block("portal")
        self.rom_membership_block(t, inp, portal)
        block("membership")
        time_e = portal[0]

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

    @property
    def device_cols(self):
        """(kind, hash_col0, index_col0, path_col0): what hk_vkd_witness takes as `cols`."""
        return (KINDS.index(self.kind), self.cols.get("hash leaf", 0), self.cols.get("get index", 0),
                self.cols.get("compute path", 0))

    def _batch_inputs(self, inputs):
        """inputs: per-subcircuit dicts (`VkdJob.inputs`): what `rom_inputs` takes and the primitives' own: leaf (66 bytes;
        "hash leaf"), sibs (L nodes; "compute path").  What a path starts from and its index word are read from the
        time-ordered entries."""
        inp = super()._batch_inputs(inputs)
        inp["leaf"] = [i.get("leaf") for i in inputs]
        inp["sibs"] = [i.get("sibs") for i in inputs]
        return inp


@functools.lru_cache(maxsize=None)
def vkd_class(curve, kind, n_levels, split, first, last, depth_exec):
    return VkdSubcircuit(curve, kind, n_levels, split, first=first, last=last, depth_exec=depth_exec)


# ---------------------------------------------------------------------------------------------------------------------
class VkdJob(PortalJob):
    """A whole VKD job: N = 8 + 2 split U subcircuits over U updates (6 paddings, write-pp, 2 split per update, the final
    equality), the addresses `SetupRomPortalManager` hands out, the VALUE TABLE every traced value is read from, the
    time-ordered trace, its address order and - once the round's challenges are in - the running evaluations, the
    execution tree and every subcircuit's inputs.  The job never builds the sparse tree: every update carries its siblings,
    or `from_directory` has hk_vkd_tree compute them from the directory's leaves on the device.

    The value table (what hk_vkd_trace writes as `values_out`), V = 3 + U (2 + 3 split) nodes / words:
        0 initial root   1 final root   2 null leaf
        base(u) = 3 + u (2 + 3 split):  + 0 hash of leaf_old (0 for an append)   + 1 hash of leaf_new
                                        + 2 + s index word s of the update's user
                                        + 2 + split + p split + s the node after segment s of path p
    ValueError: N no power of two >= 16; depth no multiple of 8 split or L < 8; a path of another length than depth; a name
    set twice; a name read before it is set (where the reference panics).

    siblings: a `DeviceBuffer` of U x depth Fr (hk_vkd_tree's siblings_mont_out) the job reads instead of the updates' own
    paths, which may then be None; `tables()["siblings"]` is that buffer.  ValueError: given with host_values, or of another
    size than U x depth Fr."""

    def __init__(self, curve, initial_root, final_root, updates, depth=128, split=4, host_values=True, siblings=None):
        self.depth_tree, self.split, self.updates = int(depth), int(split), list(updates)
        self.siblings = siblings
        S, U = self.split, len(self.updates)
        if S < 2 or depth % (8 * S) or depth // S < 8:
            raise ValueError("depth %d over %d segments: L must be a multiple of 8, at least 8, and split >= 2" % (depth, S))
        self.L = L = depth // S
        n = 8 + 2 * S * U
        if n < 16 or n & (n - 1):
            raise ValueError("8 + 2 x %d x %d updates = %d subcircuits: not a power of two >= 16" % (S, U, n))
        if siblings is not None:
            if host_values:
                raise ValueError("siblings on the device: the value table is the device's too (host_values=False)")
            fr = CURVE_PARAMS[curve]["fr_bytes"]
            if not isinstance(siblings, capi.DeviceBuffer) or siblings.nbytes != U * depth * fr:
                raise ValueError("siblings: a DeviceBuffer of %d x %d Fr" % (U, depth))
        elif any(u.path is None or len(u.path) != depth for u in self.updates):
            raise ValueError("every update carries its %d siblings" % depth)
        self._set_shape(curve, n)
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
        self._set_traces([[RomTranscriptEntry(a, 0 if s == SRC_ZERO else vals[s]) for a, s in ops] for ops in self.ops]
                         if host_values else None, lengths=[len(ops) for ops in self.ops])

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

    @classmethod
    def from_directory(cls, ctx, curve, leaves0, changes, depth=128, split=4):
        """An `on_device` job from the directory itself: hk_vkd_tree applies `changes` (`Append` / `Update`, no path needed)
        to the directory of leaves `leaves0` on the device; only the two roots come back.  The siblings stay in HBM
        (`job.siblings`, released by `free()`); `job.status` holds what each change met (ST_*)."""
        changes = list(changes)
        consts, n_consts, ld, nd = device_params(curve, FrCodec(curve))
        consts_d = capi.DeviceBuffer.from_host(ctx, consts)
        try:
            leaves0 = np.frombuffer(b"".join(bytes(x) for x in leaves0), np.uint8)
            sib, roots, status = ctx.vkd_tree(depth, leaves0, [u.kind for u in changes], leaves_table(changes),
                                              (consts_d, n_consts, ld, nd), device_out=True)
        finally:
            consts_d.free()
        try:
            initial, final = FrCodec(curve).dec(roots.to_host())
            st = status.to_host()[:len(changes)].copy()
        finally:
            roots.free()
            status.free()
        try:
            job = cls(curve, initial, final, changes, depth=depth, split=split, host_values=False, siblings=sib)
            job.dev0 = VkdStage0Device(job, ctx)
        except Exception:
            sib.free()
            raise
        job.status = st
        return job

    def free(self):
        for name in ("dev1", "dev0"):
            if getattr(self, name, None) is not None:
                getattr(self, name).free()
                setattr(self, name, None)
        if self.siblings is not None:
            self.siblings.free()
            self.siblings = None

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
    def set_challenges(self, chals, tr_chal=None, ctx=None):
        """`PortalJob.set_challenges`; an `on_device` job runs hk_exec_tree over the device's traces instead."""
        if ctx is None or self.time is not None:
            return super().set_challenges(chals, tr_chal, ctx)
        self._take_challenges(chals, tr_chal)
        self.dev1 = VkdStage1Device(self, ctx, dev0=self.dev0)
        self.root = self.dev1.root

    def inputs(self, idx):
        """The common inputs (`PortalJob.inputs`), and its primitives' own witnesses."""
        w = super().inputs(idx)
        for prim in self.prims[idx]:
            if prim[0] == "hash leaf":
                w["leaf"] = prim[1][1][1]
            elif prim[0] == "compute path":
                _, ui, _p, *s = prim[3][1]
                s = s[0] if s else self.split - 1
                w["sibs"] = self.updates[ui].path[s * self.L:(s + 1) * self.L]
        return w

    def values_bytes(self):
        """Montgomery bytes of the value table: what hk_vkd_trace writes as `values_out`."""
        return FrCodec(self.curve).enc(self.values)

    def tables(self):
        """The job as hk_vkd_desc states it (`Context.vkd_trace` takes this dict)."""
        fc = FrCodec(self.curve)
        siblings = self.siblings if self.siblings is not None else fc.enc([x for u in self.updates for x in u.path])
        return dict(depth=self.depth_tree, split=self.split, n_updates=len(self.updates),
                    kinds=np.array([u.kind for u in self.updates], np.uint32), leaves=leaves_table(self.updates),
                    siblings=siblings,
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


class VkdStage0Device(PortalStage0Device):
    """`values` (the value table) and `traces = [time, addr]` - value table and time-ordered trace computed by hk_vkd_trace -
    and `params`, the Poseidon parameters on the device."""

    def _time_trace(self):
        consts, n_consts, ld, nd = device_params(self.job.curve, FrCodec(self.job.curve))
        self.params = (self._own(capi.DeviceBuffer.from_host(self.ctx, consts)), n_consts, ld, nd)
        self.values, time = (self._own(x) for x in self.ctx.vkd_trace(self.job.tables(), self.params, device_out=True))
        return time


class VkdStage1Device(PortalStage1Device):
    """The job's value table, traces and hk_exec_tree's outputs as DeviceBuffers; `fill(circ, members, z)` writes whole
    assignment rows of one class from them (hk_vkd_witness + hk_stage1_witness) and `check(pk, z, members)` tests them where
    they lie (hk_pk_r1cs_check).  dev0: the `VkdStage0Device` to read instead of making one here."""

    def __init__(self, job, ctx, dev0=None):
        self.tables = job.tables()
        super().__init__(job, ctx, job.chal, dev0=dev0)

    def _traces(self, dev0=None):
        self.dev0 = dev0 if dev0 is not None else self._own(VkdStage0Device(self.job, self.ctx))
        return self.dev0.traces

    def _params(self):
        return self.dev0.params                            # the stage-0 device's, which stay its own

    def fill(self, circ, members, z):
        """Row b of the DeviceBuffer z (len(members) x circ.n_v Fr) <- the assignment of subcircuit members[b], all of class
        `circ`: every column of the row is written by one of the two calls."""
        members = np.ascontiguousarray(members, dtype=np.uint32)
        self.ctx.vkd_witness(self.tables, self.params, self.dev0.values, members, circ.n_v, circ.device_cols, z)
        self._stage1_witness(circ, members, z)
        return z
