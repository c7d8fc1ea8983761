"""CPU: the VKD job (hekaton_system_amd/vkd_circuit.py; distributed-prover/src/vkd/*.rs).  The hashes' chunking and
truncation, the sparse tree against a bottom-up recomputation, the subcircuit layout against workload.py's class map and the
reference's type strings, the trace against a name-keyed restatement of `SetupRomPortalManager` that knows nothing of the
value table, R1CS satisfaction of every subcircuit of jobs A and B, six tamperings and the block each breaks first, and the
two C symbols."""
import os

import pytest

from hekaton_system_amd import capi, workload
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, r1cs_bad_rows
from hekaton_system_amd.poseidon import merkle_params
from hekaton_system_amd.vkd_circuit import (Append, KINDS, NODE_BITS, NODE_MASK, SRC_ZERO, SparseTree, Update, VkdJob, chunks,
                                            compute_root, concat, get_index, hash_inner_node, hash_leaf, vkd_digest, vkd_hash)
from tests.vkd_fixtures import CHAL, DEPTH, SPLIT, job_a, job_b, job_small, updates_b

CURVES = ["bn254", "bls12_381"]
TYPES = {"padding", "write pp", "hash leaf, get index, compute path", "compute path", "compute path, equality",
         "equality, hash leaf, compute path", "equality"}                  # vkd_constraints.rs:203-214


# ---- hashes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_hashes_chunk_and_truncate_as_the_reference(curve):
    leaf_cfg, node_cfg = merkle_params(curve)
    leaf, name = bytes(range(1, 67)), bytes(range(100, 132))
    assert [len(leaf[i:i + 27]) for i in range(0, 66, 27)] == [27, 27, 12] and len(chunks(leaf)) == 3
    assert chunks(name) == [int.from_bytes(name[:27], "little"), int.from_bytes(name[27:], "little")]
    # one permutation each: 3 (2) inputs at rate 3
    for data in (leaf, name):
        trace = []
        d = vkd_digest(curve, data, trace)
        assert d == leaf_cfg.crh(chunks(data)) and len(trace) == 8 * (4 * 3 + 4) + 56 * (3 + 4)
        assert vkd_hash(curve, data) == d.to_bytes(32, "little")
    assert hash_leaf(curve, leaf) == int.from_bytes(vkd_hash(curve, leaf)[:27], "little")
    a, b = hash_leaf(curve, leaf), hash_leaf(curve, name)
    full = node_cfg.crh([a, b])
    assert hash_inner_node(curve, a, b) == int.from_bytes(full.to_bytes(32, "little")[:27], "little") == full & NODE_MASK
    assert (leaf_cfg.rate, leaf_cfg.alpha, node_cfg.rate, node_cfg.alpha) == (3, 5, 2, 17)
    circ = job_small(curve).make_class(0)
    assert circ.leaf_cfg is leaf_cfg and circ.node_cfg is node_cfg        # the gadget hashes with the same two instances
    assert get_index(curve, name, 32) == int.from_bytes(vkd_hash(curve, name)[:4], "little")
    assert concat(name, leaf[:32], 0x0201) == name + b"\x01\x02" + leaf[:32]


# ---- the tree ---------------------------------------------------------------------------------------------------------------
def _bottom_up_root(curve, depth, leaves):
    """The root of the sparse tree holding {index: leaf bytes}, level by level over the occupied nodes only."""
    empty = [hash_leaf(curve, bytes(32))]
    for _ in range(depth):
        empty.append(hash_inner_node(curve, empty[-1], empty[-1]))
    level = {i: hash_leaf(curve, x) for i, x in leaves.items()}
    for h in range(depth):
        level = {p: hash_inner_node(curve, level.get(2 * p, empty[h]), level.get(2 * p + 1, empty[h]))
                 for p in {i >> 1 for i in level}}
    return level.get(0, empty[depth])


@pytest.mark.parametrize("curve", CURVES)
def test_tree_agrees_with_a_bottom_up_recomputation(curve):
    depth = 16
    tree = SparseTree(curve, depth)
    assert tree.root == _bottom_up_root(curve, depth, {}) and tree.null_leaf == hash_leaf(curve, bytes(32))
    assert len(tree.sparse_initial_hashes) == depth + 1
    held = {}
    for k in range(4):
        name = bytes([k + 1]) * 32
        idx, leaf = get_index(curve, name, depth), concat(name, bytes([9 - k]) * 32, k)
        path = tree.lookup_path(idx)
        assert compute_root(curve, tree.null_leaf, path, idx) == tree.root                # the empty leaf is under the root
        tree.insert(idx, leaf)
        held[idx] = leaf
        assert tree.root == _bottom_up_root(curve, depth, held)
        assert compute_root(curve, hash_leaf(curve, leaf), path, idx) == tree.root        # ... and the new one after
        # a path cut into segments walks through the same nodes
        node = hash_leaf(curve, leaf)
        for s in range(2):
            node = compute_root(curve, node, path[s * 8:(s + 1) * 8], idx, s * 8)
        assert node == tree.root


@pytest.mark.parametrize("curve", CURVES)
def test_random_jobs_verify_and_tampered_ones_do_not(curve):
    for log_n in (4, 5):
        job = VkdJob.random(curve, log_n, DEPTH, SPLIT)
        assert job.n == 1 << log_n and job.verify()
        assert [u.kind for u in job.updates] == [0] + [1] * (len(job.updates) - 1)
    ups = list(job.updates)
    u = ups[1]
    v = ups[-1]
    ups[-1] = Update(v.username, v.counter, v.key1, bytes([0x55]) * 32, v.path)                      # another key
    assert not VkdJob(curve, job.initial_root, job.final_root, ups, DEPTH, SPLIT).verify()
    ups[-1] = v
    ups[1] = Update(u.username, u.counter, u.key1, u.key2, u.path[:5] + [u.path[5] ^ 1] + u.path[6:])  # another sibling
    assert not VkdJob(curve, job.initial_root, job.final_root, ups, DEPTH, SPLIT).verify()
    assert not VkdJob(curve, job.initial_root, job.final_root ^ 1, job.updates, DEPTH, SPLIT).verify()
    assert job_b(curve).verify()


# ---- the layout ---------------------------------------------------------------------------------------------------------------
def test_layout_equals_the_class_map_and_the_type_strings():
    for log_n in (4, 5, 6):
        job = VkdJob.random("bn254", log_n, DEPTH, SPLIT)
        n = job.n
        assert n == 1 << log_n and len(job.updates) == (n - 8) // 8
        for i in range(n):
            assert job.class_rep(i) == workload.representative_subcircuit("vkd", n, i), i
            assert job.type_of(i) in TYPES and job.type_of(i) == job.type_of(job.class_rep(i))
            assert job.class_of(i) == (job.type_of(i), i == 0, i == n - 1)
        assert [job.type_of(i) for i in (0, 5, 6, 7, 8, 9, 10, 11, 14, n - 1)] == \
            ["padding", "padding", "write pp", "hash leaf, get index, compute path", "compute path", "compute path",
             "compute path, equality", "compute path", "compute path", "equality"]
        if log_n > 4:
            assert job.type_of(19) == "equality, hash leaf, compute path" and job.type_of(15) == job.type_of(18) == "compute path"
            assert sorted({job.class_rep(i) for i in range(n)}) == sorted(set(workload.unique_subcircuits("vkd", n)))
        assert len(job.classes()) == (8 if log_n > 4 else 7)          # one more than the reference: subcircuit 0 is `first`
    assert set(KINDS) == TYPES
    small = job_small("bn254")
    assert (small.n, small.L, len(small.updates)) == (16, 8, 2)
    assert small.types[7:15] == ["hash leaf, get index, compute path", "compute path, equality", "compute path", "compute path",
                                 "compute path", "compute path", "equality, hash leaf, compute path", "compute path"]


def test_job_value_errors():
    curve = "bn254"
    job = job_a(curve, chal=False)
    init, fin, ups = job.initial_root, job.final_root, job.updates
    with pytest.raises(ValueError):
        VkdJob(curve, init, fin, ups[:2], DEPTH, SPLIT)                # N = 24
    with pytest.raises(ValueError):
        VkdJob(curve, init, fin, [], DEPTH, SPLIT)                     # N = 8
    with pytest.raises(ValueError):
        VkdJob(curve, init, fin, [ups[0], ups[0], ups[1]], DEPTH, SPLIT)       # a user appended twice: a name set twice
    with pytest.raises(ValueError):
        VkdJob(curve, init, fin, [ups[1], ups[2], ups[2]], DEPTH, SPLIT)       # an update of a user nothing appended
    other = Update(bytes([7]) * 32, 0, bytes(32), bytes(32), ups[1].path)
    with pytest.raises(ValueError):
        VkdJob(curve, init, fin, [ups[0], other, ups[1]], DEPTH, SPLIT)
    stale = Update(ups[1].username, 5, ups[1].key1, ups[1].key2, ups[1].path)  # a leaf1 never hashed in this batch
    with pytest.raises(ValueError):
        VkdJob(curve, init, fin, [ups[0], stale, ups[2]], DEPTH, SPLIT)
    with pytest.raises(ValueError):
        VkdJob(curve, init, fin, ups, 36, SPLIT)                       # L = 9
    with pytest.raises(ValueError):
        VkdJob(curve, init, fin, ups, 16, SPLIT)                       # L = 4
    with pytest.raises(ValueError):
        VkdJob(curve, init, fin, ups, 64, SPLIT)                       # 32 siblings for 64 levels
    with pytest.raises(ValueError):
        VkdJob.random(curve, 3, DEPTH, SPLIT)


# ---- the trace against the portal manager, restated with names ---------------------------------------------------------
def named_portal_manager_trace(curve, initial_root, final_root, updates, depth, split):
    """`get_portal_subtraces` (vkd_constraints.rs:70-193) over `SetupRomPortalManager` (rom_portal_manager.rs:34-117) and the
    primitive list of `vkd_update_to_subcircuit` (vkd.rs:362-617): a map from address strings to (addr, val), addresses from
    a counter, values from the host hashes.  Knows nothing of a value table."""
    var_map, next_addr, subtraces, L = {}, [1], [], depth // split

    def set_(name, val):
        assert name not in var_map, name
        var_map[name] = (next_addr[0], val)
        next_addr[0] += 1
        subtraces[-1].append(var_map[name])

    def get(name):
        subtraces[-1].append(var_map[name])
        return var_map[name][1]

    def hash_leaf_prim(leaf):
        set_("leaf hash %s" % leaf.hex(), hash_leaf(curve, leaf))

    def get_index_prim(name):
        idx = get_index(curve, name, depth)
        for s in range(split):
            set_("index %d of %s" % (s, name.hex()), (idx >> (s * L)) % (1 << L))

    def node_name(ui, p, s):
        return "path root %d.%d" % (ui, p) if s == split - 1 else "intermediate %d.%d.%d" % (ui, p, s)

    def path_prim(ui, p, s, first_name, u):
        node = get(node_name(ui, p, s - 1) if s else first_name)
        word = get("index %d of %s" % (s, u.username.hex()))
        for j, sib in enumerate(u.path[s * L:(s + 1) * L]):
            node = hash_inner_node(curve, sib, node) if (word >> j) & 1 else hash_inner_node(curve, node, sib)
        set_(node_name(ui, p, s), node)

    def sub(*prims):
        subtraces.append([])
        for f in prims:
            f()

    for p in range(6):
        sub(lambda p=p: set_("pad%d" % p, 0))
    sub(lambda: (set_("initial root", initial_root), set_("final root", final_root),
                 set_("null leaf", hash_leaf(curve, bytes(32)))))
    prev = "initial root"
    for ui, u in enumerate(updates):
        equal = lambda ui=ui, prev=prev: (get("path root %d.0" % ui), get(prev))
        new = "leaf hash %s" % u.leaf_new.hex()
        if isinstance(u, Append):
            for s in range(split):
                prims = [lambda s=s: path_prim(ui, 0, s, "null leaf", u)]
                if s == 0:
                    prims = [lambda: hash_leaf_prim(u.leaf_new), lambda: get_index_prim(u.username)] + prims
                if s == split - 1:
                    prims.append(equal)
                sub(*prims)
            for s in range(split):
                sub(lambda s=s: path_prim(ui, 1, s, new, u))
        else:
            for s in range(split):
                sub(lambda s=s: path_prim(ui, 0, s, "leaf hash %s" % u.leaf_old.hex(), u))
            sub(equal, lambda: hash_leaf_prim(u.leaf_new), lambda: path_prim(ui, 1, 0, new, u))
            for s in range(1, split):
                sub(lambda s=s: path_prim(ui, 1, s, new, u))
        prev = "path root %d.1" % ui
    sub(lambda: (get("final root"), get(prev)))
    return subtraces


@pytest.mark.parametrize("curve", CURVES)
def test_trace_equals_the_named_portal_manager(curve):
    for job in (job_a(curve), job_b(curve), job_small(curve)):
        want = named_portal_manager_trace(curve, job.initial_root, job.final_root, job.updates, job.depth_tree, job.split)
        assert [[(e.addr, e.val) for e in st] for st in job.time] == want
        flat = [x for st in want for x in st]
        assert job.slot_addr.tolist() == [a for a, _ in flat] and job.offsets[-1] == len(flat)
        assert [0 if s == SRC_ZERO else job.values[s] for s in job.slot_src.tolist()] == [v for _, v in flat]
        assert len(job.values) == 3 + len(job.updates) * (2 + 3 * job.split)
        # the last path root is the final root, and the addresses are 1 .. number of `set`s
        assert job.values[-1] == job.final_root and sorted(set(job.slot_addr.tolist())) == list(range(1, max(job.slot_addr) + 1))


# ---- satisfaction -----------------------------------------------------------------------------------------------------------
def _bad(job, idx, z=None, **override):
    circ = job.make_class(idx)
    z = job.assignment_ints(idx, **override) if z is None else z
    rows = r1cs_bad_rows(*circ.rows(), z, circ.r)
    return rows, [circ.block_of(x) for x in rows]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("name", ["a", "b"])
def test_every_subcircuit_satisfies_its_class(curve, name):
    job = {"a": job_a, "b": job_b}[name](curve)
    assert job.n == 32 and len(job.classes()) == 8
    for i in range(job.n):
        circ = job.make_class(i)
        assert _bad(job, i)[0] == [], (i, job.type_of(i))
        assert circ.n_v == circ.body_col0 + circ.body_cols and sum(hi - lo for r in circ.blocks.values() for lo, hi in r) == circ.n_c
    want = {"padding": {"pad"}, "write pp": set(), "equality": {"equal"},
            "compute path": {"index", "select", "hash", "bits", "canon", "trunc"}}
    for i in (1, 6, 31, 8):
        assert set(job.make_class(i).blocks) - {"portal", "membership"} == want[job.type_of(i)]


# ---- tamperings ---------------------------------------------------------------------------------------------------------------
def _path_cols(circ, level):
    """(sibling, left, first digest bit, first canon, node) columns of a level of the class's compute path."""
    nb = circ.nbits
    nc = bin(circ.r - 1).count("1") - 1
    at = circ.cols["compute path"] + circ.L + level * (2 + 392 + nb + nc + 1)
    return at, at + 1, at + 2 + 392, at + 2 + 392 + nb, at + 2 + 392 + nb + nc


def _upstream_clean(job, upto):
    return all(_bad(job, i)[0] == [] for i in range(upto))


@pytest.mark.parametrize("curve", CURVES)
def test_tamperings_break_the_named_block_first(curve):
    job = job_a(curve)
    r = CURVE_PARAMS[curve]["r"]
    idx = 12                                                        # a plain compute path: segment 1 of the new leaf's path
    circ = job.make_class(idx)
    honest = job.assignment_ints(idx)
    # a flipped index bit: the unpacking no longer sums to the word, and level 2 selects the other child
    z = list(honest)
    z[circ.cols["compute path"] + 2] ^= 1
    rows, blocks = _bad(job, idx, z)
    assert set(blocks) == {"index", "select"} and blocks[0] == "index"
    # a truncated node that keeps one bit above 216
    z = list(honest)
    z[_path_cols(circ, 3)[4]] += 1 << NODE_BITS
    rows, blocks = _bad(job, idx, z)
    assert blocks[0] == "trunc" and set(blocks) <= {"trunc", "select", "hash"}
    # the digest's bits replaced by those of digest + r: the same field element, no longer below r
    # (about a third of all digests on BN254, a tenth on BLS12-381, lie below 2^bits - r: search the job's, take the first)
    hits = [(j, l) for j in range(7, job.n - 1) for c, zz in [(job.make_class(j), job.assignment_ints(j))] for l in range(c.L)
            if sum(zz[_path_cols(c, l)[2] + i] << i for i in range(c.nbits)) + r < 1 << c.nbits]
    assert hits
    j, level = hits[0]
    c, zz = job.make_class(j), job.assignment_ints(j)
    b0 = _path_cols(c, level)[2]
    d = sum(zz[b0 + i] << i for i in range(c.nbits))
    for i in range(c.nbits):
        zz[b0 + i] = ((d + r) >> i) & 1
    rows, blocks = _bad(job, j, zz)
    assert blocks[0] == "canon" and set(blocks) <= {"canon", "trunc"}
    # a non-zero pad
    pad = job.make_class(2)
    z = job.assignment_ints(2)
    z[pad.N_INST + 1] = 1                                           # the `val` of the one time-ordered entry
    rows, blocks = _bad(job, 2, z)
    assert "pad" in blocks and set(blocks) <= {"portal", "pad"}


@pytest.mark.parametrize("curve", CURVES)
def test_wrong_sibling_and_wrong_final_root_break_an_equality(curve):
    job = job_a(curve, chal=False)
    ups = list(job.updates)
    u = ups[1]
    ups[1] = Update(u.username, u.counter, u.key1, u.key2, u.path[:9] + [u.path[9] ^ 1] + u.path[10:])
    bad = VkdJob(curve, job.initial_root, job.final_root, ups, DEPTH, SPLIT)
    bad.set_challenges(*CHAL)
    eq = 7 + 8 + 4                                                  # update 1's "equality, hash leaf, compute path"
    assert bad.type_of(eq).startswith("equality") and _upstream_clean(bad, eq)
    rows, blocks = _bad(bad, eq)
    assert blocks == ["equal"]
    wrong = VkdJob(curve, job.initial_root, job.final_root ^ 2, job.updates, DEPTH, SPLIT)
    wrong.set_challenges(*CHAL)
    assert _upstream_clean(wrong, wrong.n - 1)
    rows, blocks = _bad(wrong, wrong.n - 1)
    assert blocks == ["equal"]


def test_the_two_symbols_are_declared_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "hekaton.h")).read()
    for sym in ("hk_vkd_trace", "hk_vkd_witness"):
        assert sym in capi.EXPORTS and "hk_status %s(" % sym in header
    assert "HK_VKD_SRC_ZERO 0xFFFFFFFFu" in header and SRC_ZERO == 0xFFFFFFFF
