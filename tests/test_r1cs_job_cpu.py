"""CPU: the partitioned R1CS job (hekaton_system_amd/r1cs_circuit.py; distributed-prover/src/partitioned_r1cs_circuit.rs).
The `.meta` reader, the trace against a name-keyed restatement of `SetupRomPortalManager` that knows nothing of the closed
form 1 + g O + rank, the job's errors, R1CS satisfaction of every class of the three fixture jobs beside the imported
constraints on the circom witness itself, two tamperings and which block they break, the QAP evaluation against the CSR, the
three files on disk, and the two C symbols."""
import os

import numpy as np
import pytest

from hekaton_system_amd import capi, circom
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec, r1cs_bad_rows
from hekaton_system_amd.r1cs_circuit import (Partition, PartitionedR1csJob, R1csSubcircuit, SRC_ZERO, read_meta, write_meta)
from tests.r1cs_job_fixtures import (CHAL, JOBS, Chain, circom_bad_rows, job_parts, make_job, make_partition, owner_tampering,
                                     partition_files, solve_tx, tampered)

R = CURVE_PARAMS["bn254"]["r"]


# ---- .meta ----------------------------------------------------------------------------------------------------------
def test_meta_round_trip():
    for owned, borrowed in (([], []), ([7], []), ([], [3, 9]), ([10, 11, 4], [8, 2])):
        assert read_meta(write_meta(owned, borrowed)) == (owned, borrowed)
    # integer [1] of the first line is the owned count whatever stands around it
    assert read_meta("99 2 77 5\n4\n6\n8\n") == ([4, 6], [8])


def test_meta_first_line_as_the_reference_parses_it():
    # split on single spaces, tokens that are no unsigned integers dropped: "shared" and "-1" go, so do the empty tokens
    # of a double space; "+2" parses (Rust's usize::from_str takes a leading plus)
    assert read_meta("shared 5 -1 +2 x\n10\n20\n30\n") == ([10, 20], [30])
    assert read_meta("5  1\r\n10\r\n20\r\n") == ([10], [20])
    with pytest.raises(ValueError):
        read_meta("owned 3\n1\n2\n3\n")                # one integer only: first_line_integers[1] is out of bounds
    with pytest.raises(ValueError):
        read_meta("2 1\n10\nx\n")                      # a later line must parse
    with pytest.raises(ValueError):
        read_meta("2 1\n10\n\n")                       # an empty line does not
    with pytest.raises(ValueError):
        read_meta("2 3\n10\n20\n")                     # split_off past the end
    with pytest.raises(ValueError):
        read_meta("")


# ---- the trace against the portal manager, restated with names ------------------------------------------------------
def setup_rom_portal_manager_trace(parts, n_txs, witnesses):
    """`get_portal_subtraces` (:182-220) over `SetupRomPortalManager` (rom_portal_manager.rs:34-117): a map from variable
    names to (addr, val), addresses from a counter."""
    var_map, next_addr, subtraces = {}, [1], []

    def set_(name, val):
        assert name not in var_map, "cannot set portal wire more than once; wire '%s'" % name
        var_map[name] = (next_addr[0], val)
        next_addr[0] += 1
        subtraces[-1].append(var_map[name])

    def get(name):
        subtraces[-1].append(var_map[name])

    P = len(parts)
    for idx in range(P * n_txs):
        subtraces.append([])
        part, group = parts[idx % P], idx // P
        wit = witnesses[group][idx % P] if witnesses is not None else part.witness
        n_unique = part.n_wires - len(part.owned) - len(part.borrowed)
        for i, var_index in enumerate(part.owned):
            set_("var%d_%d" % (group, var_index), wit[n_unique + i])
        for var_index in part.borrowed:
            get("var%d_%d" % (group, var_index))
        if P == 1:
            set_("dummy%d" % idx, 0)
    return subtraces


@pytest.mark.parametrize("name", sorted(JOBS))
def test_trace_equals_the_named_portal_manager(name):
    parts, wits = job_parts(name)
    job = make_job("bn254", name, chal=None)
    want = setup_rom_portal_manager_trace(parts, JOBS[name][1], wits)
    assert [[(e.addr, e.val) for e in st] for st in job.time] == want
    assert job.offsets.tolist() == np.concatenate([[0], np.cumsum([len(st) for st in want])]).tolist()
    # subcircuit i is partition i % P of transaction i // P; a class is (partition, first, last)
    assert [job.class_of(i) for i in range(job.n)] == [(i % job.P, i == 0, i == job.n - 1) for i in range(job.n)]


def test_shared_witnesses_repeat_the_partitions_own():
    # the default: every transaction uses the partitions' own witnesses (:104, 124), under fresh addresses
    parts, _ = job_parts("p4t4")
    job = PartitionedR1csJob("bn254", parts, 4)
    assert job.tx_stride == 0 and len(job.wit_blocks) == 1
    assert [[(e.addr, e.val) for e in st] for st in job.time] == setup_rom_portal_manager_trace(parts, 4, None)
    assert job.time[0][0].val == job.time[4][0].val and job.time[4][0].addr == job.time[0][0].addr + job.sets_per_tx


def test_fixture_family_has_what_the_indexing_can_get_wrong():
    chains = JOBS["p4t4"][0]
    owner = {vid: p for p, c in enumerate(chains) for vid in c.owned}
    borrowers = {}
    for p, c in enumerate(chains):
        for vid in c.borrowed:
            borrowers.setdefault(vid, []).append(p)
    assert any(p - owner[vid] > 1 for vid, ps in borrowers.items() for p in ps)        # from a non-adjacent partition
    assert any(len(ps) >= 2 for ps in borrowers.values())                               # borrowed by two partitions
    assert any(vid not in borrowers for vid in owner)                                   # owned, borrowed by nobody
    cons = [x for c in chains for x in c.constraints()]
    assert any(len(a) >= 3 and len(c_) >= 3 for a, _b, c_ in cons) and any(len(b) >= 2 for _a, b, _c in cons)
    assert any(i == 0 and coeff != 1 for a, b, _c in cons for i, coeff in a + b)        # wire 0 under another coefficient
    assert sorted(len(c.owned) + len(c.borrowed) for c in chains) == [1, 2, 4, 5]
    parts, _ = job_parts("p4t4")
    assert [p.body_len for p in parts[:2]] == [66, 128]                                 # 67 and 130 with column 0: across a wave
    assert JOBS["p1t2"][0][0].owned == [] and JOBS["p1t2"][0][0].borrowed == []         # the dummy only


# ---- the job's errors ------------------------------------------------------------------------------------------------
def _part(chain, shared=None):
    return make_partition(chain, chain.solve(1, dict(shared or {})))


def test_job_value_errors():
    a, b = Chain(9, owned=[1]), Chain(8, borrowed=[1])
    pa, pb = _part(a), _part(b, {1: 5})
    PartitionedR1csJob("bn254", [pa, pb], 1)
    with pytest.raises(ValueError, match="cannot get portal wire"):
        PartitionedR1csJob("bn254", [pb, pa], 1)                                        # the owner comes later
    with pytest.raises(ValueError, match="cannot get portal wire"):
        PartitionedR1csJob("bn254", [pa, _part(Chain(8, borrowed=[2]), {2: 5})], 1)     # nobody owns id 2
    with pytest.raises(ValueError, match="more than once"):
        PartitionedR1csJob("bn254", [pa, _part(Chain(9, owned=[1]))], 1)                # owned by two partitions
    with pytest.raises(ValueError, match="more than once"):
        PartitionedR1csJob("bn254", [_part(Chain(9, owned=[4, 4])), pb], 1)             # twice in one partition
    for parts, n_txs in (([pa, pb], 3), ([pa], 1), ([pa, pb, pb], 1)):                  # 6, 1, 3 subcircuits
        with pytest.raises(ValueError, match="power of two"):
            PartitionedR1csJob("bn254", parts, n_txs)
    with pytest.raises(ValueError, match="no portal"):
        PartitionedR1csJob("bn254", [pa, _part(Chain(6))], 1)                           # hk_stage1_witness refuses k = 0
    with pytest.raises(ValueError):
        R1csSubcircuit("bn254", _part(Chain(6)), depth=1, dummy=False)
    with pytest.raises(ValueError):
        PartitionedR1csJob("bn254", [pa, pb], 1, witnesses=[[pa.witness]])              # witnesses[g][p]


# ---- satisfaction ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
@pytest.mark.parametrize("name", sorted(JOBS))
def test_every_class_is_satisfied(cname, name):
    job = make_job(cname, name)
    r = CURVE_PARAMS[cname]["r"]
    seen = set()
    for idx in range(job.n):
        circ = job.make_class(idx)
        assert circom_bad_rows(job.parts[idx % job.P], job.wires(idx), r) == []
        z = job.assignment_ints(idx)
        assert len(z) == circ.n_v and r1cs_bad_rows(*circ.rows(), z, r) == []
        # the layout the device calls rely on
        k, part = circ.np_, circ.part
        assert circ.n0 == 4 * k and circ.pos_col0 == 4 + 10 * k + 4 and circ.body_col0 == circ.pos_col0 + circ.pos_cols
        assert circ.n_v == circ.body_col0 + part.body_len
        assert z[circ.body_col0:] == [v % r for v in job.wires(idx)[1:part.u + part.n_owned]]
        assert z[4:4 + circ.n0] == job.stage0_ints(idx)
        seen.add(job.class_of(idx))
    assert len(seen) == {"p1t2": 2, "p2t1": 2, "p4t4": 6}[name]
    # a class is built once
    assert job.make_class(0) is job.make_class(0)


def test_closed_form_addresses_and_tables():
    job = make_job("bn254", "p4t4", chal=None)
    t = job.tables()
    assert t["sets_per_tx"] == 5 and t["slot_offsets"].tolist() == [0, 1, 3, 7, 12] and t["tx_stride"] == t["tx_len"] == 242
    assert t["wit_offsets"].tolist() == [0, 67, 197, 221, 242] and t["body_len"].tolist() == [66, 128, 21, 16]
    flat = [e for st in job.time for e in st]
    S = 12
    for e_idx, e in enumerate(flat):
        g, s = divmod(e_idx, S)
        assert e.addr == 1 + g * 5 + t["slot_rank"][s] and e.val == job.wit_blocks[g][t["slot_src"][s]]
    d = make_job("bn254", "p1t2", chal=None).tables()
    assert d["slot_src"].tolist() == [SRC_ZERO] and d["slot_rank"].tolist() == [0] and d["sets_per_tx"] == 1 and d["tx_stride"] == 0


# ---- tamperings ------------------------------------------------------------------------------------------------------
def test_tampered_owner_value_fails_an_owner_body_row():
    job, honest = owner_tampering("bn254")
    circ = job.make_class(5)
    bad = r1cs_bad_rows(*circ.rows(), job.assignment_ints(5), R)
    # the trace carries the changed value, so the `set`'s equality row holds: the imported constraint that defines the wire
    # does not, and it is the owner's LAST imported constraint
    assert bad == [circ.blocks["constraints"][1] - 1] and circ.block_of(bad[0]) == "constraints"
    lo, hi = circ.blocks["owned"]
    assert hi - lo == 1 and hi <= bad[0]
    # the borrowers of the same transaction consume the changed value: their first failing row is the borrowing constraint
    for sub in (6, 7):
        c = job.make_class(sub)
        rows = r1cs_bad_rows(*c.rows(), job.assignment_ints(sub), R)
        assert rows and all(c.block_of(x) == "constraints" for x in rows)
    # no other transaction and no earlier partition sees it
    for sub in (0, 1, 4, 9, 15):
        assert r1cs_bad_rows(*job.make_class(sub).rows(), job.assignment_ints(sub), R) == []
    assert honest.time[5] != job.time[5]


def test_tampered_borrower_copy_changes_nothing():
    # partition 2 borrows ids 10 and 20 as its wires 22 and 23: its own value for them is never read
    job, honest = tampered("bn254", 6, 23, delta=12345)
    assert job.time == honest.time and job.addr == honest.addr
    for idx in range(job.n):
        assert (job.assignment_bytes(idx) == honest.assignment_bytes(idx)).all()


# ---- key generation's view --------------------------------------------------------------------------------------------
def test_qap_evaluate_against_the_csr():
    job = make_job("bn254", "p2t1")
    circ = job.make_class(1)                           # partition 1, the last subcircuit
    fc = FrCodec("bn254")
    t_pt = 0x1f2e3d4c5b6a7988
    a, b, c, zt, m = circ.qap_evaluate(t_pt)
    assert m >= circ.n_c + circ.N_INST and zt == (pow(t_pt, m, R) - 1) % R
    # the same sums from the CSR triples and the Lagrange basis at t_pt, column by column
    g = CURVE_PARAMS["bn254"]
    w = pow(pow(g["gen"], (R - 1) >> g["two_adicity"], R), 1 << (g["two_adicity"] - (m.bit_length() - 1)), R)
    u = [zt * pow(w, i, R) % R * pow(m * (t_pt - pow(w, i, R)) % R, -1, R) % R for i in range(circ.n_c + circ.N_INST)]
    want = []
    for rp, col, val in circ.csr(fc):
        vals = fc.dec(val)
        acc = [0] * circ.n_v
        for i in range(circ.n_c):
            for k in range(int(rp[i]), int(rp[i + 1])):
                acc[int(col[k])] = (acc[int(col[k])] + u[i] * vals[k]) % R
        want.append(acc)
    for j in range(circ.N_INST):
        want[0][j] = (want[0][j] + u[circ.n_c + j]) % R
    assert [a, b, c] == want
    # the CSR rows are the tape's rows: satisfied through either
    A, B, C = circ.rows()
    assert len(A) == circ.n_c == int(circ.csr(fc)[0][0].size) - 1
    # two stages: the 4 k stage-0 columns, then the rest
    assert circ.total_num_stages() == 2


# ---- the three files on disk ------------------------------------------------------------------------------------------
def test_load_from_files(tmp_path):
    chains, n_txs, _ = JOBS["p2t1"]
    base = str(tmp_path / "circuit")
    for p, (c, w) in enumerate(zip(chains, solve_tx(chains, 1))):
        r1cs_b, json_t, meta_t = partition_files(c, w)
        for ext, data in ((".r1cs", r1cs_b), (".json", json_t.encode()), (".meta", meta_t.encode())):
            with open("%s.%d%s" % (base, p, ext), "wb") as f:
                f.write(data)
    job = PartitionedR1csJob.load("bn254", base, 2, n_txs)
    want = make_job("bn254", "p2t1", chal=None)
    assert job.time == want.time and [p.owned for p in job.parts] == [[1], []] and [p.borrowed for p in job.parts] == [[], [1]]
    assert isinstance(job.parts[0], Partition) and isinstance(job.parts[0].r1cs, circom.R1CSFile)
    job.set_challenges(CHAL)
    want.set_challenges(*CHAL)
    assert job.root == want.root and (job.assignment_bytes(1) == want.assignment_bytes(1)).all()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_library_exports_the_two_calls():
    lib = capi.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hekaton.h")).read()
    for sym in ("hk_r1cs_job_trace", "hk_r1cs_job_witness"):
        assert sym in capi.EXPORTS and sym + "(" in hdr and getattr(lib, sym) is not None
    assert "#define HK_R1CS_SRC_ZERO 0xFFFFFFFFu" in hdr and SRC_ZERO == 0xFFFFFFFF
    # the ctypes mirror has the header's fields in the header's order
    body = hdr[hdr.index("#define HK_R1CS_SRC_ZERO"):hdr.index("} hk_r1cs_job_desc;")]
    import re
    declared = re.findall(r"^\s+(?:const\s+)?(?:uint32_t|void)\*?\s+(\w+);", body, re.M)
    assert declared == [n for n, _ in capi.hk_r1cs_job_desc._fields_]
