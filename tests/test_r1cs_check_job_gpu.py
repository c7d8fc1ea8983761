"""GPU: the reference's protocol-integration test (distributed-prover/src/subcircuit_circuit.rs:311-399: build the coordinator
state, make every stage-1 request, synthesize every subcircuit, assert cs.is_satisfied()) on witnesses that were generated
on the device and never left it, for the smallest ShaMerkleJob the suite uses (8 subcircuits, 1 SHA-256 iteration, 4 portals).

Per class: the matrices go up once, the members' assignments are made where they stay - the class's word program
(hk_wprog_run), then Stage1Device.fill (hk_stage1_witness) - and ONE batched hk_r1cs_check says n_bad == 0 for all of them;
Stage1Device.check does the same through its key argument.  Then one portal value of one leaf row is overwritten on the device
and the call must report exactly the rows the host mirror reports.  The mirror runs over the rows whose A, B or C mention that
column - every other row reads the same values as before and was just found satisfied - on the class's own host assignment
(sha_circuit.assignment_ints) with the same value replaced.

The tamper check is done on the leaf class only: it is the class with more than one member besides the parents, and one
class is enough to show that (assignment, row) pairs are not mixed up; every class goes through the satisfied check."""
import random

import numpy as np
import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import CURVE_PARAMS, FrCodec, r1cs_bad_rows
from hekaton_system_amd.sha_circuit import R1csUnsatisfied, ShaMerkleJob, program_inputs

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF


class _ClassMatrices:
    """A class's matrices resident on the device, with DevicePk's r1cs_check: what Stage1Device.check needs of a key (a real
    key would add a trusted setup of ~30 000 rows per class to this test and nothing the check reads)."""

    def __init__(self, ctx, circ):
        self.ctx = ctx
        self.bufs = [tuple(capi.DeviceBuffer.from_host(ctx, x) for x in m) for m in circ.csr(circ.fc)]

    def r1cs_check(self, z, n_v=None, batch=1, cap=0, want_vals=False):
        return self.ctx.r1cs_check(*self.bufs, z, n_v=n_v, batch=batch, cap=cap, want_vals=want_vals)

    def free(self):
        for m in self.bufs:
            for x in m:
                x.free()


def _rows_mentioning(circ, col):
    """{row: (A_row, B_row, C_row)} as [(coeff, col)] lists, for the rows in which `col` occurs"""
    circ.csr(circ.fc)
    hit = set()
    for rp, cols, _val, _vidx, _table in circ._csr:
        hit.update((np.searchsorted(rp, np.flatnonzero(cols == col), side="right") - 1).tolist())
    out = {}
    for i in sorted(hit):
        out[i] = tuple([(table[vidx[k]], int(cols[k])) for k in range(int(rp[i]), int(rp[i + 1]))]
                       for rp, cols, _val, vidx, table in circ._csr)
    return out


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_every_subcircuit_of_a_job_is_satisfied_on_the_device(curve, ctx_bn254, ctx_bls):
    ctx = ctx_bn254 if curve == "bn254" else ctx_bls
    rnd = random.Random(41)
    r, fr = CURVE_PARAMS[curve]["r"], ctx.fr_bytes
    job = ShaMerkleJob(curve, 8, 1, 4, [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(4)])
    job.set_challenges(rnd.randrange(r), rnd.randrange(r))
    dev = job.stage1_device(ctx)
    classes = {}
    for i in range(job.n):
        classes.setdefault(job.class_of(i), []).append(i)
    assert len(classes) == 5 and sorted(len(m) for m in classes.values()) == [1, 1, 1, 2, 3]
    checked = 0
    try:
        for key, members in classes.items():
            circ = job.make_class(members[0])
            ws = [job.inputs(i) for i in members]
            ops, refs, vmap = circ.tape.word_program(circ.n_v)
            wp = ctx.wprog_upload(ops, refs, vmap, circ.tape.n_values, circ.tape.n_inputs)
            mats = _ClassMatrices(ctx, circ)
            z = wp.run(program_inputs(circ, ws), [], [])           # the bit columns; column 0 = 1
            try:
                dev.fill(circ, members, z)                         # the challenge-dependent columns
                verdicts, rows = mats.r1cs_check(z, batch=len(members), cap=8)
                assert verdicts == [(0, None)] * len(members), (key, verdicts, rows)
                assert (rows == NONE).all()
                assert dev.check(mats, z, members) is None
                checked += len(members)
                if key != ("leaf", False, False):
                    continue
                # one portal value of one row, overwritten where it lies: the value of the leaf's own set(node hash) entry
                b, col = 1, circ.N_INST + 2 * (job.np_ - 1) + 1
                i = members[b]
                z_host = circ.assignment_ints([ws[b]])[0]
                assert z_host[col] == job.time[i][-1][1] % r
                z_host[col] = (z_host[col] + 1) % r
                one = FrCodec(curve).enc1(z_host[col])
                capi.check(ctx.lib.hk_dev_upload(ctx.handle, z.ptr + (b * circ.n_v + col) * fr, one.ctypes.data, fr), "hk_dev_upload")
                near = _rows_mentioning(circ, col)
                assert 1 <= len(near) < 64
                idx = sorted(near)
                bad_local = r1cs_bad_rows([near[k][0] for k in idx], [near[k][1] for k in idx], [near[k][2] for k in idx], z_host, r)
                want = [idx[k] for k in bad_local]
                assert want                                        # the tampered value is constrained
                verdicts, rows = mats.r1cs_check(z, batch=len(members), cap=64)
                assert verdicts == [(len(want), want[0]) if m == b else (0, None) for m in range(len(members))]
                assert rows[b, :len(want)].tolist() == want and (rows[b, len(want):] == NONE).all()
                assert (np.delete(rows, b, axis=0) == NONE).all()
                with pytest.raises(R1csUnsatisfied) as e:
                    dev.check(mats, z, members)
                assert (e.value.subcircuit, e.value.row, e.value.n_bad) == (i, want[0], len(want))
                assert e.value.failures == [(i, len(want), want[0], want[:8])]
            finally:
                z.free()
                wp.free()
                mats.free()
    finally:
        dev.free()
    assert checked == 8
