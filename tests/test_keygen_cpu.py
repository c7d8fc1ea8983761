"""CPU: the ABI surface of device key generation (hk_qap_eval, hk_keygen) and the toxic-waste draws of
generate_parameters_device, checked against setup_host without a device (a stub context records hk_keygen's arguments)."""
import os
import re

import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.cp_groth16 import (CURVE_PARAMS, MultiStageConstraintSynthesizer, SeededRng,
                                           generate_parameters_device, setup_host)
from hekaton_system_amd.workload import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keygen_symbols_declared_listed_exported():
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    declared = set(re.findall(r"\b(hk_[a-z0-9_]+)\s*\(", hdr))
    for sym in ("hk_qap_eval", "hk_keygen"):
        assert sym in declared and sym in capi.EXPORTS
    assert "hk_keygen_desc" in hdr and "hk_keygen_out" in hdr
    if os.path.exists(capi.LIB_PATH):
        lib = capi.load()
        for sym in ("hk_qap_eval", "hk_keygen"):
            getattr(lib, sym)


class _Recorded(Exception):
    pass


class _StubCtx:
    """Stands in for capi.Context: records what generate_parameters_device hands to hk_keygen, then stops."""
    g1_bytes, g2_bytes, fr_bytes = 64, 128, 32

    def __init__(self):
        self.args = None

    def keygen(self, **kw):
        self.args = kw
        raise _Recorded()


class TwoStageCircuit(MultiStageConstraintSynthesizer):
    """The shape of the golden cases (tests/golden/gen_golden.py): two instance inputs, a committed first stage and a
    second stage that uses it."""

    def __init__(self, r):
        self.r = r

    def total_num_stages(self):
        return 2

    def generate_constraints(self, stage, cs):
        cs.initialize_stage()
        if stage == 0:
            self.w = [cs.new_witness_variable(3 + k) for k in range(5)]
        else:
            x = cs.new_input_variable(7)
            y = cs.new_input_variable(7 * 3 % self.r)
            acc = cs.new_witness_variable(3)
            cs.enforce_constraint([(1, self.w[0])], [(1, "one")], [(1, acc)])
            for k in range(1, 5):
                nxt = cs.new_witness_variable(0)
                cs.enforce_constraint([(1, self.w[k])], [(1, x)], [(1, nxt)])
                acc = nxt
            cs.enforce_constraint([(3, "one")], [(1, x)], [(1, y)])
        cs.finalize_stage()


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("kind", ["tiny", "two-stage"])
def test_device_setup_draws_the_toxic_waste_in_setup_host_order(curve, kind):
    r = CURVE_PARAMS[curve]["r"]
    mk = (lambda: make_config(curve, "tiny")) if kind == "tiny" else (lambda: TwoStageCircuit(r))
    seed = b"KEYGEN-DRAWS-0123456789abcdef!!!"
    td = setup_host(mk(), curve, SeededRng(seed)).td
    stub = _StubCtx()
    with pytest.raises(_Recorded):
        generate_parameters_device(mk(), curve, SeededRng(seed), stub)
    a = stub.args
    assert (a["alpha"], a["beta"], a["gamma"], a["t"]) == (td.alpha, td.beta, td.gamma, td.t)
    assert list(a["deltas"]) == list(td.deltas)
    assert (a["g1_scalar"], a["g2_scalar"]) == (td.g1_scalar, td.g2_scalar)
    assert [tuple(x) for x in a["stage_ranges"]] == [tuple(x) for x in td.stage_ranges]
    assert a["n_inst"] == td.n_inst
    assert a["n_v"] == td.n_inst + td.stage_ranges[-1][1]
    assert len(a["matrices"]) == 3 and all(len(M) == 3 for M in a["matrices"])
    assert a["n_constraints"] == len(a["matrices"][0][0]) - 1
