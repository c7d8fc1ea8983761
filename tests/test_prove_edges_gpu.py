"""GPU: the proof finish (k_prep_ext, k_finish_ab, k_finish_c and the ext slots of the big MSMs) and hk_commit /
hk_commit_batch at their exceptional cases - the directed r, s and kappa of tests/prove_edges.py, which put an operand of
every add of the finish at infinity, make it a doubling or a cancellation, zero a GLV half, and give A, B, both or C at
infinity - through hk_prove alone and through hk_prove_batch with infinite and finite rows inside one chunk.  Every output
is compared with ONE oracle scalar multiplication of the key's generator by the discrete log the trapdoor gives
(prove_edges.proof_logs): equality of affine points, None at infinity, no tolerance.  tests/test_prove_edges_cpu.py shows
that the cases are what they claim."""
import os
import re

import numpy as np
import pytest

from oracle.pyref.codec import Codec
from tests import prove_edges as pe
from tests.util import oracle_commit, pk_upload_from_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = int(re.search(r"#define\s+HK_PROVE_BATCH_CHUNK\s+(\d+)", open(os.path.join(ROOT, "include", "hekaton.h")).read()).group(1))
ROWS = CHUNK + pe.BATCH_ROWS_OVER_CHUNK                   # a full chunk and a ragged one per call
CTX_FIXTURE = {"bn254": "ctx_bn254", "bls12_381": "ctx_bls"}


@pytest.fixture(scope="module", params=pe.CURVE_NAMES)
def dev(request):
    """(setup, codec, device key): the oracle's key uploaded once per curve"""
    cname = request.param
    ctx = request.getfixturevalue(CTX_FIXTURE[cname])
    su = pe.setup(cname)
    cd = Codec(su.cp)
    dpk = pk_upload_from_oracle(ctx, cd, su.pk, su.cs)
    try:
        yield su, cd, dpk
    finally:
        dpk.free()


def _mismatches(su, cd, case, a, b, c):
    want = pe.proof_points(su.cname, su.td, su.cs, case)
    got = (cd.g1_from(a), cd.g2_from(b), cd.g1_from(c))
    return ["%s.%s" % (case["name"], k) for k, g, w in zip("abc", got, want) if g != w]


def test_hk_prove_at_every_case(dev):
    su, cd, dpk = dev
    bad = []
    for case in su.cases:
        a, b, c = dpk.prove(cd.fr_vec_mont(case["z"]), cd.fr_vec_mont([case["r"]]), cd.fr_vec_mont([case["s"]]),
                            cd.fr_vec_mont([case["kappa"]]))
        bad += _mismatches(su, cd, case, a, b, c)
    assert not bad, "%d outputs differ from the reference: %s" % (len(bad), " ".join(bad))


def test_hk_prove_batch_with_infinite_and_finite_rows_in_a_chunk(dev):
    su, cd, dpk = dev
    assert ROWS == 11
    bad = []
    for call in pe.batch_order(su.cases, ROWS):
        rows = [su.cases[i] for i in call]
        z = np.concatenate([cd.fr_vec_mont(c["z"]) for c in rows])
        a, b, c = dpk.prove_batch(z, cd.fr_vec_mont([c["r"] for c in rows]), cd.fr_vec_mont([c["s"] for c in rows]),
                                  cd.fr_vec_mont([c["kappa"] for c in rows]), su.n_v, ROWS)
        for j, case in enumerate(rows):
            bad += ["row%d:%s" % (j, m) for m in _mismatches(su, cd, case, a[j], b[j], c[j])]
    assert not bad, "%d outputs differ from the reference: %s" % (len(bad), " ".join(bad))


@pytest.mark.parametrize("no_small", [False, True], ids=["small", "bucket"])
def test_commitments_at_infinity_and_next_to_it(dev, no_small, monkeypatch):
    """hk_commit row by row and hk_commit_batch over the five rows (infinity at rows 1 and 3), on the element-wise path and,
    under HK_MSM_NO_SMALL (read per call), on the bucket pass."""
    su, cd, dpk = dev
    if no_small:
        monkeypatch.setenv("HK_MSM_NO_SMALL", "1")
    else:
        monkeypatch.delenv("HK_MSM_NO_SMALL", raising=False)
    cases = su.commit_cases
    want = [pe.point(su.cname, 1, su.td, pe.commit_log(su.td, su.cs, c["w"], c["kappa"])) for c in cases]
    assert [w is None for w in want] == [False, True, False, True, False]
    assert want == [oracle_commit(su.cp, su.cs, su.pk, 0, c["w"], c["kappa"]) for c in cases]
    got = [cd.g1_from(dpk.commit(0, cd.fr_vec_mont(c["w"]), cd.fr_vec_mont([c["kappa"]]))) for c in cases]
    assert got == want, [c["name"] for c, g, w in zip(cases, got, want) if g != w]
    n = len(cases[0]["w"])
    out = dpk.commit_batch(0, np.concatenate([cd.fr_vec_mont(c["w"]) for c in cases]),
                           cd.fr_vec_mont([c["kappa"] for c in cases]), n, len(cases))
    got = [cd.g1_from(row) for row in out]
    assert got == want, [c["name"] for c, g, w in zip(cases, got, want) if g != w]
