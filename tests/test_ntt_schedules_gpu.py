"""GPU: hk_ntt and hk_witness_map under pass schedules other than the default.  NttHost::passes reads HK_NTT_TILE_LOG and
HK_NTT_UPPER_MAX once per process (csrc/ntt_plan.h normalises them), so each schedule runs in a fresh child process; they
are the only way to a chain of three and more passes at a small size: tile 8 / max 1 is 8+1+1+... (eleven passes at 2^18),
8 / 3 is 8+3+3 at 2^14, 9 / 2 is 9+2+1 at 2^12.  8 / 10 is the combination whose single ten-stage upper pass had no tile
shape before upper_max was clamped to the tile (cols_bits wrapped); it now runs as 8 / 8.  The reference is the C++ oracle,
byte for byte."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = [(8, 1), (8, 3), (9, 2), (8, 10)]         # HK_NTT_TILE_LOG, HK_NTT_UPPER_MAX
LOG_MS = [9, 12, 14, 18]

_CHILD = r"""
import json, random, sys
sys.path.insert(0, %(root)r)
import numpy as np
from hekaton_system_amd import capi
from oracle.c_oracle import COracle
from oracle.pyref.codec import Codec
from oracle.pyref.params import CURVES
from tests.util import csr_from_rows, synthetic_r1cs
for cname in ("bn254", "bls12_381"):
    cp = CURVES[cname]
    co = COracle(cname)
    with capi.Context(cname, 0) as ctx:
        for log_m in %(log_ms)r:
            # 32 random bytes with the top three bits clear are below 2^253 < r: a canonical Montgomery value
            x = np.random.default_rng(log_m).integers(0, 256, size=(1 << log_m, 32), dtype=np.uint8)
            x[:, 31] &= 0x1f
            x = x.reshape(-1)
            for inverse in (0, 1):
                for coset in (0, 1):
                    want = co.ntt(x.copy(), log_m, inverse=inverse, coset=coset)
                    got = ctx.ntt(x.copy(), log_m, inverse=inverse, coset=coset)
                    print(json.dumps({"case": [cname, "ntt", log_m, inverse, coset], "ok": bool(np.array_equal(got, want))}))
        cd = Codec(cp)
        cs = synthetic_r1cs(cp, random.Random(12), 3, 10, 4093)
        A, B, C = (csr_from_rows(cd, M) for M in cs.matrices())
        z = cd.fr_vec_mont(cs.full_assignment())
        want, m_want = co.witness_map(A, B, C, cs.num_instance, 4093, z)
        got, m = ctx.witness_map(A, B, C, cs.num_instance, 4093, z)
        print(json.dumps({"case": [cname, "witness_map", 12], "ok": bool(m == m_want == 4096 and np.array_equal(got, want))}))
"""


_failed = []          # the schedules whose child failed: after the first, no further child is started


@pytest.mark.parametrize("tile_log,upper_max", SCHEDULES, ids=["tile%d-max%d" % s for s in SCHEDULES])
def test_ntt_and_witness_map_under_other_schedules(tile_log, upper_max):
    """One child per schedule, one after the other.  A child that failed may have left the device in any state, so the
    schedules after it fail without starting theirs."""
    assert not _failed, "no child started: schedule %s failed before" % (_failed[0],)
    _failed.append((tile_log, upper_max))
    env = dict(os.environ)
    env["HK_NTT_TILE_LOG"] = str(tile_log)
    env["HK_NTT_UPPER_MAX"] = str(upper_max)
    res = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "log_ms": LOG_MS}], env=env, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    cases = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
    assert len(cases) == 2 * (4 * len(LOG_MS) + 1)
    bad = [c["case"] for c in cases if not c["ok"]]
    assert not bad, bad
    _failed.pop()
