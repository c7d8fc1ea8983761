"""GPU: the frames the scratch budget is computed from (hk_kernel_info over the launch registry) against the code objects'
own, and HK_DEBUG_SYNC=1 naming every launch of the smoke shape."""
import os
import re
import subprocess
import sys

import pytest

from tests import kernel_registry as kr
from tests.kernel_registry import kernel_meta

pytestmark = pytest.mark.gpu


def test_deepest_default_path_frame_matches_the_code_objects():
    reg = kr.registry(with_frames=True)
    by_co = {}
    for name, scratch in kr.code_object_kernels():
        by_co.setdefault(kr.base_name(name), []).append(scratch)
    # every entry has a frame size the runtime reports: one of those its kernel's instantiations declare
    for name, _, frame in reg:
        assert frame in by_co[kr.base_name(name)], (name, frame)
    got = max(frame for _, env, frame in reg if not env)
    want = max(s for k, ss in by_co.items() if k not in kernel_meta.SERIAL_ONLY + (kernel_meta.PRESIZE,) for s in ss)
    print("deepest default-path frame: registry %d B, code objects %d B" % (got, want))
    assert got == want and got > 0


def test_debug_sync_names_every_launch_of_the_smoke_shape():
    """tests/golden/groth16.json, BN254 case 0: one hk_commit and one hk_prove (smoke() compares both with the golden bytes)
    in a fresh process of its own environment."""
    env = dict(os.environ, HK_DEBUG_SYNC="1")
    env["PYTHONPATH"] = kr.ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=kr.ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "smoke ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stderr.splitlines() if ln.startswith("[hk] ")]
    launched = [ln[len("[hk] launched "):] for ln in lines if ln.startswith("[hk] launched ")]
    assert launched and len(lines) == 2 * len(launched)
    for i, k in enumerate(launched):
        assert lines[2 * i] == "[hk] launched " + k and lines[2 * i + 1] == "[hk] finished %s: hipSuccess" % k, lines[2 * i:2 * i + 2]
    named = {re.match(r"\w+", k).group(0) for k in launched}
    assert {"k_spmv", "k_ntt_pass4", "k_prep_ext", "k_finish_ab", "k_finish_c", "k_msm_accum0"} <= named, sorted(named)
