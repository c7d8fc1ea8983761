"""Every header of csrc/ compiles on its own: a translation unit that includes only that header passes hipcc's syntax check
for gfx950.  A header that leans on what its includer happened to include before it (as keygen.cuh once did on
prove_impl.cuh) fails here, not in whoever next includes it elsewhere.  The set is globbed, so a new header is covered."""
import glob
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hekaton_system_amd", "csrc")
HEADERS = sorted(os.path.basename(p) for ext in ("*.cuh", "*.h") for p in glob.glob(os.path.join(CSRC, ext)))


def _hipcc():
    rocm = "/opt/rocm/bin/hipcc"                       # the Makefile's default
    return shutil.which("hipcc") or (rocm if os.path.exists(rocm) else None)


def test_headers_found():
    assert "prove_impl.cuh" in HEADERS and "hk_internal.h" in HEADERS


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("hipcc not found")
    src = tmp_path / "only.hip"
    src.write_text('#include "%s"\n' % header)
    r = subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-result", "-fsyntax-only", "-I" + CSRC,
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
