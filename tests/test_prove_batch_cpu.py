"""CPU: hk_prove_batch is part of the C ABI - declared with its chunk constant, exported by libhekaton.so, and reachable
from the Python layers (capi, worker)."""
import os
import re
import subprocess

from hekaton_system_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "hekaton.h")).read()


def test_header_declares_prove_batch_and_chunk():
    hdr = _header()
    assert re.search(r"hk_status\s+hk_prove_batch\s*\(", hdr)
    m = re.search(r"#define\s+HK_PROVE_BATCH_CHUNK\s+(\d+)", hdr)
    assert m and int(m.group(1)) >= 1


def test_library_exports_prove_batch():
    lib = capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT hk_prove_batch$", out, re.M)
    assert "hk_prove_batch" in capi.EXPORTS
    assert lib.hk_prove_batch.argtypes is not None and len(lib.hk_prove_batch.argtypes) == 12


def test_python_layers_expose_the_batched_prove():
    from hekaton_system_amd import worker
    assert callable(getattr(capi.DevicePk, "prove_batch", None))
    assert callable(getattr(worker, "process_stage1_requests_batch", None))
