"""CPU: hk_prove's coalescer (hekaton_system_amd/csrc/coalesce.h) under ThreadSanitizer, around a fake prover
(tests/host_shim/coalesce_driver.cpp): batches never mix keys, never exceed the chunk, at most K run at once, each
thread's calls run in order, a batch's error (or exception) reaches every member, and no caller is left waiting.
The hk_timings struct grew a field: the ctypes mirror must match the header."""
import os
import re
import subprocess

import pytest

from hekaton_system_amd import capi

from tests import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("coalesce") / "coalesce_driver")
    host_build.build("coalesce_driver.cpp", out, "-O1", "-g", "-fsanitize=thread", "-pthread")
    return out


@pytest.mark.parametrize("k,threads,calls,keys", [(1, 8, 150, 3), (2, 8, 150, 3), (1, 1, 40, 2), (2, 16, 60, 1),
                                                  (3, 5, 80, 4)])
def test_coalescer_under_tsan(driver, k, threads, calls, keys):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    p = subprocess.run([driver, str(k), str(threads), str(calls), str(keys)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok "), p.stdout
    assert int(re.search(r"max_running=(\d+)", p.stdout).group(1)) <= k


def test_timings_struct_matches_header():
    hdr = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} hk_timings;", hdr, re.S).group(1)
    names = re.findall(r"^\s*(?:float|uint32_t)\s+(\w+);", body, re.M)
    assert [n for n, _ in capi.hk_timings._fields_] == names
    assert names[-1] == "batch_proofs"
