"""CPU: the gather window of hk_prove's coalescer (hekaton_system_amd/csrc/coalesce.h) under
ThreadSanitizer, around a fake prover (tests/host_shim/coalesce_gather_driver.cpp): a lone caller never waits, looping
callers of one key settle into balanced batches, a caller that leaves is waited for once, and with a window the
coalescer's invariants hold as without one (keys never mix, a batch never exceeds the chunk, at most K run, each thread's
calls run in order, a batch's error or exception reaches every member, no caller is left waiting: the driver checks
them in every case here)."""
import os
import re
import subprocess

import pytest

from tests import host_build


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gather") / "coalesce_gather_driver")
    host_build.build("coalesce_gather_driver.cpp", out, "-O1", "-g", "-fsanitize=thread", "-pthread")
    return out


def _run(driver, k, threads, calls, keys, gather_us, work_us, calls_others=None):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    argv = [driver] + [str(x) for x in (k, threads, calls, keys, gather_us, work_us)]
    if calls_others is not None:
        argv.append(str(calls_others))
    p = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=300)
    print(p.stdout.strip())
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok "), p.stdout
    assert int(re.search(r"max_running=(\d+)", p.stdout).group(1)) <= k
    sizes = {int(a): int(b) for a, b in re.findall(r"(\d+):(\d+)", re.search(r"sizes=(\S+)", p.stdout).group(1))}
    return sizes, float(re.search(r"elapsed_ms=([\d.]+)", p.stdout).group(1))


def test_lone_caller_never_waits(driver):
    """One thread, W = 5 s, 40 calls of 1 ms: every batch has one member, and the run (40 ms of work) takes far less than
    one W - it would take 200 s if the caller waited for itself."""
    sizes, ms = _run(driver, 2, 1, 40, 1, 5_000_000, 1000)
    assert sizes == {1: 40}
    assert ms < 2500, ms


def test_looping_callers_form_balanced_batches(driver):
    """8 threads, one key, K = 2, 100 calls each, a prover of 5 ms, W = 25 ms: at least 90 % of the 800 items run in
    batches of exactly 4 (only the batches formed before all threads arrived, and the ones holding the threads' last
    calls, can differ)."""
    sizes, _ms = _run(driver, 2, 8, 100, 1, 25_000, 5000)
    assert max(sizes) <= 8
    assert 4 * sizes.get(4, 0) >= 0.9 * 800, sizes


def test_a_caller_that_leaves_is_waited_for_once(driver):
    """K = 1, W = 200 ms, a prover of 1 ms; thread 1 makes one call and exits, thread 0 makes 50.  Thread 0 waits for the
    caller that left at most once, W after the batch that held it: less than 50 ms + 2 W in all.  (One shared deadline
    that every batch end renews would cost W before each call, 10 s.)"""
    sizes, ms = _run(driver, 1, 2, 50, 1, 200_000, 1000, calls_others=1)
    assert sum(n * c for n, c in sizes.items()) == 51
    assert ms < 50 + 2 * 200, ms


@pytest.mark.parametrize("k,threads,calls,keys,gather_us,work_us", [
    (2, 8, 150, 3, 2000, 300),          # mixed keys; key 2 carries the erroring and the throwing batches
    (1, 8, 100, 3, 1000, 300),
    (3, 5, 80, 4, 500, 200),
    (2, 16, 60, 1, 3000, 500),
    (2, 8, 100, 3, 0, 300),             # W = 0: no window, no balancing
])
def test_invariants_hold_with_a_window(driver, k, threads, calls, keys, gather_us, work_us):
    sizes, _ms = _run(driver, k, threads, calls, keys, gather_us, work_us)
    assert sum(n * c for n, c in sizes.items()) == threads * calls
    assert max(sizes) <= 8

