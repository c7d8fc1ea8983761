"""The NTT pass plans of hekaton_system_amd/csrc/ntt_plan.h as Python data: compiles tests/host_shim/ntt_plan_driver.cpp with
g++ and parses what it prints.  Plain helper of tests/test_ntt_plan_cpu.py, tests/test_ntt_ref_cpu.py and
tests/test_ntt_device_gpu.py."""
import os
import subprocess

from tests import host_build

DEFAULT_TILE_LOG, DEFAULT_UPPER_MAX = 11, 6


def load(build_dir):
    """-> (knobs, plans): knobs[raw tile_log, raw upper_max] = (tile_log, upper_max);
    plans[logn, tile_log, raw upper_max] = (upper_max, [(lo, nst, cols_bits), ...]) in DIT order"""
    exe = os.path.join(str(build_dir), "ntt_plan_driver")
    host_build.build("ntt_plan_driver.cpp", exe, "-O1", "-Wall", "-Werror")
    knobs, plans = {}, {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        v = list(map(int, f[1:]))
        if f[0] == "knob":
            knobs[v[0], v[1]] = (v[2], v[3])
        else:
            np_ = v[4]
            assert len(v) == 5 + 3 * np_
            plans[v[0], v[1], v[2]] = (v[3], [tuple(v[5 + 3 * k:8 + 3 * k]) for k in range(np_)])
    return knobs, plans
