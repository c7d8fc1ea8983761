"""CPU, against the built libhekaton.so: the kernels the library registers at load (csrc/launch.h, read through
hk_kernel_info without a HIP call) are the kernels its code objects hold, and the launch helper is the only place that
launches."""
import os
import re

from tests import kernel_registry as kr
from tests.kernel_registry import kernel_meta

CSRC = os.path.join(kr.ROOT, "hekaton_system_amd", "csrc")


def test_registry_is_the_code_objects_kernels():
    """A kernel launched past the helper is in the code object and not in the registry; so is one that is instantiated and
    never launched.  k_scratch_presize sizes the rings and is deliberately not counted."""
    reg = kr.registry()
    assert len({name for name, _, _ in reg}) > 100
    got = {kr.base_name(name) for name, _, _ in reg}
    want = {kr.base_name(name) for name, _ in kr.code_object_kernels()}
    assert kernel_meta.PRESIZE in want and kernel_meta.PRESIZE not in got
    assert got == want - {kernel_meta.PRESIZE}, (sorted(got - want), sorted(want - got))


def test_gated_kernels_are_the_serial_pairing_path():
    gated = {(kr.base_name(name), env) for name, env, _ in kr.registry() if env}
    assert gated == {(k, "HK_PAIR_SERIAL") for k in kernel_meta.SERIAL_ONLY}
    # and no instantiation of them is registered without the switch
    assert not [name for name, env, _ in kr.registry() if not env and kr.base_name(name) in kernel_meta.SERIAL_ONLY]


def test_past_the_end_is_an_argument_error():
    from hekaton_system_amd import capi
    n = len(kr.registry())
    assert capi.load().hk_kernel_info(n, None, None, None) == capi.HK_ERR_ARG
    assert capi.load().hk_kernel_info(n - 1, None, None, None) == capi.HK_OK


def test_only_the_helper_and_the_presize_launch_are_raw():
    raw = re.compile(r"hipLaunchKernelGGL|hipExtLaunchKernelGGL|<<<")
    hits = []
    for d, _, files in os.walk(CSRC):
        for f in sorted(files):
            if f == "launch.h":
                continue
            with open(os.path.join(d, f), errors="replace") as fh:
                hits += [(f, line.strip()) for line in fh if raw.search(line)]
    # new_lane's launch of the k_scratch_presize<W> the context chose
    assert len(hits) == 1 and hits[0][0] == "hk_core.hip" and "hipLaunchKernelGGL(k, " in hits[0][1], hits
