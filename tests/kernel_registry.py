"""The two views of the kernels of libhekaton.so that tests/test_kernel_registry_cpu.py and tests/test_kernel_registry_gpu.py
hold against each other: the library's own registry (hk_kernel_info: what it launches through csrc/launch.h) and the embedded
code objects (tools/kernel_meta.py: what the compiler emitted)."""
import ctypes as C
import os
import re
import shutil
import sys

from hekaton_system_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_meta  # noqa: E402


def base_name(name):
    """'void hk::k_spmv<hk::Fp<...>>(...)' or 'hk::k_spmv(...)' -> 'k_spmv'"""
    return re.match(r"(?:void )?(?:hk::)?(\w+)", name).group(1)


def registry(with_frames=False):
    """[(name, only_with_env or None, private bytes or None)]; without frames no HIP call is made"""
    lib = capi.load()
    out = []
    while True:
        name, env, frame = C.c_char_p(), C.c_char_p(), C.c_size_t(0)
        st = lib.hk_kernel_info(len(out), C.byref(name), C.byref(frame) if with_frames else None, C.byref(env))
        if st != capi.HK_OK:
            assert st == capi.HK_ERR_ARG
            return out
        out.append((name.value.decode(), env.value.decode() if env.value else None, frame.value if with_frames else None))


def code_object_kernels():
    """[(demangled name, private_segment_fixed_size)] over every code object of the library"""
    tmp, cos = kernel_meta.code_objects(capi.LIB_PATH)
    try:
        rows = [r for co in cos for r in kernel_meta.kernels_of(co)]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    dm = kernel_meta.demangle([r["symbol"] for r in rows])
    return [(dm[r["symbol"]], r["scratch"]) for r in rows]
