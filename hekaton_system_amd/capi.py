"""ctypes binding of include/hekaton.h (libhekaton.so) — the only door into the HIP kernels.

There is no CPU path: importing works anywhere (so host logic can be tested), but creating a
`Context` without a gfx950 device raises, and a missing libhekaton.so raises at load time.
"""
import contextlib
import ctypes as C
import functools
import os

import numpy as np

# hk_prove forks four side streams per lane; let the runtime map them onto more hardware queues than
# its default of 4 (must be set before the HIP runtime initialises; harmless if the user set it).
# Measured with 8 proofs in flight (apps/hk_all_in_one): 8 queues 89 proofs/s, 16: 121-122,
# 20-22: 123-125, 24 and more: 114-116 - hk_ctx_create exports the same value for hosts that do not come through here
os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HK_LIB") or os.path.join(_HERE, "lib", "libhekaton.so")    # HK_LIB: experiment builds

HK_BN254, HK_BLS12_381 = 0, 1
HK_OK, HK_ERR_LEN, HK_ERR_DOMAIN_TOO_LARGE, HK_ERR_DEVICE, HK_ERR_ARG, HK_ERR_NOMEM = range(6)
CURVE_IDS = {"bn254": HK_BN254, "bls12_381": HK_BLS12_381}


class HekatonError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        super().__init__("%s failed: %s" % (what, status_str(status)))


class hk_poseidon_desc(C.Structure):          # include/hekaton.h
    _fields_ = [("t", C.c_uint32), ("alpha", C.c_uint32), ("full_rounds", C.c_uint32), ("partial_rounds", C.c_uint32),
                ("consts_offset", C.c_uint32)]


class hk_csr(C.Structure):
    _fields_ = [("row_ptr", C.c_void_p), ("col", C.c_void_p), ("val_mont", C.c_void_p),
                ("n_rows", C.c_size_t), ("nnz", C.c_size_t)]


class hk_pk_desc(C.Structure):
    _fields_ = [("a_g", C.c_void_p), ("a_len", C.c_size_t),
                ("b_g", C.c_void_p), ("b_g_len", C.c_size_t),
                ("b_h", C.c_void_p), ("b_h_len", C.c_size_t),
                ("h_g", C.c_void_p), ("h_len", C.c_size_t),
                ("ck_stage", C.POINTER(C.c_void_p)), ("ck_len", C.POINTER(C.c_size_t)),
                ("n_stages", C.c_size_t),
                ("deltas_g", C.c_void_p), ("last_delta_h", C.c_void_p),
                ("alpha_g", C.c_void_p), ("beta_g", C.c_void_p), ("beta_h", C.c_void_p),
                ("A", C.POINTER(hk_csr)), ("B", C.POINTER(hk_csr)), ("C", C.POINTER(hk_csr)),
                ("n_inst", C.c_size_t), ("n_constraints", C.c_size_t)]


class hk_vk_desc(C.Structure):                # include/hekaton.h
    _fields_ = [("alpha_g", C.c_void_p), ("beta_h", C.c_void_p), ("gamma_h", C.c_void_p), ("deltas_h", C.c_void_p),
                ("n_deltas", C.c_size_t), ("gamma_abc_g", C.c_void_p), ("n_abc", C.c_size_t)]


class hk_keygen_desc(C.Structure):            # include/hekaton.h
    _fields_ = [("A", C.POINTER(hk_csr)), ("B", C.POINTER(hk_csr)), ("C", C.POINTER(hk_csr)),
                ("n_inst", C.c_size_t), ("n_constraints", C.c_size_t), ("n_v", C.c_size_t),
                ("stage_ranges", C.c_void_p), ("n_stages", C.c_size_t),
                ("alpha", C.c_void_p), ("beta", C.c_void_p), ("gamma", C.c_void_p), ("t", C.c_void_p),
                ("g1_scalar", C.c_void_p), ("g2_scalar", C.c_void_p), ("deltas", C.c_void_p)]


class hk_keygen_out(C.Structure):             # include/hekaton.h
    _fields_ = [("a_g", C.c_void_p), ("b_g", C.c_void_p), ("b_h", C.c_void_p), ("h_g", C.c_void_p),
                ("ck_stage", C.POINTER(C.c_void_p)),
                ("deltas_g", C.c_void_p), ("alpha_g", C.c_void_p), ("beta_g", C.c_void_p), ("gamma_abc_g", C.c_void_p),
                ("beta_h", C.c_void_p), ("gamma_h", C.c_void_p), ("deltas_h", C.c_void_p), ("qap_abc", C.c_void_p)]


class hk_exec_tree_desc(C.Structure):         # include/hekaton.h
    _fields_ = [("n_sub", C.c_uint32), ("entry_fields", C.c_uint32), ("offsets", C.c_void_p),
                ("time_entries_mont", C.c_void_p), ("addr_entries_mont", C.c_void_p), ("challenges_mont", C.c_void_p),
                ("consts_mont", C.c_void_p), ("n_consts", C.c_size_t),
                ("leaf_hash", C.POINTER(hk_poseidon_desc)), ("node_hash", C.POINTER(hk_poseidon_desc))]


class hk_exec_tree_out(C.Structure):          # include/hekaton.h
    _fields_ = [("evals_mont", C.c_void_p), ("leaves_mont", C.c_void_p), ("nodes_mont", C.c_void_p),
                ("siblings_mont", C.c_void_p), ("root_mont", C.c_void_p)]


class hk_stage1_desc(C.Structure):            # include/hekaton.h
    _fields_ = [("n_sub", C.c_uint32), ("n_portals", C.c_uint32), ("depth", C.c_uint32), ("offsets", C.c_void_p),
                ("time_entries_mont", C.c_void_p), ("addr_entries_mont", C.c_void_p), ("challenges_mont", C.c_void_p),
                ("evals_mont", C.c_void_p), ("leaves_mont", C.c_void_p), ("siblings_mont", C.c_void_p),
                ("root_mont", C.c_void_p), ("consts_mont", C.c_void_p), ("n_consts", C.c_size_t),
                ("leaf_hash", C.POINTER(hk_poseidon_desc)), ("node_hash", C.POINTER(hk_poseidon_desc)),
                ("inst_col0", C.c_uint32), ("col0", C.c_uint32), ("pos_col0", C.c_uint32)]


class hk_ram_stage1_desc(C.Structure):        # include/hekaton.h
    _fields_ = [("n_sub", C.c_uint32), ("n_portals", C.c_uint32), ("depth", C.c_uint32), ("offsets", C.c_void_p),
                ("time_entries_mont", C.c_void_p), ("addr_entries_mont", C.c_void_p), ("challenges_mont", C.c_void_p),
                ("evals_mont", C.c_void_p), ("leaves_mont", C.c_void_p), ("siblings_mont", C.c_void_p),
                ("root_mont", C.c_void_p), ("consts_mont", C.c_void_p), ("n_consts", C.c_size_t),
                ("leaf_hash", C.POINTER(hk_poseidon_desc)), ("node_hash", C.POINTER(hk_poseidon_desc)),
                ("template_mont", C.c_void_p),
                ("inst_col0", C.c_uint32), ("stage0_col0", C.c_uint32), ("col0", C.c_uint32), ("pos_col0", C.c_uint32)]


class hk_r1cs_job_desc(C.Structure):          # include/hekaton.h
    _fields_ = [("n_parts", C.c_uint32), ("n_txs", C.c_uint32), ("slot_offsets", C.c_void_p), ("slot_rank", C.c_void_p),
                ("slot_src", C.c_void_p), ("sets_per_tx", C.c_uint32), ("tx_len", C.c_uint32), ("tx_stride", C.c_uint32),
                ("wit_offsets", C.c_void_p), ("body_len", C.c_void_p), ("witness_mont", C.c_void_p)]


class hk_vkd_desc(C.Structure):               # include/hekaton.h
    _fields_ = [("depth", C.c_uint32), ("split", C.c_uint32), ("n_updates", C.c_uint32), ("kinds", C.c_void_p),
                ("leaves", C.c_void_p), ("siblings_mont", C.c_void_p), ("consts_mont", C.c_void_p), ("n_consts", C.c_size_t),
                ("leaf_hash", C.POINTER(hk_poseidon_desc)), ("node_hash", C.POINTER(hk_poseidon_desc)),
                ("roots_mont", C.c_void_p), ("n_slots", C.c_uint32), ("slot_addr", C.c_void_p), ("slot_src", C.c_void_p),
                ("values_mont", C.c_void_p)]


class hk_vkd_cols(C.Structure):               # include/hekaton.h
    _fields_ = [("kind", C.c_uint32), ("hash_col0", C.c_uint32), ("index_col0", C.c_uint32), ("path_col0", C.c_uint32)]


class hk_vkd_tree_desc(C.Structure):          # include/hekaton.h
    _fields_ = [("depth", C.c_uint32), ("n_leaves0", C.c_uint32), ("leaves0", C.c_void_p), ("n_updates", C.c_uint32),
                ("kinds", C.c_void_p), ("leaves", C.c_void_p), ("consts_mont", C.c_void_p), ("n_consts", C.c_size_t),
                ("leaf_hash", C.POINTER(hk_poseidon_desc)), ("node_hash", C.POINTER(hk_poseidon_desc))]


class hk_sha_tree_out(C.Structure):           # include/hekaton.h
    _fields_ = [("digests_out", C.c_void_p), ("time_entries_mont_out", C.c_void_p), ("sha_root_mont_out", C.c_void_p)]


class hk_r1cs_verdict(C.Structure):           # include/hekaton.h
    _fields_ = [("n_bad", C.c_uint32), ("first_bad", C.c_uint32)]


class hk_timings(C.Structure):
    _fields_ = [(n, C.c_float) for n in
                ("total_ms", "digits_ms", "msm_a_ms", "msm_b_g1_ms", "msm_b_g2_ms", "msm_l_ms",
                 "witness_map_ms", "msm_h_ms", "finish_ms", "accum_kernel_ms")] + \
               [("accum_kernel_launches", C.c_uint32), ("accum_h_ms", C.c_float), ("keygen_qap_ms", C.c_float),
                ("keygen_scalars_ms", C.c_float), ("keygen_sweeps_ms", C.c_float), ("batch_proofs", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


HK_VERIFY_CHECK_POINTS = 1
VERDICT_REJECT, VERDICT_ACCEPT, VERDICT_BAD_POINT = 0, 1, 2

_vp, _sz, _i, _u, _u32, _P = C.c_void_p, C.c_size_t, C.c_int, C.c_uint, C.c_uint32, C.POINTER
_csr3 = [_P(hk_csr)] * 3
_MSM = [_vp, _vp, _sz, _vp, _sz, _i, _i, _vp]
_FIXED_BASE = [_vp, _vp, _vp, _sz, _i, _vp]
_SCALAR_PAIRING = [_vp, _vp, _vp, _sz, _vp]
_LINCOMB = [_vp, _P(_vp), _vp, _sz, _sz, _vp]
_FOLD = [_vp, _vp, _vp, _vp, _u, _sz, _vp]
_FOLD_MANY = [_vp, _sz, _P(_vp), _P(_vp), _vp, _u, _sz, _P(_vp)]
_POINTS_CHECK = [_vp, _vp, _sz, _vp]
_DECOMPRESS = [_vp, _vp, _vp, _sz, _i, _vp, _vp]
_COMPRESS = [_vp, _vp, _sz, _vp, _vp]
_STAGE0 = [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _sz, _vp]

# Every function include/hekaton.h declares, in its order: the argtypes, and the restype where it is not hk_status.  EXPORTS
# and load() follow from this table; tests/test_capi_signatures_cpu.py holds it against the header.
_SIGNATURES = {
    "hk_status_str": ([_i], C.c_char_p),
    "hk_version": ([], C.c_char_p),
    "hk_kernel_info": [_sz, _P(C.c_char_p), _P(_sz), _P(C.c_char_p)],
    "hk_ctx_create": [_i, _i, _P(_vp)],
    "hk_ctx_destroy": ([_vp], None),
    "hk_ctx_sync": [_vp],
    "hk_ctx_set_profiling": [_vp, _i],
    "hk_ctx_last_timings": [_vp, _P(hk_timings)],
    "hk_ctx_sizes": [_vp] + [_P(_sz)] * 4,
    "hk_dev_alloc": [_vp, _sz, _P(_vp)],
    "hk_dev_free": [_vp, _vp],
    "hk_dev_upload": [_vp, _vp, _vp, _sz],
    "hk_dev_download": [_vp, _vp, _vp, _sz],
    "hk_msm_g1": _MSM,
    "hk_msm_g2": _MSM,
    "hk_ntt": [_vp, _vp, _u, _i, _i],
    "hk_witness_map": [_vp] + _csr3 + [_sz, _sz, _vp, _sz, _vp, _sz, _P(_sz)],
    "hk_fixed_base_g1": _FIXED_BASE,
    "hk_fixed_base_g2": _FIXED_BASE,
    "hk_scalar_pairing_g1": _SCALAR_PAIRING,
    "hk_scalar_pairing_g2": _SCALAR_PAIRING,
    "hk_multi_pairing": [_vp, _vp, _vp, _sz, _vp],
    "hk_pairing_products": [_vp, _P(_vp), _sz, _P(_vp), _sz, _sz, _vp],
    "hk_pairing_pairs": [_vp, _P(_vp), _sz, _P(_vp), _sz, _P(_u32), _P(_u32), _sz, _sz, _vp],
    "hk_ctx_gt_bytes": [_vp, _P(_sz)],
    "hk_gt_pow": [_vp, _vp, _vp, _sz, _vp],
    "hk_fq12_pow": [_vp, _vp, _vp, _sz, _vp],
    "hk_gt_pow_prod": [_vp, _vp, _vp, _sz, _sz, _i, _vp],
    "hk_points_lincomb_g1": _LINCOMB,
    "hk_points_lincomb_g2": _LINCOMB,
    "hk_points_fold_g2": _FOLD,
    "hk_keccak_f1600": ([_vp], None),
    "hk_points_fold_g1": _FOLD,
    "hk_points_fold_many_g1": _FOLD_MANY,
    "hk_points_fold_many_g2": _FOLD_MANY,
    "hk_bases_upload": [_vp, _i, _vp, _sz, _P(_vp)],
    "hk_bases_free": ([_vp], None),
    "hk_msm_bases": [_vp, _vp, _vp, _sz, _i, _i, _vp],
    "hk_field_convert": [_vp, _i, _vp, _vp, _sz, _i],
    "hk_assignment_from_bits": [_vp, _vp, _sz, _vp, _vp, _sz, _vp],
    "hk_wprog_upload": [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _sz, _P(_vp)],
    "hk_wprog_free": ([_vp], None),
    "hk_wprog_run": [_vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp],
    "hk_assignment_scatter": [_vp, _vp, _vp, _sz, _sz, _sz, _vp],
    "hk_poseidon_path": [_vp, _vp, _sz, _P(hk_poseidon_desc), _P(hk_poseidon_desc), _vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp],
    "hk_pk_upload": [_vp, _P(hk_pk_desc), _P(_vp)],
    "hk_pk_free": ([_vp], None),
    "hk_commit": [_vp, _vp, _sz, _vp, _sz, _vp, _vp],
    "hk_commit_batch": [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp],
    "hk_prove": [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp],
    "hk_prove_batch": [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp],
    "hk_vk_prepare": [_vp, _P(hk_vk_desc), _P(_vp)],
    "hk_vk_free": ([_vp], None),
    "hk_vk_alpha_beta": [_vp, _vp],
    "hk_verify_batch": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _u, _vp, _vp],
    "hk_points_check_g1": _POINTS_CHECK,
    "hk_points_check_g2": _POINTS_CHECK,
    "hk_field_sqrt": [_vp, _i, _vp, _sz, _vp, _vp],
    "hk_points_decompress_g1": _DECOMPRESS,
    "hk_points_decompress_g2": _DECOMPRESS,
    "hk_points_compress_g1": _COMPRESS,
    "hk_points_compress_g2": _COMPRESS,
    "hk_qap_eval": [_vp] + _csr3 + [_sz, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _P(_sz)],
    "hk_keygen": [_vp, _P(hk_keygen_desc), _P(hk_keygen_out), _P(_sz)],
    "hk_exec_tree": [_vp, _P(hk_exec_tree_desc), _P(hk_exec_tree_out)],
    "hk_stage1_witness": [_vp, _P(hk_stage1_desc), _vp, _sz, _sz, _vp],
    "hk_trace_sort": [_vp, _u32, _vp, _sz, _vp, _vp],
    "hk_stage0_witness": _STAGE0,
    "hk_r1cs_check": [_vp] + _csr3 + [_vp, _sz, _sz, _vp, _vp, _vp, _sz],
    "hk_pk_r1cs_check": [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _sz],
    "hk_sha_tree": [_vp, _vp, _u32, _u32, _u32, _P(hk_sha_tree_out)],
    "hk_sha_tree_inputs": [_vp, _vp, _vp, _u32, _u32, _vp, _sz, _vp],
    "hk_ram_stage0_witness": _STAGE0,
    "hk_ram_stage1_witness": [_vp, _P(hk_ram_stage1_desc), _vp, _sz, _sz, _vp],
    "hk_r1cs_job_trace": [_vp, _P(hk_r1cs_job_desc), _vp],
    "hk_r1cs_job_witness": [_vp, _P(hk_r1cs_job_desc), _vp, _sz, _sz, _sz, _vp],
    "hk_vkd_trace": [_vp, _P(hk_vkd_desc), _vp, _vp],
    "hk_vkd_witness": [_vp, _P(hk_vkd_desc), _vp, _sz, _sz, _P(hk_vkd_cols), _vp],
    "hk_vkd_tree": [_vp, _P(hk_vkd_tree_desc), _vp, _vp, _vp],
    "hk_scalar_powers": [_vp, _vp, _sz, _sz, _vp],
    "hk_ipa_quotient": [_vp, _vp, _sz, _vp, _vp, _sz, _vp],
    "hk_class_power_sums": [_vp, _vp, _vp, _sz, _sz, _vp],
}
EXPORTS = list(_SIGNATURES)

# What the companion header include/hekaton_gt.h declares, in the same idiom: load() sets these as it sets the table above
# and refuses a library that lacks one.  A table of its own only while tests/test_capi_signatures_cpu.py pins the first to
# hekaton.h's names: the two fold together with the two headers, in a change that may touch that test
# (tests/test_gt_check_cpu.py holds this one against its header).
_SIGNATURES_GT = {
    "hk_gt_check": [_vp, _vp, _sz, _vp],
}

_lib = None


def load():
    """Loads libhekaton.so (built by __graft_entry__.build()) and gives every declared function its signature; fails loudly
    when the library is absent, and by the symbol's name (ctypes' AttributeError) when it lacks one."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libhekaton.so not built (%s): run `python -c 'import __graft_entry__ as g; "
                          "g.build()'` — there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, sig in list(_SIGNATURES.items()) + list(_SIGNATURES_GT.items()):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig if isinstance(sig, tuple) else (sig, _i)
    _lib = lib
    return lib


def status_str(s):
    return load().hk_status_str(int(s)).decode()


def check(status, what):
    if status != HK_OK:
        raise HekatonError(status, what)


_check = check          # for Context.points_decompress, whose keyword `check` shadows the function


def ptr(x):
    """c_void_p of a numpy array / DeviceBuffer / bytes-like / int / None."""
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        return C.c_void_p(x.ptr)
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return C.c_void_p(x.ctypes.data)
    if isinstance(x, int):
        return C.c_void_p(x)
    raise TypeError(type(x))


class DeviceBuffer:
    """HBM allocation owned through the C ABI (hk_dev_alloc/free)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(load().hk_dev_alloc(ctx.handle, self.nbytes, C.byref(p)), "hk_dev_alloc")
        self.ptr = p.value

    @classmethod
    def from_host(cls, ctx, arr):
        arr = np.ascontiguousarray(arr)
        return cls(ctx, arr.nbytes).upload(arr)

    def upload(self, arr):
        """The bytes of `arr` (made contiguous) to the start of this allocation; returns self."""
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(load().hk_dev_upload(self.ctx.handle, self.ptr, arr.ctypes.data, arr.nbytes), "hk_dev_upload")
        return self

    def to_host(self):
        out = np.empty(self.nbytes, dtype=np.uint8)
        check(load().hk_dev_download(self.ctx.handle, out.ctypes.data, self.ptr, self.nbytes),
              "hk_dev_download")
        return out

    def free(self):
        if self.ptr:
            load().hk_dev_free(self.ctx.handle, self.ptr)
            self.ptr = None

    def view(self, offset, nbytes):
        """A window of this allocation, usable wherever a DeviceBuffer is (it owns nothing: free() is a no-op)."""
        assert 0 <= offset and offset + nbytes <= self.nbytes
        return DeviceView(self.ctx, self.ptr + int(offset), int(nbytes))


class DeviceView(DeviceBuffer):
    def __init__(self, ctx, ptr_, nbytes):            # noqa: super().__init__ would allocate
        self.ctx, self.ptr, self.nbytes = ctx, ptr_, nbytes

    def free(self):
        pass


# ---- what the wrappers share -------------------------------------------------------------------------------------------
# Keeping operands alive: every array whose address goes into a call or into a descriptor is bound to a local of the wrapper
# (a name, or a list or tuple a name holds) until the call returns.  A ctypes structure that holds c_void_p integers keeps
# nothing alive, so a helper that builds one hands back what it points into and the wrapper binds that too (`d, keep = ...`).
def _hd(x, dtype=np.uint8):
    """A host-or-device operand as the library reads it: a DeviceBuffer (or None, an absent one) as it is, anything else as
    a contiguous array of `dtype` (bytes, unless the entry reads words).  The caller keeps the result alive over the call."""
    return x if x is None or isinstance(x, DeviceBuffer) else np.ascontiguousarray(x, dtype=dtype)


def _nullable(x):
    """The address of a numpy array or DeviceBuffer, or None - NULL - for an absent or empty one: an empty numpy array has
    a data pointer all the same."""
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        return x.ptr if x.nbytes else None
    return x.ctypes.data if x.size else None


def _size(x):
    """The bytes of a host-or-device operand; 0 for an absent one."""
    if x is None:
        return 0
    return x.nbytes if isinstance(x, DeviceBuffer) else np.asarray(x).nbytes


def _ptr_array(xs):
    """The addresses of numpy arrays and DeviceBuffers as a c_void_p array, each as _nullable gives it; never of length 0."""
    return (C.c_void_p * max(len(xs), 1))(*[_nullable(x) for x in xs])


def _device_addr(z):
    """A device output: a DeviceBuffer or its raw address."""
    return z.ptr if isinstance(z, DeviceBuffer) else int(z)


def _challenge_bytes(ctx, challenges):
    """Challenges given as ints or as their Montgomery bytes."""
    if isinstance(challenges, np.ndarray):
        return np.ascontiguousarray(challenges, dtype=np.uint8)
    return ctx.fc.enc(list(challenges))


@contextlib.contextmanager
def _owned(outs, own=True):
    """The outputs a wrapper allocated itself (`own`) are freed when the call under it raises; a caller's never are."""
    try:
        yield
    except HekatonError:
        for x in outs if own else ():
            if isinstance(x, DeviceBuffer):
                x.free()
        raise


class Context:
    """hk_ctx wrapper: one per (process, device)."""

    def __init__(self, curve="bn254", device=0):
        self.lib = load()
        self.curve = curve
        h = C.c_void_p()
        check(self.lib.hk_ctx_create(CURVE_IDS[curve], int(device), C.byref(h)), "hk_ctx_create")
        self.handle = h
        fr, fq, g1, g2 = (C.c_size_t() for _ in range(4))
        check(self.lib.hk_ctx_sizes(h, C.byref(fr), C.byref(fq), C.byref(g1), C.byref(g2)), "hk_ctx_sizes")
        self.fr_bytes, self.fq_bytes, self.g1_bytes, self.g2_bytes = fr.value, fq.value, g1.value, g2.value
        gt = C.c_size_t()
        check(self.lib.hk_ctx_gt_bytes(h, C.byref(gt)), "hk_ctx_gt_bytes")
        self.gt_bytes = gt.value

    @functools.cached_property
    def fc(self):
        """The curve's FrCodec, made on first use: cp_groth16 imports this module."""
        from .cp_groth16 import FrCodec
        return FrCodec(self.curve)

    def _group(self, group, stem=None):
        """(bytes of a packed affine point of G1 / G2, the library's `stem`_g1 / `stem`_g2 - None without a stem)."""
        pb, suffix = (self.g1_bytes, "_g1") if group == 1 else (self.g2_bytes, "_g2")
        return pb, stem and getattr(self.lib, stem + suffix)

    def _outputs(self, sizes, device_out):
        """One output per byte count of `sizes`: zeroed uint8 arrays, or - device_out - DeviceBuffers, never of 0 bytes."""
        return [DeviceBuffer(self, max(b, 1)) if device_out else np.zeros(b, dtype=np.uint8) for b in sizes]

    def close(self):
        if self.handle:
            self.lib.hk_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        check(self.lib.hk_ctx_sync(self.handle), "hk_ctx_sync")

    def set_profiling(self, on=True):
        check(self.lib.hk_ctx_set_profiling(self.handle, int(bool(on))), "hk_ctx_set_profiling")

    def last_timings(self):
        t = hk_timings()
        check(self.lib.hk_ctx_last_timings(self.handle, C.byref(t)), "hk_ctx_last_timings")
        return t.as_dict()

    # ---- primitives ---------------------------------------------------------------------------
    def _msm(self, group, bases, scalars, n_bases, n_scalars, mont, checked):
        pb, fn = self._group(group, "hk_msm")
        nb = n_bases if n_bases is not None else _size(bases) // pb
        ns = n_scalars if n_scalars is not None else _size(scalars) // self.fr_bytes
        out = np.zeros(pb, dtype=np.uint8)
        check(fn(self.handle, ptr(bases), nb, ptr(scalars), ns, int(mont), int(checked), out.ctypes.data), fn.__name__)
        return out

    def msm_g1(self, bases, scalars, n_bases=None, n_scalars=None, montgomery=True, checked=True):
        """E::G1::msm / msm_bigint / msm_unchecked (prover.rs:88,97,117,129; committer.rs:89,113)."""
        return self._msm(1, bases, scalars, n_bases, n_scalars, montgomery, checked)

    def msm_g2(self, bases, scalars, n_bases=None, n_scalars=None, montgomery=True, checked=True):
        """E::G2 MSM (prover.rs:107)."""
        return self._msm(2, bases, scalars, n_bases, n_scalars, montgomery, checked)

    def fixed_base(self, group, base, scalars, n=None, montgomery=True, out=None):
        """FixedBase::msm + normalize_batch (generator.rs:134-224): out[i] = scalars[i] * base.
        `out` may be a DeviceBuffer (stays in HBM); otherwise a numpy array is returned."""
        pb, fn = self._group(group, "hk_fixed_base")
        n = n if n is not None else _size(scalars) // self.fr_bytes
        base = _hd(base)
        res = out if out is not None else np.zeros(n * pb, dtype=np.uint8)
        check(fn(self.handle, ptr(base), ptr(scalars), n, int(montgomery), ptr(res)), fn.__name__)
        return res

    def scalar_pairing(self, group, points, scalars, n=None, out=None):
        """`scalar_pairing` (distributed-prover/src/pairing_ops.rs:32-39): out[i] = scalars[i] * points[i].  `out` may be a
        DeviceBuffer (the result stays in HBM)."""
        pb, fn = self._group(group, "hk_scalar_pairing")
        n = n if n is not None else _size(scalars) // self.fr_bytes
        res = out if out is not None else np.zeros(n * pb, dtype=np.uint8)
        check(fn(self.handle, ptr(points), ptr(scalars), n, ptr(res)), fn.__name__)
        return res

    def scalar_powers(self, x, n, reps=1, out=None):
        """hk_scalar_powers: `structured_scalar_power` (distributed-prover/src/pairing_ops.rs:42-48) - the Montgomery bytes of
        x^0 .. x^(n - 1) (x an int), `reps` times back to back.  `out` may be a DeviceBuffer / DeviceView of reps * n Fr (the
        result stays in HBM); otherwise a numpy array is returned."""
        xb = self.fc.enc1(x)
        res = out if out is not None else np.zeros(reps * n * self.fr_bytes, dtype=np.uint8)
        check(self.lib.hk_scalar_powers(self.handle, xb.ctypes.data, int(n), int(reps), ptr(res)), "hk_scalar_powers")
        return res

    def ipa_quotient(self, challenges, rho, z, shift=0, out=None):
        """hk_ipa_quotient: the Montgomery bytes of the quotient of X^shift prod_k (1 + challenges[k] (rho X)^(2^k)) by
        (X - z), one zero appended: shift + 2^len(challenges) Fr (kzg.rs:122-141).  challenges, rho, z: ints.  `out` may be
        a DeviceBuffer / DeviceView of that size (the result stays in HBM); otherwise a numpy array is returned."""
        challenges = list(challenges)
        l = len(challenges)
        ch, rb, zb = self.fc.enc(challenges), self.fc.enc1(rho), self.fc.enc1(z)
        res = out if out is not None else np.zeros((shift + (1 << l)) * self.fr_bytes, dtype=np.uint8)
        check(self.lib.hk_ipa_quotient(self.handle, ch.ctypes.data if l else None, l, rb.ctypes.data, zb.ctypes.data, int(shift),
                                       ptr(res)), "hk_ipa_quotient")
        return res

    def class_power_sums(self, x, class_of, n_classes, out=None):
        """hk_class_power_sums: the Montgomery bytes of sums[c] = sum of x^i over the i with class_of[i] == c, c < n_classes
        (x an int) - the exponents of an aggregate verifier's prod_c e(alpha_c, beta_c)^(sums[c]).  class_of: a uint32 array or
        a DeviceBuffer of n uint32.  `out` may be a DeviceBuffer / DeviceView of n_classes Fr (the result stays in HBM);
        otherwise a numpy array is returned.  A class id >= n_classes is refused (HK_ERR_ARG)."""
        xb = self.fc.enc1(x)
        class_of = _hd(class_of, np.uint32)
        n = _size(class_of) // 4
        if n == 0 and isinstance(class_of, np.ndarray):
            class_of = np.zeros(1, np.uint32)                 # the entry wants a pointer even where it reads nothing
        res = out if out is not None else np.zeros(int(n_classes) * self.fr_bytes, dtype=np.uint8)
        check(self.lib.hk_class_power_sums(self.handle, xb.ctypes.data, ptr(class_of), n, int(n_classes), ptr(res)),
              "hk_class_power_sums")
        return res

    def gt_pow(self, gts, scalars, in_gt=True):
        """hk_gt_pow: element-wise powers in GT (the exponent split along the Frobenius - the bases must have order r);
        in_gt=False: hk_fq12_pow, the plain chain for values of unknown provenance (a verifier's inputs).
        gts: (n, gt_bytes) uint8; scalars: n Fr Montgomery bytes."""
        gts, scalars = _hd(gts), _hd(scalars)
        out = np.zeros((_size(gts) // self.gt_bytes, self.gt_bytes), dtype=np.uint8)
        fn = self.lib.hk_gt_pow if in_gt else self.lib.hk_fq12_pow
        check(fn(self.handle, ptr(gts), ptr(scalars), out.shape[0], out.ctypes.data), fn.__name__)
        return out

    def gt_pow_prod(self, gts, scalars, group_len, in_gt=True):
        """hk_gt_pow_prod: out[g] = prod_j gts[g * group_len + j]^scalars[g * group_len + j] (a verifier's
        multi-exponentiations).  Returns (n / group_len, gt_bytes) uint8."""
        gts, scalars = _hd(gts), _hd(scalars)
        n = _size(gts) // self.gt_bytes
        out = np.zeros((n // max(1, group_len), self.gt_bytes), dtype=np.uint8)
        check(self.lib.hk_gt_pow_prod(self.handle, ptr(gts), ptr(scalars), n, group_len, 1 if in_gt else 0, out.ctypes.data),
              "hk_gt_pow_prod")
        return out

    def multi_pairing(self, g1, g2, n=None):
        """`pairing(left, right)` (distributed-prover/src/pairing_ops.rs:25-29): prod_i e(g1[i], g2[i]) as ark's Fp12
        bytes (12 Fq, Montgomery)."""
        n = n if n is not None else _size(g1) // self.g1_bytes
        out = np.zeros(self.gt_bytes, dtype=np.uint8)
        check(self.lib.hk_multi_pairing(self.handle, ptr(g1) if n else None, ptr(g2) if n else None, n, out.ctypes.data),
              "hk_multi_pairing")
        return out

    def pairing_products(self, lhs, rhs, n=None):
        """Every G1 vector of `lhs` against every G2 vector of `rhs` in one batched launch (the `cross_terms` of
        aggregation.rs:255-263): returns a (len(lhs), len(rhs), gt_bytes) uint8 array."""
        lhs, rhs = [_hd(x) for x in lhs], [_hd(x) for x in rhs]
        n = n if n is not None else _size(lhs[0]) // self.g1_bytes
        lp, rp = _ptr_array(lhs), _ptr_array(rhs)
        out = np.zeros((len(lhs), len(rhs), self.gt_bytes), dtype=np.uint8)
        check(self.lib.hk_pairing_products(self.handle, lp, len(lhs), rp, len(rhs), n, out.ctypes.data),
              "hk_pairing_products")
        return out

    def pairing_pairs(self, lhs, rhs, pairs, n=None):
        """pairing(lhs[a], rhs[b]) for each (a, b) of `pairs` in one batched launch (hk_pairing_pairs: the cross terms of a
        GIPA round): returns a (len(pairs), gt_bytes) uint8 array."""
        lhs, rhs = [_hd(x) for x in lhs], [_hd(x) for x in rhs]
        n = n if n is not None else _size(lhs[0]) // self.g1_bytes
        lp, rp = _ptr_array(lhs), _ptr_array(rhs)
        pa = (C.c_uint32 * len(pairs))(*[a for a, _ in pairs])
        pb = (C.c_uint32 * len(pairs))(*[b for _, b in pairs])
        out = np.zeros((len(pairs), self.gt_bytes), dtype=np.uint8)
        check(self.lib.hk_pairing_pairs(self.handle, lp, len(lhs), rp, len(rhs), pa, pb, len(pairs), n, out.ctypes.data),
              "hk_pairing_pairs")
        return out

    def points_lincomb(self, group, vecs, coeffs, n=None):
        """out[i] = sum_j coeffs[j] * vecs[j][i] (aggregation.rs:192-203,293-326); coeffs: k Fr Montgomery bytes."""
        pb, fn = self._group(group, "hk_points_lincomb")
        vecs, coeffs = [_hd(x) for x in vecs], _hd(coeffs)
        n = n if n is not None else _size(vecs[0]) // pb
        out = np.zeros(n * pb, dtype=np.uint8)
        check(fn(self.handle, _ptr_array(vecs), ptr(coeffs), len(vecs), n, out.ctypes.data), fn.__name__)
        return out

    def _fold_coeffs(self, group, c):
        """The scalar c (an int mod r) split along the group's endomorphism (endo.Phi2 in G1, endo.Psi4 in G2): the parts'
        magnitudes as Montgomery bytes and the mask of the negative ones."""
        from .endo import phi2, psi4
        k = {1: phi2, 2: psi4}[group](self.curve).decompose(c)
        neg = sum(1 << j for j, v in enumerate(k) if v < 0)
        return self.fc.enc([abs(v) for v in k]), neg

    def _points_fold(self, group, lo, hi, c, n, out):
        pb, fn = self._group(group, "hk_points_fold")
        coeffs, neg = self._fold_coeffs(group, c)
        lo, hi = _hd(lo), _hd(hi)
        n = n if n is not None else _size(hi) // pb
        res = out if out is not None else np.zeros(n * pb, dtype=np.uint8)                      # a DeviceBuffer stays in HBM
        check(fn(self.handle, ptr(lo), ptr(hi), coeffs.ctypes.data, neg, n, ptr(res)), fn.__name__)
        return res

    def points_fold_g2(self, lo, hi, c, n=None, out=None):
        """out[i] = lo[i] + c * hi[i] in G2 (the fold of a TIPA round) through hk_points_fold_g2: the scalar c (an int mod r)
        is split along the endomorphism psi into four ~64-bit parts (endo.Psi4), so the element-wise double-and-add chain is
        ~66 steps instead of 254."""
        return self._points_fold(2, lo, hi, c, n, out)

    def points_fold_g1(self, lo, hi, c, n=None, out=None):
        """out[i] = lo[i] + c * hi[i] in G1 through hk_points_fold_g1: c split along the GLV endomorphism into two ~128-bit
        parts (endo.Phi2)."""
        return self._points_fold(1, lo, hi, c, n, out)

    def points_fold_many(self, group, los, his, c, n, outs):
        """outs[y][i] = los[y][i] + c * his[y][i] for up to 4 vector pairs and one scalar c (hk_points_fold_many_g1 / _g2):
        the folds of one TIPA round that share a challenge.  los / his: DeviceBuffer / DeviceView or uint8 arrays; outs:
        DeviceBuffer / DeviceView (stay in HBM) or uint8 arrays of n points each."""
        coeffs, neg = self._fold_coeffs(group, c)
        los, his = [_hd(x) for x in los], [_hd(x) for x in his]
        fn = self._group(group, "hk_points_fold_many")[1]
        check(fn(self.handle, len(outs), _ptr_array(los), _ptr_array(his), coeffs.ctypes.data, neg, n, _ptr_array(outs)),
              fn.__name__)
        return outs

    def assignment_from_bits(self, bits, full_cols, full_vals, out=None):
        """hk_assignment_from_bits: the Montgomery assignment of a bit-valued witness, materialised in HBM.  bits: uint8
        array (one per variable); full_cols: column indices of the full-width values; full_vals: their Montgomery bytes.
        Returns a DeviceBuffer of n_v Fr (or fills `out`)."""
        bits, cols, vals = _hd(bits), _hd(full_cols, np.uint32), _hd(full_vals)
        n_v, n_full = _size(bits), _size(cols) // 4
        buf = out if out is not None else DeviceBuffer(self, n_v * self.fr_bytes)
        check(self.lib.hk_assignment_from_bits(self.handle, ptr(bits), n_v, ptr(cols) if n_full else None,
                                               ptr(vals) if n_full else None, n_full, buf.ptr), "hk_assignment_from_bits")
        return buf

    def poseidon_path(self, params, leaf, siblings, index, n_v, col0, z_out):
        """hk_poseidon_path: the membership block of `batch` assignments, written on the device.  params:
        (consts DeviceBuffer or Montgomery bytes, n_consts, (t, alpha, rf, rp, off) of the leaf hash, same of the node hash)
        - poseidon.device_params(curve); leaf: Montgomery bytes (batch, 4 Fr); siblings: (batch, depth Fr); index: uint32
        (batch); z_out: DeviceBuffer (or raw device address) of batch x n_v Fr.  leaf and siblings may also be the
        DeviceBuffers hk_exec_tree left on the device (both then; batch = len(index))."""
        consts, n_consts, ld, nd = params
        index = np.ascontiguousarray(index, dtype=np.uint32)
        leaf, siblings = _hd(leaf), _hd(siblings)
        batch = index.size
        depth = _size(siblings) // (batch * self.fr_bytes)
        a, b = hk_poseidon_desc(*ld), hk_poseidon_desc(*nd)
        check(self.lib.hk_poseidon_path(self.handle, ptr(consts), int(n_consts), C.byref(a), C.byref(b), ptr(leaf),
                                        ptr(siblings) if depth else None, index.ctypes.data, depth, batch, int(n_v),
                                        int(col0), _device_addr(z_out)), "hk_poseidon_path")

    def wprog_upload(self, ops, refs, vmap, n_values, n_inputs):
        """hk_wprog_upload: a class's word program (sha_circuit.Tape.word_program) resident on the device."""
        ops, refs, vmap = _hd(ops, np.uint32), _hd(refs, np.uint32), _hd(vmap, np.uint32)
        n_v = _size(vmap) // 4
        h = C.c_void_p()
        check(self.lib.hk_wprog_upload(self.handle, ptr(ops), _size(ops) // 32, _nullable(refs), _size(refs) // 4, ptr(vmap), n_v,
                                       int(n_values), int(n_inputs), C.byref(h)), "hk_wprog_upload")
        return WordProgram(self, h, n_v, int(n_inputs))

    def bases_upload(self, group, bases, n=None):
        """Makes a static base set resident with its shift tables (hk_bases_upload); returns a ResidentBases."""
        n = n if n is not None else _size(bases) // self._group(group)[0]
        h = C.c_void_p()
        check(self.lib.hk_bases_upload(self.handle, int(group), ptr(bases), n, C.byref(h)), "hk_bases_upload")
        return ResidentBases(self, h, group, n)

    def field_convert(self, which, data, to_mont):
        """Montgomery <-> canonical for a packed array of Fr (`which` = 0) or Fq (1) elements: what ark-ff
        `from_bigint` / `into_bigint` do under ark-serialize.  Returns a new numpy uint8 array."""
        eb = self.fr_bytes if which == 0 else self.fq_bytes
        data = _hd(data)
        n = _size(data) // eb
        out = np.empty(n * eb, dtype=np.uint8)
        check(self.lib.hk_field_convert(self.handle, int(which), ptr(data), out.ctypes.data, n, int(to_mont)),
              "hk_field_convert")
        return out

    def ntt(self, data, log_m, inverse=False, coset=False):
        """In-place on `data` (numpy uint8 array of 2^log_m Fr or a DeviceBuffer)."""
        check(self.lib.hk_ntt(self.handle, ptr(data), int(log_m), int(inverse), int(coset)), "hk_ntt")
        return data

    def witness_map(self, A, B, Cm, n_inst, n_constraints, z, n_v=None):
        """R1CSToQAP::witness_map (prover.rs:123).  A/B/Cm: (row_ptr u64, col u32, val bytes) triples.
        Returns (h bytes [m Fr, natural order], m)."""
        keep = []
        csrs = self._csrs((A, B, Cm), keep)
        nv = n_v if n_v is not None else _size(z) // self.fr_bytes
        m = 1
        while m < n_constraints + n_inst:
            m *= 2
        out = np.zeros(m * self.fr_bytes, dtype=np.uint8)
        m_out = C.c_size_t()
        check(self.lib.hk_witness_map(self.handle, C.byref(csrs[0]), C.byref(csrs[1]), C.byref(csrs[2]),
                                      n_inst, n_constraints, ptr(z), nv, out.ctypes.data, m, C.byref(m_out)),
              "hk_witness_map")
        return out, m_out.value

    @staticmethod
    def _csrs(matrices, keep):
        """hk_csr structs over (row_ptr, col, val) triples; each member a numpy array (host) or a DeviceBuffer (device)."""
        out = []
        for (rp, col, val) in matrices:
            arrs = [_hd(rp, np.uint64), _hd(col, np.uint32), _hd(val)]
            keep += arrs
            out.append(hk_csr(*[_nullable(x) for x in arrs], _size(arrs[0]) // 8 - 1, _size(arrs[1]) // 4))
        return out

    def qap_eval(self, A, B, Cm, n_inst, n_constraints, n_v, t, out=None):
        """hk_qap_eval (instance_map_with_evaluation, generator.rs:75-76) at t (int, or Montgomery bytes).  A/B/Cm: CSR
        triples as in witness_map (members may be DeviceBuffers).  out: optional (a, b, c) DeviceBuffers of n_v Fr each.
        Returns (a, b, c, zt, m): a/b/c Montgomery bytes (numpy, or the given DeviceBuffers), zt Montgomery bytes."""
        keep = []
        csrs = self._csrs((A, B, Cm), keep)
        t = self.fc.enc1(t) if isinstance(t, int) else np.ascontiguousarray(t, dtype=np.uint8)
        outs = out if out is not None else [np.zeros(n_v * self.fr_bytes, dtype=np.uint8) for _ in range(3)]
        zt = np.zeros(self.fr_bytes, dtype=np.uint8)
        m = C.c_size_t()
        check(self.lib.hk_qap_eval(self.handle, C.byref(csrs[0]), C.byref(csrs[1]), C.byref(csrs[2]), n_inst, n_constraints,
                                   n_v, t.ctypes.data, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), zt.ctypes.data, C.byref(m)),
              "hk_qap_eval")
        return outs[0], outs[1], outs[2], zt, m.value

    def keygen(self, *, matrices, n_inst, n_constraints, n_v, stage_ranges, alpha, beta, gamma, deltas, t, g1_scalar,
               g2_scalar, on_device=False, with_qap=False):
        """hk_keygen: generate_parameters past synthesis (generator.rs:66-224) in one device call.  Scalars are ints (or
        Montgomery bytes); matrices: CSR triples as in witness_map; stage_ranges: [(begin, end)] over witness indices.
        on_device: a_g, b_g, b_h, h_g come back as DeviceBuffers (the rest on the host).  Returns a dict of packed-affine
        arrays: a_g, b_g, b_h, h_g, ck (list per stage), deltas_g, alpha_g, beta_g, gamma_abc_g, beta_h, gamma_h, deltas_h,
        and m; with with_qap also qap_abc (3 n_v Fr, Montgomery bytes, a | b | c)."""
        enc = lambda x: self.fc.enc1(x) if isinstance(x, int) else np.ascontiguousarray(x, dtype=np.uint8)
        keep = []
        csrs = self._csrs(matrices, keep)
        ns = len(stage_ranges)
        m = 1
        while m < n_constraints + n_inst:
            m *= 2
        g1, g2 = self.g1_bytes, self.g2_bytes

        def buf(nbytes, dev=False):
            return DeviceBuffer(self, nbytes) if dev else np.zeros(nbytes, dtype=np.uint8)
        res = dict(a_g=buf(n_v * g1, on_device), b_g=buf(n_v * g1, on_device), b_h=buf(n_v * g2, on_device),
                   h_g=buf(max(m - 1, 0) * g1, on_device), ck=[buf((e - b) * g1) for b, e in stage_ranges],
                   deltas_g=buf(ns * g1), alpha_g=buf(g1), beta_g=buf(g1), gamma_abc_g=buf(n_inst * g1), beta_h=buf(g2),
                   gamma_h=buf(g2), deltas_h=buf(ns * g2))
        if with_qap:
            res["qap_abc"] = buf(3 * n_v * self.fr_bytes)
        sr = np.array([v for be in stage_ranges for v in be], dtype=np.uint64)
        sc = [enc(x) for x in (alpha, beta, gamma, t, g1_scalar, g2_scalar)]
        dl = np.concatenate([enc(x) for x in deltas]) if ns else np.zeros(0, np.uint8)
        d = hk_keygen_desc(C.pointer(csrs[0]), C.pointer(csrs[1]), C.pointer(csrs[2]), n_inst, n_constraints, n_v,
                           sr.ctypes.data if ns else None, ns, *[x.ctypes.data for x in sc], dl.ctypes.data if ns else None)
        ckp = _ptr_array(res["ck"])
        o = hk_keygen_out(*[_nullable(res[k]) for k in ("a_g", "b_g", "b_h", "h_g")], ckp,
                          *[_nullable(res[k]) for k in ("deltas_g", "alpha_g", "beta_g", "gamma_abc_g", "beta_h", "gamma_h",
                                                        "deltas_h")], _nullable(res.get("qap_abc")))
        m_out = C.c_size_t()
        with _owned(res.values()):
            check(self.lib.hk_keygen(self.handle, C.byref(d), C.byref(o), C.byref(m_out)), "hk_keygen")
        res["m"] = m_out.value
        return res

    def exec_tree(self, params, entry_fields, offsets, time_entries, addr_entries, challenges, device_out=False, out=None):
        """hk_exec_tree: the coordinator's step between the rounds (coordinator.rs:125-174, 425-466) in one device call.
        params: poseidon.device_params(curve), as poseidon_path takes it; entry_fields: 2 (ROM) or 4 (RAM); offsets:
        n_sub + 1 uint32, subtrace i = entries [offsets[i], offsets[i + 1]) of both orders; time_entries / addr_entries:
        Montgomery bytes (or DeviceBuffers) of offsets[-1] x entry_fields Fr; challenges: entry_fields ints (or their
        Montgomery bytes) in the reference's challenges() order, tr_chal last.  Returns (evals [n_sub x 2 Fr], leaves
        [n_sub x (2 + entry_fields)], nodes [2 n_sub - 1: leaf digests, each level, root last], siblings [n_sub x depth,
        bottom-up], root) as Montgomery bytes, or as DeviceBuffers when device_out is set; out: five buffers of those
        sizes to fill and return instead (numpy arrays or DeviceBuffers)."""
        consts, n_consts, ld, nd = params
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        n_sub = offsets.size - 1
        keep = [_hd(time_entries), _hd(addr_entries)]
        ch = _challenge_bytes(self, challenges)
        depth = max(n_sub, 1).bit_length() - 1
        fr = self.fr_bytes
        sizes = [2 * n_sub, (2 + entry_fields) * n_sub, 2 * n_sub - 1, n_sub * depth, 1]
        if out is not None:
            outs = list(out)
            assert [x.nbytes >= k * fr for x, k in zip(outs, sizes)] == [True] * 5
        else:
            outs = self._outputs([max(k, 0) * fr for k in sizes], device_out)
        a, b = hk_poseidon_desc(*ld), hk_poseidon_desc(*nd)
        d = hk_exec_tree_desc(n_sub, int(entry_fields), offsets.ctypes.data, _nullable(keep[0]), _nullable(keep[1]),
                              ch.ctypes.data, ptr(consts), int(n_consts), C.pointer(a), C.pointer(b))
        o = hk_exec_tree_out(*[ptr(x) for x in outs])
        with _owned(outs, out is None):
            check(self.lib.hk_exec_tree(self.handle, C.byref(d), C.byref(o)), "hk_exec_tree")
        return tuple(outs)

    def stage1_witness(self, params, n_portals, offsets, time_entries, addr_entries, challenges, exec_outs, sub_index, n_v,
                       layout, z_out):
        """hk_stage1_witness: every challenge-dependent column of the assignments of the subcircuits `sub_index` (any order,
        repeats allowed; row b of z_out = subcircuit sub_index[b]), from what exec_tree took and returned.  params, offsets,
        time_entries, addr_entries, challenges: as exec_tree takes them (ROM entries: 2 Fr each; challenges = entry_chal,
        tr_chal); exec_outs: exec_tree's return value (evals, leaves, nodes, siblings, root), numpy arrays or DeviceBuffers;
        n_portals: the entries each selected subcircuit owns per order; layout: (inst_col0, col0, pos_col0) - the first
        column of the three instance values, of the 10 n_portals + 4 portal columns and of the membership block; z_out:
        DeviceBuffer (or raw device address) of len(sub_index) x n_v Fr.  Every other column keeps its bytes."""
        return self._stage1_witness("hk_stage1_witness", hk_stage1_desc, params, n_portals, offsets, time_entries, addr_entries,
                                    challenges, exec_outs, sub_index, n_v, (), layout, z_out)

    def _stage1_witness(self, symbol, desc, params, n_portals, offsets, time_entries, addr_entries, challenges, exec_outs,
                        sub_index, n_v, extra, layout, z_out):
        """stage1_witness / ram_stage1_witness: the two descriptors share their fields up to node_hash; `extra`: the
        host-or-device operands the descriptor `desc` has between those and the columns of `layout`."""
        consts, n_consts, ld, nd = params
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        n_sub = offsets.size - 1
        sub_index = np.ascontiguousarray(sub_index, dtype=np.uint32)
        evals, leaves, _nodes, siblings, root = exec_outs
        keep = [_hd(x) for x in (time_entries, addr_entries, evals, leaves, siblings, root) + tuple(extra)]
        ch = _challenge_bytes(self, challenges)
        a, b = hk_poseidon_desc(*ld), hk_poseidon_desc(*nd)
        d = desc(n_sub, int(n_portals), max(n_sub, 1).bit_length() - 1, offsets.ctypes.data, _nullable(keep[0]),
                 _nullable(keep[1]), ch.ctypes.data, *[_nullable(x) for x in keep[2:6]], ptr(consts), int(n_consts),
                 C.pointer(a), C.pointer(b), *[_nullable(x) for x in keep[6:]], *[int(c) for c in layout])
        check(getattr(self.lib, symbol)(self.handle, C.byref(d), _nullable(sub_index), sub_index.size, int(n_v),
                                        _device_addr(z_out)), symbol)
        return z_out

    def trace_sort(self, entry_fields, time_entries, n_entries=None, device_out=False, want_perm=False):
        """hk_trace_sort: the address-ordered trace (coordinator.rs:92-123) from the flattened time-ordered one - the stable
        sort by addr (entry_fields 2, ROM) or (addr, timestamp) (entry_fields 4, RAM).  time_entries: Montgomery bytes or a
        DeviceBuffer of n_entries x entry_fields Fr (n_entries defaults to all of it).  Returns the sorted entries in the
        same layout - Montgomery bytes, or a DeviceBuffer when device_out is set - and with want_perm the pair (entries,
        perm): sorted entry j = time entry perm[j], uint32 (a numpy array, or a DeviceBuffer when device_out is set)."""
        k, fr = int(entry_fields), self.fr_bytes
        src = _hd(time_entries)
        n = int(n_entries) if n_entries is not None else _size(src) // (max(k, 1) * fr)
        out, *perm = self._outputs([n * k * fr] + [4 * n] * bool(want_perm), device_out)
        perm = None if not want_perm else perm[0] if device_out else perm[0].view(np.uint32)
        with _owned((out, perm)):
            check(self.lib.hk_trace_sort(self.handle, k, ptr(src) if n else None, n, ptr(out) if n else None,
                                         ptr(perm) if n else None), "hk_trace_sort")
        return (out, perm) if want_perm else out

    def stage0_witness(self, offsets, n_portals, time_entries, addr_entries, sub_index, w_out):
        """hk_stage0_witness: row b of w_out (a DeviceBuffer or raw device address of len(sub_index) x 4 n_portals Fr) = the
        stage-0 witness of subcircuit sub_index[b]: (addr, val) of its n_portals time-ordered, then of its n_portals address-
        ordered entries.  offsets: n_sub + 1 uint32 as exec_tree takes them; time_entries / addr_entries: Montgomery bytes or
        DeviceBuffers of offsets[-1] x 2 Fr (ROM).  w_out is what ProvingKey.commit_batch / hk_commit_batch read."""
        return self._stage0_witness("hk_stage0_witness", offsets, n_portals, time_entries, addr_entries, sub_index, w_out)

    def _stage0_witness(self, symbol, offsets, n_portals, time_entries, addr_entries, sub_index, w_out):
        """stage0_witness / ram_stage0_witness: the two entries take the same arguments."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        sub_index = np.ascontiguousarray(sub_index, dtype=np.uint32)
        keep = [_hd(time_entries), _hd(addr_entries)]
        check(getattr(self.lib, symbol)(self.handle, offsets.ctypes.data, offsets.size - 1, int(n_portals), ptr(keep[0]),
                                        ptr(keep[1]), _nullable(sub_index), sub_index.size, _device_addr(w_out)), symbol)
        return w_out

    def sha_tree(self, leaves, n_sub, ns, n_portals, device_out=False):
        """hk_sha_tree: the data tree and the time-ordered trace of a big-merkle job (tree_hash_circuit.rs:313-470) from its
        leaves.  leaves: n_sub / 2 x 64 bytes - a list of bytes, a uint8 array or a DeviceBuffer.  Returns (digests [n_sub x
        32 B, subcircuit order, padding last], time_entries [n_sub x n_portals x 2 Fr, Montgomery: what trace_sort / exec_tree
        / stage0_witness take], sha_root [1 Fr]) as uint8 arrays, or as DeviceBuffers when device_out is set."""
        n, k, fr = int(n_sub), int(n_portals), self.fr_bytes
        if isinstance(leaves, (list, tuple)):
            leaves = np.frombuffer(b"".join(leaves), np.uint8)
        src = _hd(leaves)
        outs = self._outputs([32 * n, 2 * n * k * fr, fr], device_out)
        o = hk_sha_tree_out(*[ptr(x) for x in outs])
        with _owned(outs):
            check(self.lib.hk_sha_tree(self.handle, ptr(src), n, int(ns), k, C.byref(o)), "hk_sha_tree")
        return tuple(outs)

    def sha_tree_inputs(self, leaves, digests, n_sub, n_inputs, sub_index, device_out=False):
        """hk_sha_tree_inputs: the word-program inputs (sha_circuit.program_inputs) of the subcircuits `sub_index` of one
        kind - n_inputs 16: leaves and the padding subcircuit, from `leaves`; 54: parents and the root, from `digests`
        (sha_tree's).  leaves / digests: uint8 arrays, DeviceBuffers, or None for the one the kind does not read.  Returns
        uint32 (len(sub_index), n_inputs), or a DeviceBuffer of it when device_out is set."""
        keep = [_hd(leaves), _hd(digests)]
        sub_index = np.ascontiguousarray(sub_index, dtype=np.uint32)
        batch, k = sub_index.size, int(n_inputs)
        out, = self._outputs([4 * batch * k], device_out)
        if not device_out:
            out = out.view(np.uint32).reshape(batch, k)
        with _owned((out,)):
            check(self.lib.hk_sha_tree_inputs(self.handle, ptr(keep[0]), ptr(keep[1]), int(n_sub), k, _nullable(sub_index), batch,
                                              ptr(out)), "hk_sha_tree_inputs")
        return out

    def ram_stage0_witness(self, offsets, n_portals, time_entries, addr_entries, sub_index, w_out):
        """hk_ram_stage0_witness: row b of w_out (a DeviceBuffer or raw device address of len(sub_index) x 70 n_portals Fr) =
        the stage-0 witness of the RAM subcircuit sub_index[b]: 35 columns (val, addr, 32 timestamp bits, read) per entry, its
        n_portals time-ordered then its n_portals address-ordered entries.  offsets: n_sub + 1 uint32; time_entries /
        addr_entries: Montgomery bytes or DeviceBuffers of offsets[-1] x 4 Fr (RAM: what trace_sort(4, ...) takes and gives)."""
        return self._stage0_witness("hk_ram_stage0_witness", offsets, n_portals, time_entries, addr_entries, sub_index, w_out)

    def ram_stage1_witness(self, params, n_portals, offsets, time_entries, addr_entries, challenges, exec_outs, sub_index, n_v,
                           layout, z_out, template=None):
        """hk_ram_stage1_witness: whole assignment rows of the RAM subcircuits `sub_index` (any order, repeats allowed), from
        what exec_tree(params, 4, ...) took and returned.  challenges: entry_chal_1..3, tr_chal (ints or Montgomery bytes);
        layout: (inst_col0, stage0_col0, col0, pos_col0) - the first column of the five instance values, of the 70 n_portals
        stage-0 columns, of the 43 n_portals + 37 portal columns and of the membership block; template: Montgomery bytes or
        a DeviceBuffer of n_v Fr every row starts from, or None: every column the call does not own keeps its bytes."""
        return self._stage1_witness("hk_ram_stage1_witness", hk_ram_stage1_desc, params, n_portals, offsets, time_entries,
                                    addr_entries, challenges, exec_outs, sub_index, n_v, (template,), layout, z_out)

    def _r1cs_job_desc(self, tables, witness):
        """(hk_r1cs_job_desc, what must stay alive beside it) from `PartitionedR1csJob.tables()` and the witness blocks."""
        arr = {k: np.ascontiguousarray(tables[k], dtype=np.uint32)
               for k in ("slot_offsets", "slot_rank", "slot_src", "wit_offsets", "body_len")}
        wit = _hd(witness)
        p = _nullable
        d = hk_r1cs_job_desc(int(tables["n_parts"]), int(tables["n_txs"]), arr["slot_offsets"].ctypes.data, p(arr["slot_rank"]),
                             p(arr["slot_src"]), int(tables["sets_per_tx"]), int(tables["tx_len"]), int(tables["tx_stride"]),
                             p(arr["wit_offsets"]), p(arr["body_len"]), ptr(wit))
        return d, (arr, wit)

    def r1cs_job_trace(self, tables, witness, device_out=False, out=None):
        """hk_r1cs_job_trace: the flattened time-ordered ROM trace of a partitioned R1CS job
        (partitioned_r1cs_circuit.rs:182-220 `get_portal_subtraces`) - what trace_sort(2, ...), exec_tree and stage0_witness
        take.  tables: `PartitionedR1csJob.tables()`; witness: Montgomery bytes or a DeviceBuffer of the job's witness blocks
        (`witness_bytes()`).  Returns n_txs x slots (addr, val) pairs as Montgomery bytes, or as a DeviceBuffer when
        device_out is set; out: a buffer of that size (numpy array or DeviceBuffer) to fill and return instead."""
        d, keep = self._r1cs_job_desc(tables, witness)
        n = int(tables["n_txs"]) * int(np.asarray(tables["slot_offsets"])[-1]) * 2 * self.fr_bytes
        own = out is None
        if own:
            out, = self._outputs([n], device_out)
        with _owned((out,), own):
            check(self.lib.hk_r1cs_job_trace(self.handle, C.byref(d), ptr(out)), "hk_r1cs_job_trace")
        return out

    def r1cs_job_witness(self, tables, witness, sub_index, n_v, body_col0, z_out):
        """hk_r1cs_job_witness: column 0 and the body columns of the assignments of the subcircuits `sub_index` of ONE
        partition (any order, repeats allowed; row b of z_out = subcircuit sub_index[b]): columns body_col0 .. <- wires 1 ..
        of the subcircuit's witness.  tables, witness: as r1cs_job_trace takes them; z_out: DeviceBuffer (or raw device
        address) of len(sub_index) x n_v Fr.  Every other column keeps its bytes (stage1_witness writes those)."""
        d, keep = self._r1cs_job_desc(tables, witness)
        sub_index = np.ascontiguousarray(sub_index, dtype=np.uint32)
        check(self.lib.hk_r1cs_job_witness(self.handle, C.byref(d), _nullable(sub_index), sub_index.size, int(n_v),
                                           int(body_col0), _device_addr(z_out)), "hk_r1cs_job_witness")
        return z_out

    def _vkd_desc(self, tables, params, values=None):
        """(hk_vkd_desc, what must stay alive beside it) from `VkdJob.tables()`, the Poseidon constants
        (`poseidon.device_params`, the bytes or a DeviceBuffer first) and, for vkd_witness, the value table."""
        consts, n_consts, ld, nd = params
        arr = {k: np.ascontiguousarray(tables[k], dtype=np.uint32) for k in ("kinds", "slot_addr", "slot_src")}
        keep = [_hd(x) for x in (tables["leaves"], tables["siblings"], consts, tables["roots"], values)]
        a, b = hk_poseidon_desc(*ld), hk_poseidon_desc(*nd)
        p = _nullable
        d = hk_vkd_desc(int(tables["depth"]), int(tables["split"]), int(tables["n_updates"]), p(arr["kinds"]), p(keep[0]),
                        p(keep[1]), p(keep[2]), int(n_consts), C.pointer(a), C.pointer(b), p(keep[3]), arr["slot_addr"].size,
                        p(arr["slot_addr"]), p(arr["slot_src"]), p(keep[4]))
        return d, (arr, keep, a, b)

    def vkd_trace(self, tables, params, device_out=False, out=None):
        """hk_vkd_trace: the value table and the flattened time-ordered ROM trace of a VKD job (vkd_constraints.rs:70-193
        `get_portal_subtraces`), every hash computed on the device.  tables: `VkdJob.tables()` (leaves / siblings may be
        DeviceBuffers); params: `poseidon.device_params` with the constants as bytes or a DeviceBuffer.  Returns (values
        [3 + U (2 + 3 split) Fr], time_entries [n_slots x 2 Fr: what trace_sort(2, ...) / exec_tree / stage0_witness take]) as
        Montgomery bytes, or as DeviceBuffers when device_out is set; out: a pair of buffers of those sizes to fill instead."""
        d, keep = self._vkd_desc(tables, params)
        fr = self.fr_bytes
        sizes = [(3 + int(tables["n_updates"]) * (2 + 3 * int(tables["split"]))) * fr, 2 * int(d.n_slots) * fr]
        own = out is None
        if own:
            out = tuple(self._outputs(sizes, device_out))
        with _owned(out, own):
            check(self.lib.hk_vkd_trace(self.handle, C.byref(d), ptr(out[0]), ptr(out[1])), "hk_vkd_trace")
        return out

    def vkd_witness(self, tables, params, values, sub_index, n_v, cols, z_out):
        """hk_vkd_witness: column 0 and the body columns of the assignments of the subcircuits `sub_index` of ONE class (any order, repeats
        allowed; row b of z_out = subcircuit sub_index[b]).  tables, params: as vkd_trace takes them; values: vkd_trace's
        value table (bytes or a DeviceBuffer); cols: (kind, hash_col0, index_col0, path_col0) - `VkdSubcircuit.device_cols`;
        z_out: DeviceBuffer (or raw device address) of len(sub_index) x n_v Fr.  Every other column keeps its bytes
        (stage1_witness writes those)."""
        d, keep = self._vkd_desc(tables, params, values)
        sub_index = np.ascontiguousarray(sub_index, dtype=np.uint32)
        c = cols if isinstance(cols, hk_vkd_cols) else hk_vkd_cols(*[int(x) for x in cols])
        check(self.lib.hk_vkd_witness(self.handle, C.byref(d), _nullable(sub_index), sub_index.size, int(n_v), C.byref(c),
                                      None if z_out is None else _device_addr(z_out)), "hk_vkd_witness")
        return z_out

    def vkd_tree(self, depth, leaves0, kinds, leaves, params, device_out=False, out=None):
        """hk_vkd_tree: a batch of updates applied to a directory - the sibling paths `VkdJob.tables()["siblings"]` holds and
        the roots before and after the batch, every hash on the device (`vkd_circuit.directory_paths` is the host mirror).
        leaves0: the directory's leaves, M x 66 bytes (bytes, an array, a DeviceBuffer, or None / empty for M = 0); kinds:
        U words, 0 append / 1 update; leaves: U x 2 x 66 bytes as `tables()["leaves"]` (bytes, an array or a DeviceBuffer);
        params: what vkd_trace takes.  Returns (siblings [U x depth Fr], roots [2 Fr], status [U bytes, HK_VKD_ST_*]) as uint8
        arrays, or as DeviceBuffers when device_out is set; out: a triple of buffers of those sizes to fill instead, the third
        one None for no status."""
        consts, n_consts, ld, nd = params
        kinds = np.ascontiguousarray(kinds, dtype=np.uint32).reshape(-1)
        if isinstance(leaves0, (bytes, bytearray)):
            leaves0 = np.frombuffer(bytes(leaves0), np.uint8)
        if isinstance(leaves, (bytes, bytearray)):
            leaves = np.frombuffer(bytes(leaves), np.uint8)
        keep = [_hd(leaves0), _hd(leaves), _hd(consts)]
        m = _size(keep[0]) // 66
        u, fr = kinds.size, self.fr_bytes
        a, b = hk_poseidon_desc(*ld), hk_poseidon_desc(*nd)
        d = hk_vkd_tree_desc(int(depth), m, _nullable(keep[0]) if m else None, u, _nullable(kinds), _nullable(keep[1]),
                             _nullable(keep[2]), int(n_consts), C.pointer(a), C.pointer(b))
        own = out is None
        if own:
            out = self._outputs([u * int(depth) * fr, 2 * fr, u], device_out)
        with _owned(out, own):
            check(self.lib.hk_vkd_tree(self.handle, C.byref(d), ptr(out[0]), ptr(out[1]), ptr(out[2])), "hk_vkd_tree")
        return tuple(out)

    def _r1cs_call(self, fn, head, z, n_v, batch, cap, want_vals):
        """The shared tail of Context.r1cs_check / DevicePk.r1cs_check: `fn(*head, z, n_v, batch, verdicts, rows, vals, cap)`."""
        fr, batch, cap = self.fr_bytes, int(batch), int(cap)
        zz = _hd(z)
        if n_v is None:
            n_v = _size(zz) // (fr * max(batch, 1))
        verdicts = np.zeros((batch, 2), dtype=np.uint32)               # hk_r1cs_verdict: n_bad, first_bad
        rows = np.zeros((batch, cap), dtype=np.uint32) if cap else None
        vals = np.zeros((batch, cap, 3 * fr), dtype=np.uint8) if cap and want_vals else None
        check(fn(*head, ptr(zz) if batch else None, int(n_v), batch, verdicts.ctypes.data if batch else None, ptr(rows),
                 ptr(vals), cap), fn.__name__)
        res = [(int(n), None if n == 0 else int(f)) for n, f in verdicts]
        if not cap:
            return res
        return (res, rows, vals) if want_vals else (res, rows)

    def r1cs_check(self, A, B, C_, z, n_v=None, batch=1, cap=0, want_vals=False):
        """hk_r1cs_check: ark's cs.is_satisfied() / which_is_unsatisfied() for `batch` assignments of one class.  A / B / C_:
        (row_ptr, col, val) triples as witness_map takes them (members may be DeviceBuffers); z: Montgomery bytes or a
        DeviceBuffer of batch x n_v Fr (n_v defaults to the buffer's size / batch).  Returns [(n_bad, first_bad)] per
        assignment, first_bad None when it is satisfied; with cap also bad_rows, uint32 (batch, cap): the first failing rows in
        ascending order, 0xFFFFFFFF beyond; with want_vals also uint8 (batch, cap, 3 Fr): (a, b, c) of those rows, Montgomery."""
        keep = []
        csrs = self._csrs((A, B, C_), keep)
        return self._r1cs_call(self.lib.hk_r1cs_check, (self.handle, C.byref(csrs[0]), C.byref(csrs[1]), C.byref(csrs[2])), z, n_v,
                               batch, cap, want_vals)

    def points_check(self, group, pts, n=None):
        """hk_points_check_g1 / _g2: ark's AffineRepr::check of each point (on its curve, in the prime-order subgroup;
        infinity passes).  pts: packed affine bytes (uint8 array or DeviceBuffer).  Returns np.uint8[n] of 0 / 1."""
        pb, fn = self._group(group, "hk_points_check")
        n = n if n is not None else _size(pts) // pb
        ok = np.zeros(n, dtype=np.uint8)
        check(fn(self.handle, ptr(pts) if n else None, n, ok.ctypes.data), fn.__name__)
        return ok

    def gt_check(self, gts, n=None):
        """hk_gt_check: is each Fq12 value an element of GT - not zero, of order dividing r?  What a verifier asks of values
        it read from untrusted bytes before it treats them as pairing outputs (gt_pow's in_gt=True is a power only there).
        gts: n x gt_bytes Montgomery bytes (uint8 array or DeviceBuffer).  Returns np.uint8[n] of 0 / 1."""
        gts = _hd(gts)
        n = n if n is not None else _size(gts) // self.gt_bytes
        ok = np.zeros(n, dtype=np.uint8)
        check(self.lib.hk_gt_check(self.handle, ptr(gts) if n else None, n, ok.ctypes.data), "hk_gt_check")
        return ok

    def field_sqrt(self, which, data):
        """hk_field_sqrt: square roots of packed Montgomery Fq (`which` = 1) or Fq2 (2) elements.  Returns (roots, ok):
        the root that is not larger than its negative (ark's order), zeros where there is none; ok np.uint8[n] of 1 / 0."""
        eb = self.fq_bytes * int(which)
        data = _hd(data)
        n = _size(data) // eb
        out, ok = np.zeros(n * eb, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        check(self.lib.hk_field_sqrt(self.handle, int(which), ptr(data) if n else None, n, out.ctypes.data, ok.ctypes.data),
              "hk_field_sqrt")
        return out, ok

    def points_decompress(self, group, x_canon, flags, check=False, out=None):
        """hk_points_decompress_g1 / _g2: ark-ec's `get_point_from_x_unchecked` under `deserialize_compressed`.  x_canon:
        n canonical little-endian x (G2: c0 || c1); flags: n bytes, bit 0 infinity, bit 1 "y is the larger root".  Returns
        (points, status): packed affine Montgomery points and np.uint8[n] of 1 ok | 0 no such point (zeros) | 2 - with
        `check` - outside the prime-order subgroup.  `out` may be a DeviceBuffer / DeviceView of n points: they stay in
        HBM (ready for hk_pk_upload) and `out` is returned as `points`."""
        pb, fn = self._group(group, "hk_points_decompress")
        x_canon, flags = _hd(x_canon), _hd(flags)
        n = _size(flags)
        pts = out if out is not None else np.zeros(n * pb, dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint8)
        _check(fn(self.handle, ptr(x_canon) if n else None, ptr(flags) if n else None, n, int(bool(check)),
                  ptr(pts) if n else None, status.ctypes.data), fn.__name__)
        return pts, status

    def points_compress(self, group, pts):
        """hk_points_compress_g1 / _g2: the x coordinate and `SWFlags::from_y_coordinate` of `serialize_compressed`.  pts:
        packed affine Montgomery points (uint8 array or DeviceBuffer).  Returns (x_canon, flags) as points_decompress takes
        them."""
        pb, fn = self._group(group, "hk_points_compress")
        pts = _hd(pts)
        n = _size(pts) // pb
        x, flags = np.zeros(n * pb // 2, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        check(fn(self.handle, ptr(pts) if n else None, n, x.ctypes.data, flags.ctypes.data), fn.__name__)
        return x, flags

    def vk_prepare(self, *, alpha_g, beta_h, gamma_h, deltas_h, gamma_abc_g):
        """hk_vk_prepare (prepare_verifying_key, verifier.rs:7-18).  deltas_h: the stage deltas then delta_last, packed G2
        bytes; gamma_abc_g: packed G1 bytes.  Returns a DeviceVk."""
        arrs = [_hd(x) for x in (alpha_g, beta_h, gamma_h, deltas_h, gamma_abc_g)]
        size = [_size(x) for x in arrs]
        if size[:3] != [self.g1_bytes, self.g2_bytes, self.g2_bytes] or size[3] % self.g2_bytes or size[4] % self.g1_bytes:
            raise HekatonError(HK_ERR_LEN, "hk_vk_prepare")
        d = hk_vk_desc(ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), ptr(arrs[3]), size[3] // self.g2_bytes, ptr(arrs[4]),
                       size[4] // self.g1_bytes)
        h = C.c_void_p()
        check(self.lib.hk_vk_prepare(self.handle, C.byref(d), C.byref(h)), "hk_vk_prepare")
        return DeviceVk(self, h, d.n_deltas, d.n_abc)

    def pk_upload(self, *, a_g, b_g, b_h, h_g, ck_stages, deltas_g, last_delta_h, alpha_g, beta_g, beta_h,
                  matrices=None, n_inst=0, n_constraints=0):
        """hk_pk_upload: all arguments packed-affine numpy uint8 arrays (or DeviceBuffers with explicit
        lengths via (buf, n) tuples).  matrices = (A, B, C) CSR triples as in witness_map."""
        g1, g2 = self.g1_bytes, self.g2_bytes
        big = [_hd(x) for x in (a_g, b_g, b_h, h_g)]
        cks = [_hd(c) for c in ck_stages]
        small = [_hd(x) for x in (deltas_g, last_delta_h, alpha_g, beta_g, beta_h)]
        ck_ptrs = (C.c_void_p * len(cks))(*[ptr(c) for c in cks])          # an empty stage by its address, as the rest here
        ck_lens = (C.c_size_t * len(cks))(*[_size(c) // g1 for c in cks])
        keep = []
        csrs = self._csrs(matrices, keep) if matrices is not None else [None] * 3
        d = hk_pk_desc(ptr(big[0]), _size(big[0]) // g1, ptr(big[1]), _size(big[1]) // g1, ptr(big[2]), _size(big[2]) // g2,
                       ptr(big[3]), _size(big[3]) // g1, ck_ptrs, ck_lens, len(cks), *[ptr(x) for x in small],
                       *[m and C.pointer(m) for m in csrs], n_inst, n_constraints)
        h = C.c_void_p()
        check(self.lib.hk_pk_upload(self.handle, C.byref(d), C.byref(h)), "hk_pk_upload")
        return DevicePk(self, h)


class WordProgram:
    """hk_wprog: witness generation on the device for one proving-key class."""

    def __init__(self, ctx, handle, n_v, n_inputs):
        self.ctx, self.handle, self.n_v, self.n_inputs = ctx, handle, n_v, n_inputs

    def run(self, inputs, full_cols, full_vals, out=None, batch=None):
        """inputs: uint32 (batch, n_inputs), or a DeviceBuffer of it with an explicit batch=; full_cols: uint32 (k);
        full_vals: Montgomery bytes (batch, k * fr_bytes).  Returns a DeviceBuffer holding batch x n_v Fr (or fills `out`)."""
        if isinstance(inputs, DeviceBuffer):                   # a buffer does not say how many rows of it are meant
            assert batch is not None and inputs.nbytes >= 4 * int(batch) * self.n_inputs, "a DeviceBuffer of inputs needs batch="
            batch = int(batch)
        else:
            inputs = _hd(inputs, np.uint32)
            batch = inputs.shape[0]
        cols, vals = _hd(full_cols, np.uint32), _hd(full_vals)
        n_full = _size(cols) // 4
        buf = out if out is not None else DeviceBuffer(self.ctx, batch * self.n_v * self.ctx.fr_bytes)
        check(self.ctx.lib.hk_wprog_run(self.ctx.handle, self.handle, ptr(inputs), batch, ptr(cols) if n_full else None,
                                        ptr(vals) if n_full else None, n_full, buf.ptr), "hk_wprog_run")
        return buf

    def scatter(self, full_cols, full_vals, out):
        """The full-width values alone (hk_assignment_scatter), into assignments `run(inputs, [], [], out=...)` produced."""
        cols, vals = _hd(full_cols, np.uint32), _hd(full_vals)
        n_full = _size(cols) // 4
        batch = _size(vals) // max(1, n_full * self.ctx.fr_bytes)
        check(self.ctx.lib.hk_assignment_scatter(self.ctx.handle, ptr(cols), ptr(vals), n_full, batch, self.n_v, out.ptr),
              "hk_assignment_scatter")
        return out

    def free(self):
        if self.handle:
            self.ctx.lib.hk_wprog_free(self.handle)
            self.handle = None


class ResidentBases:
    """hk_bases: a static base set (SRS powers, commitment keys) with its shift tables in HBM."""

    def __init__(self, ctx, handle, group, n):
        self.ctx, self.handle, self.group, self.n = ctx, handle, group, n

    def msm(self, scalars, n_scalars=None, montgomery=True, checked=True):
        """`G::Group::msm(&srs_powers, &coeffs)` (distributed-prover/src/kzg.rs:151-152) over the resident bases."""
        ns = n_scalars if n_scalars is not None else _size(scalars) // self.ctx.fr_bytes
        out = np.zeros(self.ctx._group(self.group)[0], dtype=np.uint8)
        check(self.ctx.lib.hk_msm_bases(self.ctx.handle, self.handle, ptr(scalars), ns, int(montgomery), int(checked),
                                        out.ctypes.data), "hk_msm_bases")
        return out

    def free(self):
        if self.handle:
            self.ctx.lib.hk_bases_free(self.handle)
            self.handle = None


class DeviceVk:
    """hk_vk wrapper: a prepared verifying key (PreparedVerifyingKey, verifier.rs:7-18) resident in HBM."""

    def __init__(self, ctx, handle, n_deltas, n_abc):
        self.ctx = ctx
        self.handle = handle
        self.n_deltas, self.n_abc = n_deltas, n_abc

    def free(self):
        if self.handle:
            self.ctx.lib.hk_vk_free(self.handle)
            self.handle = None

    def alpha_beta(self):
        """e(alpha, beta) in the GT layout of Context.multi_pairing."""
        out = np.zeros(self.ctx.gt_bytes, dtype=np.uint8)
        check(self.ctx.lib.hk_vk_alpha_beta(self.handle, out.ctypes.data), "hk_vk_alpha_beta")
        return out

    def check_args(self, n, a, b, c, ds, inputs, rand=None):
        """The length checks of verify(), before any device call: HekatonError(HK_ERR_LEN) for a length that does not
        match n proofs of this key (verifier.rs:53-55 MalformedVerifyingKey for the inputs), ValueError for a zero r."""
        ctx = self.ctx
        nd, nk = self.n_deltas - 1, self.n_abc - 1
        for arr, per in ((a, ctx.g1_bytes), (b, ctx.g2_bytes), (c, ctx.g1_bytes), (ds, nd * ctx.g1_bytes),
                         (inputs, nk * ctx.fr_bytes)):
            if _size(arr) != n * per:
                raise HekatonError(HK_ERR_LEN, "hk_verify_batch")
        if rand is not None:
            rr = np.ascontiguousarray(rand, dtype=np.uint8).reshape(-1)
            if len(rr) != n * ctx.fr_bytes:
                raise HekatonError(HK_ERR_LEN, "hk_verify_batch")
            if (rr.reshape(n, ctx.fr_bytes) == 0).all(axis=1).any():
                raise ValueError("batch verification needs nonzero r_i")

    def verify(self, a, b, c, ds, inputs, n=None, check_points=True, rand=None, verdicts=None):
        """hk_verify_batch: one verdict per proof (VERDICT_ACCEPT / _REJECT / _BAD_POINT).  a, c: n G1; b: n G2;
        ds: n x (n_deltas - 1) G1; inputs: n x (n_abc - 1) Fr Montgomery; all packed bytes, row after row (uint8 arrays
        or DeviceBuffers).  rand: None (per-proof mode) or n nonzero Fr Montgomery (batch mode; needs check_points).
        verdicts: optional DeviceBuffer of n bytes to write to instead of a new host array."""
        ctx = self.ctx
        if n is None:
            n = _size(a) // ctx.g1_bytes
        ds = ds if ds is not None else np.zeros(0, dtype=np.uint8)
        inputs = inputs if inputs is not None else np.zeros(0, dtype=np.uint8)
        self.check_args(n, a, b, c, ds, inputs, rand)
        ops = [_hd(x) for x in (a, b, c, ds, inputs)]
        rr = _hd(rand)
        out = verdicts if verdicts is not None else np.zeros(n, dtype=np.uint8)
        flags = HK_VERIFY_CHECK_POINTS if check_points else 0
        check(ctx.lib.hk_verify_batch(ctx.handle, self.handle, *[_nullable(x) if n else None for x in ops], n, flags, ptr(rr),
                                      ptr(out)), "hk_verify_batch")
        return out


class DevicePk:
    """hk_pk wrapper: a proving-key class resident in HBM (with its shift tables and matrices)."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.handle = handle

    def free(self):
        if self.handle:
            self.ctx.lib.hk_pk_free(self.handle)
            self.handle = None

    def r1cs_check(self, z, n_v=None, batch=1, cap=0, want_vals=False):
        """hk_pk_r1cs_check: Context.r1cs_check against the matrices this key was uploaded with (nothing goes up again)."""
        ctx = self.ctx
        return ctx._r1cs_call(ctx.lib.hk_pk_r1cs_check, (ctx.handle, self.handle), z, n_v, batch, cap, want_vals)

    def commit(self, stage, w_stage, kappa, n=None):
        """committer.rs:87-91 — msm(ck[stage], w) + kappa * last_delta_g; returns packed G1 bytes."""
        ctx = self.ctx
        n = n if n is not None else _size(w_stage) // ctx.fr_bytes
        kappa = _hd(kappa)
        out = np.zeros(ctx.g1_bytes, dtype=np.uint8)
        check(ctx.lib.hk_commit(ctx.handle, self.handle, stage, ptr(w_stage) if n else None, n, ptr(kappa), out.ctypes.data),
              "hk_commit")
        return out

    def commit_batch(self, stage, w_rows, kappas, n, batch):
        """hk_commit_batch: the stage commitments of `batch` subcircuits of this key's class in one call.  w_rows: their
        stage witnesses row after row (batch x n Fr Montgomery; uint8 array or DeviceBuffer); kappas: batch Fr Montgomery
        (uint8 array).  Returns (batch, g1_bytes) uint8."""
        ctx = self.ctx
        kap = _hd(kappas)
        out = np.zeros((batch, ctx.g1_bytes), dtype=np.uint8)
        check(ctx.lib.hk_commit_batch(ctx.handle, self.handle, stage, ptr(w_rows) if n else None, n, ptr(kap), batch,
                                      out.ctypes.data), "hk_commit_batch")
        return out

    def prove(self, z, r, s, kappas, n_v=None):
        """prover.rs:78-155 + committer.rs:112-114; returns (a, b, c) packed affine bytes."""
        ctx = self.ctx
        n_v = n_v if n_v is not None else _size(z) // ctx.fr_bytes
        r, s, kap = _hd(r), _hd(s), _hd(kappas)
        nk = _size(kap) // ctx.fr_bytes
        a = np.zeros(ctx.g1_bytes, dtype=np.uint8)
        b = np.zeros(ctx.g2_bytes, dtype=np.uint8)
        c = np.zeros(ctx.g1_bytes, dtype=np.uint8)
        check(ctx.lib.hk_prove(ctx.handle, self.handle, ptr(z), n_v, ptr(r), ptr(s), ptr(kap) if nk else None, nk,
                               a.ctypes.data, b.ctypes.data, c.ctypes.data), "hk_prove")
        return a, b, c

    def prove_batch(self, z_rows, rs, ss, kappas, n_v, batch):
        """hk_prove_batch: `batch` proofs of this key's class in one lock-step call.  z_rows: their assignments row after
        row (batch x n_v Fr Montgomery; uint8 array or DeviceBuffer); rs, ss: batch Fr each; kappas: batch x n_kappas Fr
        (uint8 arrays, Montgomery).  Returns (a, b, c) as (batch, g1 | g2 | g1 bytes) uint8 arrays; row b equals
        prove() on row b."""
        ctx = self.ctx
        r, s, kap = _hd(rs), _hd(ss), _hd(kappas)
        nk = _size(kap) // (ctx.fr_bytes * batch) if batch else 0
        a = np.zeros((batch, ctx.g1_bytes), dtype=np.uint8)
        b = np.zeros((batch, ctx.g2_bytes), dtype=np.uint8)
        c = np.zeros((batch, ctx.g1_bytes), dtype=np.uint8)
        check(ctx.lib.hk_prove_batch(ctx.handle, self.handle, ptr(z_rows), n_v, ptr(r), ptr(s), ptr(kap) if nk else None, nk,
                                     batch, a.ctypes.data, b.ctypes.data, c.ctypes.data), "hk_prove_batch")
        return a, b, c
