"""ctypes binding of include/hekaton.h (libhekaton.so) — the only door into the HIP kernels.

There is no CPU path: importing works anywhere (so host logic can be tested), but creating a
`Context` without a gfx950 device raises, and a missing libhekaton.so raises at load time.
"""
import contextlib
import ctypes as C
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


# every symbol include/hekaton.h declares (tests check the library exports all of them)
EXPORTS = ["hk_status_str", "hk_version", "hk_ctx_create", "hk_ctx_destroy", "hk_ctx_sync",
           "hk_ctx_set_profiling", "hk_ctx_last_timings", "hk_ctx_sizes", "hk_dev_alloc", "hk_dev_free",
           "hk_dev_upload", "hk_dev_download", "hk_msm_g1", "hk_msm_g2", "hk_ntt", "hk_witness_map",
           "hk_pk_upload", "hk_pk_free", "hk_commit", "hk_prove", "hk_fixed_base_g1", "hk_fixed_base_g2", "hk_scalar_pairing_g1", "hk_scalar_pairing_g2", "hk_field_convert", "hk_bases_upload", "hk_bases_free",
           "hk_msm_bases", "hk_multi_pairing", "hk_pairing_products", "hk_ctx_gt_bytes",
           "hk_points_lincomb_g1", "hk_points_lincomb_g2", "hk_points_fold_g2", "hk_points_fold_g1", "hk_points_fold_many_g1", "hk_points_fold_many_g2", "hk_pairing_pairs", "hk_keccak_f1600", "hk_assignment_from_bits", "hk_wprog_upload", "hk_wprog_free", "hk_wprog_run", "hk_gt_pow", "hk_fq12_pow", "hk_gt_pow_prod", "hk_poseidon_path", "hk_assignment_scatter", "hk_commit_batch",
           "hk_prove_batch", "hk_vk_prepare", "hk_vk_free", "hk_vk_alpha_beta", "hk_verify_batch", "hk_points_check_g1",
           "hk_points_check_g2", "hk_qap_eval", "hk_keygen", "hk_exec_tree", "hk_stage1_witness",
           "hk_trace_sort", "hk_stage0_witness", "hk_r1cs_check", "hk_pk_r1cs_check",
           "hk_sha_tree", "hk_sha_tree_inputs", "hk_ram_stage0_witness", "hk_ram_stage1_witness",
           "hk_r1cs_job_trace", "hk_r1cs_job_witness", "hk_vkd_trace", "hk_vkd_witness", "hk_vkd_tree",
           "hk_scalar_powers", "hk_ipa_quotient", "hk_class_power_sums", "hk_field_sqrt", "hk_points_decompress_g1", "hk_points_decompress_g2",
           "hk_points_compress_g1", "hk_points_compress_g2"]

HK_VERIFY_CHECK_POINTS = 1
VERDICT_REJECT, VERDICT_ACCEPT, VERDICT_BAD_POINT = 0, 1, 2

_lib = None


def load():
    """Loads libhekaton.so (built by __graft_entry__.build()); fails loudly when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libhekaton.so not built (%s): run `python -c 'import __graft_entry__ as g; "
                          "g.build()'` — there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    lib.hk_status_str.restype = C.c_char_p
    lib.hk_status_str.argtypes = [i]
    lib.hk_version.restype = C.c_char_p
    lib.hk_ctx_create.argtypes = [i, i, C.POINTER(vp)]
    lib.hk_ctx_destroy.argtypes = [vp]
    lib.hk_ctx_destroy.restype = None
    lib.hk_ctx_sync.argtypes = [vp]
    lib.hk_ctx_set_profiling.argtypes = [vp, i]
    lib.hk_ctx_last_timings.argtypes = [vp, C.POINTER(hk_timings)]
    lib.hk_ctx_sizes.argtypes = [vp] + [C.POINTER(sz)] * 4
    lib.hk_dev_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    lib.hk_dev_free.argtypes = [vp, vp]
    lib.hk_dev_upload.argtypes = [vp, vp, vp, sz]
    lib.hk_dev_download.argtypes = [vp, vp, vp, sz]
    for f in (lib.hk_msm_g1, lib.hk_msm_g2):
        f.argtypes = [vp, vp, sz, vp, sz, i, i, vp]
    lib.hk_ntt.argtypes = [vp, vp, C.c_uint, i, i]
    for f in (lib.hk_fixed_base_g1, lib.hk_fixed_base_g2):
        f.argtypes = [vp, vp, vp, sz, i, vp]
    for f in (lib.hk_scalar_pairing_g1, lib.hk_scalar_pairing_g2):
        f.argtypes = [vp, vp, vp, sz, vp]
    lib.hk_field_convert.argtypes = [vp, i, vp, vp, sz, i]
    lib.hk_bases_upload.argtypes = [vp, i, vp, sz, C.POINTER(vp)]
    lib.hk_bases_free.argtypes = [vp]
    lib.hk_bases_free.restype = None
    lib.hk_msm_bases.argtypes = [vp, vp, vp, sz, i, i, vp]
    if hasattr(lib, "hk_multi_pairing"):          # absent only from older experiment builds loaded through HK_LIB
        lib.hk_multi_pairing.argtypes = [vp, vp, vp, sz, vp]
        lib.hk_pairing_products.argtypes = [vp, C.POINTER(vp), sz, C.POINTER(vp), sz, sz, vp]
        lib.hk_pairing_pairs.argtypes = [vp, C.POINTER(vp), sz, C.POINTER(vp), sz, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), sz, sz, vp]
        lib.hk_ctx_gt_bytes.argtypes = [vp, C.POINTER(sz)]
        for f in (lib.hk_points_lincomb_g1, lib.hk_points_lincomb_g2):
            f.argtypes = [vp, C.POINTER(vp), vp, sz, sz, vp]
    if hasattr(lib, "hk_points_fold_g2"):
        lib.hk_points_fold_g2.argtypes = [vp, vp, vp, vp, C.c_uint, sz, vp]
    if hasattr(lib, "hk_points_fold_g1"):
        lib.hk_points_fold_g1.argtypes = [vp, vp, vp, vp, C.c_uint, sz, vp]
    for name in ("hk_points_fold_many_g1", "hk_points_fold_many_g2"):
        getattr(lib, name).argtypes = [vp, sz, C.POINTER(vp), C.POINTER(vp), vp, C.c_uint, sz, C.POINTER(vp)]
    if hasattr(lib, "hk_assignment_from_bits"):
        lib.hk_assignment_from_bits.argtypes = [vp, vp, sz, vp, vp, sz, vp]
        lib.hk_wprog_upload.argtypes = [vp, vp, sz, vp, sz, vp, sz, sz, sz, C.POINTER(vp)]
        lib.hk_wprog_free.argtypes = [vp]
        lib.hk_wprog_free.restype = None
        lib.hk_wprog_run.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp]
        lib.hk_assignment_scatter.argtypes = [vp, vp, vp, sz, sz, sz, vp]
    if hasattr(lib, "hk_gt_pow"):
        lib.hk_gt_pow.argtypes = [vp, vp, vp, sz, vp]
        lib.hk_fq12_pow.argtypes = [vp, vp, vp, sz, vp]
        lib.hk_gt_pow_prod.argtypes = [vp, vp, vp, sz, sz, C.c_int, vp]
    lib.hk_poseidon_path.argtypes = [vp, vp, sz, C.POINTER(hk_poseidon_desc), C.POINTER(hk_poseidon_desc), vp, vp, vp, sz, sz,
                                     sz, sz, vp]
    lib.hk_witness_map.argtypes = [vp, C.POINTER(hk_csr), C.POINTER(hk_csr), C.POINTER(hk_csr), sz, sz,
                                   vp, sz, vp, sz, C.POINTER(sz)]
    lib.hk_pk_upload.argtypes = [vp, C.POINTER(hk_pk_desc), C.POINTER(vp)]
    lib.hk_pk_free.argtypes = [vp]
    lib.hk_pk_free.restype = None
    lib.hk_commit.argtypes = [vp, vp, sz, vp, sz, vp, vp]
    lib.hk_commit_batch.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp]
    lib.hk_prove.argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp]
    lib.hk_prove_batch.argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, sz, vp, vp, vp]
    lib.hk_vk_prepare.argtypes = [vp, C.POINTER(hk_vk_desc), C.POINTER(vp)]
    lib.hk_vk_free.argtypes = [vp]
    lib.hk_vk_free.restype = None
    lib.hk_vk_alpha_beta.argtypes = [vp, vp]
    lib.hk_verify_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, C.c_uint, vp, vp]
    lib.hk_points_check_g1.argtypes = [vp, vp, sz, vp]
    lib.hk_points_check_g2.argtypes = [vp, vp, sz, vp]
    lib.hk_qap_eval.argtypes = [vp, C.POINTER(hk_csr), C.POINTER(hk_csr), C.POINTER(hk_csr), sz, sz, sz, vp, vp, vp, vp, vp,
                                C.POINTER(sz)]
    lib.hk_keygen.argtypes = [vp, C.POINTER(hk_keygen_desc), C.POINTER(hk_keygen_out), C.POINTER(sz)]
    lib.hk_exec_tree.argtypes = [vp, C.POINTER(hk_exec_tree_desc), C.POINTER(hk_exec_tree_out)]
    lib.hk_stage1_witness.argtypes = [vp, C.POINTER(hk_stage1_desc), vp, sz, sz, vp]
    lib.hk_trace_sort.argtypes = [vp, C.c_uint32, vp, sz, vp, vp]
    lib.hk_stage0_witness.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, sz, vp]
    lib.hk_r1cs_check.argtypes = [vp, C.POINTER(hk_csr), C.POINTER(hk_csr), C.POINTER(hk_csr), vp, sz, sz, vp, vp, vp, sz]
    lib.hk_pk_r1cs_check.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, sz]
    lib.hk_sha_tree.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(hk_sha_tree_out)]
    lib.hk_sha_tree_inputs.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, vp, sz, vp]
    lib.hk_ram_stage0_witness.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, sz, vp]
    lib.hk_ram_stage1_witness.argtypes = [vp, C.POINTER(hk_ram_stage1_desc), vp, sz, sz, vp]
    lib.hk_r1cs_job_trace.argtypes = [vp, C.POINTER(hk_r1cs_job_desc), vp]
    lib.hk_r1cs_job_witness.argtypes = [vp, C.POINTER(hk_r1cs_job_desc), vp, sz, sz, sz, vp]
    lib.hk_vkd_trace.argtypes = [vp, C.POINTER(hk_vkd_desc), vp, vp]
    lib.hk_vkd_witness.argtypes = [vp, C.POINTER(hk_vkd_desc), vp, sz, sz, C.POINTER(hk_vkd_cols), vp]
    lib.hk_vkd_tree.argtypes = [vp, C.POINTER(hk_vkd_tree_desc), vp, vp, vp]
    lib.hk_scalar_powers.argtypes = [vp, vp, sz, sz, vp]
    lib.hk_ipa_quotient.argtypes = [vp, vp, sz, vp, vp, sz, vp]
    lib.hk_class_power_sums.argtypes = [vp, vp, vp, sz, sz, vp]
    if hasattr(lib, "hk_field_sqrt"):             # absent only from older experiment builds loaded through HK_LIB
        lib.hk_field_sqrt.argtypes = [vp, i, vp, sz, vp, vp]
        for f in (lib.hk_points_decompress_g1, lib.hk_points_decompress_g2):
            f.argtypes = [vp, vp, vp, sz, i, vp, vp]
        for f in (lib.hk_points_compress_g1, lib.hk_points_compress_g2):
            f.argtypes = [vp, vp, sz, vp, vp]
    _lib = lib
    return lib


def status_str(s):
    return load().hk_status_str(int(s)).decode()


def check(status, what):
    if status != HK_OK:
        raise HekatonError(status, what)


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
        buf = cls(ctx, arr.nbytes)
        check(load().hk_dev_upload(ctx.handle, buf.ptr, arr.ctypes.data, arr.nbytes), "hk_dev_upload")
        return buf

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


def _ptr_array(xs):
    """The addresses of numpy arrays and DeviceBuffers as a c_void_p array, each as _nullable gives it; never of length 0."""
    return (C.c_void_p * max(len(xs), 1))(*[_nullable(x) for x in xs])


def _device_addr(z):
    """A device output: a DeviceBuffer or its raw address."""
    return z.ptr if isinstance(z, DeviceBuffer) else int(z)


def _challenge_bytes(curve, challenges):
    """Challenges given as ints or as their Montgomery bytes."""
    if isinstance(challenges, np.ndarray):
        return np.ascontiguousarray(challenges, dtype=np.uint8)
    from .cp_groth16 import FrCodec
    return FrCodec(curve).enc(list(challenges))


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
        gt = C.c_size_t(12 * fq.value)
        if hasattr(self.lib, "hk_ctx_gt_bytes"):
            check(self.lib.hk_ctx_gt_bytes(h, C.byref(gt)), "hk_ctx_gt_bytes")
        self.gt_bytes = gt.value

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
    def _msm(self, fn, nbytes, bases, n_bases, scalars, n_scalars, mont, checked):
        out = np.zeros(nbytes, dtype=np.uint8)
        check(fn(self.handle, ptr(bases), n_bases, ptr(scalars), n_scalars, int(mont), int(checked),
                 out.ctypes.data), fn.__name__)
        return out

    def msm_g1(self, bases, scalars, n_bases=None, n_scalars=None, montgomery=True, checked=True):
        """E::G1::msm / msm_bigint / msm_unchecked (prover.rs:88,97,117,129; committer.rs:89,113)."""
        nb = n_bases if n_bases is not None else len(bases) // self.g1_bytes
        ns = n_scalars if n_scalars is not None else len(scalars) // self.fr_bytes
        return self._msm(self.lib.hk_msm_g1, self.g1_bytes, bases, nb, scalars, ns, montgomery, checked)

    def msm_g2(self, bases, scalars, n_bases=None, n_scalars=None, montgomery=True, checked=True):
        """E::G2 MSM (prover.rs:107)."""
        nb = n_bases if n_bases is not None else len(bases) // self.g2_bytes
        ns = n_scalars if n_scalars is not None else len(scalars) // self.fr_bytes
        return self._msm(self.lib.hk_msm_g2, self.g2_bytes, bases, nb, scalars, ns, montgomery, checked)

    def fixed_base(self, group, base, scalars, n=None, montgomery=True, out=None):
        """FixedBase::msm + normalize_batch (generator.rs:134-224): out[i] = scalars[i] * base.
        `out` may be a DeviceBuffer (stays in HBM); otherwise a numpy array is returned."""
        pb = self.g1_bytes if group == 1 else self.g2_bytes
        n = n if n is not None else len(scalars) // self.fr_bytes
        fn = self.lib.hk_fixed_base_g1 if group == 1 else self.lib.hk_fixed_base_g2
        base = _hd(base)
        res = out if out is not None else np.zeros(n * pb, dtype=np.uint8)
        check(fn(self.handle, ptr(base), ptr(scalars), n, int(montgomery), ptr(res)), fn.__name__)
        return res

    def scalar_pairing(self, group, points, scalars, n=None, out=None):
        """`scalar_pairing` (distributed-prover/src/pairing_ops.rs:32-39): out[i] = scalars[i] * points[i].  `out` may be a
        DeviceBuffer (the result stays in HBM)."""
        pb = self.g1_bytes if group == 1 else self.g2_bytes
        n = n if n is not None else len(scalars) // self.fr_bytes
        fn = self.lib.hk_scalar_pairing_g1 if group == 1 else self.lib.hk_scalar_pairing_g2
        res = out if out is not None else np.zeros(n * pb, dtype=np.uint8)
        check(fn(self.handle, ptr(points), ptr(scalars), n, ptr(res)), fn.__name__)
        return res

    def scalar_powers(self, x, n, reps=1, out=None):
        """hk_scalar_powers: `structured_scalar_power` (distributed-prover/src/pairing_ops.rs:42-48) - the Montgomery bytes of
        x^0 .. x^(n - 1) (x an int), `reps` times back to back.  `out` may be a DeviceBuffer / DeviceView of reps * n Fr (the
        result stays in HBM); otherwise a numpy array is returned."""
        from .cp_groth16 import FrCodec
        xb = FrCodec(self.curve).enc1(x)
        res = out if out is not None else np.zeros(reps * n * self.fr_bytes, dtype=np.uint8)
        check(self.lib.hk_scalar_powers(self.handle, xb.ctypes.data, int(n), int(reps), ptr(res)), "hk_scalar_powers")
        return res

    def ipa_quotient(self, challenges, rho, z, shift=0, out=None):
        """hk_ipa_quotient: the Montgomery bytes of the quotient of X^shift prod_k (1 + challenges[k] (rho X)^(2^k)) by
        (X - z), one zero appended: shift + 2^len(challenges) Fr (kzg.rs:122-141).  challenges, rho, z: ints.  `out` may be
        a DeviceBuffer / DeviceView of that size (the result stays in HBM); otherwise a numpy array is returned."""
        from .cp_groth16 import FrCodec
        fc = FrCodec(self.curve)
        challenges = list(challenges)
        l = len(challenges)
        ch, rb, zb = fc.enc(challenges), fc.enc1(rho), fc.enc1(z)
        res = out if out is not None else np.zeros((shift + (1 << l)) * self.fr_bytes, dtype=np.uint8)
        check(self.lib.hk_ipa_quotient(self.handle, ch.ctypes.data if l else None, l, rb.ctypes.data, zb.ctypes.data, int(shift),
                                       ptr(res)), "hk_ipa_quotient")
        return res

    def class_power_sums(self, x, class_of, n_classes, out=None):
        """hk_class_power_sums: the Montgomery bytes of sums[c] = sum of x^i over the i with class_of[i] == c, c < n_classes
        (x an int) - the exponents of an aggregate verifier's prod_c e(alpha_c, beta_c)^(sums[c]).  class_of: a uint32 array or
        a DeviceBuffer of n uint32.  `out` may be a DeviceBuffer / DeviceView of n_classes Fr (the result stays in HBM);
        otherwise a numpy array is returned.  A class id >= n_classes is refused (HK_ERR_ARG)."""
        from .cp_groth16 import FrCodec
        xb = FrCodec(self.curve).enc1(x)
        class_of = _hd(class_of, np.uint32)
        n = class_of.nbytes // 4
        if n == 0 and not isinstance(class_of, DeviceBuffer):
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
        out = np.zeros((gts.nbytes // self.gt_bytes, self.gt_bytes), dtype=np.uint8)
        fn = self.lib.hk_gt_pow if in_gt else self.lib.hk_fq12_pow
        check(fn(self.handle, ptr(gts), ptr(scalars), out.shape[0], out.ctypes.data), fn.__name__)
        return out

    def gt_pow_prod(self, gts, scalars, group_len, in_gt=True):
        """hk_gt_pow_prod: out[g] = prod_j gts[g * group_len + j]^scalars[g * group_len + j] (a verifier's
        multi-exponentiations).  Returns (n / group_len, gt_bytes) uint8."""
        gts, scalars = _hd(gts), _hd(scalars)
        n = gts.nbytes // self.gt_bytes
        out = np.zeros((n // max(1, group_len), self.gt_bytes), dtype=np.uint8)
        check(self.lib.hk_gt_pow_prod(self.handle, ptr(gts), ptr(scalars), n, group_len, 1 if in_gt else 0, out.ctypes.data),
              "hk_gt_pow_prod")
        return out

    def multi_pairing(self, g1, g2, n=None):
        """`pairing(left, right)` (distributed-prover/src/pairing_ops.rs:25-29): prod_i e(g1[i], g2[i]) as ark's Fp12
        bytes (12 Fq, Montgomery)."""
        n = n if n is not None else len(g1) // self.g1_bytes
        out = np.zeros(self.gt_bytes, dtype=np.uint8)
        check(self.lib.hk_multi_pairing(self.handle, ptr(g1) if n else None, ptr(g2) if n else None, n, out.ctypes.data),
              "hk_multi_pairing")
        return out

    def pairing_products(self, lhs, rhs, n=None):
        """Every G1 vector of `lhs` against every G2 vector of `rhs` in one batched launch (the `cross_terms` of
        aggregation.rs:255-263): returns a (len(lhs), len(rhs), gt_bytes) uint8 array."""
        n = n if n is not None else len(lhs[0]) // self.g1_bytes
        lhs, rhs = [_hd(x) for x in lhs], [_hd(x) for x in rhs]
        lp, rp = _ptr_array(lhs), _ptr_array(rhs)
        out = np.zeros((len(lhs), len(rhs), self.gt_bytes), dtype=np.uint8)
        check(self.lib.hk_pairing_products(self.handle, lp, len(lhs), rp, len(rhs), n, out.ctypes.data),
              "hk_pairing_products")
        return out

    def pairing_pairs(self, lhs, rhs, pairs, n=None):
        """pairing(lhs[a], rhs[b]) for each (a, b) of `pairs` in one batched launch (hk_pairing_pairs: the cross terms of a
        GIPA round): returns a (len(pairs), gt_bytes) uint8 array."""
        n = n if n is not None else len(lhs[0]) // self.g1_bytes
        lhs, rhs = [_hd(x) for x in lhs], [_hd(x) for x in rhs]
        lp, rp = _ptr_array(lhs), _ptr_array(rhs)
        pa = (C.c_uint32 * len(pairs))(*[a for a, _ in pairs])
        pb = (C.c_uint32 * len(pairs))(*[b for _, b in pairs])
        out = np.zeros((len(pairs), self.gt_bytes), dtype=np.uint8)
        check(self.lib.hk_pairing_pairs(self.handle, lp, len(lhs), rp, len(rhs), pa, pb, len(pairs), n, out.ctypes.data),
              "hk_pairing_pairs")
        return out

    def points_lincomb(self, group, vecs, coeffs, n=None):
        """out[i] = sum_j coeffs[j] * vecs[j][i] (aggregation.rs:192-203,293-326); coeffs: k Fr Montgomery bytes."""
        pb = self.g1_bytes if group == 1 else self.g2_bytes
        n = n if n is not None else len(vecs[0]) // pb
        vecs, coeffs = [_hd(x) for x in vecs], _hd(coeffs)
        out = np.zeros(n * pb, dtype=np.uint8)
        fn = self.lib.hk_points_lincomb_g1 if group == 1 else self.lib.hk_points_lincomb_g2
        check(fn(self.handle, _ptr_array(vecs), ptr(coeffs), len(vecs), n, out.ctypes.data), fn.__name__)
        return out

    def _fold_coeffs(self, group, c):
        """The scalar c (an int mod r) split along the group's endomorphism (endo.Phi2 in G1, endo.Psi4 in G2): the parts'
        magnitudes as Montgomery bytes and the mask of the negative ones."""
        from .cp_groth16 import FrCodec
        from .endo import phi2, psi4
        k = (phi2 if group == 1 else psi4)(self.curve).decompose(c)
        neg = sum(1 << j for j, v in enumerate(k) if v < 0)
        return np.ascontiguousarray(FrCodec(self.curve).enc([abs(v) for v in k]), dtype=np.uint8), neg

    def _points_fold(self, group, lo, hi, c, n, out):
        pb = self.g1_bytes if group == 1 else self.g2_bytes
        n = n if n is not None else len(hi) // pb
        coeffs, neg = self._fold_coeffs(group, c)
        lo, hi = _hd(lo), _hd(hi)
        res = out if out is not None else np.zeros(n * pb, dtype=np.uint8)                      # a DeviceBuffer stays in HBM
        fn = self.lib.hk_points_fold_g1 if group == 1 else self.lib.hk_points_fold_g2
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
        fn = self.lib.hk_points_fold_many_g1 if group == 1 else self.lib.hk_points_fold_many_g2
        check(fn(self.handle, len(outs), _ptr_array(los), _ptr_array(his), coeffs.ctypes.data, neg, n, _ptr_array(outs)),
              fn.__name__)
        return outs

    def assignment_from_bits(self, bits, full_cols, full_vals, out=None):
        """hk_assignment_from_bits: the Montgomery assignment of a bit-valued witness, materialised in HBM.  bits: uint8
        array (one per variable); full_cols: column indices of the full-width values; full_vals: their Montgomery bytes.
        Returns a DeviceBuffer of n_v Fr (or fills `out`)."""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        cols = np.ascontiguousarray(full_cols, dtype=np.uint32)
        vals = np.ascontiguousarray(full_vals, dtype=np.uint8)
        n_v = bits.size
        buf = out if out is not None else DeviceBuffer(self, n_v * self.fr_bytes)
        check(self.lib.hk_assignment_from_bits(self.handle, bits.ctypes.data, n_v, cols.ctypes.data if cols.size else None,
                                               vals.ctypes.data if cols.size else None, cols.size, buf.ptr),
              "hk_assignment_from_bits")
        return buf

    def poseidon_path(self, params, leaf, siblings, index, n_v, col0, z_out):
        """hk_poseidon_path: the membership block of `batch` assignments, written on the device.  params:
        (consts DeviceBuffer or Montgomery bytes, n_consts, (t, alpha, rf, rp, off) of the leaf hash, same of the node hash)
        - poseidon.device_params(curve); leaf: Montgomery bytes (batch, 4 Fr); siblings: (batch, depth Fr); index: uint32
        (batch); z_out: DeviceBuffer (or raw device address) of batch x n_v Fr.  leaf and siblings may also be the
        DeviceBuffers hk_exec_tree left on the device (both then; batch = len(index))."""
        consts, n_consts, ld, nd = params
        index = np.ascontiguousarray(index, dtype=np.uint32)
        if isinstance(leaf, DeviceBuffer):
            batch = index.size
            depth = siblings.nbytes // (batch * self.fr_bytes)
        else:
            leaf = np.ascontiguousarray(leaf, dtype=np.uint8)
            batch = leaf.shape[0]
            siblings = np.ascontiguousarray(siblings, dtype=np.uint8).reshape(batch, -1)
            depth = siblings.shape[1] // self.fr_bytes
        a, b = hk_poseidon_desc(*ld), hk_poseidon_desc(*nd)
        check(self.lib.hk_poseidon_path(self.handle, ptr(consts), int(n_consts), C.byref(a), C.byref(b), ptr(leaf),
                                        ptr(siblings) if depth else None, index.ctypes.data, depth, batch, int(n_v),
                                        int(col0), _device_addr(z_out)), "hk_poseidon_path")

    def wprog_upload(self, ops, refs, vmap, n_values, n_inputs):
        """hk_wprog_upload: a class's word program (sha_circuit.Tape.word_program) resident on the device."""
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        refs = np.ascontiguousarray(refs, dtype=np.uint32)
        vmap = np.ascontiguousarray(vmap, dtype=np.uint32)
        h = C.c_void_p()
        check(self.lib.hk_wprog_upload(self.handle, ops.ctypes.data, ops.shape[0], refs.ctypes.data if refs.size else None,
                                       refs.size, vmap.ctypes.data, vmap.size, int(n_values), int(n_inputs), C.byref(h)),
              "hk_wprog_upload")
        return WordProgram(self, h, vmap.size, int(n_inputs))

    def bases_upload(self, group, bases, n=None):
        """Makes a static base set resident with its shift tables (hk_bases_upload); returns a ResidentBases."""
        pb = self.g1_bytes if group == 1 else self.g2_bytes
        n = n if n is not None else len(bases) // pb
        h = C.c_void_p()
        check(self.lib.hk_bases_upload(self.handle, int(group), ptr(bases), n, C.byref(h)), "hk_bases_upload")
        return ResidentBases(self, h, group, n)

    def field_convert(self, which, data, to_mont):
        """Montgomery <-> canonical for a packed array of Fr (`which` = 0) or Fq (1) elements: what ark-ff
        `from_bigint` / `into_bigint` do under ark-serialize.  Returns a new numpy uint8 array."""
        eb = self.fr_bytes if which == 0 else self.fq_bytes
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        n = data.size // eb
        out = np.empty(n * eb, dtype=np.uint8)
        check(self.lib.hk_field_convert(self.handle, int(which), data.ctypes.data, out.ctypes.data, n, int(to_mont)),
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
        csrs = []
        for (rp, col, val) in (A, B, Cm):
            rp = np.ascontiguousarray(rp, dtype=np.uint64)
            col = np.ascontiguousarray(col, dtype=np.uint32)
            val = np.ascontiguousarray(val, dtype=np.uint8)
            keep += [rp, col, val]
            csrs.append(hk_csr(rp.ctypes.data, col.ctypes.data, val.ctypes.data, len(rp) - 1, len(col)))
        nv = n_v if n_v is not None else len(z) // self.fr_bytes
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
            n_rows = arrs[0].nbytes // 8 - 1
            nnz = arrs[1].nbytes // 4
            out.append(hk_csr(*[_nullable(x) for x in arrs], n_rows, nnz))
        return out

    def qap_eval(self, A, B, Cm, n_inst, n_constraints, n_v, t, out=None):
        """hk_qap_eval (instance_map_with_evaluation, generator.rs:75-76) at t (int, or Montgomery bytes).  A/B/Cm: CSR
        triples as in witness_map (members may be DeviceBuffers).  out: optional (a, b, c) DeviceBuffers of n_v Fr each.
        Returns (a, b, c, zt, m): a/b/c Montgomery bytes (numpy, or the given DeviceBuffers), zt Montgomery bytes."""
        from .cp_groth16 import FrCodec
        keep = []
        csrs = self._csrs((A, B, Cm), keep)
        t = FrCodec(self.curve).enc1(t) if isinstance(t, int) else np.ascontiguousarray(t, dtype=np.uint8)
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
        from .cp_groth16 import FrCodec
        fc = FrCodec(self.curve)
        enc = lambda x: fc.enc1(x) if isinstance(x, int) else np.ascontiguousarray(x, dtype=np.uint8)
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
        keep += [sr, dl] + sc
        d = hk_keygen_desc(C.pointer(csrs[0]), C.pointer(csrs[1]), C.pointer(csrs[2]), n_inst, n_constraints, n_v,
                           sr.ctypes.data if ns else None, ns, *[x.ctypes.data for x in sc], dl.ctypes.data if ns else None)
        ckp = _ptr_array(res["ck"])
        o = hk_keygen_out(*[_nullable(res[k]) for k in ("a_g", "b_g", "b_h", "h_g")], ckp,
                          *[_nullable(res[k]) for k in ("deltas_g", "alpha_g", "beta_g", "gamma_abc_g", "beta_h", "gamma_h",
                                                        "deltas_h")], _nullable(res.get("qap_abc")))
        m_out = C.c_size_t()
        try:
            check(self.lib.hk_keygen(self.handle, C.byref(d), C.byref(o), C.byref(m_out)), "hk_keygen")
        except HekatonError:
            for k in ("a_g", "b_g", "b_h", "h_g"):
                if isinstance(res[k], DeviceBuffer):
                    res[k].free()
            raise
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
        ch = _challenge_bytes(self.curve, challenges)
        depth = max(n_sub, 1).bit_length() - 1
        fr = self.fr_bytes
        sizes = [2 * n_sub, (2 + entry_fields) * n_sub, 2 * n_sub - 1, n_sub * depth, 1]
        if out is not None:
            outs = list(out)
            assert [x.nbytes >= k * fr for x, k in zip(outs, sizes)] == [True] * 5
        else:
            outs = [DeviceBuffer(self, max(k, 1) * fr) if device_out else np.zeros(max(k, 0) * fr, dtype=np.uint8) for k in sizes]
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
        ch = _challenge_bytes(self.curve, challenges)
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
        if n_entries is None:
            n_entries = (src.nbytes if isinstance(src, DeviceBuffer) else src.size) // (max(k, 1) * fr)
        n = int(n_entries)
        if device_out:
            out = DeviceBuffer(self, max(n * k * fr, 1))
            perm = DeviceBuffer(self, max(4 * n, 1)) if want_perm else None
        else:
            out = np.zeros(n * k * fr, dtype=np.uint8)
            perm = np.zeros(n, dtype=np.uint32) if want_perm else None
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
        sizes = [32 * n, 2 * n * k * fr, fr]
        outs = [DeviceBuffer(self, max(b, 1)) if device_out else np.zeros(b, dtype=np.uint8) for b in sizes]
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
        out = DeviceBuffer(self, max(4 * batch * k, 1)) if device_out else np.zeros((batch, k), dtype=np.uint32)
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
            out = DeviceBuffer(self, max(n, 1)) if device_out else np.zeros(n, dtype=np.uint8)
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
            out = tuple(DeviceBuffer(self, max(b, 1)) if device_out else np.zeros(b, dtype=np.uint8) for b in sizes)
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
        m = 0 if keep[0] is None else (keep[0].nbytes if isinstance(keep[0], DeviceBuffer) else keep[0].size) // 66
        u, fr = kinds.size, self.fr_bytes
        a, b = hk_poseidon_desc(*ld), hk_poseidon_desc(*nd)
        d = hk_vkd_tree_desc(int(depth), m, _nullable(keep[0]) if m else None, u, _nullable(kinds), _nullable(keep[1]),
                             _nullable(keep[2]), int(n_consts), C.pointer(a), C.pointer(b))
        own = out is None
        if own:
            sizes = [u * int(depth) * fr, 2 * fr, u]
            out = tuple(DeviceBuffer(self, max(n, 1)) if device_out else np.zeros(n, dtype=np.uint8) for n in sizes)
        with _owned(out, own):
            check(self.lib.hk_vkd_tree(self.handle, C.byref(d), ptr(out[0]), ptr(out[1]), ptr(out[2])), "hk_vkd_tree")
        return tuple(out)

    def _r1cs_call(self, fn, head, z, n_v, batch, cap, want_vals):
        """The shared tail of Context.r1cs_check / DevicePk.r1cs_check: `fn(*head, z, n_v, batch, verdicts, rows, vals, cap)`."""
        fr, batch, cap = self.fr_bytes, int(batch), int(cap)
        zz = z if isinstance(z, DeviceBuffer) else np.ascontiguousarray(z, dtype=np.uint8).reshape(-1)
        if n_v is None:
            n_v = (zz.nbytes if isinstance(zz, DeviceBuffer) else zz.size) // (fr * max(batch, 1))
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
        pb = self.g1_bytes if group == 1 else self.g2_bytes
        n = n if n is not None else len(pts) // pb
        ok = np.zeros(n, dtype=np.uint8)
        fn = self.lib.hk_points_check_g1 if group == 1 else self.lib.hk_points_check_g2
        check(fn(self.handle, ptr(pts) if n else None, n, ok.ctypes.data), fn.__name__)
        return ok

    def field_sqrt(self, which, data):
        """hk_field_sqrt: square roots of packed Montgomery Fq (`which` = 1) or Fq2 (2) elements.  Returns (roots, ok):
        the root that is not larger than its negative (ark's order), zeros where there is none; ok np.uint8[n] of 1 / 0."""
        eb = self.fq_bytes * int(which)
        data = _hd(data)
        n = (data.nbytes if isinstance(data, DeviceBuffer) else data.size) // eb
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
        xb = self.fq_bytes * (1 if group == 1 else 2)
        x_canon, flags = _hd(x_canon), _hd(flags)
        n = flags.nbytes if isinstance(flags, DeviceBuffer) else flags.size
        pts = out if out is not None else np.zeros(2 * n * xb, dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint8)
        fn = self.lib.hk_points_decompress_g1 if group == 1 else self.lib.hk_points_decompress_g2
        st = fn(self.handle, ptr(x_canon) if n else None, ptr(flags) if n else None, n, int(bool(check)),
                ptr(pts) if n else None, status.ctypes.data)
        if st != HK_OK:                                    # the module's check() is shadowed by the keyword
            raise HekatonError(st, fn.__name__)
        return pts, status

    def points_compress(self, group, pts):
        """hk_points_compress_g1 / _g2: the x coordinate and `SWFlags::from_y_coordinate` of `serialize_compressed`.  pts:
        packed affine Montgomery points (uint8 array or DeviceBuffer).  Returns (x_canon, flags) as points_decompress takes
        them."""
        xb = self.fq_bytes * (1 if group == 1 else 2)
        pts = _hd(pts)
        n = (pts.nbytes if isinstance(pts, DeviceBuffer) else pts.size) // (2 * xb)
        x, flags = np.zeros(n * xb, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        fn = self.lib.hk_points_compress_g1 if group == 1 else self.lib.hk_points_compress_g2
        check(fn(self.handle, ptr(pts) if n else None, n, x.ctypes.data, flags.ctypes.data), fn.__name__)
        return x, flags

    def vk_prepare(self, *, alpha_g, beta_h, gamma_h, deltas_h, gamma_abc_g):
        """hk_vk_prepare (prepare_verifying_key, verifier.rs:7-18).  deltas_h: the stage deltas then delta_last, packed G2
        bytes; gamma_abc_g: packed G1 bytes.  Returns a DeviceVk."""
        arrs = [np.ascontiguousarray(x, dtype=np.uint8).reshape(-1) for x in (alpha_g, beta_h, gamma_h, deltas_h, gamma_abc_g)]
        if len(arrs[0]) != self.g1_bytes or len(arrs[1]) != self.g2_bytes or len(arrs[2]) != self.g2_bytes:
            raise HekatonError(HK_ERR_LEN, "hk_vk_prepare")
        if len(arrs[3]) % self.g2_bytes or len(arrs[4]) % self.g1_bytes:
            raise HekatonError(HK_ERR_LEN, "hk_vk_prepare")
        d = hk_vk_desc(arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data,
                       len(arrs[3]) // self.g2_bytes, arrs[4].ctypes.data, len(arrs[4]) // self.g1_bytes)
        h = C.c_void_p()
        check(self.lib.hk_vk_prepare(self.handle, C.byref(d), C.byref(h)), "hk_vk_prepare")
        return DeviceVk(self, h, d.n_deltas, d.n_abc)

    def pk_upload(self, *, a_g, b_g, b_h, h_g, ck_stages, deltas_g, last_delta_h, alpha_g, beta_g, beta_h,
                  matrices=None, n_inst=0, n_constraints=0):
        """hk_pk_upload: all arguments packed-affine numpy uint8 arrays (or DeviceBuffers with explicit
        lengths via (buf, n) tuples).  matrices = (A, B, C) CSR triples as in witness_map."""
        def arr(x):
            return x if isinstance(x, DeviceBuffer) else np.ascontiguousarray(x, dtype=np.uint8)

        def addr(x):
            return x.ptr if isinstance(x, DeviceBuffer) else x.ctypes.data

        def nbytes(x):
            return x.nbytes
        keep = []
        d = hk_pk_desc()
        a_g, b_g, b_h, h_g = arr(a_g), arr(b_g), arr(b_h), arr(h_g)
        keep += [a_g, b_g, b_h, h_g]
        d.a_g, d.a_len = addr(a_g), nbytes(a_g) // self.g1_bytes
        d.b_g, d.b_g_len = addr(b_g), nbytes(b_g) // self.g1_bytes
        d.b_h, d.b_h_len = addr(b_h), nbytes(b_h) // self.g2_bytes
        d.h_g, d.h_len = addr(h_g), nbytes(h_g) // self.g1_bytes
        cks = [arr(c) for c in ck_stages]
        keep += cks
        ck_ptrs = (C.c_void_p * len(cks))(*[addr(c) for c in cks])
        ck_lens = (C.c_size_t * len(cks))(*[nbytes(c) // self.g1_bytes for c in cks])
        d.ck_stage, d.ck_len, d.n_stages = ck_ptrs, ck_lens, len(cks)
        small = [arr(x) for x in (deltas_g, last_delta_h, alpha_g, beta_g, beta_h)]
        keep += small
        d.deltas_g, d.last_delta_h, d.alpha_g, d.beta_g, d.beta_h = [addr(s) for s in small]
        csrs = []
        if matrices is not None:
            for (rp, col, val) in matrices:
                rp = np.ascontiguousarray(rp, dtype=np.uint64)
                col = np.ascontiguousarray(col, dtype=np.uint32)
                val = arr(val)
                keep += [rp, col, val]
                csrs.append(hk_csr(rp.ctypes.data, col.ctypes.data, val.ctypes.data, len(rp) - 1, len(col)))
            d.A, d.B, d.C = C.pointer(csrs[0]), C.pointer(csrs[1]), C.pointer(csrs[2])
        d.n_inst, d.n_constraints = n_inst, n_constraints
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
        if isinstance(inputs, DeviceBuffer):
            assert batch is not None and inputs.nbytes >= 4 * int(batch) * self.n_inputs, "a DeviceBuffer of inputs needs batch="
            batch, in_ptr = int(batch), inputs.ptr
        else:
            inputs = np.ascontiguousarray(inputs, dtype=np.uint32)
            batch, in_ptr = inputs.shape[0], inputs.ctypes.data
        cols = np.ascontiguousarray(full_cols, dtype=np.uint32)
        vals = np.ascontiguousarray(full_vals, dtype=np.uint8)
        buf = out if out is not None else DeviceBuffer(self.ctx, batch * self.n_v * self.ctx.fr_bytes)
        check(self.ctx.lib.hk_wprog_run(self.ctx.handle, self.handle, in_ptr, batch,
                                        cols.ctypes.data if cols.size else None, vals.ctypes.data if cols.size else None,
                                        cols.size, buf.ptr), "hk_wprog_run")
        return buf

    def scatter(self, full_cols, full_vals, out):
        """The full-width values alone (hk_assignment_scatter), into assignments `run(inputs, [], [], out=...)` produced."""
        cols = np.ascontiguousarray(full_cols, dtype=np.uint32)
        vals = np.ascontiguousarray(full_vals, dtype=np.uint8)
        batch = vals.size // max(1, cols.size * self.ctx.fr_bytes)
        check(self.ctx.lib.hk_assignment_scatter(self.ctx.handle, cols.ctypes.data, vals.ctypes.data, cols.size, batch, self.n_v,
                                                 out.ptr), "hk_assignment_scatter")
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
        ns = n_scalars if n_scalars is not None else len(scalars) // self.ctx.fr_bytes
        out = np.zeros(self.ctx.g1_bytes if self.group == 1 else self.ctx.g2_bytes, dtype=np.uint8)
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
            size = arr.nbytes if isinstance(arr, DeviceBuffer) else (0 if arr is None else np.asarray(arr).nbytes)
            if size != n * per:
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
            n = (a.nbytes if isinstance(a, DeviceBuffer) else np.asarray(a).nbytes) // ctx.g1_bytes
        ds = ds if ds is not None else np.zeros(0, dtype=np.uint8)
        inputs = inputs if inputs is not None else np.zeros(0, dtype=np.uint8)
        self.check_args(n, a, b, c, ds, inputs, rand)
        keep = [x if isinstance(x, DeviceBuffer) else np.ascontiguousarray(x, dtype=np.uint8) for x in (a, b, c, ds, inputs)]
        rr = None if rand is None else np.ascontiguousarray(rand, dtype=np.uint8).reshape(-1)
        out = verdicts if verdicts is not None else np.zeros(n, dtype=np.uint8)
        flags = HK_VERIFY_CHECK_POINTS if check_points else 0
        nz = lambda x: ptr(x) if n and (x.nbytes if isinstance(x, DeviceBuffer) else x.size) else None
        check(ctx.lib.hk_verify_batch(ctx.handle, self.handle, nz(keep[0]), nz(keep[1]), nz(keep[2]), nz(keep[3]),
                                      nz(keep[4]), n, flags, None if rr is None else rr.ctypes.data, ptr(out)),
              "hk_verify_batch")
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
        n = n if n is not None else len(w_stage) // ctx.fr_bytes
        kappa = np.ascontiguousarray(kappa, dtype=np.uint8)
        out = np.zeros(ctx.g1_bytes, dtype=np.uint8)
        check(ctx.lib.hk_commit(ctx.handle, self.handle, stage, ptr(w_stage) if n else None, n,
                                kappa.ctypes.data, out.ctypes.data), "hk_commit")
        return out

    def commit_batch(self, stage, w_rows, kappas, n, batch):
        """hk_commit_batch: the stage commitments of `batch` subcircuits of this key's class in one call.  w_rows: their
        stage witnesses row after row (batch x n Fr Montgomery; uint8 array or DeviceBuffer); kappas: batch Fr Montgomery
        (uint8 array).  Returns (batch, g1_bytes) uint8."""
        ctx = self.ctx
        kap = np.ascontiguousarray(kappas, dtype=np.uint8)
        out = np.zeros((batch, ctx.g1_bytes), dtype=np.uint8)
        check(ctx.lib.hk_commit_batch(ctx.handle, self.handle, stage, ptr(w_rows) if n else None, n, kap.ctypes.data, batch,
                                      out.ctypes.data), "hk_commit_batch")
        return out

    def prove(self, z, r, s, kappas, n_v=None):
        """prover.rs:78-155 + committer.rs:112-114; returns (a, b, c) packed affine bytes."""
        ctx = self.ctx
        n_v = n_v if n_v is not None else len(z) // ctx.fr_bytes
        r = np.ascontiguousarray(r, dtype=np.uint8)
        s = np.ascontiguousarray(s, dtype=np.uint8)
        kap = np.ascontiguousarray(kappas, dtype=np.uint8)
        nk = len(kap) // ctx.fr_bytes
        a = np.zeros(ctx.g1_bytes, dtype=np.uint8)
        b = np.zeros(ctx.g2_bytes, dtype=np.uint8)
        c = np.zeros(ctx.g1_bytes, dtype=np.uint8)
        check(ctx.lib.hk_prove(ctx.handle, self.handle, ptr(z), n_v, r.ctypes.data, s.ctypes.data,
                               kap.ctypes.data if nk else None, nk, a.ctypes.data, b.ctypes.data,
                               c.ctypes.data), "hk_prove")
        return a, b, c

    def prove_batch(self, z_rows, rs, ss, kappas, n_v, batch):
        """hk_prove_batch: `batch` proofs of this key's class in one lock-step call.  z_rows: their assignments row after
        row (batch x n_v Fr Montgomery; uint8 array or DeviceBuffer); rs, ss: batch Fr each; kappas: batch x n_kappas Fr
        (uint8 arrays, Montgomery).  Returns (a, b, c) as (batch, g1 | g2 | g1 bytes) uint8 arrays; row b equals
        prove() on row b."""
        ctx = self.ctx
        r = np.ascontiguousarray(rs, dtype=np.uint8).reshape(-1)
        s = np.ascontiguousarray(ss, dtype=np.uint8).reshape(-1)
        kap = np.ascontiguousarray(kappas, dtype=np.uint8).reshape(-1)
        nk = len(kap) // (ctx.fr_bytes * batch) if batch else 0
        a = np.zeros((batch, ctx.g1_bytes), dtype=np.uint8)
        b = np.zeros((batch, ctx.g2_bytes), dtype=np.uint8)
        c = np.zeros((batch, ctx.g1_bytes), dtype=np.uint8)
        check(ctx.lib.hk_prove_batch(ctx.handle, self.handle, ptr(z_rows), n_v, r.ctypes.data, s.ctypes.data,
                                     kap.ctypes.data if nk else None, nk, batch, a.ctypes.data, b.ctypes.data,
                                     c.ctypes.data), "hk_prove_batch")
        return a, b, c
