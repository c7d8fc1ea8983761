"""Loaders and integer packing for the test-only device shims: tests/device_shim/field_dev_shim.hip (plain helper of
tests/test_field_device_gpu.py and tests/test_wave_f12_gpu.py), tests/device_shim/ec_dev_shim.hip (of
tests/test_ec_device_gpu.py and tests/test_msm_plan_device_gpu.py), tests/device_shim/pair_dev_shim.hip (of
tests/test_pair_device_gpu.py), tests/device_shim/ntt_dev_shim.hip (of tests/test_ntt_device_gpu.py and
tests/test_scan_gpu.py), tests/device_shim/sweep_dev_shim.hip (of tests/test_sweep_device_gpu.py) and
tests/device_shim/sublist_dev_shim.hip (of tests/test_msm_sublist_gpu.py).  The shims run in the calling process.

A shim is one class: LIBS (variant -> library file), SIGS (the argtypes of its entry points, with a restype where it is not
int) and USES_ASM (the entry point that tells the variant, where there is one), on the loader of Shim."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"asm": "libfield_dev_shim.so", "noasm": "libfield_dev_shim_noasm.so"}

# FieldOp / WaveOp of field_dev_shim.hip
ADD, SUB, MUL, SQR, NEG, DBL, HALVE, CANON, TO_MONT, FROM_MONT, INV, IS_ZERO, EQ, CHAIN = range(14)
W_MUL, W_SQR, W_CYC_SQR, W_CONJ, W_FROB1, W_FROB2, W_FROB3, W_INV = range(8)
ALIAS_NONE, ALIAS_A, ALIAS_B, ALIAS_ALL = range(4)

# ec_dev_shim.hip
EC_VARIANTS = {"asm": "libec_dev_shim.so", "noasm": "libec_dev_shim_noasm.so"}
(G_MADD, G_MADD_NI, G_ADD, G_ADD_NI, G_DBL, G_DBL_NI, G_DBL_AFFINE, G_NEG, G_TO_AFFINE, G_MUL_SMALL, G_MUL_LIMBS,
 G_MADD_CHAIN) = range(12)
HIP_NOT_SUPPORTED = 801
# what the -DHK_NO_ASM_MUL build leaves out, by group id: with the C++ product these forms outgrow the code-object bounds
# (see op_built in ec_dev_shim.hip); the shim answers hipErrorNotSupported for them.  EcShim.built asserts that this table
# and the shim's op_built agree
EC_NOASM_NOT_BUILT = {
    1: {G_MADD, G_MADD_NI, G_ADD, G_ADD_NI, G_MUL_SMALL, G_MUL_LIMBS, G_MADD_CHAIN},
    2: {G_MADD, G_MADD_CHAIN},
}

# pair_dev_shim.hip: built as shipped only (its -DHK_NO_ASM_MUL twin outgrows the code-object bounds: see the header of
# tests/device_shim/Makefile)
PAIR_VARIANTS = {"asm": "libpair_dev_shim.so"}
Q_MUL, Q_SQR, Q_MUL_BY_CHAR, Q_PSI = range(4)
FORM_LANE, FORM_QUAD = 0, 1

# ntt_dev_shim.hip
NTT_VARIANTS = {"asm": "libntt_dev_shim.so", "noasm": "libntt_dev_shim_noasm.so"}
NTT_REFUSED = 1000           # SHIM_REFUSED of shim_common.cuh: arguments outside a kernel's contract, nothing launched
FR_BYTES = 32

# sweep_dev_shim.hip: built as shipped only (see the header of tests/device_shim/Makefile)
SWEEP_LIB = "libsweep_dev_shim.so"
SPLIT_K_LANE, SPLIT_QUAD = 0, 1
MUL_PLAIN, MUL_ENDO = 0, 1

# sublist_dev_shim.hip: integer kernels only, one build
SUBLIST_LIB = "libsublist_dev_shim.so"

_loaded = {}                 # library file name -> its shim object

vp, ui, up, sz, ci = ctypes.c_char_p, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint), ctypes.c_size_t, ctypes.c_int


def pack(elems, nbytes):
    """elements (an int, or a tuple of ints for an extension element) -> little-endian limbs, nbytes per int"""
    if isinstance(elems[0], int):
        return b"".join(x.to_bytes(nbytes, "little") for x in elems)
    return b"".join(c.to_bytes(nbytes, "little") for x in elems for c in x)


def unpack(buf, nbytes, width=1):
    ints = [int.from_bytes(buf[i:i + nbytes], "little") for i in range(0, len(buf), nbytes)]
    if width == 1:
        return ints
    return [tuple(ints[i:i + width]) for i in range(0, len(ints), width)]


def check(st, what):
    """every entry point answers 0, minus a hipError_t, or (> 0) a refusal of the shim's or the product's hk_status"""
    assert st == 0, "%s: %s %d" % (what, "HIP error" if st < 0 else "status", abs(st))


class Shim:
    LIBS, SIGS, USES_ASM = {}, {}, None

    def __init__(self, variant="asm"):
        path = os.path.join(ROOT, "hekaton_system_amd", "lib", self.LIBS[variant])
        assert os.path.exists(path), "build the device shim first (python __graft_entry__.py)"
        self.variant = variant
        self.lib = ctypes.CDLL(path)
        for name, sig in self.SIGS.items():
            fn = getattr(self.lib, name)
            if isinstance(sig, tuple):
                sig, fn.restype = sig
            fn.argtypes = sig
        if self.USES_ASM:
            assert getattr(self.lib, self.USES_ASM)() == (1 if variant == "asm" else 0)

    @classmethod
    def load(cls, variant="asm"):
        name = cls.LIBS[variant]
        if name not in _loaded:
            _loaded[name] = cls(variant)
        return _loaded[name]


class DevShim(Shim):
    LIBS, USES_ASM = VARIANTS, "dshim_uses_asm"
    SIGS = {"dshim_field_op": [ci, ci, vp, vp, vp, sz, ci, ci], "dshim_wave_op": [ci, ci, vp, vp, vp, sz, ci]}

    def field_op(self, fid, op, nbytes, a, b=None, raw=0, chain=0):
        """a, b: lists of ints (base fields) or of (c0, c1) tuples (Fq2), as raw limbs -> the same shape back"""
        width = 1 if isinstance(a[0], int) else len(a[0])
        abuf = pack(a, nbytes)
        bbuf = None if b is None else pack(b, nbytes)
        out = ctypes.create_string_buffer(len(abuf))
        st = self.lib.dshim_field_op(fid, op, abuf, bbuf, out, len(a), raw, chain)
        check(st, "dshim_field_op(field %d, op %d)" % (fid, op))
        return unpack(out.raw, nbytes, width)

    def wave_op(self, cid, op, nbytes, a, b=None, alias=ALIAS_NONE):
        """a, b: lists of 12-tuples of raw Fq limbs values -> list of 13-tuples (canonical; the last is the padding slot)"""
        abuf = pack(a, nbytes)
        bbuf = None if b is None else pack(b, nbytes)
        out = ctypes.create_string_buffer(len(a) * 13 * nbytes)
        st = self.lib.dshim_wave_op(cid, op, abuf, bbuf, out, len(a), alias)
        check(st, "dshim_wave_op(curve %d, op %d, alias %d)" % (cid, op, alias))
        return unpack(out.raw, nbytes, 13)


load = DevShim.load


class EcShim(Shim):
    """Points travel as slots of four coordinate-field elements (x, y, zz, zzz; an affine point fills the first two), each an
    int (G1) or a (c0, c1) tuple (G2) of RAW limbs: Montgomery values, possibly non-canonical representatives."""

    LIBS, USES_ASM = EC_VARIANTS, "dshim_ec_uses_asm"
    SIGS = {"dshim_group_op": [ci, ci, vp, vp, vp, sz, ci, ui], "dshim_batch_affine": [ci, vp, vp, sz, ui],
            "dshim_msm": [ci] + [ui] * 6 + [vp, vp, ci, vp, up]}

    def __init__(self, variant):
        super().__init__(variant)
        assert self.lib.dshim_ec_has_msm() == (1 if variant == "asm" else 0)

    def built(self, gid, op):
        """whether this build holds `op` for group `gid`: the table above, which must agree with the shim's own op_built"""
        want = self.variant == "asm" or op not in EC_NOASM_NOT_BUILT.get(gid, ())
        assert bool(self.lib.dshim_ec_op_built(gid, op)) == want, "EC_NOASM_NOT_BUILT and op_built differ: g%d op %d" % (gid, op)
        return want

    def group_op_status(self, gid, op, nbytes, a, b=None, raw=0, k=0):
        """-> (status, slots): status 0, or minus the hipError_t"""
        width = 1 if isinstance(a[0][0], int) else len(a[0][0])
        abuf = b"".join(pack(list(slot), nbytes) for slot in a)
        bbuf = None if b is None else b"".join(pack(list(slot), nbytes) for slot in b)
        assert bbuf is None or len(bbuf) == len(abuf)
        out = ctypes.create_string_buffer(len(abuf))
        st = self.lib.dshim_group_op(gid, op, abuf, bbuf, out, len(a), raw, k)
        if st != 0:
            return st, None
        elems = unpack(out.raw, nbytes, width)
        return 0, [tuple(elems[i:i + 4]) for i in range(0, len(elems), 4)]

    def group_op(self, gid, op, nbytes, a, b=None, raw=0, k=0):
        st, slots = self.group_op_status(gid, op, nbytes, a, b, raw, k)
        check(st, "dshim_group_op(group %d, op %d)" % (gid, op))
        return slots

    def batch_affine(self, gid, nbytes, pts, chunk):
        """pts: XYZZ slots as they lie in memory -> list of (x, y)"""
        width = 1 if isinstance(pts[0][0], int) else len(pts[0][0])
        buf = b"".join(pack(list(slot), nbytes) for slot in pts)
        out = ctypes.create_string_buffer(len(buf) // 2)
        st = self.lib.dshim_batch_affine(gid, buf, out, len(pts), chunk)
        check(st, "dshim_batch_affine(group %d, n %d, chunk %d)" % (gid, len(pts), chunk))
        elems = unpack(out.raw, nbytes, width)
        return [tuple(elems[i:i + 2]) for i in range(0, len(elems), 2)]

    def msm(self, gid, c, WP, n, bases, scalars, mont, batch=1, n_bases=None, idx_off=0, point_bytes=0):
        """bases: bytes of n_bases affine points (memory form), scalars: bytes of batch x n Fr -> (status, bytes of batch
        affine points or None, plan words W, F, NB, n_levels, T[0], T[1], Lmin0, K, lanes).  status: 0, the product's hk_status
        (> 0), or minus a hipError_t."""
        if n_bases is None:
            n_bases = n
        assert len(bases) == n_bases * point_bytes and len(scalars) == batch * n * 32
        out = ctypes.create_string_buffer(batch * point_bytes)
        plan = (ctypes.c_uint * 9)()
        st = self.lib.dshim_msm(gid, c, WP, batch, n, n_bases, idx_off, bytes(bases) if n_bases else None, bytes(scalars),
                                1 if mont else 0, out, plan)
        return st, (out.raw if st == 0 else None), list(plan)


load_ec = EcShim.load


class PairShim(Shim):
    """The stages of the multi-pairing pipeline.  f2q_op takes and gives integers (raw limbs in, canonical Montgomery values
    out); the pipeline stages take and give the bytes the kernels read and write (Montgomery, little-endian; nb bytes per Fq):
    an affine G1 point is 2 Fq, a G2 point 4, a raw line 6 (c0, c1, c2 in Fq2), an Fq12 value 12."""

    LIBS, USES_ASM = PAIR_VARIANTS, "dshim_pair_uses_asm"
    SIGS = {"dshim_f2q_op": [ci, ci, vp, vp, vp, sz], "dshim_pair_lines": [ci, ci, vp, ui, ui, vp, up],
            "dshim_pair_tree_lines": [ci, vp, vp, ui, ui, ui, ui, ui, up, up, ui, vp], "dshim_pair_tree": [ci, vp, ui, ui, ui, vp],
            "dshim_pair_horner": [ci, vp, ui, vp], "dshim_pair_steps": ([ci], ui)}

    def steps(self, cid):
        return self.lib.dshim_pair_steps(cid)

    def f2q_op(self, cid, op, nbytes, a, b=None):
        """a, b: lists of (c0, c1) raw limb values -> per element the four lanes' results: (c0, c1) each, or for the point ops
        (a = the x, b = the y of the points) ((x0, x1), (y0, y1)) each"""
        per = 2 if op in (Q_MUL_BY_CHAR, Q_PSI) else 1
        abuf = pack(a, nbytes)
        bbuf = None if b is None else pack(b, nbytes)
        out = ctypes.create_string_buffer(len(a) * 4 * per * 2 * nbytes)
        st = self.lib.dshim_f2q_op(cid, op, abuf, bbuf, out, len(a))
        check(st, "dshim_f2q_op(curve %d, op %d)" % (cid, op))
        f2 = unpack(out.raw, nbytes, 2)
        if per == 2:
            f2 = [tuple(f2[i:i + 2]) for i in range(0, len(f2), 2)]
        return [f2[4 * i:4 * i + 4] for i in range(len(a))]

    def pair_lines(self, cid, form, nb, g2, n, n_r):
        """g2: bytes of n_r x n affine G2 points -> (bytes of the n_r x S x n raw lines, S)"""
        assert len(g2) == n_r * n * 4 * nb
        S = self.steps(cid)
        out = ctypes.create_string_buffer(n_r * S * n * 6 * nb)
        got_S = ctypes.c_uint(0)
        st = self.lib.dshim_pair_lines(cid, form, bytes(g2), n, n_r, out, ctypes.byref(got_S))
        check(st, "dshim_pair_lines(curve %d, form %d, n %d, n_r %d)" % (cid, form, n, n_r))
        assert got_S.value == S
        return out.raw, S

    def pair_tree_lines(self, cid, nb, lines, g1, n, c, n_l, n_r, S, pairs=None):
        """lines: bytes of n_r x S x n raw lines, g1: bytes of n_l x n affine G1 points, pairs: [(lhs, rhs)] or None for
        the n_l x n_r grid -> bytes of count x S x ceil(n / c) Fq12"""
        assert len(lines) == n_r * S * n * 6 * nb and len(g1) == n_l * n * 2 * nb
        count = len(pairs) if pairs else n_l * n_r
        pa = (ctypes.c_uint * count)(*[a for a, _ in pairs]) if pairs else None
        pb = (ctypes.c_uint * count)(*[b for _, b in pairs]) if pairs else None
        out = ctypes.create_string_buffer(count * S * ((n + c - 1) // c) * 12 * nb)
        st = self.lib.dshim_pair_tree_lines(cid, bytes(lines), bytes(g1), n, c, n_l, n_r, S, pa, pb, len(pairs) if pairs else 0,
                                            out)
        check(st, "dshim_pair_tree_lines(curve %d, n %d)" % (cid, n))
        return out.raw

    def pair_tree(self, cid, nb, vals, n, c, count):
        """vals: bytes of count x n Fq12 -> bytes of count x ceil(n / c) Fq12"""
        assert len(vals) == count * n * 12 * nb
        out = ctypes.create_string_buffer(count * ((n + c - 1) // c) * 12 * nb)
        st = self.lib.dshim_pair_tree(cid, bytes(vals), n, c, count, out)
        check(st, "dshim_pair_tree(curve %d, n %d, c %d)" % (cid, n, c))
        return out.raw

    def pair_horner(self, cid, nb, L, count):
        """L: bytes of count x S Fq12 -> bytes of count Fq12"""
        assert len(L) == count * self.steps(cid) * 12 * nb
        out = ctypes.create_string_buffer(count * 12 * nb)
        st = self.lib.dshim_pair_horner(cid, bytes(L), count, out)
        check(st, "dshim_pair_horner(curve %d, count %d)" % (cid, count))
        return out.raw


load_pair = PairShim.load


class NttShim(Shim):
    """One launch per call of the Fr transform layer.  Fr vectors travel as bytes: canonical Montgomery values, 32 bytes
    each, little-endian - what the kernels read and write.  `curve` is 0 (BN254 Fr) or 1 (BLS12-381 Fr).  The *_status forms
    give (status, bytes or None): 0, NTT_REFUSED, or minus a hipError_t."""

    LIBS, USES_ASM = NTT_VARIANTS, "dshim_ntt_uses_asm"
    SIGS = {"dshim_ntt_tables": [ci, ui, vp, vp], "dshim_pow_table": [ci, vp, ui, ui, vp],
            "dshim_pow_from_tables": [ci, vp, up, ui, ui, vp],
            "dshim_ntt_pass": [ci, ci, vp, sz, ui, vp, ui, ui, ui, ui, ui, ci, ui, vp, vp, vp, vp],
            "dshim_scale_pow": [ci, vp, sz, ui, vp, vp, ui, ci, ci], "dshim_bitrev": [ci, vp, ui],
            "dshim_mul_pointwise": [ci, vp, vp, sz],
            "dshim_spmv": [ci, ctypes.POINTER(ctypes.c_ulonglong), up, vp, sz, vp, sz, vp, ui, ui, ui],
            "dshim_scan_u32": [ctypes.c_void_p, ctypes.c_void_p, ui], "dshim_ntt_scan_pad": ([], ui)}

    def __init__(self, variant):
        super().__init__(variant)
        self.scan_pad = self.lib.dshim_ntt_scan_pad()

    def ntt_tables(self, curve, log_table, sq):
        """sq: bytes of log_table entries w^(2^k) -> bytes of the 2^log_table - 1 stage-table entries"""
        assert len(sq) == log_table * FR_BYTES
        out = ctypes.create_string_buffer(((1 << log_table) - 1) * FR_BYTES)
        st = self.lib.dshim_ntt_tables(curve, log_table, bytes(sq), out)
        check(st, "dshim_ntt_tables(curve %d, log_table %d)" % (curve, log_table))
        return out.raw

    def pow_table(self, curve, sq, count, nbits):
        assert len(sq) == nbits * FR_BYTES
        out = ctypes.create_string_buffer(count * FR_BYTES)
        st = self.lib.dshim_pow_table(curve, bytes(sq), count, nbits, out)
        check(st, "dshim_pow_table(curve %d, count %d, nbits %d)" % (curve, count, nbits))
        return out.raw

    def pow_from_tables(self, curve, pw, js, logn):
        assert len(pw) == 3 * 2048 * FR_BYTES
        out = ctypes.create_string_buffer(len(js) * FR_BYTES)
        st = self.lib.dshim_pow_from_tables(curve, bytes(pw), (ctypes.c_uint * len(js))(*js), len(js), logn, out)
        check(st, "dshim_pow_from_tables(curve %d, logn %d)" % (curve, logn))
        return out.raw

    def ntt_pass_status(self, curve, dit, data, stride, batch, tws, logn, lo, nst, cols_bits, threads, post=0, npost=0xffffffff,
                        scale=None, pw=None, sub=None, kc=None):
        """data: bytes of batch x stride elements (vector v at v * stride) -> the same after one k_ntt_pass4 launch.
        tws: the 2^logn - 1 stage-table entries; scale, kc: one element; pw: 3 x 2048; sub: 2^logn"""
        assert len(data) == batch * stride * FR_BYTES and len(tws) == ((1 << logn) - 1) * FR_BYTES
        assert sub is None or len(sub) == FR_BYTES << logn
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        st = self.lib.dshim_ntt_pass(curve, dit, buf, stride, batch, bytes(tws), logn, lo, nst, cols_bits, threads, post, npost,
                                     scale, pw, sub, kc)
        return st, (buf.raw if st == 0 else None)

    def ntt_pass(self, curve, dit, data, stride, batch, tws, logn, lo, nst, cols_bits, threads, **ep):
        st, out = self.ntt_pass_status(curve, dit, data, stride, batch, tws, logn, lo, nst, cols_bits, threads, **ep)
        check(st, "dshim_ntt_pass(curve %d, dit %d, logn %d, lo %d, nst %d, cols_bits %d, threads %d)" % (
            curve, dit, logn, lo, nst, cols_bits, threads))
        return out

    def scale_pow(self, curve, data, stride, batch, pw, scale, logn, bitrev_index, use_pow):
        assert len(data) == batch * stride * FR_BYTES
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        st = self.lib.dshim_scale_pow(curve, buf, stride, batch, pw, scale, logn, bitrev_index, use_pow)
        check(st, "dshim_scale_pow(curve %d, logn %d)" % (curve, logn))
        return buf.raw

    def bitrev(self, curve, data, logn):
        assert len(data) == FR_BYTES << logn
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        st = self.lib.dshim_bitrev(curve, buf, logn)
        check(st, "dshim_bitrev(curve %d, logn %d)" % (curve, logn))
        return buf.raw

    def mul_pointwise(self, curve, a, b):
        assert len(a) == len(b)
        buf = ctypes.create_string_buffer(bytes(a), len(a))
        st = self.lib.dshim_mul_pointwise(curve, buf, bytes(b), len(a) // FR_BYTES)
        check(st, "dshim_mul_pointwise(curve %d, m %d)" % (curve, len(a) // FR_BYTES))
        return buf.raw

    def spmv(self, curve, row_ptr, col, val, z, out, n_copy):
        """row_ptr, col: lists; val, z: bytes; out: bytes of the m elements as they lie before the launch -> after it"""
        n_rows, nnz, m = len(row_ptr) - 1, len(col), len(out) // FR_BYTES
        assert len(val) == nnz * FR_BYTES
        buf = ctypes.create_string_buffer(bytes(out), len(out))
        st = self.lib.dshim_spmv(curve, (ctypes.c_ulonglong * (n_rows + 1))(*row_ptr), (ctypes.c_uint * max(nnz, 1))(*col),
                                 bytes(val), nnz, bytes(z), len(z) // FR_BYTES, buf, n_rows, n_copy, m)
        check(st, "dshim_spmv(curve %d, n_rows %d, n_copy %d, m %d)" % (curve, n_rows, n_copy, m))
        return buf.raw

    def scan_u32(self, counts, out):
        """counts: numpy uint32 of n; out: numpy uint32 of n + scan_pad, as it lies before the call (changed in place)"""
        n = len(counts)
        assert counts.dtype.name == "uint32" and out.dtype.name == "uint32" and len(out) == n + self.scan_pad
        assert counts.flags["C_CONTIGUOUS"] and out.flags["C_CONTIGUOUS"]
        st = self.lib.dshim_scan_u32(counts.ctypes.data if n else None, out.ctypes.data, n)
        check(st, "dshim_scan_u32(n %d)" % n)


load_ntt = NttShim.load


class SweepShim(Shim):
    """One launch per call of the group sweeps (fixed_base.cuh, endo.cuh).  Everything travels as the bytes the kernels read
    and write: affine points and Fr scalars in memory form (pb bytes per affine point, 32 per scalar), XYZZ results as stored
    (2 pb bytes: x, y, zz, zzz).  `gid`: 0 bn254 G1, 1 bn254 G2, 2 bls G1, 3 bls G2.  The *_status forms give (status, bytes
    or None): 0 or minus a hipError_t."""

    LIBS = {"asm": SWEEP_LIB}
    SIGS = {"dshim_fb_table": [ci, vp, vp], "dshim_fb_mul": [ci, vp, vp, ci, ui, vp], "dshim_points_lincomb": [ci, vp, vp, ui, ui, vp],
            "dshim_scalar_mul": [ci, ci, vp, vp, ui, vp], "dshim_points_fold_endo": [ci, vp, vp, vp, ui, ui, vp],
            "dshim_points_mul_split": [ci, ci, ci, vp, vp, vp, ui, ui, ui, ui, ci, vp], "dshim_points_sum": [ci, vp, ui, vp],
            "dshim_points_sum_seg": [ci, vp, ui, ui, vp]}

    def sum_threads(self, gid):
        return self.lib.dshim_sweep_sum_threads(gid)

    def split_elems(self, gid, form):
        """elements per workgroup of k_points_mul_split in the K-lane (SPLIT_K_LANE) or quad (SPLIT_QUAD; 0 in G1) form"""
        return self.lib.dshim_sweep_split_elems(gid, form)

    def split_nd(self, gid):
        return self.lib.dshim_sweep_split_nd(gid)

    def split_steps(self, gid):
        return self.lib.dshim_sweep_split_steps(gid)

    @staticmethod
    def _done(st, what, out):
        check(st, what)
        return out.raw

    def fb_table(self, gid, pb, base):
        assert len(base) == pb
        out = ctypes.create_string_buffer(32 * 256 * pb)
        return self._done(self.lib.dshim_fb_table(gid, bytes(base), out), "dshim_fb_table(g%d)" % gid, out)

    def fb_mul(self, gid, pb, table, scalars, mont):
        n = len(scalars) // FR_BYTES
        assert len(table) == 32 * 256 * pb and len(scalars) == n * FR_BYTES
        out = ctypes.create_string_buffer(n * 2 * pb)
        return self._done(self.lib.dshim_fb_mul(gid, bytes(table), bytes(scalars), 1 if mont else 0, n, out),
                          "dshim_fb_mul(g%d, n %d)" % (gid, n), out)

    def lincomb(self, gid, pb, vecs, coeffs, k, n):
        assert len(vecs) == k * n * pb and len(coeffs) == k * FR_BYTES
        out = ctypes.create_string_buffer(n * 2 * pb)
        return self._done(self.lib.dshim_points_lincomb(gid, bytes(vecs), bytes(coeffs), k, n, out),
                          "dshim_points_lincomb(g%d, k %d, n %d)" % (gid, k, n), out)

    def scalar_mul(self, gid, pb, kind, pts, scalars):
        n = len(scalars) // FR_BYTES
        assert len(pts) == n * pb
        out = ctypes.create_string_buffer(n * 2 * pb)
        return self._done(self.lib.dshim_scalar_mul(gid, kind, bytes(pts), bytes(scalars), n, out),
                          "dshim_scalar_mul(g%d, kind %d, n %d)" % (gid, kind, n), out)

    def fold_endo(self, gid, pb, lo, hi, coeffs, neg):
        n = len(hi) // pb
        assert len(lo) == n * pb
        out = ctypes.create_string_buffer(n * 2 * pb)
        return self._done(self.lib.dshim_points_fold_endo(gid, bytes(lo), bytes(hi), bytes(coeffs), neg, n, out),
                          "dshim_points_fold_endo(g%d, n %d)" % (gid, n), out)

    def mul_split_status(self, gid, pb, form, uniform, pts, scalars, n, lo=None, neg=0, pts_mod=0, vectors=1, mont=1):
        """pts: vectors x (pts_mod or n) points; lo: vectors x n points or None; scalars: the K magnitudes (uniform) or n Fr
        -> vectors x n XYZZ"""
        assert len(pts) == vectors * (pts_mod or n) * pb and (lo is None or len(lo) == vectors * n * pb)
        out = ctypes.create_string_buffer(vectors * n * 2 * pb)
        st = self.lib.dshim_points_mul_split(gid, form, 1 if uniform else 0, None if lo is None else bytes(lo), bytes(pts),
                                             bytes(scalars), neg, n, pts_mod, vectors, mont, out)
        return st, (out.raw if st == 0 else None)

    def mul_split(self, gid, pb, form, uniform, pts, scalars, n, **kw):
        st, out = self.mul_split_status(gid, pb, form, uniform, pts, scalars, n, **kw)
        check(st, "dshim_points_mul_split(g%d, form %d, uniform %d, n %d, %r)" % (gid, form, uniform, n, sorted(kw)))
        return out

    def points_sum(self, gid, pb, pts):
        n = len(pts) // (2 * pb)
        out = ctypes.create_string_buffer(2 * pb)
        return self._done(self.lib.dshim_points_sum(gid, bytes(pts), n, out), "dshim_points_sum(g%d, n %d)" % (gid, n), out)

    def points_sum_seg(self, gid, pb, pts, seg, batch):
        assert len(pts) == seg * batch * 2 * pb
        out = ctypes.create_string_buffer(batch * 2 * pb)
        return self._done(self.lib.dshim_points_sum_seg(gid, bytes(pts), seg, batch, out),
                          "dshim_points_sum_seg(g%d, seg %d, batch %d)" % (gid, seg, batch), out)


load_sweep = SweepShim.load


class SublistShim(Shim):
    """MsmSort::sublist on a caller-supplied sorted list (BN254 Fr, WP = 1); the arrays are C-contiguous numpy uint32"""
    LIBS = {"asm": SUBLIST_LIB}
    SIGS = {"dshim_sublist_plan": [ui, ui, ui, up], "dshim_msm_sublist": [ui, ui, ui, ui] + [ctypes.c_void_p] * 5}

    def plan(self, c, n, n_dst):
        """-> W, NB, gshift_src, gshift_dst, sorted stride src, sorted stride dst, tiles per proof"""
        out = (ctypes.c_uint * 7)()
        check(self.lib.dshim_sublist_plan(c, n, n_dst, out), "dshim_sublist_plan(c %d, n %d, n_dst %d)" % (c, n, n_dst))
        return list(out)

    def sublist(self, c, batch, n, n_dst, sorted_src, start_src, rank, sorted_dst, start_dst):
        """sorted_dst, start_dst: as they lie before the call, changed in place"""
        arrays = (sorted_src, start_src, rank, sorted_dst, start_dst)
        assert all(a.dtype.name == "uint32" and a.flags["C_CONTIGUOUS"] for a in arrays)
        check(self.lib.dshim_msm_sublist(c, batch, n, n_dst, *[a.ctypes.data for a in arrays]), "dshim_msm_sublist")


load_sublist = SublistShim.load
