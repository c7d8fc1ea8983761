"""Loader and integer packing for the test-only device shim (tests/device_shim/field_dev_shim.hip): plain helper of
tests/test_field_device_gpu.py and tests/test_wave_f12_gpu.py.  The shim runs in the calling process."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"asm": "libfield_dev_shim.so", "noasm": "libfield_dev_shim_noasm.so"}

# FieldOp / WaveOp of field_dev_shim.hip
ADD, SUB, MUL, SQR, NEG, DBL, HALVE, CANON, TO_MONT, FROM_MONT, INV, IS_ZERO, EQ, CHAIN = range(14)
W_MUL, W_SQR, W_CYC_SQR, W_CONJ, W_FROB1, W_FROB2, W_FROB3, W_INV = range(8)
ALIAS_NONE, ALIAS_A, ALIAS_B, ALIAS_ALL = range(4)

_loaded = {}


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


class DevShim:
    def __init__(self, variant):
        path = os.path.join(ROOT, "hekaton_system_amd", "lib", VARIANTS[variant])
        assert os.path.exists(path), "build the device shim first (python __graft_entry__.py)"
        self.variant = variant
        self.lib = ctypes.CDLL(path)
        self.lib.dshim_field_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                            ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
        self.lib.dshim_wave_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                           ctypes.c_size_t, ctypes.c_int]
        assert self.lib.dshim_uses_asm() == (1 if variant == "asm" else 0)

    def field_op(self, fid, op, nbytes, a, b=None, raw=0, chain=0):
        """a, b: lists of ints (base fields) or of (c0, c1) tuples (Fq2), as raw limbs -> the same shape back"""
        width = 1 if isinstance(a[0], int) else len(a[0])
        abuf = pack(a, nbytes)
        bbuf = None if b is None else pack(b, nbytes)
        out = ctypes.create_string_buffer(len(abuf))
        st = self.lib.dshim_field_op(fid, op, abuf, bbuf, out, len(a), raw, chain)
        assert st == 0, "dshim_field_op(field %d, op %d): HIP error %d" % (fid, op, st)
        return unpack(out.raw, nbytes, width)

    def wave_op(self, cid, op, nbytes, a, b=None, alias=ALIAS_NONE):
        """a, b: lists of 12-tuples of raw Fq limbs values -> list of 13-tuples (canonical; the last is the padding slot)"""
        abuf = pack(a, nbytes)
        bbuf = None if b is None else pack(b, nbytes)
        out = ctypes.create_string_buffer(len(a) * 13 * nbytes)
        st = self.lib.dshim_wave_op(cid, op, abuf, bbuf, out, len(a), alias)
        assert st == 0, "dshim_wave_op(curve %d, op %d, alias %d): HIP error %d" % (cid, op, alias, st)
        return unpack(out.raw, nbytes, 13)


def load(variant):
    if variant not in _loaded:
        _loaded[variant] = DevShim(variant)
    return _loaded[variant]
