"""CPU: the fused two-product Montgomery primitive, r = (a b + c d) / R with one reduction (Fp::mul2 of csrc/field.cuh,
HK_MONT2_ASM_<FIELD> of csrc/mont_asm.h), without a GPU.

  * host shim (tests/host_shim/mul2_shim.cpp, g++): the C++ fallback of Fp::mul2 / mulsub / neg_operand on canonical values of
    the four base fields, against Python integers;
  * the recurrence restated on integers (tests/mul2_cases.py mul2_columns: columns of three sums, 32-bit limbs, a 96-bit
    accumulator): per modulus the bound before the correction, the generator's correction decision against 8p + R > 2R, and
    that the value fits N limbs;
  * the generated text itself, HK_MONT2_ASM_<FIELD> and HK_NEG2P_ASM_<FIELD>, interpreted on integers (tests/asm_interp.py)
    over the same tuples.
"""
import ctypes
import os
import random
import re
import sys

import pytest

from tests import asm_interp as ai
from tests import field_edges as fe
from tests import host_build
from tests import mul2_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hekaton_system_amd", "csrc")
FIELD_NAMES = list(mc.FIELDS)


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, CSRC)
    try:
        import gen_mont_asm
    finally:
        sys.path.remove(CSRC)
    return gen_mont_asm


# ---- host shim ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim") / "mul2_shim.so")
    host_build.build("mul2_shim.cpp", out, "-O1", "-Wall", "-Werror", *host_build.SHARED)
    lib = host_build.load(out)
    lib.shim_mul2.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_char_p] * 5 + [ctypes.c_size_t]
    return lib


def canonical_tuples(f):
    """host code holds canonical values only"""
    p = f.p
    rnd = random.Random("%s/mul2-host" % f.name)
    g = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, f.one, (1 << (32 * (f.N - 1))) - 1]
    out = [(a, b, c, d) for a in g for b in g for c in g for d in g]
    out += [tuple(rnd.randrange(p) for _ in range(4)) for _ in range(2000)]
    for _ in range(32):
        a, b, c = (rnd.randrange(1, p) for _ in range(3))
        out.append((a, b, c, (-a * b * pow(c, -1, p)) % p))
    return out


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_host_fallback(name, shim):
    f = mc.FIELDS[name]
    nb = 4 * f.N
    ts = canonical_tuples(f)
    cols = [b"".join(t[k].to_bytes(nb, "little") for t in ts) for k in range(4)]
    for op, sign in ((0, 1), (1, -1), (2, -1)):
        out = ctypes.create_string_buffer(len(ts) * nb)
        assert shim.shim_mul2(fe.FIELD_IDS[name], op, *cols, out, len(ts)) == 0
        for i, (a, b, c, d) in enumerate(ts):
            r = int.from_bytes(out.raw[i * nb:(i + 1) * nb], "little")
            assert r == (a * b + sign * c * d) * f.Rinv % f.p, "%s op %d tuple %d" % (name, op, i)
    assert shim.shim_mul2(7, 0, *cols, out, 1) == 1 and shim.shim_mul2(0, 3, *cols, out, 1) == 1


# ---- the recurrence on integers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIELD_NAMES)
def test_bound_and_correction_decision(name, gen):
    f = mc.FIELDS[name]
    p, R, B = f.p, f.R, f.B
    # operands up to the bound ITSELF (neg_operand gives 2p for 0): m < R, so the value is below (4 B^2 / 2 + R p) / R
    worst = (2 * B * B + R * p) // R + 1
    if f.lazy:
        assert gen.mul2_needs_correction(p, f.N) == (8 * p + R > 2 * R) == mc.needs_correction(f)
        assert worst <= p + (8 * p * p) // R + 1
        assert worst <= 4 * p <= R                             # one subtraction of 2p suffices, and N limbs hold it
        if not mc.needs_correction(f):
            assert worst <= 2 * p
    else:
        assert worst <= 2 * p <= R                             # canonical operands: reduce_once, as after mul
    text = open(os.path.join(CSRC, "mont_asm.h"), encoding="utf-8").read()
    flag = int(re.search(r"#define HK_MONT2_FIX_%s (\d)" % name, text).group(1))
    assert flag == (int(mc.needs_correction(f)) if f.lazy else 1)

    ts = mc.tuples(f, n_random=400, n_zero=16)[::7] + mc.tuples(f, 0, 0)[-16:] + [(B - 1, B - 1, B - 1, B), (0, 0, 0, 0)]
    top = 0
    for a, b, c, d in ts:
        v, peak = mc.mul2_columns(f, a, b, c, d)
        assert v == mc.mul2_exact(f, a, b, c, d)               # the columns compute the one exact quotient
        assert v < worst and v < R and peak < 1 << 96
        assert (v * R - a * b - c * d) % p == 0
        top = max(top, v)
    if f.lazy:
        assert (top >= 2 * p) == mc.needs_correction(f)        # the largest tuples reach the corrected range exactly where one exists
    print("%s: largest value %.4f p, bound %.4f p" % (name, top / p, worst / p))


# ---- the generated text ----------------------------------------------------------------------------------------------------
def fused_blocks(text):
    """HK_MONT2_ASM_<F>(r, a, b, c, d) as a two-parameter block the interpreter knows: a and c, b and d concatenated.
    HK_NEG2P_ASM_<F> under a name without a digit.  (asm_interp.parse_header reads HK_<LETTERS>_ASM_ macros.)"""
    out = {}
    for name, f in mc.FIELDS.items():
        m = re.search(r"#define HK_MONT2_ASM_%s\(r, a, b, c, d\).*?\} while \(0\)" % name, text, re.S)
        body = m.group(0).replace("HK_MONT2_ASM_%s(r, a, b, c, d)" % name, "HK_FUSED_ASM_%s(r, a, b)" % name)
        body = re.sub(r"\bc\.v\[(\d+)\]", lambda k: "a.v[%d]" % (f.N + int(k.group(1))), body)
        body = re.sub(r"\bd\.v\[(\d+)\]", lambda k: "b.v[%d]" % (f.N + int(k.group(1))), body)
        out[("FUSED", name)] = ai.parse_header(body + "\n")[("FUSED", name)]
        m = re.search(r"#define HK_NEG2P_ASM_%s\(r, a\).*?\} while \(0\)" % name, text, re.S)
        assert bool(m) == f.lazy
        if m:
            body = m.group(0).replace("HK_NEG2P_ASM_", "HK_NEGOP_ASM_")
            out[("NEGOP", name)] = ai.parse_header(body + "\n")[("NEGOP", name)]
    return out


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_generated_text(name):
    f = mc.FIELDS[name]
    N = f.N
    blocks = fused_blocks(open(os.path.join(CSRC, "mont_asm.h"), encoding="utf-8").read())
    blk = blocks[("FUSED", name)]
    n2 = N * N
    assert sum(i.startswith("v_mad_u64_u32") for i in blk.instrs) == 3 * n2      # two separate products run 4 N^2
    fn = blk.compile()                        # also: nothing read before written, every written register clobbered
    cov = [0] * len(blk.instrs)
    ts = mc.tuples(f, n_random=1500)
    if f.lazy:
        ts += [(f.B - 1, f.B - 1, f.B - 1, f.B), (1, 0, f.B - 1, f.B)]           # an operand of neg_operand(0)
    for a, b, c, d in ts:
        r = fe.from_limbs(fn(fe.to_limbs(a, N) + fe.to_limbs(c, N), fe.to_limbs(b, N) + fe.to_limbs(d, N), cov))
        assert r == mc.mul2_exact(f, a, b, c, d), "%s: a=%#x b=%#x c=%#x d=%#x got %#x" % (name, a, b, c, d, r)
    if f.lazy:
        neg = blocks[("NEGOP", name)].compile()
        ncov = [0] * len(blocks[("NEGOP", name)].instrs)
        for a in fe.all_values(f):
            assert fe.from_limbs(neg(fe.to_limbs(a, N), fe.to_limbs(0, N), ncov)) == 2 * f.p - a
