"""GPU: the fused two-product Montgomery primitive on the device, against Python integers.

tests/device_shim/mul2/mul2_dev_shim.hip compiles Fp::mul2 / mulsub (and the extension's mul2 / mulsub / mul) and the G1
mixed add of csrc/ec.cuh for gfx950, as shipped ("asm": HK_MONT2_ASM_<FIELD> with its correction) and with -DHK_NO_ASM_MUL
("noasm": the sum of two products).  Operands are raw limbs below the representative bound B (tests/mul2_cases.py):

  * per base field all 8^4 grid tuples, 3000 random tuples, tuples with a b + c d = 0 (mod p) and the largest tuples:
    r = (a b + c d) / R (mod p) and r < B, which on a canonical field means r is canonical;  mulsub likewise, where d = 0
    makes the negated operand 2p;
  * the same tuples as pairs of extension elements through Fp2::mul2, mulsub and mul (the extension has one path: it does
    not use the fused block);
  * chains of 64 mixed adds on one lane per case, the registers read back after every step: normalised, every step equals
    affine addition on integers, through P == Q, P == -Q, an accumulator at infinity and a base at infinity.  As shipped
    the registers also equal the integer model of the lazy arithmetic (mul2_cases.LazyModel) bit for bit, and on BN254
    that model's y passes through the corrected range [2p, 2.52 p) - a wrong bound shows only when such a y is fed back.
"""
import ctypes
import random

import pytest

from tests import dev_shim as ds
from tests import field_edges as fe
from tests import mul2_cases as mc

pytestmark = pytest.mark.gpu

M_MUL2, M_MULSUB, M_MUL = range(3)
FIELD_NAMES = list(mc.FIELDS)
FP2 = {4: "BN254_FQ", 5: "BLS12_381_FQ"}
CURVES = {"bn254": (0, "BN254_FQ", 3), "bls12_381": (1, "BLS12_381_FQ", 4)}       # shim id, coordinate field, b of y^2 = x^3 + b
STEPS, CASES = 64, 12


class Mul2Shim(ds.Shim):
    LIBS, USES_ASM = {"asm": "libmul2_dev_shim.so", "noasm": "libmul2_dev_shim_noasm.so"}, "dshim_mul2_uses_asm"
    SIGS = {"dshim_mul2_op": [ds.ci, ds.ci, ds.vp, ds.vp, ds.vp, ds.vp, ds.vp, ds.sz],
            "dshim_madd_chain": [ds.ci, ds.vp, ds.vp, ds.vp, ds.sz, ds.ui]}

    def op(self, fid, op, nbytes, cols):
        """cols: four lists of ints (base field) or of (c0, c1) tuples -> the raw results, same shape"""
        width = 1 if isinstance(cols[0][0], int) else 2
        bufs = [ds.pack(c, nbytes) for c in cols]
        out = ctypes.create_string_buffer(len(bufs[0]))
        ds.check(self.lib.dshim_mul2_op(fid, op, *bufs, out, len(cols[0])), "dshim_mul2_op(field %d, op %d)" % (fid, op))
        return ds.unpack(out.raw, nbytes, width)

    def chain_status(self, cid, nbytes, accs, bases, steps):
        """accs: per case (x, y, zz, zzz), bases: per case `steps` (x, y) -> (status, per case per step (x, y, zz, zzz))"""
        abuf = b"".join(ds.pack(list(a), nbytes) for a in accs)
        bbuf = b"".join(ds.pack(list(q), nbytes) for case in bases for q in case)
        out = ctypes.create_string_buffer(len(accs) * steps * 4 * nbytes)
        st = self.lib.dshim_madd_chain(cid, abuf, bbuf, out, len(accs), steps)
        if st:
            return st, None
        v = ds.unpack(out.raw, nbytes, 4)
        return 0, [v[i * steps:(i + 1) * steps] for i in range(len(accs))]


@pytest.fixture(scope="module", params=["asm", "noasm"])
def shim(request):
    return Mul2Shim.load(request.param)


_tuples = {}


def columns(f):
    if f.name not in _tuples:
        ts = mc.tuples(f)
        _tuples[f.name] = [[t[k] for t in ts] for k in range(4)]
    return _tuples[f.name]


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_base_field_mul2(shim, name):
    f = mc.FIELDS[name]
    fid, nb, p = fe.FIELD_IDS[name], 4 * f.N, f.p
    cols = columns(f)
    assert len(cols[0]) >= 8 ** 4 + 3000 and (f.B - 1,) * 4 in zip(*cols)
    for op, sign in ((M_MUL2, 1), (M_MULSUB, -1)):
        got = shim.op(fid, op, nb, cols)
        for k, (a, b, c, d, r) in enumerate(zip(*cols, got)):
            want = (a * b + sign * c * d) * f.Rinv % p
            assert r < f.B and (r - want) % p == 0, "%s/%s op %d #%d: a=%#x b=%#x c=%#x d=%#x -> %#x (B = %#x), want %#x" % (
                shim.variant, name, op, k, a, b, c, d, r, f.B, want)


@pytest.mark.parametrize("fid", sorted(FP2))
def test_extension_products(shim, fid):
    f = mc.FIELDS[FP2[fid]]
    nb, p = 4 * f.N, f.p
    base = columns(f)
    n = len(base[0])
    # element k of column j pairs the tuple's operand with the next tuple's: every grid value meets every other in both slots
    cols = [[(col[k], col[(k + 1) % n]) for k in range(n)] for col in base]

    def mul(x, y):
        return ((x[0] * y[0] - x[1] * y[1]) * f.Rinv % p, (x[0] * y[1] + x[1] * y[0]) * f.Rinv % p)

    for op in (M_MUL2, M_MULSUB, M_MUL):
        got = shim.op(fid, op, nb, cols)
        for k, (a, b, c, d, r) in enumerate(zip(*cols, got)):
            ab, cd = mul(a, b), mul(c, d)
            want = ab if op == M_MUL else tuple((u + (1 if op == M_MUL2 else -1) * v) % p for u, v in zip(ab, cd))
            assert all(x < f.B and (x - w) % p == 0 for x, w in zip(r, want)), "%s/field %d op %d #%d: %r, want %r" % (
                shim.variant, fid, op, k, r, want)


# ---- mixed-add chains ----------------------------------------------------------------------------------------------------
# Where a random mixed add puts its fused y into [2p, 2.52 p) about once in 10^4 tries, the start accumulator's z is chosen:
# case k starts under z number Z_INDEX[field][k] of z_of(), found by find_z() below, so that its FIRST step lands there and 63
# steps feed the corrected y back.  BLS12-381 Fq has no such range.
Z_INDEX = {"BN254_FQ": {1: 154, 3: 15820}}


def z_of(f, idx):
    return random.Random("%s/mul2-chain-z/%d" % (f.name, idx)).randrange(1, f.p)


def start_acc(f, pt, z, lazy):
    """the affine point under zz = z^2, zzz = z^3, as raw Montgomery limbs; `lazy` picks which two sit above p"""
    p = f.p
    return (mont(f, pt[0] * z * z % p, lazy), mont(f, pt[1] * z * z * z % p, not lazy), mont(f, z * z % p, lazy),
            mont(f, z * z * z % p, not lazy))


def mont(f, v, lazy):
    v = v * f.R % f.p
    return v + f.p if lazy and v + f.p < f.B else v


def find_z(f, b, k, tries=100000):
    """how Z_INDEX was made: the first z whose first step of case k arrives in the corrected range"""
    acc, bases, _after, pt = chain_cases(f, b)[k]
    for idx in range(tries):
        model = mc.LazyModel(f)
        model.madd(start_acc(f, pt, z_of(f, idx), bool(k & 1)), bases[0])
        if model.corrected:
            return idx
    return None


def chain_cases(f, b):
    """-> per case (raw start accumulator, the raw bases, the affine value after every step, the affine start).
    Step 7 adds a base at infinity, step 15 the accumulated point itself (P == Q), step 23 its negative (the sum is infinity),
    steps 24 and 25 therefore meet an accumulator at infinity with a base at infinity and with a point; case 0 also starts
    from an accumulator at infinity.  Bases are canonical or, every other one, their representative above p."""
    p = f.p
    rnd = random.Random("%s/mul2-chain" % f.name)
    cases = []
    for k in range(CASES):
        if k == 0:
            acc, cur = (0, 0, 0, 0), None
        else:
            cur = mc.random_point(p, b, rnd)
            acc = start_acc(f, cur, z_of(f, Z_INDEX.get(f.name, {}).get(k, k)), bool(k & 1))
        start = cur
        bases, after = [], []
        for s in range(STEPS):
            if s in (7, 24):
                q = None
            elif s == 15:
                q = cur
            elif s == 23:
                q = (cur[0], (-cur[1]) % p)
            else:
                q = mc.random_point(p, b, rnd)
            bases.append((0, 0) if q is None else (mont(f, q[0], s & 1), mont(f, q[1], s & 2)))
            cur = mc.affine_add(p, cur, q)
            after.append(cur)
        assert after[23] is None and after[24] is None and after[25] is not None and after[14] is not None
        cases.append((acc, bases, after, start))
    return cases


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_mixed_add_chain(shim, curve):
    cid, fname, b = CURVES[curve]
    f = mc.FIELDS[fname]
    p, nb = f.p, 4 * f.N
    cases = chain_cases(f, b)
    st, got = shim.chain_status(cid, nb, [c[0] for c in cases], [c[1] for c in cases], STEPS)
    if shim.variant == "noasm" and f.N > 8:                    # that build leaves the 12-limb chain out (chain_built)
        assert st == -ds.HIP_NOT_SUPPORTED
        return
    ds.check(st, "dshim_madd_chain(%s)" % curve)
    model = mc.LazyModel(f)
    for k, ((acc, bases, after, _start), steps) in enumerate(zip(cases, got)):
        for s, (raw, want) in enumerate(zip(steps, after)):
            what = "%s/%s case %d step %d" % (shim.variant, curve, k, s)
            assert all(v < f.B for v in raw), what
            x, y, zz, zzz = raw
            if want is None:
                assert zz % p == 0, what
            else:
                assert zz % p and (zz ** 3 - zzz ** 2 * f.R) % p == 0, what          # Montgomery values: zz^3 = zzz^2
                assert (x * pow(zz, -1, p) % p, y * pow(zzz, -1, p) % p) == want, what
            if shim.variant == "asm":
                acc = model.madd(acc, bases[s])
                assert raw == acc, what + ": the registers differ from the integer model of the lazy arithmetic"
    if shim.variant == "asm":
        print("%s: %d of %d fused values arrived in the corrected range" % (curve, model.corrected, CASES * STEPS))
        assert model.corrected >= len(Z_INDEX.get(fname, {})) and (model.corrected > 0) == mc.needs_correction(f)
