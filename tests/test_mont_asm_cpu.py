"""CPU: the generated inline assembly of csrc/mont_asm.h, interpreted on Python integers (tests/asm_interp.py) over the
operand sets of tests/field_edges.py - the text the device build of field.cuh runs and no host-compiled test reaches.

  * values: MONT = a b R^-1 (mod p) and < 2p; ADD / SUB / DBL congruent and below the representative bound B;
    RED subtracts B exactly when t >= B; CANON gives a mod p exactly (lazy fields);
  * carry coverage: every VCC consumer (v_addc / v_subb / v_cndmask) sees both VCC states somewhere in the set, except
    the instructions of EXCLUDED, each of which cannot see a carry-in by a bound that column_bounds() recomputes;
  * sharpness: three textual mutations per field (a dropped third-word carry, a v_cndmask with its data operands
    swapped, a wrong modulus limb) are each rejected by the value checks;
  * the generated headers regenerate byte for byte.
"""
import os
import re
import subprocess
import sys

import pytest

from tests import asm_interp as ai
from tests import field_edges as fe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hekaton_system_amd", "csrc")
M32 = 0xFFFFFFFF
FIELD_NAMES = list(fe.FIELDS)


def header_text():
    with open(os.path.join(CSRC, "mont_asm.h"), encoding="utf-8") as fh:
        return fh.read()


def kinds_of(f):
    return ["MONT", "ADD", "SUB", "DBL", "RED"] + (["CANON"] if f.lazy else [])


_limbs = {}


def limbs(x, n):
    v = _limbs.get((x, n))
    if v is None:
        v = _limbs[(x, n)] = fe.to_limbs(x, n)
    return v


def run_kind(blocks, f, kind, stop_at_first=False):
    """-> (mismatches [(a, b, got)], cov) of one block over its operand set."""
    blk = blocks[(kind, f.name)]
    fn = blk.compile()
    cov = [0] * len(blk.instrs)
    p, B, N = f.p, f.B, f.N
    pairs = fe.pair_list(f)
    if kind == "MONT":
        cases = ((a, b, lambda r, a=a, b=b: r < 2 * p and (r - a * b * f.Rinv) % p == 0) for a, b in pairs)
    elif kind == "ADD":
        cases = ((a, b, lambda r, a=a, b=b: r < B and (r - a - b) % p == 0) for a, b in pairs)
    elif kind == "SUB":
        cases = ((a, b, lambda r, a=a, b=b: r < B and (r - a + b) % p == 0) for a, b in pairs)
    else:
        singles = fe.all_values(f) + [a for a, _b in pairs[-512:]]
        if kind == "DBL":
            cases = ((a, 0, lambda r, a=a: r < B and (r - 2 * a) % p == 0) for a in singles)
        elif kind == "RED":                       # t in [0, 2B) and below R: the sums the reduction is applied to
            ts = fe._dedup(singles + [a + B for a in singles] + [a + b for a, b in pairs[:2048]])
            ts = [t for t in ts if t < min(2 * B, f.R)]
            cases = ((t, 0, lambda r, t=t: r == (t - B if t >= B else t)) for t in ts)
        elif kind == "CANON":
            cases = ((a, 0, lambda r, a=a: r == a % p) for a in singles)
        else:
            raise AssertionError(kind)
    bad = []
    zero = limbs(0, N)
    for a, b, ok in cases:
        r = fe.from_limbs(fn(limbs(a, N), limbs(b, N) if "b" in blk.params else zero, cov))
        if not ok(r):
            bad.append((a, b, r))
            if stop_at_first:
                break
    return bad, cov


def rejected(text, f, kind):
    """"value" when the value checks reject the header text for this block, "static" when the interpreter's checks do
    before any operand runs, None when the text passes."""
    try:
        bad, _cov = run_kind(ai.parse_header(text), f, kind, stop_at_first=True)
    except ai.AsmError:
        return "static"
    return "value" if bad else None


@pytest.fixture(scope="module")
def blocks():
    return ai.parse_header(header_text())


@pytest.fixture(scope="module")
def results(blocks):
    """(field, kind) -> (mismatches, coverage), computed once for the value and the coverage tests."""
    return {(name, kind): run_kind(blocks, f, kind) for name, f in fe.FIELDS.items() for kind in kinds_of(f)}


def test_every_macro_of_the_header_is_known(blocks):
    want = {(kind, name) for name, f in fe.FIELDS.items() for kind in kinds_of(f)}
    assert set(blocks) == want          # a new macro kind has to get its check here


def test_operand_sets_respect_the_bound():
    for f in fe.FIELDS.values():
        pairs = fe.pair_list(f)
        assert all(0 <= a < f.B and 0 <= b < f.B for a, b in pairs)
        assert len(pairs) >= 4096 + len(fe.structured_values(f)) ** 2
        for a, b in fe.fp2_pair_list(f):
            assert all(0 <= c < f.B for c in a + b)
        assert pairs == fe.pair_list(f)                                   # deterministic


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_values(name, results):
    f = fe.FIELDS[name]
    for kind in kinds_of(f):
        bad, _cov = results[(name, kind)]
        assert not bad, "%s %s: %d mismatches, first a=%#x b=%#x got=%#x" % ((name, kind, len(bad)) + bad[0])


# ---- carry coverage ------------------------------------------------------------------------------------------
# Instructions that never see VCC = 1 in the operand set, keyed by (field, kind, instruction index), with the bound
# argument why a carry-in cannot occur.  All of them are third-word carries (v_addc after a v_mad_u64_u32) of a MONT
# block: the v_mad carries out only when the low 64 bits of the column accumulator plus the product reach 2^64, and
# column_bounds() below recomputes for every entry an upper bound of that sum which stays under 2^64.
FIRST = "first product of the block: the addend is the constant 0 and a 32x32 product is < 2^64"
COL1 = ("first product of column 1: column 0 is a0 b0 + m0 p0 <= 2^65 - 2^34 + 2, so the accumulator carried in is "
        "<= 2^33 - 4 and the sum with a product <= 2^64 - 2^33 + 1 stays <= 2^64 - 3")
M0P0 = "p[0] = 1 in this field: a0 b0 + m0 p0 <= (2^64 - 2^33 + 1) + (2^32 - 1) < 2^64"
TOP = ("every product of the column up to here has a top-limb factor (a[N-1], b[N-1] <= top limb of B, or p[N-1]): "
       "their sum plus the carried-in accumulator (< 2^37) is < 2^64")


def _excl(first, col1, top, m0p0=()):
    d = {i: FIRST for i in first}
    d.update({i: COL1 for i in col1})
    d.update({i: M0P0 for i in m0p0})
    d.update({i: TOP for i in top})
    return d


_BN254 = _excl([10], [16], [136, 138, 170, 172, 200, 202, 226, 228, 248, 250, 266, 268, 280, 282, 284, 290, 292])
EXCLUDED = {}
for _name, _d in (
        ("BN254_FR", _BN254),
        ("BN254_FQ", _BN254),
        # (284 fires here: a[7] b[6] follows two products bounded by the larger top limb of this p)
        ("BLS12_381_FR", _excl([10], [16], [136, 138, 170, 172, 200, 202, 226, 228, 248, 250, 266, 268, 280, 282, 290, 292],
                               m0p0=[13])),
        ("BLS12_381_FQ", _excl([14], [20], [300, 302, 350, 352, 396, 398, 438, 440, 476, 478, 510, 512, 540, 542, 566, 568,
                                            588, 590, 606, 608, 620, 622, 624, 626, 630, 632]))):
    for _i, _why in _d.items():
        EXCLUDED[(_name, "MONT", _i)] = _why
EXCLUSION_CAPS = {"BN254_FR": 19, "BN254_FQ": 19, "BLS12_381_FR": 26, "BLS12_381_FQ": 28}


def column_bounds(blk, f):
    """Upper bound of (column accumulator + product) at every v_mad_u64_u32 of a MONT block, keyed by the index of the
    v_addc that consumes its carry: below 2^64 it rules a carry out.  Operand limbs are bounded by 2^32 - 1, the top
    limb of an input by the top limb of B - 1 (inputs are < B), a modulus limb by its literal; a column starts from the
    previous column's bound shifted down by one word (the v_mov between the two accumulator pairs)."""
    top = (f.B - 1) >> (32 * (f.N - 1))
    nout = len(blk.outs)
    mx = {}
    for k, (con, var) in enumerate(blk.outs):
        e = blk.inits.get(var) if con.startswith("+") else None
        mx["%%%d" % k] = top if e and e.endswith("[%d]" % (f.N - 1)) else M32
    for k, (_con, e) in enumerate(blk.ins):
        mx["%%%d" % (nout + k)] = top if e.endswith("[%d]" % (f.N - 1)) else M32
    ub, out = 0, {}
    for i, text in enumerate(blk.instrs):
        mn, _, rest = text.partition(" ")
        ops = [o.strip() for o in rest.split(",")]
        if mn == "s_mov_b32":
            mx[ops[0]] = int(ops[1], 16)
        elif mn == "v_mad_u64_u32":
            prod = mx.get(ops[2], M32) * mx.get(ops[3], M32)
            ub = prod if ops[4] == "0" else ub + prod
            assert blk.instrs[i + 1].startswith("v_addc_co_u32")
            out[i + 1] = ub
        elif mn == "v_mov_b32":
            if re.fullmatch(r"v\d+", ops[0]) and re.fullmatch(r"v\d+", ops[1]):
                ub >>= 32                          # column shift: middle word -> low word of the other pair
            else:
                mx[ops[0]] = M32                   # a result word replaces the operand
    return out


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_carry_coverage(name, blocks, results):
    f = fe.FIELDS[name]
    mine = {k: why for k, why in EXCLUDED.items() if k[0] == name}
    assert len(mine) <= EXCLUSION_CAPS[name]
    assert all(k[1] == "MONT" for k in mine), "only the products may hold an excluded instruction"
    assert all(why and len(why.splitlines()) == 1 for why in mine.values())
    bounds = column_bounds(blocks[("MONT", name)], f)
    for (_n, _k, idx), why in mine.items():
        assert bounds[idx] < 1 << 64, "exclusion %d of %s has no bound: %s" % (idx, name, why)
    for kind in kinds_of(f):
        blk = blocks[(kind, name)]
        _bad, cov = results[(name, kind)]
        consumers = blk.vcc_consumers()
        cold = [i for i in consumers if cov[i] != 3 and (name, kind, i) not in EXCLUDED]
        stale = [i for i in consumers if cov[i] == 3 and (name, kind, i) in EXCLUDED]
        assert not cold, "%s %s: VCC consumers that saw one state only: %s" % (
            name, kind, [(i, blk.instrs[i], cov[i]) for i in cold])
        assert not stale, "%s %s: excluded instructions that do fire: %s" % (name, kind, stale)
        assert all(k[2] in consumers for k in mine if k[1] == kind)
        print("%s %s: %d VCC consumers, %d in both states, %d excluded" % (
            name, kind, len(consumers), sum(cov[i] == 3 for i in consumers),
            sum((name, kind, i) in EXCLUDED for i in consumers)))


# ---- sharpness -----------------------------------------------------------------------------------------------
def _macro_span(text, kind, name):
    start = text.index("#define HK_%s_ASM_%s(" % (kind, name))
    return start, text.index("} while (0)", start)


def _mutate(text, kind, name, edit):
    start, end = _macro_span(text, kind, name)
    body = edit(text[start:end])
    assert body != text[start:end]
    return text[:start] + body + text[end:]


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_mutations_are_rejected(name, blocks, results):
    f = fe.FIELDS[name]
    text = header_text()
    assert rejected(text, f, "ADD") is None                                 # the unmutated text passes the same gate

    # 1. drop one third-word v_addc of a middle column of MONT (one whose carry-in the operand set does fire)
    blk = blocks[("MONT", name)]
    _bad, cov = results[(name, "MONT")]
    third = [i for i in blk.vcc_consumers() if re.fullmatch(r"v_addc_co_u32 (v\d+), vcc, 0, \1, vcc", blk.instrs[i])
             and cov[i] == 3]
    victim = min(third, key=lambda i: abs(i - len(blk.instrs) // 2))
    nth = sum(1 for i in range(victim) if blk.instrs[i] == blk.instrs[victim])

    def drop(body):
        pat = blk.instrs[victim] + "\\n\\t"
        pos = -1
        for _ in range(nth + 1):
            pos = body.index(pat, pos + 1)
        return body[:pos] + body[pos + len(pat):]
    mutated = _mutate(text, "MONT", name, drop)
    assert len(ai.parse_header(mutated)[("MONT", name)].instrs) == len(blk.instrs) - 1
    assert rejected(mutated, f, "MONT") == "value"

    # 2. swap the two data operands of one v_cndmask of ADD
    def swap(body):
        return re.sub(r"v_cndmask_b32 (%\d+), (v\d+), (%\d+), vcc", r"v_cndmask_b32 \1, \3, \2, vcc", body, count=1)
    assert rejected(_mutate(text, "ADD", name, swap), f, "ADD") == "value"

    # 3. change one modulus limb literal of SUB
    def limb(body):
        m = list(re.finditer(r"s_mov_b32 s\d+, 0x([0-9a-f]{8})", body))[f.N // 2]
        return body[:m.start(1)] + "%08x" % (int(m.group(1), 16) ^ 0x00010000) + body[m.end(1):]
    assert rejected(_mutate(text, "SUB", name, limb), f, "SUB") == "value"


def test_the_interpreter_rejects_what_it_does_not_know():
    text = header_text()
    with pytest.raises(ai.AsmError, match="unknown mnemonic"):
        ai.parse_header(text.replace("v_and_b32", "v_or_b32"))[("SUB", "BN254_FR")].compile()
    # the tied form without its initialisers reads registers that were never written
    start, end = _macro_span(text, "MONT", "BLS12_381_FQ")
    untied = text[:start] + re.sub(r"(t\d+) = a\.v\[\d+\]", r"\1", text[start:end]) + text[end:]
    with pytest.raises(ai.AsmError, match="no initialiser"):
        ai.parse_header(untied)[("MONT", "BLS12_381_FQ")].compile()
    with pytest.raises(ai.AsmError, match="read before"):
        ai.parse_header(text.replace("v_mov_b32 v10, 0x", "v_mov_b32 v30, 0x"))[("ADD", "BN254_FR")].compile()
    with pytest.raises(ai.AsmError, match="clobber"):
        ai.parse_header(text.replace('"vcc", "v4", "v5", "s64"', '"vcc", "v4", "s64"'))[("SUB", "BN254_FR")].compile()


# ---- reproducibility -----------------------------------------------------------------------------------------
# generator module -> (function, header it writes); called with a temporary path so that nothing in the tree is rewritten
# (run as a script, gen_tower_params.py writes hk_wave_f12.h next to itself)
GENERATED = [("gen_mont_asm", "main", "mont_asm.h"), ("gen_params", "main", "hk_params.h"),
             ("gen_tower_params", "main", "hk_tower_params.h"), ("gen_tower_params", "emit_wave", "hk_wave_f12.h")]


@pytest.mark.parametrize("module, func, header", GENERATED)
def test_generated_header_regenerates_byte_for_byte(module, func, header, tmp_path):
    out = tmp_path / header
    code = "import sys; sys.path.insert(0, sys.argv[1]); import %s as g; g.%s(sys.argv[2])" % (module, func)
    subprocess.check_call([sys.executable, "-c", code, CSRC, str(out)], cwd=str(tmp_path))
    with open(os.path.join(CSRC, header), "rb") as fh:
        assert out.read_bytes() == fh.read(), "%s.%s no longer reproduces the committed %s" % (module, func, header)
