"""CPU, no GPU: what hk_gt_check rests on and how it is bound.  The two gcd identities that make "cyclotomic, and
x^q == x^(t - 1)" the same as "order divides r"; the premise of every case of tests/gt_check_cases.py (so that a refusal on
the device is a refusal for the stated reason); GtField.in_gt - the plain x != 0 and x^r == 1 - giving the table's verdict;
and the companion header include/hekaton_gt.h against capi's second signature table and load()."""
import ctypes as C
import math
import os
import re

import pytest

from hekaton_system_amd import capi
from hekaton_system_amd.gt import GtField
from oracle.pyref import pairing
from oracle.pyref.params import CURVES
from tests import gt_check_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hekaton_gt.h")
RESTYPES = {"void": None, "const char*": C.c_char_p, "hk_status": C.c_int}


# ---- the arithmetic ------------------------------------------------------------------------------------------------------
def test_gcd_identity_bn254():
    cp, u = CURVES["bn254"], gc.curve_u("bn254")
    t1 = gc.trace_minus_one("bn254")
    assert t1 == 6 * u * u and cp.q + 1 - (t1 + 1) == cp.r                   # q + 1 - t = r: the curve has prime order
    assert cp.q - t1 == cp.r and gc.phi12(cp.q) % cp.r == 0
    assert math.gcd(gc.phi12(cp.q), cp.q - t1) == cp.r


def test_gcd_identity_bls12_381():
    cp, u = CURVES["bls12_381"], gc.curve_u("bls12_381")
    assert u < 0 and gc.trace_minus_one("bls12_381") == u
    assert cp.r == u ** 4 - u ** 2 + 1 and (u - 1) ** 2 % 3 == 0
    assert cp.q - u == cp.r * ((u - 1) ** 2 // 3)
    assert gc.phi12(cp.q) % cp.r == 0 and math.gcd(gc.phi12(cp.q), (u - 1) ** 2 // 3) == 1
    assert math.gcd(gc.phi12(cp.q), cp.q - u) == cp.r


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_the_device_chains_exponent_is_the_curves(cname):
    """pow_x raises to |u|: the generated TowerParams::X and its sign are the oracle's x, and the kernel picks BN254's
    t - 1 = 6 u^2 by TWIST_IS_D, which is set on BN254 alone."""
    T = pairing.tower(cname)
    hdr = open(os.path.join(ROOT, "hekaton_system_amd", "csrc", "hk_tower_params.h")).read()
    key = "HK_BN254_TW" if cname == "bn254" else "HK_BLS12_381_TW"
    m = re.search(r"#define %s_X\s+(0x[0-9a-fA-F]+)ull" % key, hdr)
    assert m and int(m.group(1), 16) == T.x
    m = re.search(r"#define %s_X_IS_NEGATIVE\s+(\d)" % key, hdr)
    assert m and bool(int(m.group(1))) == T.x_is_negative
    m = re.search(r"#define %s_TWIST_IS_D\s+(\d)" % key, hdr)
    assert m and bool(int(m.group(1))) == (cname == "bn254")


# ---- the cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_case_premises(cname):
    F, cp = GtField(cname), CURVES[cname]
    q, r = cp.q, cp.r
    c, g = gc.case(cname, "c"), gc.case(cname, "g")
    assert F.pow(c, gc.phi12(q)) == F.one                                  # cyclotomic ...
    assert F.pow(c, r) != F.one                                            # ... and not of order r
    assert F.pow(g, r) == F.one and g != F.one
    gcv = gc.case(cname, "g*c")
    assert F.pow(gcv, gc.phi12(q)) == F.one and F.pow(gcv, r) != F.one
    assert F.mul(gc.case(cname, "conj(g)"), g) == F.one
    assert F.mul(gc.case(cname, "-1"), gc.case(cname, "-1")) == F.one
    names = [nm for nm, _x, _w in gc.cases(cname)]
    assert len(set(names)) == len(names) == (13 if cname == "bls12_381" else 12)
    assert all(0 <= v < q for _nm, x, _w in gc.cases(cname) for v in x)   # canonical: the readers' form


def test_omega_premises():
    """omega satisfies the Frobenius equation in exact arithmetic and fails the cyclotomic one."""
    cname = "bls12_381"
    F, cp, u = GtField(cname), CURVES[cname], gc.curve_u(cname)
    q, w = cp.q, gc.omega(cname)
    assert w != 1 and pow(w, 3, q) == 1 and (u - 1) % 3 == 0 and (q - 1) % 3 == 0
    assert pow(w, q, q) == w == pow(w, u % 3, q) and u % 3 == 1           # omega^q = omega = omega^u
    x = gc.case(cname, "omega")
    assert x == gc.embed(F, w)
    assert F.pow(x, q) == x and F.mul(F.pow(x, -u), x) == F.one           # the same in Fq12: x^(-u) x = 1
    assert F.mul(F.pow(x, q ** 4), x) != F.pow(x, q ** 2)                  # condition 2 refuses it
    assert F.pow(x, cp.r) == x                                             # r = 1 mod 3


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_in_gt_gives_the_tables_verdicts(cname):
    want = [w for _nm, _x, w in gc.cases(cname)]
    assert list(gc.host_verdicts(cname)) == want, [nm for (nm, _x, w), h in zip(gc.cases(cname), gc.host_verdicts(cname)) if w != h]
    F = GtField(cname)
    assert F.in_gt(tuple(v + F.q for v in F.one)) and not F.in_gt([F.q] * 12)       # reduces what it is given


@pytest.mark.parametrize("cname", gc.CURVE_NAMES)
def test_the_conditions_agree_with_in_gt_on_the_cases(cname):
    """The device's route, in GtField integers: x != 0, x^(q^4) x == x^(q^2), x^q == x^(t - 1) (a negative exponent through the
    true inverse x^(Phi_12(q) - ...) is not available off the cyclotomic subgroup, so it is only evaluated where 2 holds)."""
    F, cp = GtField(cname), CURVES[cname]
    q, t1 = cp.q, gc.trace_minus_one(cname)
    for (nm, x, want) in gc.cases(cname):
        ok = any(x) and F.mul(F.pow(x, q ** 4), x) == F.pow(x, q ** 2)
        if ok:
            ok = F.pow(x, q) == F.pow(x, t1 % gc.phi12(q))
        assert bool(ok) == want, nm


# ---- the binding -----------------------------------------------------------------------------------------------------------
def _declarations():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t]*?[\w*])\s+(hk_\w+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        out.append((" ".join(ret.replace("*", " * ").split()).replace(" *", "*"), name,
                    0 if params in ("", "void") else len(params.split(","))))
    return out


def test_companion_header_declares_hk_gt_check():
    decls = _declarations()
    assert [n for _r, n, _p in decls] == ["hk_gt_check"]
    assert decls[0] == ("hk_status", "hk_gt_check", 4)
    text = open(HEADER).read()
    assert '#include "hekaton.h"' in text
    main = open(os.path.join(ROOT, "include", "hekaton.h")).read()
    assert "hk_gt_check" not in main and "hk_gt_check" not in capi._SIGNATURES


def test_second_table_matches_the_companion_header():
    assert list(capi._SIGNATURES_GT) == [n for _r, n, _p in _declarations()]
    for ret, name, n_params in _declarations():
        sig = capi._SIGNATURES_GT[name]
        argtypes, restype = (sig[0], sig[1]) if isinstance(sig, tuple) else (sig, C.c_int)
        assert len(argtypes) == n_params, name
        assert restype is RESTYPES[ret], name


class _Lib:
    """Stands in for what ctypes.CDLL returns: a library that has every symbol but `missing`."""

    def __init__(self, missing=None):
        self._missing = missing

    def __getattr__(self, name):
        if not name.startswith("hk_") or name == self._missing:
            raise AttributeError("undefined symbol: " + name)
        fn = type("fn", (), {"restype": C.c_int})()
        setattr(self, name, fn)
        return fn


def _load(monkeypatch, tmp_path, lib):
    path = tmp_path / "libhekaton.so"
    path.write_bytes(b"")
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", str(path))
    monkeypatch.setattr(C, "CDLL", lambda p: lib)
    return capi.load()


def test_load_sets_the_signature(monkeypatch, tmp_path):
    lib = _load(monkeypatch, tmp_path, _Lib())
    assert len(lib.hk_gt_check.argtypes) == 4 and lib.hk_gt_check.restype is C.c_int


def test_load_names_a_missing_hk_gt_check(monkeypatch, tmp_path):
    with pytest.raises(AttributeError, match="hk_gt_check"):
        _load(monkeypatch, tmp_path, _Lib(missing="hk_gt_check"))
    assert capi._lib is None


def test_wrapper_marshals_count_and_pointers():
    """Context.gt_check over a stub: n from the bytes or as given, NULL input at n = 0, one verdict byte per element."""
    import numpy as np
    seen = []

    class _Stub:
        def hk_gt_check(self, handle, gts, n, ok):
            seen.append((handle, gts if gts is None else gts.value, n, ok))
            C.memset(ok, 1, n)
            return capi.HK_OK

    ctx = object.__new__(capi.Context)
    ctx.lib, ctx.handle, ctx.gt_bytes = _Stub(), 77, 384
    gts = np.zeros(3 * 384, np.uint8)
    assert ctx.gt_check(gts).tolist() == [1, 1, 1] and seen[-1][:3] == (77, gts.ctypes.data, 3)
    assert ctx.gt_check(gts, n=2).tolist() == [1, 1] and seen[-1][:3] == (77, gts.ctypes.data, 2)
    assert ctx.gt_check(np.zeros(0, np.uint8)).shape == (0,) and seen[-1][1:3] == (None, 0)


def test_the_built_library_exports_it():
    assert getattr(capi.load(), "hk_gt_check") is not None
