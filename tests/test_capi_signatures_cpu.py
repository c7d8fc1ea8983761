"""CPU, no built library: capi's signature table against include/hekaton.h - every declared function is in the table and
nothing else is, in the header's order, with as many argtypes as the declaration has parameters and the restype its return
type asks for (void: None, const char*: c_char_p, hk_status: ctypes' default int)."""
import ctypes as C
import os
import re

import pytest

from hekaton_system_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hekaton.h")
RESTYPES = {"void": None, "const char*": C.c_char_p, "hk_status": C.c_int}


def _declarations():
    """[(return type, name, number of parameters)] of every `type hk_name ( params ) ;` of the header, comments stripped."""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t]*?[\w*])\s+(hk_\w+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        out.append((" ".join(ret.replace("*", " * ").split()).replace(" *", "*"), name,
                    0 if params in ("", "void") else len(params.split(","))))
    return out


def test_header_parse():
    decls = _declarations()
    names = [n for _, n, _ in decls]
    assert len(decls) == 82 and len(set(names)) == 82
    assert {r for r, _, _ in decls} == set(RESTYPES)


def test_table_names_and_order():
    assert list(capi._SIGNATURES) == [n for _, n, _ in _declarations()]
    assert capi.EXPORTS == list(capi._SIGNATURES)


def test_arity_and_restype():
    for ret, name, n_params in _declarations():
        sig = capi._SIGNATURES[name]
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


def test_load_sets_every_signature(monkeypatch, tmp_path):
    lib = _load(monkeypatch, tmp_path, _Lib())
    for ret, name, n_params in _declarations():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n_params and fn.restype is RESTYPES[ret], name


def test_load_names_a_missing_symbol(monkeypatch, tmp_path):
    """A library that lacks a declared symbol is refused at load, by that symbol's name, and is not kept."""
    with pytest.raises(AttributeError, match="hk_vkd_tree"):
        _load(monkeypatch, tmp_path, _Lib(missing="hk_vkd_tree"))
    assert capi._lib is None
