"""CPU checks of the entry points of csrc/logits.hip: both are in the ctypes table, declared in the header and exported; every
refusal the header lists returns a status < 0 with a message before any launch (no GPU here: a launch would fail differently), and
a call with no rows returns 0."""
import ctypes
import os

import pytest

from conftest import ROOT
from gear_amd import _lib

P = 0x1000          # a non-null pointer the refused calls never touch


def _params(penalty=1.3, ngram=0, min_new=0, n_eos=0, n_bias=0, bias=None):
    return _lib.LogitsParamsC(penalty, ngram, min_new, n_eos, (ctypes.c_int * 8)(), n_bias, 0, bias)


def _call(logits=P, out=P, B=2, V=100, ld=100, ld_out=100, hist=P, hist_cap=16, pos0=4, params=None, null_params=False):
    p = params if params is not None else _params()
    return _lib.load().gear_logits_process(logits, out, 0, B, V, ld, ld_out, hist, hist_cap, None, pos0, None, 0,
                                           None if null_params else ctypes.byref(p), None)


def test_bound_declared_exported():
    header = open(os.path.join(ROOT, "include", "gear_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, decl in (("gear_logits_process", "int gear_logits_process(const void* logits, void* out, int logits_fp32, int B, int V"),
                       ("gear_eos_update", "int gear_eos_update(int64_t* tok, int32_t* done, int B, const int* eos, int n_eos")):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and decl in header
    assert len(_lib.SIGNATURES["gear_logits_process"][1]) == 15 and len(_lib.SIGNATURES["gear_eos_update"][1]) == 8
    assert "gear_logits_params;" in header and ctypes.sizeof(_lib.LogitsParamsC) == 64
    assert _lib.load().gear_abi_version() == _lib.ABI_VERSION


REFUSED = [
    ("null logits", dict(logits=None), b"null"),
    ("null out", dict(out=None), b"null"),
    ("null hist", dict(hist=None), b"null"),
    ("null params", dict(null_params=True), b"null params"),
    ("V = 0", dict(V=0, ld=0, ld_out=0), b"V = 0"),
    ("V < 0", dict(V=-5), b"V = -5"),
    ("V too large", dict(V=262145, ld=262145, ld_out=262145), b"V = 262145"),
    ("ld < V", dict(ld=99), b"pitch"),
    ("ld_out < V", dict(ld_out=99), b"pitch"),
    ("B < 0", dict(B=-1), b"B = -1"),
    ("penalty 0", dict(params=_params(penalty=0.0)), b"repetition_penalty"),
    ("penalty < 0", dict(params=_params(penalty=-1.5)), b"repetition_penalty"),
    ("penalty NaN", dict(params=_params(penalty=float("nan"))), b"repetition_penalty"),
    ("ngram < 0", dict(params=_params(ngram=-1)), b"no_repeat_ngram"),
    ("min_new < 0", dict(params=_params(min_new=-1)), b"min_new_tokens"),
    ("n_eos 9", dict(params=_params(n_eos=9)), b"n_eos = 9"),
    ("n_eos < 0", dict(params=_params(n_eos=-1)), b"n_eos = -1"),
    ("n_bias < 0", dict(params=_params(n_bias=-1)), b"n_bias = -1"),
    ("n_bias with a null table", dict(params=_params(n_bias=3)), b"null bias table"),
    ("pos0 < 0", dict(pos0=-1), b"pos0 = -1"),
    ("hist_cap 0", dict(hist_cap=0), b"hist_cap = 0"),
    ("hist_cap < 0", dict(hist_cap=-4), b"hist_cap = -4"),
]


@pytest.mark.parametrize("what,kw,msg", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
def test_process_refusals(what, kw, msg):
    lib = _lib.load()
    assert _call(B=0) == 0                                   # (clears nothing, launches nothing)
    rc = _call(**kw)
    assert rc < 0, what
    assert msg in lib.gear_last_error(), (what, lib.gear_last_error())


def test_no_rows_is_no_launch():
    assert _call(B=0) == 0
    assert _lib.load().gear_eos_update(P, P, 0, None, 0, 0, P, None) == 0


def test_eos_update_refusals():
    lib = _lib.load()
    ids = (ctypes.c_int * 8)(1, 2)
    for args, msg in (((None, P, 2, ids, 2, 0, P, None), b"null"), ((P, None, 2, ids, 2, 0, P, None), b"null"),
                      ((P, P, 2, ids, 2, 0, None, None), b"null"), ((P, P, -1, ids, 2, 0, P, None), b"B = -1"),
                      ((P, P, 2, ids, 9, 0, P, None), b"n_eos = 9"), ((P, P, 2, ids, -1, 0, P, None), b"n_eos = -1"),
                      ((P, P, 2, None, 2, 0, P, None), b"null ids")):
        rc = lib.gear_eos_update(*args)
        assert rc < 0 and msg in lib.gear_last_error(), (args, lib.gear_last_error())
