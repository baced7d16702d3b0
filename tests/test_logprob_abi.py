"""CPU checks of the scoring entry point gear_token_logprobs: it is in the ctypes table, declared in the header and exported, the
ABI version is unchanged, and every argument error comes back as a status < 0 with its message before anything is launched."""
import ctypes
import os

from gear_amd import _lib

FAKE = 4096            # never dereferenced: every failing case fails its argument check first, N == 0 returns before a launch


def _call(logits=FAKE, ref=None, ids=FAKE, N=4, V=1000, ld=None, k_top=0, lp=FAKE, lse=None, rank=None, kl=None, agree=None,
          top_idx=None, top_lp=None):
    lib = _lib.load()
    return lib.gear_token_logprobs(logits, ref, ids, N, V, V if ld is None else ld, k_top, lp, lse, rank, kl, agree, top_idx,
                                   top_lp, None)


def test_logprob_entry_is_bound_declared_and_exported():
    assert "gear_token_logprobs" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["gear_token_logprobs"]
    assert res is ctypes.c_int and len(args) == 15
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "gear_token_logprobs")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gear_hip.h")).read()
    assert "int gear_token_logprobs(const void* logits, const void* ref_logits, const int64_t* ids, int64_t N, int V" in header


def test_abi_version_is_still_5():
    assert _lib.ABI_VERSION == 5 and _lib.load().gear_abi_version() == 5


def test_logprob_argument_errors_without_gpu():
    lib = _lib.load()
    for kw in (dict(logits=None), dict(ids=None), dict(lp=None)):
        assert _call(**kw) < 0 and b"null logits / ids / lp" in lib.gear_last_error(), kw
    for V in (0, -3):
        assert _call(V=V) < 0 and b"V = " in lib.gear_last_error()
    assert _call(N=-1) < 0 and b"N = -1" in lib.gear_last_error()
    assert _call(N=2 ** 31) < 0 and b"N = " in lib.gear_last_error()
    assert _call(V=1000, ld=999) < 0 and b"ld = 999 < V = 1000" in lib.gear_last_error()
    for k in (-1, 9):
        assert _call(k_top=k, top_idx=FAKE, top_lp=FAKE) < 0 and b"k_top = " in lib.gear_last_error()
    assert _call(V=7, k_top=8, top_idx=FAKE, top_lp=FAKE) < 0 and b"k_top = 8 > V = 7" in lib.gear_last_error()
    assert _call(kl=FAKE) < 0 and b"without ref_logits" in lib.gear_last_error()
    assert _call(agree=FAKE) < 0 and b"without ref_logits" in lib.gear_last_error()


def test_logprob_zero_rows_return_0_without_a_launch():
    assert _call(N=0) == 0
    assert _call(N=0, ref=FAKE, kl=FAKE, agree=FAKE, k_top=8, top_idx=FAKE, top_lp=FAKE, lse=FAKE, rank=FAKE) == 0
    # the argument checks still come first
    assert _call(N=0, V=0) < 0


def test_python_wrapper_refuses_cpu_tensors():
    import pytest
    import torch
    from gear_amd.scoring import token_logprobs
    with pytest.raises(_lib.GearError, match="GPU only"):
        token_logprobs(torch.zeros(2, 8, dtype=torch.float16), torch.zeros(2, dtype=torch.int64))
