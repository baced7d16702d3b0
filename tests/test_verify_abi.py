"""CPU checks of the speculative-verify entry points (gear_attn_verify_cache / gear_attn_verify_workspace): they are in the ctypes
table and exported, the workspace grows with the draft size, and argument errors surface as a status < 0 with a message before
anything is launched."""
import ctypes

from gear_amd import _lib


def _view(Hkv=2, tcap=128, wcap=64):
    v = _lib.CacheView()
    v.B, v.Hkv, v.D, v.tcap, v.wcap = 1, Hkv, 128, tcap, wcap
    v.ldk, v.lsk, v.group, v.bits, v.mode = tcap // 16, tcap // 64, 64, 2, 0
    return v


def _call(v, Hq=4, n=4, T=0, W=0, ws=None, ws_bytes=0):
    lib = _lib.load()
    fake = 4096            # never dereferenced: every case below fails its argument check first
    return lib.gear_attn_verify_cache(ctypes.byref(v), fake, Hq, n, T, W, fake, fake, 0.088, fake, None, ws, ws_bytes, None)


def test_verify_entries_are_bound_and_exported():
    for name in ("gear_attn_verify_cache", "gear_attn_verify_workspace"):
        assert name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    lib = _lib.load()
    assert lib.gear_abi_version() == _lib.ABI_VERSION == 5
    sizes = [lib.gear_attn_verify_workspace(1, 32, n, 4096, 10) for n in (1, 2, 4, 8, 16)]
    assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3] < sizes[4]
    assert lib.gear_attn_verify_workspace(1, 32, 0, 4096, 10) == 0


def test_verify_argument_errors_without_gpu():
    lib = _lib.load()
    v = _view()
    for n in (0, 17):
        assert _call(v, n=n) < 0 and b"n = " in lib.gear_last_error()
    assert b"gear_attn_extend_cache" in lib.gear_last_error()          # the message points to the chunk path
    assert _call(v, Hq=3) < 0 and b"multiple of Hkv" in lib.gear_last_error()
    assert _call(v, W=65) < 0 and b"wcap" in lib.gear_last_error()
    assert _call(v, T=100) < 0 and b"multiple of 64" in lib.gear_last_error()
    assert _call(v, ws=None, ws_bytes=0) < 0 and b"workspace" in lib.gear_last_error()
    assert _call(v, ws=4096, ws_bytes=64) < 0 and b"workspace" in lib.gear_last_error()
    bad = _view()
    bad.D = 64
    assert _call(bad) < 0 and b"head_dim" in lib.gear_last_error()
    assert lib.gear_attn_verify_cache(None, None, 4, 4, 0, 0, None, None, 1.0, None, None, None, 0, None) < 0
    assert b"null cache view" in lib.gear_last_error()
