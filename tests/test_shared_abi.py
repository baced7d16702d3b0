"""CPU checks of the shared-prefix entry points (gear_attn_decode_shared / gear_attn_decode_shared_workspace): they are in the ctypes
table and exported, the ABI version did not move, the workspace grows with the number of sequences, and every argument error
surfaces as a status < 0 with a message before anything is launched (the device pointers below are never dereferenced)."""
import ctypes

from gear_amd import _lib


def _view(B=1, Hkv=2, tcap=256, wcap=64, bits=2, group=64, rk=8, rv=8):
    v = _lib.CacheView()
    v.B, v.Hkv, v.D, v.tcap, v.wcap = B, Hkv, 128, tcap, wcap
    v.ldk, v.lsk, v.group, v.bits, v.mode = tcap // (32 // bits), tcap // group, group, bits, 0
    v.rk, v.rv = rk, rv
    return v


def _call(prefix, tail, Tp=128, T=0, W=1, Hq=4, ws=4096, ws_bytes=1 << 40):
    lib = _lib.load()
    fake = 4096
    p = ctypes.byref(prefix) if prefix is not None else None
    t = ctypes.byref(tail) if tail is not None else None
    return lib.gear_attn_decode_shared(p, Tp, t, T, W, fake, Hq, 0.088, fake, None, ws, ws_bytes, None)


def test_shared_entries_are_bound_and_exported():
    for name in ("gear_attn_decode_shared", "gear_attn_decode_shared_workspace"):
        assert name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    lib = _lib.load()
    assert lib.gear_abi_version() == _lib.ABI_VERSION == 5


def test_shared_workspace_is_positive_and_monotone():
    lib = _lib.load()
    w = lib.gear_attn_decode_shared_workspace
    by_s = [w(S, 32, 4096, 64, 2) for S in (1, 2, 3, 4, 8, 16)]
    assert by_s[0] > 0 and all(a < b for a, b in zip(by_s, by_s[1:]))
    by_tp = [w(4, 32, Tp, 64, 2) for Tp in (64, 1024, 4096, 8192, 16384)]
    assert by_tp[0] > 0 and all(a <= b for a, b in zip(by_tp, by_tp[1:]))
    assert w(0, 32, 4096, 64, 2) == 0 and w(4, 32, 0, 64, 2) == 0
    # it covers the partial slots of both dispatches
    assert w(4, 32, 4096, 64, 2) >= lib.gear_attn_decode_workspace(1, 4 * 32, 4096, 2) + lib.gear_attn_decode_workspace(4, 32, 64, 2)


def test_shared_argument_errors_without_gpu():
    lib = _lib.load()
    err = lib.gear_last_error
    pre, tail = _view(B=1), _view(B=4)
    assert _call(None, tail) < 0 and b"null cache view" in err()
    assert _call(pre, None) < 0 and b"null cache view" in err()
    assert _call(_view(B=2), tail) < 0 and b"B == 1" in err()
    for kw in (dict(Hkv=4), dict(bits=4), dict(group=32), dict(rk=4), dict(rv=4)):
        assert _call(pre, _view(B=4, **kw)) < 0 and b"disagree" in err(), kw
    bad = _view(B=4)
    bad.D = 64
    assert _call(pre, bad) < 0 and b"disagree" in err()
    bad = _view(B=4)
    bad.mode = 1
    assert _call(pre, bad) < 0 and b"disagree" in err()
    for Tp in (0, -64, 100, 320):                           # not positive, not a multiple of 64, past tcap = 256
        assert _call(pre, tail, Tp=Tp) < 0 and b"Tp = " in err(), Tp
    assert _call(pre, tail, T=100) < 0 and b"T = 100" in err() and b"multiple of 64" in err()
    assert _call(pre, tail, W=65) < 0 and b"wcap" in err()
    assert _call(pre, tail, Hq=3) < 0 and b"multiple of Hkv" in err()
    assert _call(pre, tail, ws=None, ws_bytes=0) < 0 and b"workspace" in err()
    assert _call(pre, tail, ws=4096, ws_bytes=64) < 0 and b"workspace" in err()
    assert _call(pre, _view(B=4096), Hq=32) < 0 and b"query rows" in err()
