"""CPU checks of the shared-prefix chunk-attention entry points (gear_attn_extend_shared / gear_attn_extend_shared_workspace): they
are in the ctypes table and exported, the ABI version did not move, the workspace is 0 for invalid shapes and grows with the number
of sequences, the chunk and the prefix, and every argument error surfaces as a status < 0 with a message before anything is launched
(the device pointers below are never dereferenced)."""
import ctypes

from gear_amd import _lib

FAKE = 4096


def _view(B=1, Hkv=2, tcap=256, wcap=64, bits=2, group=64, rk=8, rv=8):
    v = _lib.CacheView()
    v.B, v.Hkv, v.D, v.tcap, v.wcap = B, Hkv, 128, tcap, wcap
    v.ldk, v.lsk, v.group, v.bits, v.mode = tcap // (32 // bits), tcap // group, group, bits, 0
    v.rk, v.rv = rk, rv
    for name in ("kcode", "kscale", "kmn", "vcode", "vscale", "vmn", "kP", "kQ", "vP", "vQ", "kwin", "vwin"):
        setattr(v, name, FAKE)
    return v


def _call(prefix, tail, Tp=128, T=0, W=1, Hq=4, n=3, q=FAKE, k=FAKE, v=FAKE, out=FAKE, ws=FAKE, ws_bytes=1 << 40):
    lib = _lib.load()
    p = ctypes.byref(prefix) if prefix is not None else None
    t = ctypes.byref(tail) if tail is not None else None
    return lib.gear_attn_extend_shared(p, Tp, t, T, W, q, Hq, n, k, v, 0.088, out, None, ws, ws_bytes, None)


def test_extend_shared_entries_are_bound_and_exported():
    for name in ("gear_attn_extend_shared", "gear_attn_extend_shared_workspace"):
        assert name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    lib = _lib.load()
    assert lib.gear_abi_version() == _lib.ABI_VERSION == 5


def test_extend_shared_workspace_is_zero_positive_and_monotone():
    lib = _lib.load()
    w = lib.gear_attn_extend_shared_workspace
    for bad in ((0, 32, 64, 4096, 64, 32), (4, 0, 64, 4096, 64, 32), (4, 32, 0, 4096, 64, 32), (4, 32, 64, 0, 64, 32),
                (4, 32, 64, 4096, -64, 32), (4, 32, 64, 4096, 64, -1), (-1, 32, 64, 4096, 64, 32)):
        assert w(*bad) == 0, bad
    by_s = [w(S, 32, 64, 4096, 64, 32) for S in (1, 2, 3, 4, 8, 16)]
    assert by_s[0] > 0 and all(a < b for a, b in zip(by_s, by_s[1:]))
    by_n = [w(4, 32, n, 4096, 64, 32) for n in (1, 7, 16, 64, 256, 2048)]
    assert by_n[0] > 0 and all(a < b for a, b in zip(by_n, by_n[1:]))
    by_tp = [w(4, 32, 16, Tp, 64, 32) for Tp in (64, 128, 1024, 4096, 16384)]
    assert by_tp[0] > 0 and all(a <= b for a, b in zip(by_tp, by_tp[1:])) and by_tp[0] < by_tp[-1]
    # it covers the tail pass's slots (the plain chunk call over the batch-S tails) and the prefix pass's on top
    assert w(4, 32, 64, 4096, 64, 32) > lib.gear_attn_extend_workspace(4, 32, 64, 64, 32)


def test_extend_shared_argument_errors_without_gpu():
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
    assert _call(pre, tail, T=320) < 0 and b"T = 320" in err()
    assert _call(pre, tail, T=-64) < 0 and b"T = -64" in err()
    for W in (-1, 65):
        assert _call(pre, tail, W=W) < 0 and b"wcap" in err(), W
    for n in (0, -1, 2049):
        assert _call(pre, tail, n=n) < 0 and b"n = " in err() and b"[1, 2048]" in err(), n
    big = _view(B=1, tcap=65536), _view(B=4, tcap=65536)
    assert _call(*big, Tp=64000, T=1472, W=60, n=4) < 0 and b"positions" in err()         # 65536 positions
    assert _call(pre, _view(B=40000), Hq=2) < 0 and b"at most 65535" in err()             # S Hkv = 80000
    assert _call(pre, tail, Hq=3) < 0 and b"multiple of Hkv" in err()
    assert _call(pre, tail, Hq=0) < 0 and b"multiple of Hkv" in err()
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(out=None)):
        assert _call(pre, tail, **kw) < 0 and b"null q / k_new / v_new / out" in err(), kw
    nowin = _view(B=4)
    nowin.kwin = None
    assert _call(pre, nowin, W=1) < 0 and b"window tensors" in err()
    nopay = _view(B=1)
    nopay.kcode = None
    assert _call(nopay, tail) < 0 and b"quantized payload" in err()
    assert _call(pre, tail, ws=None, ws_bytes=0) < 0 and b"workspace" in err()
    assert _call(pre, tail, ws=FAKE, ws_bytes=64) < 0 and b"workspace" in err()
    need = lib.gear_attn_extend_shared_workspace(4, 4, 3, 128, 0, 1)
    assert _call(pre, tail, ws=FAKE, ws_bytes=need // 64) < 0 and b"gear_attn_extend_shared_workspace" in err()
