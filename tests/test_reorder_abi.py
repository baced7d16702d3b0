"""CPU checks of the beam-search gather (gear_cache_reorder / gear_cache_reorder_workspace): both are in the ctypes table and
exported, the ABI version did not move, the workspace is positive and monotone in batch, T, W and the number of layers, and every
argument error surfaces as a status < 0 with a message before anything is launched (the device pointers below are never
dereferenced)."""
import ctypes

from gear_amd import _lib

FAKE = 1 << 20       # a "device pointer": 16-byte aligned, never dereferenced


def _view(B=4, Hkv=2, tcap=512, wcap=64, bits=2, group=64, rk=4, rv=4, sparse=True):
    v = _lib.CacheView()
    v.B, v.Hkv, v.D, v.tcap, v.wcap = B, Hkv, 128, tcap, wcap
    v.ldk, v.lsk, v.group, v.bits, v.mode = tcap // (32 // bits), tcap // group, group, bits, 0
    v.rk, v.rv, v.seglen, v.seg0 = rk, rv, wcap, 128
    names = ["kcode", "kscale", "kmn", "vcode", "vscale", "vmn", "kwin", "vwin"]
    if rk:
        names += ["kP", "kQ", "vP", "vQ"]
    if sparse:
        v.kk0, v.kkb, v.kk_cap, v.kv, v.nbk_pitch = 5, 1, 5 + tcap // wcap, 5, tcap // 128 + 2
        v.nck, v.ktile_cap, v.nblk, v.vtile_cap = tcap // 128 + 1, 512, 2 * (tcap // 128 + 1), 256
        names += ["koidx", "koval", "kochunk", "voidx", "voval", "vochunk", "ktile", "kcnt", "vtile", "vcnt"]
    for i, n in enumerate(names):
        setattr(v, n, FAKE * (i + 1))
    return v


def _ws(v, n_layers=1, batch=4, T=256, W=17):
    return _lib.load().gear_cache_reorder_workspace(ctypes.byref(v), n_layers, batch, T, W)


def _call(v, n_layers=1, batch=4, T=256, W=17, idx=FAKE * 64, ws=FAKE * 65, ws_bytes=1 << 40):
    p = ctypes.byref(v) if v is not None else None
    return _lib.load().gear_cache_reorder(p, n_layers, batch, T, W, idx, ws, ws_bytes, None)


def test_reorder_entries_are_bound_and_exported():
    for name in ("gear_cache_reorder", "gear_cache_reorder_workspace"):
        assert name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    lib = _lib.load()
    assert lib.gear_abi_version() == _lib.ABI_VERSION == 5


def test_reorder_workspace_is_positive_and_monotone():
    for sparse, rk in ((True, 4), (False, 4), (False, 0)):
        mk = lambda B: _view(B=B, rk=rk, rv=rk, sparse=sparse)
        by_b = [_ws(mk(B), batch=B) for B in (1, 2, 3, 4, 5, 16)]
        assert by_b[0] > 0 and all(a < b for a, b in zip(by_b, by_b[1:])), by_b
        by_t = [_ws(mk(4), T=T) for T in (0, 64, 128, 192, 256, 512)]
        assert by_t[0] > 0 and all(a <= b for a, b in zip(by_t, by_t[1:])) and by_t[0] < by_t[-1], by_t
        by_w = [_ws(mk(4), W=W) for W in (0, 1, 17, 63, 64)]
        assert by_w[0] > 0 and all(a <= b for a, b in zip(by_w, by_w[1:])) and by_w[0] < by_w[-1], by_w
        by_l = [_ws(mk(4 * n), n_layers=n) for n in (1, 2, 3, 32)]
        assert all(a < b for a, b in zip(by_l, by_l[1:])), by_l
        assert by_l[1] == 2 * by_l[0]
    assert _ws(_view(B=0), batch=0) == 0
    assert _ws(_view(), T=0, W=0) == 0                       # nothing is live: nothing to move
    # live ranges, not capacities: the window rows and the compressed tokens are what it grows with
    v = _view()
    assert _ws(v, T=0, W=17) == 2 * 4 * v.Hkv * 17 * 128 * 2
    assert _ws(v, T=64, W=0) < _ws(v, T=512, W=0)


def test_reorder_argument_errors_without_gpu():
    err = _lib.load().gear_last_error
    v = _view()
    need = _ws(v)
    assert _call(None) < 0 and b"null cache view" in err()
    assert _call(v, idx=None) < 0 and b"null index" in err()
    assert _call(v, n_layers=0) < 0 and b"n_layers = 0" in err()
    assert _call(v, batch=0) < 0 and b"batch = 0" in err()
    assert _call(v, batch=-4) < 0 and b"batch = -4" in err()
    assert _call(v, batch=3) < 0 and b"B = 4" in err() and b"n_layers * batch" in err()
    assert _call(v, n_layers=2) < 0 and b"n_layers * batch" in err()
    for T in (100, -64, 576):                                # no multiple of 64, negative, past tcap = 512
        assert _call(v, T=T) < 0 and b"T = " in err() and b"multiple of 64" in err(), T
    for W in (-1, 65):
        assert _call(v, W=W) < 0 and b"wcap" in err(), W
    assert _call(v, ws=None, ws_bytes=0) < 0 and b"workspace" in err()
    assert _call(v, ws=None) < 0 and b"workspace" in err()
    assert _call(v, ws_bytes=need - 1) < 0 and b"workspace" in err() and str(need).encode() in err()
    nowin = _view()
    nowin.kwin = None
    assert _call(nowin) < 0 and b"window" in err()
