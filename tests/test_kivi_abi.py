"""CPU checks of the KIVI-cache entry points (csrc/kivi.hip: gear_kivi_rope_append / gear_kivi_append / gear_attn_decode_kivi /
gear_attn_decode_kivi_workspace): they are in the ctypes table with the declared signatures and exported, the ABI version did not
move, the workspace is monotone and zero for bad arguments, and every argument error surfaces as a status < 0 with a message
before anything is launched (the device pointers below are never dereferenced)."""
import ctypes

from gear_amd import _lib

_vp, _i, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
FAKE = 4096


def _view(B=1, Hkv=2, tcap=256, R=64, bits=2, group=64, **kw):
    v = _lib.CacheView()
    for f in ("kcode", "kscale", "kmn", "vcode", "vscale", "vmn", "kwin", "vwin"):
        setattr(v, f, FAKE)
    v.B, v.Hkv, v.D, v.tcap, v.wcap = B, Hkv, 128, tcap, R
    v.ldk, v.lsk, v.group, v.bits, v.mode = tcap // (32 // max(bits, 1)), tcap // 64, group, bits, 0
    for k, x in kw.items():
        setattr(v, k, x)
    return v


def _attend(view, L=100, Tk=64, Nv=35, Hq=4, ws=FAKE, ws_bytes=1 << 40, q=FAKE, out=FAKE):
    p = ctypes.byref(view) if view is not None else None
    return _lib.load().gear_attn_decode_kivi(p, q, Hq, L, Tk, Nv, 0.088, out, None, ws, ws_bytes, None)


def _append(rope=True, B=1, Hq=4, Hkv=2, D=128, kslot=3, n=70, R=64, evict=5, tcap=256, group=64, bits=2, src=FAKE, codes=FAKE):
    lib = _lib.load()
    if rope:
        return lib.gear_kivi_rope_append(src, B, Hq, Hkv, D, n, 10000.0, FAKE, FAKE, kslot, FAKE, n, R, evict, codes, codes, codes,
                                         tcap, group, bits, None)
    return lib.gear_kivi_append(src, src, B, Hkv, D, FAKE, kslot, FAKE, n, R, evict, codes, codes, codes, tcap, group, bits, None)


def test_kivi_entries_are_bound_and_exported():
    want = {
        "gear_kivi_rope_append": (_i, [_vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
        "gear_kivi_append": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
        "gear_attn_decode_kivi_workspace": (_sz, [_i, _i, _i, _i]),
        "gear_attn_decode_kivi": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    }
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        assert hasattr(raw, name), name
    assert _lib.load().gear_abi_version() == _lib.ABI_VERSION == 5


def test_kivi_header_declares_the_entries():
    import os
    with open(os.path.join(os.path.dirname(_lib._HERE), "include", "gear_hip.h")) as f:
        text = f.read()
    for decl in ("int gear_kivi_rope_append(const void* qkv, int B, int Hq, int Hkv, int D, int pos, float theta, void* q_out,",
                 "int gear_kivi_append(const void* k_new, const void* v_new, int B, int Hkv, int D, void* kwin, int kslot,",
                 "size_t gear_attn_decode_kivi_workspace(int B, int Hq, int T, int bits);",
                 "int gear_attn_decode_kivi(const gear_cache_view* c, const void* q, int Hq, int L, int Tk, int Nv, float qscale,"):
        assert decl in text, decl


def test_kivi_workspace_is_monotone_and_zero_for_bad_arguments():
    lib = _lib.load()
    w = lib.gear_attn_decode_kivi_workspace
    by_b = [w(B, 32, 4096, 2) for B in (1, 2, 3, 4, 8, 16)]
    assert by_b[0] > 0 and all(a < b for a, b in zip(by_b, by_b[1:]))
    by_h = [w(2, Hq, 4096, 4) for Hq in (1, 2, 8, 32)]
    assert all(a < b for a, b in zip(by_h, by_h[1:]))
    by_t = [w(4, 32, T, 2) for T in (0, 64, 1024, 4096, 8192, 16384)]
    assert by_t[0] > 0 and all(a <= b for a, b in zip(by_t, by_t[1:]))
    # it covers the partial slots of the dispatch below the seam
    assert w(4, 32, 4096, 2) >= lib.gear_attn_decode_workspace(4, 32, 4096, 2)
    for bad in ((0, 32, 64, 2), (4, 0, 64, 2), (4, 32, -1, 2), (4, 32, 64, 3), (-1, 32, 64, 4)):
        assert w(*bad) == 0, bad


def test_kivi_attend_argument_errors_without_gpu():
    err = _lib.load().gear_last_error
    assert _attend(None) < 0 and b"null cache view" in err()
    assert _attend(_view(), q=None) < 0 and b"null q / out" in err()
    assert _attend(_view(), out=None) < 0 and b"null q / out" in err()
    assert _attend(_view(kcode=None)) < 0 and b"packed K missing" in err()
    assert _attend(_view(vscale=None)) < 0 and b"packed V missing" in err()
    assert _attend(_view(vwin=None)) < 0 and b"ring missing" in err()
    assert _attend(_view(bits=3)) < 0 and b"bits must be 2 or 4 (got 3)" in err()
    assert _attend(_view(group=32)) < 0 and b"group must be 64 (got 32)" in err()
    assert _attend(_view(R=96)) < 0 and b"must be 64 or 128 (got 96)" in err()
    assert _attend(_view(mode=1)) < 0 and b"mode 0" in err()
    assert _attend(_view(rk=4)) < 0 and b"no low-rank factors and no outliers" in err()
    assert _attend(_view(kv=3)) < 0 and b"no low-rank factors and no outliers" in err()
    bad = _view()
    bad.D = 64
    assert _attend(bad) < 0 and b"head_dim must be 128" in err()
    assert _attend(_view(), Hq=3) < 0 and b"bad head counts" in err()
    assert _attend(_view(B=4096), Hq=32) < 0 and b"query rows" in err()
    assert _attend(_view(), L=0, Tk=0, Nv=0) < 0 and b"L = 0" in err()
    assert _attend(_view(), L=100, Nv=101) < 0 and b"Nv = 101" in err()                     # Nv > L
    assert _attend(_view(), L=100, Nv=-1) < 0 and b"Nv = -1" in err()
    assert _attend(_view(), L=100, Tk=64, Nv=34) < 0 and b"fp16 V rows" in err()            # 66 rows, the ring holds 65
    assert _attend(_view(), L=100, Tk=32) < 0 and b"Tk % R != 0" in err()
    assert _attend(_view(R=128), L=200, Tk=64, Nv=71) < 0 and b"Tk % R != 0" in err()
    assert _attend(_view(), L=140, Tk=64, Nv=75) < 0 and b"K window" in err()               # 76 window tokens, R = 64
    assert _attend(_view(), L=100, Tk=128, Nv=35) < 0 and b"K window" in err()              # Tk > L
    assert _attend(_view(), L=330, Tk=320, Nv=265) < 0 and b"tcap" in err()                 # past the capacity
    assert _attend(_view(R=128), L=200, Tk=0, Nv=71) < 0 and b"K window" in err()           # 200 window tokens, R = 128
    assert _attend(_view(), ws=None, ws_bytes=0) < 0 and b"workspace" in err()
    assert _attend(_view(), ws=FAKE, ws_bytes=64) < 0 and b"workspace of 64 bytes" in err()


def test_kivi_append_argument_errors_without_gpu():
    err = _lib.load().gear_last_error
    for rope, name in ((True, b"gear_kivi_rope_append"), (False, b"gear_kivi_append")):
        assert _append(rope, D=64) < 0 and name in err() and b"head_dim must be 128" in err()
        assert _append(rope, bits=3) < 0 and b"bits must be 2 or 4 (got 3)" in err()
        assert _append(rope, group=32) < 0 and b"group must be 64 (got 32)" in err()
        assert _append(rope, R=96, evict=-1) < 0 and b"must be 64 or 128 (got 96)" in err()
        assert _append(rope, src=None) < 0 and b"null pointer" in err()
        assert _append(rope, kslot=64) < 0 and b"K window slot 64" in err()
        assert _append(rope, kslot=-1) < 0 and b"K window slot -1" in err()
        assert _append(rope, n=70, evict=4) < 0 and b"evict_row = 4" in err()               # the slot of token 70 holds token 5
        assert _append(rope, n=30, evict=-35) < 0 and b"evict_row = -35" in err()
        assert _append(rope, n=70, evict=5, codes=None) < 0 and b"needs vcode" in err()
        assert _append(rope, n=400, evict=335, tcap=256) < 0 and b"tcap" in err()
        assert _append(rope, B=0) < 0 and b"bad shape" in err()
    assert _append(True, Hq=0) < 0 and b"Hq 0" in err()
