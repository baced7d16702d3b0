"""CPU checks of the tree-verify entry points (gear_attn_verify_tree / gear_attn_verify_tree_workspace): they are in the header,
the ctypes table and the library, the ABI version did not move, the workspace is gear_attn_verify_workspace's, and argument errors
surface as a status < 0 with a message before anything is launched."""
import ctypes
import os
import re

from gear_amd import _lib

NAMES = ("gear_attn_verify_tree", "gear_attn_verify_tree_workspace")


def _view(Hkv=2, tcap=128, wcap=64):
    v = _lib.CacheView()
    v.B, v.Hkv, v.D, v.tcap, v.wcap = 1, Hkv, 128, tcap, wcap
    v.ldk, v.lsk, v.group, v.bits, v.mode = tcap // 16, tcap // 64, 64, 2, 0
    return v


def _call(v, Hq=4, n=4, T=0, W=0, anc=4096, ws=None, ws_bytes=0):
    lib = _lib.load()
    fake = 4096            # never dereferenced: every case below fails its argument check first
    return lib.gear_attn_verify_tree(ctypes.byref(v), fake, Hq, n, T, W, fake, fake, anc, 0.088, fake, None, ws, ws_bytes, None)


def test_tree_entries_are_declared_bound_and_exported():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "gear_hip.h")
    with open(header) as f:
        text = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert hasattr(raw, name)
    assert "const void* anc" in text
    lib = _lib.load()
    assert lib.gear_abi_version() == _lib.ABI_VERSION == 5
    for B, Hq, n, T, W in ((1, 32, 1, 4096, 10), (1, 32, 4, 4096, 32), (2, 8, 16, 128, 63), (2, 2, 5, 0, 5), (1, 4, 16, 8256, 0)):
        want = lib.gear_attn_verify_workspace(B, Hq, n, T, W)
        assert want > 0 and lib.gear_attn_verify_tree_workspace(B, Hq, n, T, W) == want
    assert lib.gear_attn_verify_tree_workspace(1, 32, 0, 4096, 10) == 0
    assert lib.gear_attn_verify_tree_workspace(1, 32, -1, 4096, 10) == 0


def test_tree_argument_errors_without_gpu():
    lib = _lib.load()
    v = _view()
    for n in (0, 17):
        assert _call(v, n=n) < 0 and b"gear_attn_verify_tree: n = " in lib.gear_last_error()
    assert _call(v, Hq=3) < 0 and b"multiple of Hkv" in lib.gear_last_error()
    assert _call(v, W=65) < 0 and b"wcap" in lib.gear_last_error()
    assert _call(v, T=100) < 0 and b"multiple of 64" in lib.gear_last_error()
    assert _call(v, anc=None) < 0 and b"null anc" in lib.gear_last_error()
    assert _call(v, ws=None, ws_bytes=0) < 0 and b"workspace" in lib.gear_last_error()
    assert _call(v, ws=4096, ws_bytes=64) < 0 and b"workspace" in lib.gear_last_error()
    bad = _view()
    bad.D = 64
    assert _call(bad) < 0 and b"head_dim" in lib.gear_last_error()
    assert lib.gear_attn_verify_tree(None, None, 4, 4, 0, 0, None, None, None, 1.0, None, None, None, 0, None) < 0
    assert b"gear_attn_verify_tree: null cache view" in lib.gear_last_error()
    # the chain entry point still names itself
    assert lib.gear_attn_verify_cache(None, None, 4, 4, 0, 0, None, None, 1.0, None, None, None, 0, None) < 0
    assert b"gear_attn_verify_cache: null cache view" in lib.gear_last_error()
