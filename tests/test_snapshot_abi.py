"""CPU checks of the cache snapshots (gear_cache_snapshot_bytes / gear_cache_snapshot / gear_cache_restore, snapshot.CacheSnapshot,
prefix_store.PrefixStore): the entry points are in the header, the ctypes table and the library and the ABI version did not move;
the blob size is a host-side function with the stated properties; every argument error surfaces as a status < 0 with a message
before anything is launched (the device pointers below are never dereferenced); the Python containers work on CPU tensors."""
import ctypes
import io
import os

import pytest
import torch

from gear_amd import _lib
from gear_amd.prefix_store import PrefixStore
from gear_amd.snapshot import CacheSnapshot, geometry_key
from test_reorder_abi import FAKE, _view

NAMES = ("gear_cache_snapshot_bytes", "gear_cache_snapshot", "gear_cache_restore")


def _bytes(v, n_layers=1, batch=4, T=256, W=17, n_seq=4):
    return _lib.load().gear_cache_snapshot_bytes(ctypes.byref(v), n_layers, batch, T, W, n_seq)


def _snap(v, n_layers=1, batch=4, T=256, W=17, seq0=0, n_seq=4, blob=FAKE * 65, blob_bytes=1 << 40):
    p = ctypes.byref(v) if v is not None else None
    return _lib.load().gear_cache_snapshot(p, n_layers, batch, T, W, seq0, n_seq, blob, blob_bytes, None)


def _rest(v, n_layers=1, batch=4, T=256, W=17, seq0=0, n_seq=4, blob=FAKE * 65, blob_bytes=1 << 40, blob_seqs=None):
    p = ctypes.byref(v) if v is not None else None
    return _lib.load().gear_cache_restore(p, n_layers, batch, T, W, seq0, n_seq, blob, blob_bytes,
                                          n_seq if blob_seqs is None else blob_seqs, None)


def test_snapshot_entries_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "gear_hip.h")).read()
    for name in NAMES:
        assert name + "(" in header
        assert name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.load().gear_abi_version() == _lib.ABI_VERSION == 5


def _full_slab_bytes(v):
    """Bytes of ONE sequence's full slabs over every field of the view (capacities, not live ranges)."""
    H, D, tcap, fpi = v.Hkv, v.D, v.tcap, 32 // v.bits
    n = H * D * v.ldk * 4 + 2 * H * D * v.lsk * 2 + H * tcap * (D // fpi) * 4 + 2 * H * tcap * (D // v.group) * 2
    n += 2 * H * v.wcap * D * 2
    nseg = 1 + tcap // v.seglen
    for r in (v.rk, v.rv):
        if r:
            n += nseg * H * D * r * 2 + H * tcap * r * 2
    if v.kk_cap:
        n += 2 * H * D * 2 * v.kk_cap * 2 + H * D * 2 * v.nbk_pitch
        n += 2 * tcap * 2 * v.kv * 2 + tcap * 2 * (H + 1)
        n += H * v.nck * v.ktile_cap * 4 + H * v.nck * 4 + H * v.nblk * v.vtile_cap * 4 + H * v.nblk * 4
    return n


def test_snapshot_bytes_properties():
    for sparse, rk in ((True, 4), (False, 4), (False, 0)):
        v = _view(rk=rk, rv=rk, sparse=sparse)
        assert _bytes(v, T=0, W=0) == 0                             # nothing is live
        one = _bytes(v, n_seq=1)
        assert one > 0
        assert [_bytes(v, n_seq=n) for n in (1, 2, 3, 4)] == [one, 2 * one, 3 * one, 4 * one]     # exactly linear in n_seq
        by_t = [_bytes(v, T=T) for T in (0, 64, 128, 192, 256, 320, 512)]
        assert all(a <= b for a, b in zip(by_t, by_t[1:])) and by_t[0] < by_t[-1], by_t
        by_w = [_bytes(v, W=W) for W in (0, 1, 17, 63, 64)]
        assert all(a <= b for a, b in zip(by_w, by_w[1:])) and by_w[0] < by_w[-1], by_w
        for T in (0, 64, 256, 512):
            for W in (0, 1, 17, 64):
                for n in (1, 3):
                    assert _bytes(v, T=T, W=W, n_seq=n) % 16 == 0
        for T in (0, 64, 256, 448):                                 # live ranges, not capacities
            assert _bytes(v, T=T, W=64, n_seq=4) < 4 * _full_slab_bytes(v), T
        assert _bytes(v, T=512, W=64, n_seq=1) <= _full_slab_bytes(v) + 16 * 22
        assert _bytes(v, T=100) == 0 and _bytes(v, T=576) == 0 and _bytes(v, T=-64) == 0
        assert _bytes(v, n_seq=5) == 0 and _bytes(v, n_seq=0) == 0
        assert _bytes(v, batch=3, n_seq=3) == 0                     # n_layers * batch != B
    # pooled: layers multiply it; the same geometry gives the same bytes whatever the pointers are
    assert _bytes(_view(B=8), n_layers=2) == 2 * _bytes(_view(B=4))
    v = _view()
    assert _bytes(v, T=0, W=17, n_seq=4) == 2 * 4 * v.Hkv * 17 * 128 * 2       # the window rows alone
    # a K list row with an odd live length (kk0 = 5 entries of 2 bytes) is padded to 16 per row
    v.seg0 = 256
    assert _bytes(v, T=256, W=0, n_seq=1) - _bytes(_view(sparse=False), T=256, W=0, n_seq=1) > 2 * v.Hkv * 128 * 2 * 16 - 1


def test_snapshot_argument_errors_without_gpu():
    err = _lib.load().gear_last_error
    v = _view()
    need = _bytes(v)
    for call, fn in ((_snap, b"gear_cache_snapshot"), (_rest, b"gear_cache_restore")):
        assert call(None) < 0 and b"null cache view" in err() and fn in err()
        assert call(v, blob=None) < 0 and b"null blob" in err()
        assert call(v, batch=3, n_seq=3) < 0 and b"B = 4" in err() and b"n_layers * batch" in err()
        assert call(v, n_layers=2) < 0 and b"n_layers * batch" in err()
        for T in (100, -64, 576):                                   # no multiple of 64, negative, past tcap = 512
            assert call(v, T=T) < 0 and b"T = " in err() and b"multiple of 64" in err(), T
        for W in (-1, 65):
            assert call(v, W=W) < 0 and b"wcap" in err(), W
        assert call(v, seq0=-1, n_seq=1) < 0 and b"seq0 = -1" in err()
        assert call(v, n_seq=0) < 0 and b"n_seq = 0" in err()
        assert call(v, seq0=1, n_seq=4) < 0 and b"batch = 4" in err()
        assert call(v, n_seq=5) < 0 and b"batch = 4" in err()
        assert call(v, blob_bytes=need - 1) < 0 and b"blob of" in err() and str(need).encode() in err()
        assert call(v, blob_bytes=0) < 0 and b"blob of" in err()
        for off in (1, 2, 4, 8):
            assert call(v, blob=FAKE * 65 + off) < 0 and b"16-byte aligned" in err(), off
        nowin = _view()
        nowin.kwin = None
        assert call(nowin) < 0 and b"window" in err()
        # a field beyond 2^31 units per sequence: a view whose (fake) capacity is out of any real range
        big = _view(B=1, Hkv=64, tcap=1 << 22, sparse=False)
        assert call(big, batch=1, n_seq=1, T=1 << 22) < 0 and b"2^31" in err()
        assert _bytes(big, batch=1, n_seq=1, T=1 << 22) == 0
        # a grid too large: each field stays below 2^31 units per sequence, all sequences together do not
        wide = _view(B=1 << 17, Hkv=64, tcap=1 << 16, sparse=False)
        assert call(wide, batch=1 << 17, n_seq=1 << 17, T=1 << 16, blob_bytes=1 << 62) < 0 and b"exceed the grid" in err()
    wide = _view(B=1 << 17, sparse=False)                           # a broadcast has its destinations on grid.y
    assert _rest(wide, batch=1 << 17, n_seq=1 << 17, T=64, blob_seqs=1) < 0 and b"exceed the grid" in err()
    # restore: the blob holds the destinations' sequences or one
    one = _bytes(v, n_seq=1)
    for bad in (0, 2, 3, 5, -1):
        assert _rest(v, blob_seqs=bad) < 0 and b"blob_seqs = " in err(), bad
    assert _rest(v, blob_seqs=1, blob_bytes=one - 1) < 0 and str(one).encode() in err()      # sized by the blob's own sequences
    assert _rest(v, n_seq=2, seq0=1, blob_seqs=2, blob_bytes=2 * one - 1) < 0 and str(2 * one).encode() in err()


# ------------------------------------------------------------------------------------------------ CacheSnapshot
CC = dict(compress_method="gearslKIVI", group_size=64, residual=64, quantize_bit=2, rank=4, rankv=4, loop=3, left=0.02)


def _cpu_snapshot(n=1000, n_seq=2):
    from gear_amd.cache import _cache_dims
    _, d = _cache_dims(n_seq, 2, 256, CC)
    g = torch.Generator().manual_seed(3)
    blob = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    return CacheSnapshot(blob, 1, n_seq, (128, 7, 64, 3), geometry_key(d, 2, 128), True, None, [g.get_state()])


def test_cache_snapshot_state_dict_roundtrip_and_moves():
    s = _cpu_snapshot()
    assert s.nbytes == 1000 and (s.n_comp, s.n_win, s.seg0, s.kk0) == (128, 7, 64, 3)
    f = io.BytesIO()
    torch.save(s.state_dict(), f)
    f.seek(0)
    t = CacheSnapshot.from_state_dict(torch.load(f))
    assert torch.equal(t.blob, s.blob) and t.blob.dtype == torch.uint8
    assert (t.n_layers, t.n_seq, t.counters, t.geometry, t.whole) == (s.n_layers, s.n_seq, s.counters, s.geometry, s.whole)
    assert t.pool_gen is None and len(t.gens) == 1 and torch.equal(t.gens[0], s.gens[0])
    u = s.to("cpu")
    assert u.blob is s.blob and u.counters == s.counters          # already there: the identity
    assert s.cpu().blob is s.blob


def test_restore_refuses_another_geometry_before_anything_changes():
    from gear_amd.cache import GearKVCache
    c = GearKVCache(2, 2, 256, CC, "cpu")
    s = _cpu_snapshot()
    s.geometry = dict(s.geometry, rk=8)
    before = (c.n_comp, c.n_win, c.seg0, c.kk0)
    with pytest.raises(ValueError, match="rk = 8"):
        c.restore(s)
    h = _cpu_snapshot()
    h.geometry = dict(h.geometry, H=4)
    with pytest.raises(ValueError, match="H = 4"):
        c.restore(h)
    big = _cpu_snapshot()
    big.counters = (320, 0, 64, 3)                                # more compressed tokens than the capacity of 256
    with pytest.raises(_lib.GearError, match="capacity"):
        c.restore(big)
    odd = _cpu_snapshot()
    odd.counters = (100, 0, 64, 3)                                # not a state a cache can be in: a message of its own
    with pytest.raises(_lib.GearError, match="multiple of 64"):
        c.restore(odd)
    with pytest.raises(ValueError):
        c.restore({"blob": s.blob})
    assert (c.n_comp, c.n_win, c.seg0, c.kk0) == before and not c.kcode.any()


# ------------------------------------------------------------------------------------------------ PrefixStore
def _entry(n):
    return _cpu_snapshot(n)


def test_prefix_store_lru_bytes_and_refusals():
    st = PrefixStore(2500, device="cpu")
    assert len(st) == 0 and st.bytes_used == 0 and st.lookup([1, 2, 3]) is None
    a, b, c = _entry(1000), _entry(1000), _entry(400)
    st.add([1, 2, 3], a)
    st.add(torch.tensor([[4, 5]]), b)                               # ids as a tensor of any shape
    st.add((6,), c)
    assert len(st) == 3 and st.bytes_used == 2400
    assert st.lookup([1, 2]) is None and st.lookup([1, 2, 3, 4]) is None      # exact ids only
    assert st.lookup([4, 5]).blob is b.blob
    assert st.lookup(torch.tensor([1, 2, 3])).blob is a.blob        # now [6] is the least recently used, then [4, 5]
    d = _entry(500)
    st.add([7], d)                                                  # 2400 + 500 > 2500: evicts [6] (400), which is enough
    assert len(st) == 3 and st.bytes_used == 2500 and st.lookup([6]) is None
    e = _entry(1200)
    st.add([8], e)                                                  # evicts down to fit: [4, 5] and [1, 2, 3] go, [7] stays
    assert st.lookup([4, 5]) is None and st.lookup([1, 2, 3]) is None
    assert len(st) == 2 and st.bytes_used == 1700 and st.lookup([7]).blob is d.blob
    with pytest.raises(ValueError):
        st.add([9], _entry(2501))                                   # larger than the store: refused, nothing evicted
    assert len(st) == 2 and st.bytes_used == 1700
    st.add([7], _entry(100))                                        # the same ids: replaced, not counted twice
    assert len(st) == 2 and st.bytes_used == 1300
    st.add([10], _entry(2500))                                      # exactly max_bytes fits, alone
    assert len(st) == 1 and st.bytes_used == 2500 and st.lookup([10]) is not None
