"""GPU tests of the cache snapshots (gear_cache_snapshot / gear_cache_restore: GearKVCache / GearKVCachePool .snapshot / .restore,
FastGearDecoder.snapshot / restore / load_prefix, PrefixStore).

The shapes, the twin construction and the comparison are those of tests/test_gpu_reorder.py (imported, not copied): two identical
stores, bit-for-bit equality of (a) every part of attn_probe.decompose, (b) attention output and LSE through the tiles, the chunk
index and the plain lists (attend_shared over a small fixed prefix where the cache has outliers: see that module's docstring),
(c) both again after the same new rows took both stores across a further block boundary.  All comparisons are equalities.

What stands in for a stale state.  Before a restore every buffer of the store is overwritten with the byte 0xA5 (no field of a
fresh cache, and no zero that a skipped byte could pass for).  After the restore, and BEFORE any kernel follows an index of the
restored store, _raw_gate compares bytes: a new snapshot of the store equals the restored blob and the twin's (every live byte
arrived), and every byte of the full slabs that is no longer 0xA5 equals the twin's (nothing else was written).  Only then does
the comparison of (a), (b), (c) run, so a wrong restore fails at the byte compare and no attention kernel walks garbage lists.
The bytes past the live ranges still hold 0xA5 during (b) and (c): the restore's reliance on nothing reading past the counters is
under test as well.  The per-field check then puts ANOTHER SEQUENCE's rows into one field at a time (a roll along the batch
axis; every sequence has its own random data), as test_reorder_checks_catch_every_field does."""
import ctypes

import numpy as np
import pytest
import torch

import attn_probe as AP
import test_gpu_reorder as TR
from test_gpu_reorder import CONFIGS, HQ, STATES, Store, _make
from test_gpu_attn_probe import _cc
from test_gpu_verify import _tiny

pytestmark = pytest.mark.gpu

CASES = [(c, s, p) for c in CONFIGS for s in STATES for p in (False, True)]
IDS = [f"{c}-{s}-{'pool' if p else 'cache'}" for c, s, p in CASES]


def _obj(s):
    return s.pool if s.pooled else s.caches[0]


def _q(B, seed):
    return torch.randn(B, HQ, 1, 128, generator=torch.Generator().manual_seed(seed)).half().cuda()


def _extend_both(a, b, n, seed):
    a.extend(n, torch.Generator().manual_seed(seed)), b.extend(n, torch.Generator().manual_seed(seed))


PATTERN = 0xA5


def _poison(s):
    """Every byte of every buffer of the store becomes PATTERN."""
    for t in s.bufs.values():
        t.view(torch.uint8).fill_(PATTERN)


def _raw_gate(a, b, snap):
    """Byte checks of a restore of `snap` into the poisoned store a against its twin b; no kernel reads an index of a here (a
    snapshot walks host-planned ranges only)."""
    now = _obj(a).snapshot()
    assert now.counters == snap.counters and torch.equal(now.blob, snap.blob), "the live bytes differ from the restored blob"
    assert torch.equal(now.blob, _obj(b).snapshot().blob), "the live bytes differ from the twin's"
    for name, t in a.bufs.items():
        x, y = t.view(torch.uint8), b.bufs[name].view(torch.uint8)
        m = x != PATTERN
        assert torch.equal(x[m], y[m]), f"{name}: bytes written that the twin does not hold"


def _parts_diff(x, y):
    """test_gpu_reorder._parts_diff, with the channel factors kP / vP compared in the segments that hold tokens (parts["seg"]).
    decompose() hands out segment 0 even when no token belongs to it (a cache without a prompt segment, or without compressed
    tokens at all); no token reads it, no live range covers it while the cache holds no compressed token, and here it may hold
    0xA5 on one side."""
    px, py = AP.decompose(x), AP.decompose(y)
    bad = []
    for k in px:
        a, b = px[k], py[k]
        if k in ("kP", "vP") and a is not None and b is not None and np.array_equal(px["seg"], py["seg"]):
            used = np.unique(px["seg"])
            a, b = a[used], b[used]
        if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
            if a is None or b is None or a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
                bad.append(k)
        elif a != b:
            bad.append(k)
    return bad


def _diff(sx, sy, q):
    """Every difference (a) and (b) find between the stores sx and sy."""
    bad = []
    for l, (x, y) in enumerate(zip(sx.caches, sy.caches)):
        bad += [f"L{l}:{k}" for k in _parts_diff(x, y)] + [f"L{l}:attend[{m}]" for m in TR._attend_diff(x, y, q)]
    return bad


def _full(s):
    return {k: t.clone() for k, t in s.bufs.items()}


# ------------------------------------------------------------------------------------------------ 1, 2: round trip
@pytest.mark.parametrize("config,state,pooled", CASES, ids=IDS)
def test_snapshot_restore_round_trip(config, state, pooled):
    """snapshot, R + 5 more rows (every live range moves, a block boundary is crossed, the generators advance), every buffer
    overwritten with 0xA5, restore: the store equals its untouched twin in (a), (b) and the counters, and again in (c) after R + 5 further rows
    -- which needs the restored generator states, list heads, tile counts and factor segments to be right."""
    n = CASES.index((config, state, pooled))
    B, H = (1, 2, 5)[n % 3], 1 + (n // 3) % 2
    (a, b), R = _make(config, state, pooled, B, H, seed=31 + n)
    assert a.caches[0].Tmax <= 512 and a.counters() == b.counters()
    q = _q(B, n)
    snap = _obj(a).snapshot()
    assert snap.n_seq == B and snap.n_layers == len(a.caches) and snap.whole and snap.counters == a.counters()[0]
    assert snap.blob.dtype == torch.uint8 and snap.blob.is_cuda and snap.nbytes % 16 == 0
    assert snap.nbytes < sum(t.numel() * t.element_size() for t in a.bufs.values())
    a.extend(R + 5, torch.Generator().manual_seed(5))
    assert a.counters() != b.counters()
    _poison(a)
    _obj(a).restore(snap)
    assert a.counters() == b.counters()
    _raw_gate(a, b, snap)
    assert _diff(a, b, q) == []
    _extend_both(a, b, R + 5, 99)
    assert a.counters() == b.counters() and a.caches[0].n_comp > snap.n_comp
    assert _diff(a, b, q) == [], "after the next boundary"


def test_snapshot_checks_catch_every_field():
    """The comparison has teeth for the restore: after a round trip as above (restored into buffers of 0xA5), each of the 22 fields in turn is made stale alone
    (it holds another sequence's rows) and (a), (b) or (c) notices.  The shape is test_reorder_checks_catch_every_field's, where
    no field is equal across the sequences by construction."""
    B, H, R = 4, 2, 64
    cc = _cc("gearslKIVI", 2, 64, R, 8, left=0.02)
    a, b = (Store(False, cc, B, H, 512, 21) for _ in range(2))
    for s in (a, b):
        s.fill(256, 2 * R + 30, torch.Generator().manual_seed(21))
    assert len(a.bufs) == 22 and a.caches[0].kk0 > 0
    q = _q(B, 3)
    snap = a.caches[0].snapshot()
    a.extend(R + 5, torch.Generator().manual_seed(5))
    _poison(a)
    a.caches[0].restore(snap)
    _raw_gate(a, b, snap)
    assert _diff(a, b, q) == []
    sa, sb = a.snapshot(), b.snapshot()                            # (Store.snapshot: full-slab torch clones)
    missed = []
    for field in sorted(a.bufs):
        a.restore(sa), b.restore(sb)
        a.bufs[field].copy_(a.bufs[field].roll(1, a.axis(field)))
        found = _diff(a, b, q)
        if not found:
            _extend_both(a, b, R + 3, 4)
            found = _diff(a, b, q)
        print(f"stale {field}: {found[:4]}")
        if not found:
            missed.append(field)
    assert missed == []


# ------------------------------------------------------------------------------------------------ 3: slot restore
@pytest.mark.parametrize("pooled", [False, True], ids=["cache", "pool"])
def test_restore_into_one_slot(pooled):
    """Sequence 3 of a batch-5 store goes into slot 1 of its twin: slot 1 then holds the source's sequence 3 (against a twin in
    which torch copied the full slabs), every byte of the other sequences' full slabs and of a store that was not passed in is
    unchanged, the generators are left alone, and unequal counters raise ValueError before anything changes."""
    (a, b), R = _make("gearsl-r8", "seg0+2blocks-W30", pooled, 5, 2, seed=5)
    (ref, other), _ = _make("gearsl-r8", "seg0+2blocks-W30", pooled, 5, 2, seed=5)
    before, obefore = _full(b), _full(other)
    gens = [c.gen.get_state() for c in b.caches]
    snap = _obj(a).snapshot(seq=3)
    whole = _obj(a).snapshot()
    assert snap.n_seq == 1 and not snap.whole and snap.gens == [] and 5 * snap.nbytes == whole.nbytes
    _obj(b).restore(snap, seq=1)
    torch.cuda.synchronize()
    for name, t in b.bufs.items():
        ax = b.axis(name)
        for s in (0, 2, 3, 4):
            assert torch.equal(t.select(ax, s), before[name].select(ax, s)), (name, s)
    assert not torch.equal(b.bufs["kwin"], before["kwin"]) and not torch.equal(b.bufs["kcode"], before["kcode"])
    for name, t in other.bufs.items():
        assert torch.equal(t, obefore[name]), name
    assert all(torch.equal(c.gen.get_state(), g) for c, g in zip(b.caches, gens)) and b.counters() == a.counters()
    ref.gather_torch([0, 3, 2, 3, 4])
    q = _q(5, 1)
    assert _diff(b, ref, q) == []
    _extend_both(b, ref, R + 3, 8)
    assert _diff(b, ref, q) == [], "after the next boundary"
    # unequal counters: refused, nothing written
    (c, d), _ = _make("gearsl-r8", "seg0+2blocks-W30", pooled, 5, 2, seed=5)
    c.extend(3, torch.Generator().manual_seed(1))
    late = _obj(c).snapshot(seq=3)
    dbefore, dcount = _full(d), d.counters()
    with pytest.raises(ValueError, match="lockstep"):
        _obj(d).restore(late, seq=1)
    with pytest.raises(ValueError):
        _obj(d).restore(snap, seq=5)
    with pytest.raises(ValueError):
        _obj(d).restore(whole, seq=1)                             # five sequences do not go into one slot
    torch.cuda.synchronize()
    assert d.counters() == dcount
    for name, t in d.bufs.items():
        assert torch.equal(t, dbefore[name]), name


# ------------------------------------------------------------------------------------------------ 4: broadcast
@pytest.mark.parametrize("config,pooled", [("gearsl-r8", True), ("gearsl-r8", False), ("gearl-R128", True), ("KIVI4", False)])
def test_restore_broadcasts_one_sequence(config, pooled):
    """A batch-1 snapshot into a batch-5 store in another state: all five sequences equal the source (against a batch-5 store into
    which torch expanded the source's full slabs), the counters are set, the destination's generators are left alone."""
    method, bits, R, rank, left = CONFIGS[config]
    cc = _cc(method, bits, 64, R, rank, left=left)
    src, dst, ref = Store(pooled, cc, 1, 2, 512, 7), Store(pooled, cc, 5, 2, 512, 8), Store(pooled, cc, 5, 2, 512, 8)
    src.fill(128, 2 * R + 30, torch.Generator().manual_seed(7))
    for s in (dst, ref):
        s.fill(R, R + 9, torch.Generator().manual_seed(8))          # other counters, other data
    assert dst.counters() != src.counters()
    gens = [c.gen.get_state() for c in dst.caches]
    snap = _obj(src).snapshot()
    assert snap.n_seq == 1
    _obj(dst).restore(snap)
    assert dst.counters() == [src.counters()[0]] * len(dst.caches)
    assert all(torch.equal(c.gen.get_state(), g) for c, g in zip(dst.caches, gens))
    for name, t in ref.bufs.items():
        t.copy_(src.bufs[name].expand_as(t))
    for c, cnt in zip(ref.caches, src.counters()):
        c.n_comp, c.n_win, c.seg0, c.kk0 = cnt
    q = _q(5, 2)
    assert _diff(dst, ref, q) == []
    _extend_both(dst, ref, R + 3, 9)
    assert _diff(dst, ref, q) == [], "after the next boundary"


def test_whole_batch1_snapshot_crosses_pool_and_standalone():
    """A whole snapshot of a batch-1 standalone cache carries no pool generator state: a one-layer batch-1 pool takes it as a
    one-sequence blob (buffers and counters; its own generators left alone), and the reverse.  With more sequences the mismatch
    of the generator states is refused before anything changes."""
    from gear_amd.cache import GearKVCache, GearKVCachePool
    method, bits, R, rank, left = CONFIGS["gearsl-r8"]
    cc = _cc(method, bits, 64, R, rank, left=left)
    src = GearKVCache(1, 2, 512, cc, "cuda", seed=3)
    src.prefill(*TR._kv(1, 2, 128, torch.Generator().manual_seed(3)))
    src.extend(*TR._kv(1, 2, R + 9, torch.Generator().manual_seed(4)))
    pool = GearKVCachePool(1, 1, 2, 512, cc, "cuda", seed=9)
    layer = GearKVCache(1, 2, 512, cc, "cuda", seed=10, pool=pool, layer=0)
    snap = src.snapshot()
    assert snap.whole and snap.n_seq == 1 and snap.pool_gen is None
    gens = (pool.gen.get_state(), layer.gen.get_state())
    pool.restore(snap)
    assert (layer.n_comp, layer.n_win, layer.seg0, layer.kk0) == snap.counters
    assert torch.equal(pool.gen.get_state(), gens[0]) and torch.equal(layer.gen.get_state(), gens[1])
    back = pool.snapshot()
    assert back.pool_gen is not None and torch.equal(back.blob, snap.blob)
    assert _parts_diff(layer, src) == []
    dst = GearKVCache(1, 2, 512, cc, "cuda", seed=11)
    g = dst.gen.get_state()
    dst.restore(back)
    assert torch.equal(dst.gen.get_state(), g) and _parts_diff(dst, src) == []
    assert torch.equal(dst.snapshot().blob, snap.blob)
    # two sequences: no broadcast to fall back on
    src2, pool2 = GearKVCache(2, 2, 512, cc, "cuda", seed=3), GearKVCachePool(1, 2, 2, 512, cc, "cuda", seed=9)
    layer2 = GearKVCache(2, 2, 512, cc, "cuda", seed=10, pool=pool2, layer=0)
    src2.prefill(*TR._kv(2, 2, 17, torch.Generator().manual_seed(3)))
    with pytest.raises(ValueError, match="generator states"):
        pool2.restore(src2.snapshot())
    assert layer2.n_win == 0 and not pool2.buf["kwin"].any()


# ------------------------------------------------------------------------------------------------ 5: host trip
@pytest.mark.parametrize("pin", [False, True], ids=["pageable", "pinned"])
def test_snapshot_host_round_trip(pin):
    from gear_amd import _lib
    from gear_amd.cache import _view
    from gear_amd.snapshot import CacheSnapshot
    (a, b), R = _make("gearsl-r8", "seg0+2blocks-W30", True, 2, 2, seed=17)
    q = _q(2, 5)
    snap = a.pool.snapshot()
    c0 = a.caches[0]
    view = _view(a.bufs, a.pool.dims, 3 * 2, 2, 128, c0.kk0, c0.seg0, kwin=True)
    assert snap.nbytes == _lib.load().gear_cache_snapshot_bytes(ctypes.byref(view), 3, 2, c0.n_comp, c0.n_win, 2)
    assert snap.nbytes < sum(t.numel() * t.element_size() for t in a.bufs.values())
    host = snap.cpu(pin_memory=pin)
    assert host.blob.device.type == "cpu" and host.blob.is_pinned() == pin and host.nbytes == snap.nbytes
    back = CacheSnapshot.from_state_dict(host.state_dict()).to("cuda", non_blocking=pin)
    assert back.blob.is_cuda and torch.equal(back.blob, snap.blob)
    a.extend(R + 5, torch.Generator().manual_seed(5))
    _poison(a)
    a.pool.restore(back)
    assert a.counters() == b.counters()
    _raw_gate(a, b, snap)
    assert _diff(a, b, q) == []
    _extend_both(a, b, R + 5, 99)
    assert _diff(a, b, q) == []
    # a from 0xA5 through the host blob (moved by the restore itself), b over the stale state that the extension left past the
    # live ranges: nothing is cleared and nothing needs to be
    _poison(a)
    a.pool.restore(host)
    b.pool.restore(snap)
    assert a.counters() == b.counters()
    _raw_gate(a, b, snap)
    assert _diff(a, b, q) == []
    _extend_both(a, b, R + 5, 99)
    assert _diff(a, b, q) == [], "after the next boundary"


# ------------------------------------------------------------------------------------------------ 6 - 8: decoder
def _record(dec):
    """Every logits tensor dec.step() returns from now on."""
    log, step = [], dec.step

    def wrapped(tok):
        out = step(tok)
        log.append(out.clone())
        return out
    dec.step = wrapped
    return log


def _prompts():
    g = torch.Generator().manual_seed(23)
    return torch.randint(0, 1000, (1, 150), generator=g).cuda(), torch.randint(0, 1000, (1, 200), generator=g).cuda()


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("store", [None, "cpu"], ids=["direct", "cpu-store"])
def test_decoder_prompt_swap(sampled, store):
    """P1 = 150 tokens (128 compressed + 22 remainder rows), P2 = 200 (192 + 8).  Decoder 1 prefills P1 and snapshots the prefix;
    decoder 2 prefills P2 and generates 70 tokens (its tails cross a boundary), then loads P1's snapshot and generates from P1 with
    reuse_prefix; decoder 3, fresh, generates from P1 with a real prefill.  Tokens and the logits of every step agree bit for bit."""
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.prefix_store import PrefixStore
    from gear_amd.sampling import SamplingParams
    model = _tiny("gearslKIVI", 2, left=0.02)
    sp = SamplingParams(0.8, 50, 0.95, seed=7) if sampled else None
    P1, P2 = _prompts()
    mk = lambda: FastGearDecoder(model, 256, batch=3, seed=4, shared_prefix_tokens=192)
    d1, d2, d3 = mk(), mk(), mk()
    d1.prefill_shared(P1)
    snap = d1.snapshot("prefix")
    assert snap.what == "prefix" and snap.tail is None and snap.prefix.n_comp == 128 and snap.shared_rem[0][0].shape[2] == 22
    if store:
        ps = PrefixStore(4 * snap.nbytes, device=store)
        ps.add(P1, snap)
        assert len(ps) == 1 and ps.bytes_used == snap.nbytes and ps.lookup(P2) is None
        del snap
        assert ps._entries[tuple(P1.reshape(-1).tolist())][0].prefix.blob.device.type == "cpu"
    d2.generate(P2, 270, sampling=sp, shared_prefix=True)
    assert d2.layers[0]["prefix"].n_comp == 192 and d2.layers[0]["cache"].n_comp == 64
    snap = ps.lookup(P1) if store else snap
    assert snap.prefix.blob.is_cuda
    d2._state_dirty = False
    d2.load_prefix(snap)
    c = d2.layers[0]["cache"]
    assert d2._state_dirty and d2.shared_live and d2.pos == 150 and (c.n_comp, c.n_win, c.seg0, c.kk0) == (0, 22, 0, 0)
    assert d2.layers[0]["prefix"].n_comp == 128
    l2, l3 = _record(d2), _record(d3)
    t2 = d2.generate(P1, 220, sampling=sp, shared_prefix=True, reuse_prefix=True)
    t3 = d3.generate(P1, 220, sampling=sp, shared_prefix=True)
    assert t2.shape == (3, 220) and torch.equal(t2, t3)
    assert len(l2) == len(l3) == 69 and all(torch.equal(x, y) for x, y in zip(l2, l3))
    assert torch.equal(d2._shared_saved["logits"], d3._shared_saved["logits"])
    assert d2.layers[0]["cache"].n_comp == 64                      # the tails crossed a boundary again
    # a fresh decoder that never ran a prefill takes the stored prompt as well
    d4 = mk()
    d4.load_prefix(snap)
    t4 = d4.generate(P1, 220, sampling=sp, shared_prefix=True, reuse_prefix=True)
    assert torch.equal(t4, t3)
    with pytest.raises(ValueError):
        d4.generate(P2, 270, shared_prefix=True, reuse_prefix=True)      # P2 is not the stored prompt


@pytest.mark.parametrize("shared", [True, False], ids=["shared-prefix", "plain"])
def test_decoder_pause_resume(shared):
    """snapshot("all") after 70 steps, 70 more steps, restore, the same 70 tokens again: bit-identical logits (the second leg
    crosses a block boundary, so the restored generator states matter).  Plain decoder: a model without outliers (step() then
    attends through attend(), whose outlier sums are not run-to-run reproducible)."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02) if shared else _tiny("gearlKIVI", 2)
    g = torch.Generator().manual_seed(29)
    S, P, n = 3, 150, 70
    t1 = torch.randint(0, 1000, (S, n), generator=g).cuda()
    t2 = torch.randint(0, 1000, (S, n), generator=g).cuda()
    if shared:
        d = FastGearDecoder(model, 256, batch=S, seed=4, shared_prefix_tokens=128)
        d.prefill_shared(torch.randint(0, 1000, (1, P), generator=g).cuda())
    else:
        d = FastGearDecoder(model, 512, batch=S, seed=4)
        d.prefill(torch.randint(0, 1000, (S, P), generator=g).cuda())
    for i in range(n):
        d.step(t1[:, i])
    snap = d.snapshot("all")
    c = d.layers[0]["cache"]
    at = (c.n_comp, c.n_win, d.pos)
    assert snap.what == "all" and snap.pos == P + n and (snap.prefix is not None) == shared
    first = [d.step(t2[:, i]).clone() for i in range(n)]
    assert c.n_comp == at[0] + 64
    d._state_dirty = False
    d.restore(snap)
    assert d._state_dirty and (c.n_comp, c.n_win, d.pos) == at
    again = [d.step(t2[:, i]) for i in range(n)]
    assert all(torch.equal(x, y) for x, y in zip(first, again))


def test_decoder_snapshot_refusals():
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("KIVI", 2)
    f = FastGearDecoder(model, 256, batch=2, cache_kind="fp16")
    for call in (lambda d: d.snapshot(), lambda d: d.restore(None), lambda d: d.load_prefix(None)):
        with pytest.raises(NotImplementedError):
            call(f)
    dec = FastGearDecoder(model, 256, batch=2)
    with pytest.raises(ValueError):
        dec.snapshot("prefix")                                    # no shared prefix
    with pytest.raises(ValueError):
        dec.snapshot("tails")
    snap = dec.snapshot()
    with pytest.raises(ValueError):
        dec.load_prefix(snap)                                     # holds no stored prompt
    dec.tp_world = 2                                              # (a head-sharded decoder needs a process group to construct)
    for call in (lambda d: d.snapshot(), lambda d: d.restore(snap), lambda d: d.load_prefix(snap)):
        with pytest.raises(NotImplementedError):
            call(dec)
