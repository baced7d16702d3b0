"""GPU tests of the beam-search gather (gear_cache_reorder: GearKVCache.reorder, GearKVCachePool.reorder, FastGearDecoder.reorder).

The reference is torch: two identical caches (same seed, same K / V, every sequence its own random data), reorder(idx) on one,
buf.index_select(batch axis, idx) over the FULL slab of every buffer of the other.  Equality is checked bit for bit in three ways:
(a) every part of attn_probe.decompose, (b) attention output and LSE on the same queries (through the tiles, through lists + chunk
index, through plain lists), (c) both again after the same new rows took both caches across a further block boundary -- what a
stale list head, tile count or factor segment would only disturb at the next append.

(b) on a cache without outliers is attend().  On a cache WITH outliers attend() adds the outlier terms as float sums through LDS
atomics, in whatever order the waves run: two calls on the same bytes need not agree in the last bit (tests/test_gpu_shared.py,
test_decoder_shared_sampling).  There (b) is attend_shared() over one small fixed prefix cache -- gear_attn_decode_shared reads the
same tail fields through the same tiles / chunk indices / lists, with the outlier terms as integer sums, and is bit-reproducible
(test_attend_shared_is_bit_reproducible) -- so the comparison stays an equality."""
import numpy as np
import pytest
import torch

import attn_probe as AP
from test_gpu_attn_probe import _cc
from test_gpu_verify import _tiny

pytestmark = pytest.mark.gpu

HQ = 4
ATTEND_MODES = ((True, True), (False, True), (False, False))      # (use_tiles, use_chunk_index)


def _kv(B, H, n, g):
    return torch.randn(B, H, n, 128, generator=g).half().cuda(), torch.randn(B, H, n, 128, generator=g).half().cuda()


class Store:
    """A standalone GearKVCache (L = 1) or a GearKVCachePool of L = 3 layers behind one interface."""

    def __init__(self, pooled, cc, B, H, cap, seed):
        from gear_amd.cache import GearKVCache, GearKVCachePool
        self.pooled, self.B, self.H = pooled, B, H
        if pooled:
            self.pool = GearKVCachePool(3, B, H, cap, cc, "cuda", seed=seed)
            self.caches = [GearKVCache(B, H, cap, cc, "cuda", seed=seed + i, pool=self.pool, layer=i) for i in range(3)]
            self.bufs = self.pool.buf
        else:
            self.pool = None
            self.caches = [GearKVCache(B, H, cap, cc, "cuda", seed=seed)]
            self.bufs = self.caches[0].bufs

    def axis(self, name):
        return (2 if name in ("kPseg", "vPseg") else 1) if self.pooled else (1 if name in ("kPseg", "vPseg") else 0)

    def fill(self, prompt, more, g):
        if prompt:
            for c in self.caches:
                c.prefill(*_kv(self.B, self.H, prompt, g))
        if more:
            self.extend(more, g)

    def extend(self, n, g):
        rows = [_kv(self.B, self.H, n, g) for _ in self.caches]
        if self.pooled:
            self.pool.extend_all([r[0] for r in rows], [r[1] for r in rows])
        else:
            self.caches[0].extend(*rows[0])

    def reorder(self, idx):
        (self.pool if self.pooled else self.caches[0]).reorder(idx)

    def gather_torch(self, idx, skip=()):
        """The reference: index_select along the batch axis over the full slab of every buffer (but those in `skip`)."""
        idx = torch.as_tensor(idx, dtype=torch.long, device="cuda")
        for name, t in self.bufs.items():
            if name not in skip:
                t.copy_(t.index_select(self.axis(name), idx))

    def snapshot(self):
        gens = [c.gen.get_state() for c in self.caches] + ([self.pool.gen.get_state()] if self.pooled else [])
        return ({k: t.clone() for k, t in self.bufs.items()}, [(c.n_comp, c.n_win, c.seg0, c.kk0) for c in self.caches], gens)

    def restore(self, snap):
        bufs, counters, gens = snap
        for k, t in self.bufs.items():
            t.copy_(bufs[k])
        for c, (n_comp, n_win, seg0, kk0), g in zip(self.caches, counters, gens):
            c.n_comp, c.n_win, c.seg0, c.kk0 = n_comp, n_win, seg0, kk0
            c.gen.set_state(g)
        if self.pooled:
            self.pool.gen.set_state(gens[-1])

    def counters(self):
        return [(c.n_comp, c.n_win, c.seg0, c.kk0) for c in self.caches]


def _parts_diff(x, y):
    """Names of the decompose parts in which caches x and y differ (bit for bit)."""
    px, py = AP.decompose(x), AP.decompose(y)
    bad = []
    for k in px:
        a, b = px[k], py[k]
        if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
            if a is None or b is None or a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
                bad.append(k)
        elif a != b:
            bad.append(k)
    return bad


_PREFIX = {}


def _prefix_for(c):
    """A fixed 64-token batch-1 prefix cache of c's configuration (one per configuration and head count)."""
    from gear_amd.cache import GearKVCache
    key = (c.H, c.bits, c.group, c.R, c.rk, c.rv, c.kv, c.kk_blk)
    if key not in _PREFIX:
        cc = dict(compress_method="gearslKIVI", group_size=c.group, residual=c.R, quantize_bit=c.bits, rank=c.rk, rankv=c.rv, loop=3,
                  left=0.02)
        pre = GearKVCache(1, c.H, c.R, cc, "cuda", seed=77)
        pre.prefill(*_kv(1, c.H, c.R, torch.Generator().manual_seed(77)))
        assert (pre.kv, pre.kk_blk, pre.n_win) == (c.kv, c.kk_blk, 0)
        _PREFIX[key] = pre
    return _PREFIX[key]


def _attention(c, q):
    if c.kv or c.kk_blk:
        return c.attend_shared(q, _prefix_for(c), return_lse=True)
    return c.attend(q, return_lse=True)


def _attend_diff(x, y, q):
    """Attention modes under which the attention over caches x and y differs in output or LSE (bit for bit)."""
    bad = []
    for tiles, chunk in ATTEND_MODES:
        res = []
        for c in (x, y):
            c.use_tiles, c.use_chunk_index = tiles, chunk
            try:
                res.append(_attention(c, q))
            finally:
                c.use_tiles = c.use_chunk_index = True
        if not (torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])):
            bad.append(("tiles" if tiles else "lists") + ("+chunk-index" if chunk else ""))
    return bad


def _diff(sx, sy, q):
    """Every difference (a) and (b) find between the stores sx and sy."""
    bad = []
    for l, (x, y) in enumerate(zip(sx.caches, sy.caches)):
        bad += [f"L{l}:{k}" for k in _parts_diff(x, y)] + [f"L{l}:attend[{m}]" for m in _attend_diff(x, y, q)]
    return bad


def _index_cases(B):
    rep = [min(2, B - 1)] * B
    mixed = [1, 0, 0, 3, 4][:B] if B >= 4 else [1, 0]
    return {"identity": list(range(B)), "swap": [1, 0] + list(range(2, B)), "repeat": rep,
            "shift": [(b + 1) % B for b in range(B)], "repeat+cycle": mixed}


CONFIGS = {"KIVI4": ("KIVI", 4, 64, 4, 0.0), "gearl-R128": ("gearlKIVI", 2, 128, 4, 0.0), "gearsl-r8": ("gearslKIVI", 2, 64, 8, 0.02)}
# state -> (prompt tokens, tokens committed after the prompt) for a residual of R
STATES = {"T0-W17": lambda R: (17, 0),                          # a prompt shorter than the residual: the window alone
          "seg0+2blocks-W30": lambda R: (128, 2 * R + 30),      # a prompt segment, two decode-time blocks, 30 window rows
          "W0-after-boundary": lambda R: (R, R),                # an empty window right after a boundary
          "tail-seg0=0": lambda R: (0, 2 * R + 5)}              # what a shared-prefix tail looks like: no prompt segment
CASES = [(c, s, p) for c in CONFIGS for s in STATES for p in (False, True)]


def _make(config, state, pooled, B, H, seed):
    method, bits, R, rank, left = CONFIGS[config]
    cc = _cc(method, bits, 64, R, rank, left=left)
    prompt, more = STATES[state](R)
    cap = min(512, prompt + more + R + 3)                       # room for the R + 3 rows of (c)
    out = []
    for _ in range(2):
        s = Store(pooled, cc, B, H, cap, seed)
        s.fill(prompt, more, torch.Generator().manual_seed(seed))
        out.append(s)
    return out, R


@pytest.mark.parametrize("config,state,pooled", CASES, ids=[f"{c}-{s}-{'pool' if p else 'cache'}" for c, s, p in CASES])
def test_reorder_equals_torch_gather(config, state, pooled):
    n = CASES.index((config, state, pooled))
    B, H = (2, 4, 5)[n % 3], 1 + (n // 3) % 2
    (a, b), R = _make(config, state, pooled, B, H, seed=11 + n)
    c0 = a.caches[0]
    assert c0.Tmax <= 512 and a.counters() == b.counters()
    want = {"T0-W17": (0, 17, 0), "seg0+2blocks-W30": (128 + 2 * R, 30, 128), "W0-after-boundary": (2 * R, 0, R),
            "tail-seg0=0": (2 * R, 5, 0)}[state]
    assert (c0.n_comp, c0.n_win, c0.seg0) == want
    q = torch.randn(B, HQ, 1, 128, generator=torch.Generator().manual_seed(n)).half().cuda()
    assert _diff(a, b, q) == []                                 # the two builds are the same cache
    sa, sb = a.snapshot(), b.snapshot()
    for name, idx in _index_cases(B).items():
        a.restore(sa), b.restore(sb)
        form = {"identity": idx, "swap": torch.tensor(idx), "repeat": torch.tensor(idx, dtype=torch.int32).cuda()}.get(
            name, torch.tensor(idx).cuda())                     # a list, a CPU tensor, int32 and int64 device tensors
        a.reorder(form)
        b.gather_torch(idx)
        assert a.counters() == b.counters() == sa[1], name
        assert _diff(a, b, q) == [], (name, idx)
        g1, g2 = torch.Generator().manual_seed(99), torch.Generator().manual_seed(99)
        a.extend(R + 3, g1), b.extend(R + 3, g2)                # (c): across one more block boundary
        assert a.counters() == b.counters() and a.caches[0].n_comp == want[0] + R * (1 + (want[1] + 3) // R)
        assert _diff(a, b, q) == [], (name, idx, "after the next boundary")


@pytest.mark.parametrize("pooled", [False, True], ids=["cache", "pool"])
def test_reorder_leaves_fixed_rows_and_other_caches_alone(pooled):
    """A partial permutation: every byte of every buffer that belongs to a sequence with idx[b] == b is unchanged (full slab, dead
    capacity included), the moved rows hold their sources' live state, and a second cache that was not passed in is unchanged."""
    (a, other), R = _make("gearsl-r8", "seg0+2blocks-W30", pooled, 5, 2, seed=5)
    before, obefore = a.snapshot()[0], other.snapshot()[0]
    idx = [0, 3, 2, 1, 4]
    a.reorder(idx)
    torch.cuda.synchronize()
    for name, t in a.bufs.items():
        ax = a.axis(name)
        for b in (0, 2, 4):
            assert torch.equal(t.select(ax, b), before[name].select(ax, b)), (name, b)
    assert not torch.equal(a.bufs["kwin"], before["kwin"]) and not torch.equal(a.bufs["kcode"], before["kcode"])
    for name, t in other.bufs.items():
        assert torch.equal(t, obefore[name]), name
    other.gather_torch(idx)
    q = torch.randn(5, HQ, 1, 128, generator=torch.Generator().manual_seed(1)).half().cuda()
    assert _diff(a, other, q) == []


def test_reorder_rejects_bad_host_indices():
    (a, _), R = _make("KIVI4", "T0-W17", False, 4, 1, seed=2)
    before = a.snapshot()[0]
    for bad in ([0, 1, 2], [0, 1, 2, 4], [0, -1, 2, 3], torch.tensor([0, 1, 2, 7]), torch.tensor([0.0, 1.0, 2.0, 3.0]), 3):
        with pytest.raises(ValueError):
            a.reorder(bad)
    with pytest.raises(ValueError):
        a.reorder(torch.zeros(3, dtype=torch.long).cuda())
    # a device index is not read on the host: entries outside [0, B) are treated as identity by the kernel
    a.reorder(torch.tensor([0, 9, -3, 3]).cuda())
    torch.cuda.synchronize()
    for name, t in a.bufs.items():
        assert torch.equal(t, before[name]), name


def test_reorder_checks_catch_every_field():
    """The test has teeth: for each field of the cache, a reference in which that ONE field is not gathered differs from the
    reordered cache in (a), (b) or (c).  Shape chosen so that no field is equal across the sequences by construction: 2 KV heads
    (the V tile counts of a head depend on where a token row's outliers fall), a prompt segment of 256 tokens = two K chunks (the
    prompt's K outliers split between them differently per sequence).  No field of the view is exempt."""
    B, H, R = 4, 2, 64
    cc = _cc("gearslKIVI", 2, 64, R, 8, left=0.02)
    mk = lambda: Store(False, cc, B, H, 512, 21)
    a, b = mk(), mk()
    for s in (a, b):
        s.fill(256, 2 * R + 30, torch.Generator().manual_seed(21))
    assert (a.caches[0].n_comp, a.caches[0].n_win, a.caches[0].seg0) == (384, 30, 256) and a.caches[0].kk0 > 0
    assert set(a.bufs) == {"kcode", "kscale", "kmn", "vcode", "vscale", "vmn", "kwin", "vwin", "kPseg", "kQtok", "vPseg", "vQtok",
                           "koidx", "koval", "kochunk", "voidx", "voval", "vochunk", "ktile", "kcnt", "vtile", "vcnt"}
    idx = [1, 2, 3, 0]
    q = torch.randn(B, HQ, 1, 128, generator=torch.Generator().manual_seed(3)).half().cuda()
    sb = b.snapshot()
    a.reorder(idx)
    sa = a.snapshot()
    b.gather_torch(idx)
    assert _diff(a, b, q) == []
    missed = []
    for field in sorted(a.bufs):
        a.restore(sa), b.restore(sb)
        b.gather_torch(idx, skip=(field,))
        found = _diff(a, b, q)
        if not found:
            a.extend(R + 3, torch.Generator().manual_seed(4)), b.extend(R + 3, torch.Generator().manual_seed(4))
            found = _diff(a, b, q)
        print(f"stale {field}: {found[:4]}")
        if not found:
            missed.append(field)
    assert missed == []


# ------------------------------------------------------------------------------------------------ decoder
def _gather_pool(pool, idx):
    idx = torch.as_tensor(idx, dtype=torch.long, device="cuda")
    for name, t in pool.buf.items():
        t.copy_(t.index_select(2 if name in ("kPseg", "vPseg") else 1, idx))


def test_decoder_reorder_window_only_equals_permuted_histories():
    """S = 3 over a shared prefix, distinct tokens per row for fewer than `residual` steps, reorder([2, 0, 0]), then on through a tail
    block boundary: the logits equal, bit for bit, those of a decoder whose rows were fed the permuted histories from the start (up
    to the reorder nothing depends on the slot a row sits in; afterwards both compress the same rows in the same slots)."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    g = torch.Generator().manual_seed(13)
    P, n1, n2, idx = 150, 20, 30, [2, 0, 0]
    ids = torch.randint(0, 1000, (1, P), generator=g).cuda()
    t1 = torch.randint(0, 1000, (3, n1), generator=g).cuda()
    t2 = torch.randint(0, 1000, (3, n2), generator=g).cuda()
    assert len({tuple(r.tolist()) for r in t1}) == 3
    a = FastGearDecoder(model, 256, batch=3, seed=4, shared_prefix_tokens=128)
    b = FastGearDecoder(model, 256, batch=3, seed=4, shared_prefix_tokens=128)
    a.prefill_shared(ids), b.prefill_shared(ids)
    for i in range(n1):
        a.step(t1[:, i]), b.step(t1[idx, i])
    prefix_before = {k: t.clone() for k, t in a.prefix_pool.buf.items()}
    a._state_dirty = False
    a.reorder(idx)
    assert a._state_dirty and a.layers[0]["cache"].n_win == 22 + n1 < 64
    for i in range(n2):
        la, lb = a.step(t2[:, i]), b.step(t2[:, i])
        assert torch.equal(la, lb), i
    assert a.layers[0]["cache"].n_comp == 64 and a.layers[0]["cache"].n_win == 22 + n1 + n2 - 64
    for k, t in a.prefix_pool.buf.items():
        assert torch.equal(t, prefix_before[k]), k


@pytest.mark.parametrize("shared", [True, False], ids=["shared-prefix", "plain"])
def test_decoder_reorder_with_compressed_tails_equals_torch_gather(shared):
    """Tails that hold compressed blocks (their factors start from per-(sequence, head) random bases, so a permuted-from-the-start
    decoder is no reference): against a decoder whose pool buffers are gathered with torch, logits bit for bit, across the next
    boundary.  Also on a plain decoder, where the prompt segment moves with the rest (there with a model without outliers: step()
    then attends through attend(), whose outlier sums are not bit-reproducible -- see the module docstring)."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02) if shared else _tiny("gearlKIVI", 2)
    g = torch.Generator().manual_seed(17)
    S, P, n1, n2, idx = 4, 150, 60, 60, [1, 0, 0, 3]
    t1 = torch.randint(0, 1000, (S, n1), generator=g).cuda()
    t2 = torch.randint(0, 1000, (S, n2), generator=g).cuda()
    decs = []
    for _ in range(2):
        if shared:
            d = FastGearDecoder(model, 256, batch=S, seed=4, shared_prefix_tokens=128)
            d.prefill_shared(torch.randint(0, 1000, (1, P), generator=torch.Generator().manual_seed(1)).cuda())
        else:
            d = FastGearDecoder(model, 512, batch=S, seed=4)
            d.prefill(torch.randint(0, 1000, (S, P), generator=torch.Generator().manual_seed(1)).cuda())
        decs.append(d)
    a, b = decs
    for i in range(n1):
        la, lb = a.step(t1[:, i]), b.step(t1[:, i])
    assert torch.equal(la, lb)
    c = a.layers[0]["cache"]
    assert (c.n_comp, c.n_win) == ((64, 18) if shared else (192, 18))
    a.reorder(torch.tensor(idx).cuda())
    _gather_pool(b.pool, idx)
    for i in range(n2):
        la, lb = a.step(t2[:, i]), b.step(t2[:, i])
        assert torch.equal(la, lb), i
    assert c.n_comp == (128 if shared else 256)
    for k, t in a.pool.buf.items():
        if k in ("kwin", "vwin", "kcode", "vcode", "kcnt", "vcnt"):
            assert torch.equal(t, b.pool.buf[k]), k


def test_decoder_reorder_refusals():
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("KIVI", 2)
    with pytest.raises(NotImplementedError):
        FastGearDecoder(model, 256, batch=2, cache_kind="fp16").reorder([1, 0])
    dec = FastGearDecoder(model, 256, batch=2)
    dec.tp_world = 2                                            # (a head-sharded decoder needs a process group to construct)
    with pytest.raises(NotImplementedError):
        dec.reorder([1, 0])
