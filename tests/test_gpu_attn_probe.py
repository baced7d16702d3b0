"""Attention kernels at one-token resolution, LSE included (tests/attn_probe.py): aimed queries through the unmodified library --
gear_attn_decode_idx (decode_attention), gear_attn_decode_cache (GearKVCache.attend), gear_attn_extend_cache
(GearKVCache.attend_extend) and gear_attn_decode_f16 -- against the float64 reference (row_err <= ROW_BOUND, lse_err <= LSE_BOUND),
and against every mutated reference that applies to the case (> 5x a bound: the probes reach each mutation site on real
payloads).  Nothing is mutated on the device."""
import numpy as np
import pytest
import torch

import attn_probe as AP

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for tag, (r, e, m) in sorted(WORST.items()):
        print(f"PROBE {tag}: row_err {r:.3e} lse_err {e:.3e} min mutation signal {m:.1f} (5 = the required margin)")


def host(t):
    return t.detach().cpu().numpy()


# M6 on real payloads: the low-rank term at an outlier is small (a 4-bit payload's quantization error is), and at a V outlier it is
# 1.5 - 3.5 % of the row's largest element (the outlier itself): leaving it out moves the probes by 2 - 5 x a bound -- past the
# bound the exact check holds, short of the 5x margin the synthetic caches of test_attn_probe_sensitivity show
MIN_SIGNAL = {"M6-v-no-lr": 1.5, "M6-k-no-lr": 3.0}


def _verify(tag, parts, Hq, rounds, aimed, mutations=True):
    """rounds: [(q [B,Hq,nq,D], kernel out, kernel lse, probe rows | None)] -- each round against the exact reference, and every
    mutated reference that applies against all rounds together (the largest signal of any round)."""
    kv = AP.keys(parts)
    r = e = 0.0
    for q, out, lse, _ in rounds:
        assert np.isfinite(out).all() and np.isfinite(lse).all()
        ro, rl = AP.ref(q, parts, kv=kv)
        r, e = max(r, AP.row_err(out, ro)), max(e, AP.lse_err(lse, rl))
    assert r <= AP.ROW_BOUND and e <= AP.LSE_BOUND, (tag, r, e)
    m = float("inf")
    if mutations:
        sites = AP.mutation_sites(parts, Hq, aimed)
        assert "M1-drop" in {k for k, _ in sites}
        for kind, where in sites:
            mp = AP.mutate(parts, kind, where)
            sig = 0.0
            for q, out, lse, used in rounds:
                rows = np.arange(q.shape[2]) if used is None else np.nonzero(used.any(axis=(0, 1)))[0]
                mo, ml = AP.ref(q[:, :, rows], mp, rows=rows)
                sig = max(sig, AP.signal(out[:, :, rows], lse[:, :, rows], mo, ml))
            assert sig >= MIN_SIGNAL.get(kind, 5.0), (tag, kind, where, sig)
            m = min(m, sig / MIN_SIGNAL.get(kind, 5.0) * 5.0)
    w = WORST.get(tag, (0.0, 0.0, float("inf")))
    WORST[tag] = (max(w[0], r), max(w[1], e), min(w[2], m))


def _run_decode(fn, parts, Hq, seed):
    """Every probe batch through one decode call -> ([(q, out, lse, None)] stacked along the query-row axis, aimed positions)."""
    qs, aimed = AP.decode_batches(parts, Hq, np.random.default_rng(seed))
    outs, lses = [], []
    for q in qs:
        o, l = fn(torch.tensor(q, dtype=torch.float16, device="cuda"))
        outs.append(host(o).astype(np.float64))
        lses.append(host(l).astype(np.float64)[:, :, None])
    return [(np.concatenate(qs, 2), np.concatenate(outs, 2), np.concatenate(lses, 2), None)], aimed


@pytest.fixture
def options():
    """Set library options for one test; every one is restored to its default 0."""
    from gear_amd import _lib as L
    names = []

    def setter(**kw):
        for k, v in kw.items():
            L.set_option(k, v)
            names.append(k)
    yield setter
    for k in names:
        L.set_option(k, 0)


# ------------------------------------------------------------------------------------------------ decode_attention (plain)
PLAIN = [  # B, Hq, Hkv, T, W, bits, mode, rank, k_out
    (1, 8, 2, 1024, 63, 2, "fp32", 4, 10),
    (1, 4, 4, 192, 1, 4, "fp16", 8, 3),
    (1, 2, 1, 2112, 0, 2, "fp32", 16, 10),
    (1, 4, 2, 1024, 0, 4, "fp16", 0, 0),
    (1, 2, 2, 8320, 1, 2, "fp32", 8, 20),
]


@pytest.mark.parametrize("generic", [0, 1], ids=["planned", "generic"])
@pytest.mark.parametrize("case", PLAIN, ids=[f"T{c[3]}-W{c[4]}-b{c[5]}-{c[6]}-r{c[7]}-k{c[8]}-{c[1]}x{c[2]}" for c in PLAIN])
def test_decode_attention_probes(options, case, generic):
    from gear_amd import compress as C
    from gear_amd.attention import decode_attention
    B, Hq, Hkv, T, W, bits, mode, rank, k_out = case
    options(attn_generic=generic)
    g = torch.Generator().manual_seed(T + W)
    k = (torch.randn(B, Hkv, T, 128, generator=g) * (1 + 2 * (torch.rand(1, Hkv, 1, 128, generator=g) > 0.95))).half().cuda()
    v = torch.randn(B, Hkv, T, 128, generator=g).half().cuda()
    kw = torch.randn(B, Hkv, W, 128, generator=g).half().cuda() if W else None
    vw = torch.randn(B, Hkv, W, 128, generator=g).half().cuda() if W else None
    pk = C.compress_key(k, bits, 64, k_out=k_out, rank=rank, loop=3, mode=mode)
    pv = C.compress_value(v, bits, 64, k_out=k_out, rank=rank, loop=3, mode=mode)
    parts = AP.decompose((pk, pv), kw, vw)
    rounds, aimed = _run_decode(lambda x: decode_attention(x, pk, pv, kw, vw, return_lse=True), parts, Hq, T)
    _verify(f"decode_attention[{'generic' if generic else 'planned'}]", parts, Hq, rounds, aimed)


# ------------------------------------------------------------------------------------------------ GearKVCache.attend
def _cc(method="gearslKIVI", bits=2, group=64, R=64, rank=4, rankv=None, left=0.02):
    return dict(compress_method=method, group_size=group, residual=R, quantize_bit=bits, rank=rank,
                rankv=rank if rankv is None else rankv, loop=3, left=left)


def _filled(cc, B, Hkv, T0, more, seed):
    """A cache after a prompt of T0 tokens (not a multiple of 64) and `more` committed tokens: several factor segments."""
    from gear_amd.cache import GearKVCache
    g = torch.Generator().manual_seed(seed)
    c = GearKVCache(B, Hkv, T0 + more + 128, cc, "cuda", seed=seed)
    c.prefill(torch.randn(B, Hkv, T0, 128, generator=g).half().cuda(), torch.randn(B, Hkv, T0, 128, generator=g).half().cuda())
    if more:
        c.extend(torch.randn(B, Hkv, more, 128, generator=g).half().cuda(), torch.randn(B, Hkv, more, 128, generator=g).half().cuda())
    return c


ATTEND_OPTS = {
    "default": {}, "lists": {"_tiles": False}, "no-chunk-index": {"_chunk_index": False}, "generic": {"attn_generic": 1},
    "mfma": {"attn_mfma": 1}, "vector": {"attn_mfma": -1}, "gqa-group": {"attn_gqa_group": 1},
    "win-in-reduce": {"attn_win_chunk": -1}, "win-chunk": {"attn_win_chunk": 1}, "fold": {"attn_fold": 1},
}


def _attend_probe(tag, c, Hq, options, opt, seed):
    from gear_amd import _lib as L
    c.use_tiles = opt.get("_tiles", True)
    c.use_chunk_index = opt.get("_chunk_index", True)
    set_opts = {k: v for k, v in opt.items() if not k.startswith("_")}
    try:
        for k, v in set_opts.items():
            L.set_option(k, v)
        parts = AP.decompose(c)
        rounds, aimed = _run_decode(lambda x: c.attend(x, return_lse=True), parts, Hq, seed)
        _verify(tag, parts, Hq, rounds, aimed)
        q = rounds[0][0]
        if set_opts.get("attn_fold"):      # an LSE request keeps the merge in its own launch: the folded merge, output only
            o2 = np.concatenate([host(c.attend(torch.tensor(q[:, :, i:i + 1], dtype=torch.float16, device="cuda"))).astype(np.float64)
                                 for i in range(q.shape[2])], 2)
            assert AP.row_err(o2, AP.ref(q, parts)[0]) <= AP.ROW_BOUND
    finally:
        for k in set_opts:
            L.set_option(k, 0)
        c.use_tiles = c.use_chunk_index = True


@pytest.fixture(scope="module")
def caches():
    return {}


@pytest.mark.parametrize("opt", list(ATTEND_OPTS))
def test_cache_attend_probes(caches, options, opt):
    if "main" not in caches:
        caches["main"] = _filled(_cc(), 1, 2, 200, 150, seed=21)          # seg0 = 192, four decode-time blocks, W = 30
    c = caches["main"]
    assert c.seg0 == 192 and c.n_comp == 320 and c.n_win == 30
    _attend_probe(f"attend[{opt}]", c, 8, options, ATTEND_OPTS[opt], seed=5)


@pytest.mark.parametrize("rk,rv", [(4, 8), (8, 4)])
def test_cache_attend_unequal_ranks(options, rk, rv):
    c = _filled(_cc(rank=rk, rankv=rv), 1, 2, 130, 140, seed=rk)
    assert (c.rk, c.rv) == (rk, rv) and c.kQtok.shape[-1] == rk and c.vQtok.shape[-1] == rv
    for opt in ("default", "mfma", "generic"):
        _attend_probe(f"attend[r{rk}/{rv}]", c, 4, options, ATTEND_OPTS[opt], seed=6)


def test_cache_attend_overflowed_tiles(options):
    """test_gpu_fast_decode.test_matrix_core_attention_with_overflowed_tiles' cache: tiles that overflowed send the kernels to
    the sorted lists."""
    from gear_amd.cache import GearKVCache
    torch.manual_seed(74)
    B, Hkv, T0 = 1, 4, 512
    k = torch.randn(B, Hkv, T0, 128)
    v = torch.randn(B, Hkv, T0, 128)
    k[:, :, :100] *= 12.0
    v[:, 1] *= 12.0
    c = GearKVCache(B, Hkv, T0 + 128, _cc(rank=8, left=0.04), "cuda")
    c.prefill(k.half().cuda(), v.half().cuda())
    assert int((c.kcnt[:, :, :4] < 0).sum()) > 0 and int((c.vcnt[:, 1, :8] < 0).sum()) > 0
    c.append(torch.randn(B, Hkv, 1, 128).half().cuda(), torch.randn(B, Hkv, 1, 128).half().cuda())
    for opt in ("mfma", "vector"):
        _attend_probe(f"attend[overflowed-{opt}]", c, 8, options, ATTEND_OPTS[opt], seed=7)


# ------------------------------------------------------------------------------------------------ GearKVCache.attend_extend
def _extend_probe(tag, c, Hq, n, seed, mutations=True):
    g = torch.Generator().manual_seed(seed)
    kn = torch.randn(c.B, c.H, n, 128, generator=g).half().cuda()
    vn = torch.randn(c.B, c.H, n, 128, generator=g).half().cuda()
    parts = AP.decompose(c, kn=kn, vn=vn)
    qr, aimed = AP.extend_queries(parts, Hq, np.random.default_rng(seed), max_rounds=16 if mutations else 1)
    rounds = []
    for q, used in qr:
        out, lse = c.attend_extend(torch.tensor(q, dtype=torch.float16, device="cuda"), kn, vn, return_lse=True)
        rounds.append((q, host(out).astype(np.float64), host(lse).astype(np.float64), used))
    _verify(tag, parts, Hq, rounds, aimed, mutations)


EXT = [  # method, bits, group, residual, rank, left, Hq, Hkv, prompt, committed, n  (test_gpu_extend.CASES, one n each, + GQA 3 / 5 / 6 / 7)
    ("gearslKIVI", 2, 64, 64, 4, 0.02, 8, 2, 200, 150, 200),
    ("gearlKIVI", 4, 32, 128, 8, 0.0, 4, 4, 300, 300, 64),
    ("KIVI", 2, 32, 64, 0, 0.05, 2, 1, 130, 140, 7),
    ("gearslKIVI", 4, 64, 128, 16, 0.05, 1, 1, 260, 280, 200),
    ("gearslKIVI", 2, 64, 64, 8, 0.02, 8, 8, 70, 130, 64),
    ("gearlKIVI", 2, 64, 64, 4, 0.0, 2, 2, 30, 0, 200),          # T = 0
    ("gearslKIVI", 2, 32, 64, 4, 0.05, 4, 2, 128, 64, 7),        # W = 0
    ("gearslKIVI", 2, 64, 64, 4, 0.03, 3, 1, 200, 100, 37),      # n G = 111: ends mid-tile
    ("gearslKIVI", 2, 64, 64, 8, 0.03, 5, 1, 150, 70, 29),       # 145
    ("gearslKIVI", 4, 64, 64, 4, 0.03, 6, 2, 260, 64, 45),       # 270
    ("gearlKIVI", 2, 64, 64, 4, 0.0, 7, 1, 100, 90, 23),         # 161
    ("gearslKIVI", 2, 32, 128, 4, 0.02, 4, 2, 300, 260, 50),     # group 32, residual 128
    ("gearslKIVI", 2, 64, 64, 4, 0.02, 8, 2, 3000, 1100, 5),     # long context, small n: many splits
]


@pytest.mark.parametrize("case", EXT, ids=[f"{c[0]}-b{c[1]}-g{c[2]}-R{c[3]}-r{c[4]}-s{c[5]}-{c[6]}x{c[7]}-{c[8]}+{c[9]}-n{c[10]}"
                                           for c in EXT])
def test_attend_extend_probes(case):
    method, bits, group, R, rank, left, Hq, Hkv, T0, more, n = case
    c = _filled(_cc(method, bits, group, R, rank, left=left), 2 if Hkv <= 2 else 1, Hkv, T0, more, seed=11)
    if T0 == 30:
        assert c.n_comp == 0
    if T0 == 128:
        assert c.n_win == 0
    _extend_probe(f"attend_extend[G{Hq // Hkv}]", c, Hq, n, seed=n)


def test_attend_extend_single_split():
    """B Hkv ceil(n G / 64) >= 1024 work items: the split planner gives every M-tile all pieces in ONE workgroup (nsplit = 1)."""
    c = _filled(_cc(), 4, 16, 100, 0, seed=12)
    _extend_probe("attend_extend[nsplit=1]", c, 16, 1024, seed=3, mutations=False)


# ------------------------------------------------------------------------------------------------ decode_attention_f16
@pytest.mark.parametrize("B,Hq,Hkv,T", [(1, 4, 2, 77), (2, 8, 2, 1000), (1, 2, 1, 4096), (1, 2, 2, 8320)])
def test_decode_attention_f16_probes(B, Hq, Hkv, T):
    from gear_amd.attention import decode_attention_f16
    g = torch.Generator().manual_seed(T)
    tcap = T + 64 if T < 8320 else T
    k = torch.randn(B, Hkv, tcap, 128, generator=g).half().cuda()
    v = torch.randn(B, Hkv, tcap, 128, generator=g).half().cuda()
    parts = AP.window_parts(k[:, :, :T], v[:, :, :T])
    rounds, aimed = _run_decode(lambda x: decode_attention_f16(x, k, v, T, return_lse=True), parts, Hq, T)
    _verify("decode_attention_f16", parts, Hq, rounds, aimed)
