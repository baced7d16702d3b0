"""GPU tests of shared-prefix decoding: gear_attn_decode_shared (GearKVCache.attend_shared) -- S sequences over ONE stored prompt --
probed at one-token resolution against float64, LSE included (tests/attn_probe.py; bounds AP.ROW_BOUND / AP.LSE_BOUND), across
the cache configurations, the attention options and the matrix-core kernel forced on and off (A); one-token sensitivity of those
probes (B); composition with a plain cache (C); no state change (D); FastGearDecoder's shared-prefix mode (E) and what it
allocates (F)."""
import numpy as np
import pytest
import torch

import attn_probe as AP
from test_gpu_attn_probe import ATTEND_OPTS, _cc
from test_gpu_verify import _compare, _cos, _greedy, _threshold, _tiny

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for tag, (r, e) in sorted(WORST.items()):
        print(f"SHARED {tag}: row_err {r:.3e} (bound {AP.ROW_BOUND:g}) lse_err {e:.3e} (bound {AP.LSE_BOUND:g})")


def host(t):
    return t.detach().cpu().numpy()


def _randn_kv(B, Hkv, T, g):
    k = (torch.randn(B, Hkv, T, 128, generator=g) * (1 + 2 * (torch.rand(1, Hkv, 1, 128, generator=g) > 0.95))).half().cuda()
    return k, torch.randn(B, Hkv, T, 128, generator=g).half().cuda()


def _pair(cc, S, Hkv, Tp, more, seed):
    """A prefix cache (B = 1, Tp compressed tokens) and a tail cache (B = S, different K / V per sequence) filled through extend:
    `more` tokens = more // R block boundaries + a window of more % R rows."""
    from gear_amd.cache import GearKVCache
    g = torch.Generator().manual_seed(seed)
    pre = GearKVCache(1, Hkv, Tp, cc, "cuda", seed=seed)
    pre.prefill(*_randn_kv(1, Hkv, Tp, g))
    assert (pre.n_comp, pre.n_win, pre.seg0) == (Tp, 0, Tp)
    tail = GearKVCache(S, Hkv, more + 128, cc, "cuda", seed=seed + 1)
    assert (tail.n_comp, tail.seg0, tail.kk0) == (0, 0, 0)
    if more:
        tail.extend(*_randn_kv(S, Hkv, more, g))
    return pre, tail


def _joint_keys(pre, tail):
    """(tail parts, (K, V) [S, Hkv, Tp + T + W, D]): the prefix's keys broadcast to the S sequences in front of each sequence's own."""
    tp = AP.decompose(tail)
    Kp, Vp = AP.keys(AP.decompose(pre))
    Kt, Vt = AP.keys(tp)
    S = Kt.shape[0]
    bc = lambda x: np.broadcast_to(x, (S,) + x.shape[1:])
    return tp, (np.concatenate([bc(Kp), Kt], 2), np.concatenate([bc(Vp), Vt], 2))


def _queries(tp, kv, Hq, Tp, rng):
    """Probe batches q [S, Hq, 1, D]: AP.decode_batches over the joint keys (its positions < T + W lie in the prefix), aimed probes
    at the prefix's chunk edges, at each sequence's compressed tail and window and over the prefix | tail | window boundaries,
    and Gaussian queries.  Returns (list of q, the joint key positions the extra probes aim at)."""
    Kall = kv[0]
    S, Hkv, N = Kall.shape[:3]
    T, W = tp["T"], tp["W"]
    G = Hq // Hkv
    qs, _ = AP.decode_batches(tp, Hq, rng, Kall=Kall)
    tg = [[p] for p in sorted({0, 63, 64, 127, 128, Tp // 2 - 1, Tp // 2, Tp - 1} | ({Tp, Tp + 63, Tp + 64, Tp + T - 1} if T else set())
                              | ({Tp + T, Tp + T + W - 1} if W else set())) if 0 <= p < N]
    tg += [[a, a + 1] for a in {Tp - 1, Tp + T - 1} if a + 1 < N]
    per = {}
    for s in range(S):
        for h in range(Hkv):
            pr = [q for q in (AP.aim(Kall[s, h], t) for t in tg) if q is not None]
            assert len(pr) >= len(tg) // 2, (s, h, len(pr), len(tg))
            for g in range(G):
                per[s, h * G + g] = pr[g::G] if len(pr) >= G else pr
    for j in range(max(len(v) for v in per.values())):
        q = np.zeros((S, Hq, 1, AP.D))
        for (s, hq), pr in per.items():
            q[s, hq, 0] = pr[j] if j < len(pr) else AP.f16(rng.standard_normal(AP.D))
        qs.append(q)
    qs += [AP.f16(rng.standard_normal((S, Hq, 1, AP.D))) for _ in range(2)]
    return qs, {p for t in tg for p in t}


def _run(pre, tail, qs):
    outs, lses = [], []
    for q in qs:
        o, l = tail.attend_shared(torch.tensor(q, dtype=torch.float16, device="cuda"), pre, return_lse=True)
        outs.append(host(o).astype(np.float64))
        lses.append(host(l).astype(np.float64)[:, :, None])
    return np.concatenate(outs, 2), np.concatenate(lses, 2)


def _under(opt, tail, fn):
    from gear_amd import _lib as L
    tail.use_tiles = opt.get("_tiles", True)
    tail.use_chunk_index = opt.get("_chunk_index", True)
    set_opts = {k: v for k, v in opt.items() if not k.startswith("_")}
    try:
        for k, v in set_opts.items():
            L.set_option(k, v)
        return fn()
    finally:
        for k in set_opts:
            L.set_option(k, 0)
        tail.use_tiles = tail.use_chunk_index = True


def _check(tag, out, lse, ro, rl):
    assert np.isfinite(out).all() and np.isfinite(lse).all(), tag
    r, e = AP.row_err(out, ro), AP.lse_err(lse, rl)
    print(f"shared probe {tag}: row_err {r:.3e} lse_err {e:.3e}")
    w = WORST.get(tag.split("|")[0], (0.0, 0.0))
    WORST[tag.split("|")[0]] = (max(w[0], r), max(w[1], e))
    assert r <= AP.ROW_BOUND and e <= AP.LSE_BOUND, (tag, r, e)


# ------------------------------------------------------------------------------------------------ A. probes against float64
SHARED = [  # method, bits, rank, residual, Hq, Hkv, S, Tp, tail tokens (T + W)
    ("gearslKIVI", 2, 8, 64, 8, 8, 16, 4096, 64 + 17),      # MHA, P = 16: two groups of 8 per KV head (the 7B shape at S = 16)
    ("gearslKIVI", 2, 4, 64, 8, 2, 3, 1024, 192 + 1),       # G 4, P = 12: groups of 4; three block boundaries
    ("KIVI", 4, 4, 64, 8, 1, 2, 64, 17),                    # G 8, P = 16; one prefix block; T = 0
    ("gearlKIVI", 4, 8, 128, 4, 4, 1, 1024, 64),            # S = 1, P = 1; residual 128: W = 64, T = 0
    ("gearlKIVI", 2, 4, 64, 4, 1, 4, 64, 64 + 1),           # G 4, P = 16
    ("gearslKIVI", 4, 4, 64, 2, 2, 8, 1024, 192 + 17),      # MHA, P = 8
    ("gearslKIVI", 2, 8, 64, 8, 1, 1, 4096, 64 + 1),        # G 8 at S = 1
    ("KIVI", 2, 4, 64, 4, 4, 3, 1024, 64 + 17),             # P = 3: one row per workgroup
    ("gearslKIVI", 2, 8, 64, 4, 4, 2, 1024, 1),             # P = 2, T = 0, W = 1
    ("gearslKIVI", 2, 4, 64, 4, 4, 4, 4096, 192 + 17),      # MHA, P = 4
]


@pytest.mark.parametrize("case", SHARED, ids=[f"{c[0]}-b{c[1]}-r{c[2]}-R{c[3]}-{c[4]}x{c[5]}-S{c[6]}-Tp{c[7]}+{c[8]}" for c in SHARED])
def test_attend_shared_probes(case):
    method, bits, rank, R, Hq, Hkv, S, Tp, more = case
    cc = _cc(method, bits, 64, R, rank, left=0.02 if method == "gearslKIVI" else 0.0)
    pre, tail = _pair(cc, S, Hkv, Tp, more, seed=Tp + more + S)
    assert (tail.n_comp, tail.n_win) == (more - more % R, more % R)
    tp, kv = _joint_keys(pre, tail)
    qs, _ = _queries(tp, kv, Hq, Tp, np.random.default_rng(S))
    ro, rl = AP.ref(np.concatenate(qs, 2), tp, kv=kv)
    for name in ("default", "mfma", "vector"):                 # attn_mfma by its rule, forced on, forced off
        out, lse = _under(ATTEND_OPTS[name], tail, lambda: _run(pre, tail, qs))
        _check(f"attend_shared[P{Hq // Hkv * S}]|{case}|{name}", out, lse, ro, rl)


@pytest.fixture(scope="module")
def main_pair():
    pre, tail = _pair(_cc(), 4, 2, 1024, 192 + 30, seed=21)                # G 4, S = 4: P = 16; three decode-time blocks, W = 30
    tp, kv = _joint_keys(pre, tail)
    qs, aimed = _queries(tp, kv, 8, 1024, np.random.default_rng(5))
    q = np.concatenate(qs, 2)
    return pre, tail, tp, kv, qs, q, AP.ref(q, tp, kv=kv), aimed


# every option with attn_mfma by its rule, forced on and forced off (the two options that ARE attn_mfma: once)
OPT_CASES = [(opt, m) for opt in ATTEND_OPTS for m in (0, 1, -1) if m == 0 or "attn_mfma" not in ATTEND_OPTS[opt]]


@pytest.mark.parametrize("opt,mfma", OPT_CASES, ids=[f"{o}-{('rule', 'mfma-on', 'mfma-off')[m]}" for o, m in OPT_CASES])
def test_attend_shared_probes_under_options(main_pair, opt, mfma):
    pre, tail, tp, kv, qs, q, (ro, rl), _ = main_pair
    o = dict(ATTEND_OPTS[opt])
    if mfma:
        o["attn_mfma"] = mfma
    out, lse = _under(o, tail, lambda: _run(pre, tail, qs))
    _check(f"attend_shared[{opt}]|mfma{mfma}", out, lse, ro, rl)


def test_attend_shared_long_prefix_generic_kernel():
    """Tp > 8192: the prefix goes through the long-context kernel (rows mapped to q in place there too)."""
    pre, tail = _pair(_cc(), 3, 1, 8320, 64 + 5, seed=9)
    tp, kv = _joint_keys(pre, tail)
    qs, _ = _queries(tp, kv, 4, 8320, np.random.default_rng(2))
    ro, rl = AP.ref(np.concatenate(qs, 2), tp, kv=kv)
    out, lse = _run(pre, tail, qs)
    _check("attend_shared[Tp8320]", out, lse, ro, rl)


@pytest.mark.parametrize("opt", ["default", "lists", "no-chunk-index", "vector", "mfma", "gqa-group", "generic"])
def test_attend_shared_is_bit_reproducible(main_pair, opt):
    """The same call on the same caches (2 % outliers, through tiles and through lists) gives the same bits every time: out and LSE
    of 12 repeats are equal to the first.  Bound: equality -- no sum in the call depends on the order in which waves run (fixed merge
    orders; outlier terms as integer sums, or scattered into the matrix-core tile)."""
    pre, tail, tp, kv, qs, q, _, _ = main_pair
    first = _under(ATTEND_OPTS[opt], tail, lambda: _run(pre, tail, qs))
    for i in range(12):
        again = _under(ATTEND_OPTS[opt], tail, lambda: _run(pre, tail, qs))
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), (opt, i)


def test_attend_shared_long_prefix_is_bit_reproducible():
    """The same through the long-context kernel (Tp > 8192), whose outlier terms went through float atomics too."""
    pre, tail = _pair(_cc(), 3, 1, 8320, 64 + 5, seed=9)
    rng = np.random.default_rng(4)
    qs = [AP.f16(rng.standard_normal((3, 4, 1, AP.D))) for _ in range(4)]
    first = _run(pre, tail, qs)
    for i in range(12):
        again = _run(pre, tail, qs)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), i


# ------------------------------------------------------------------------------------------------ B. one-token sensitivity
def test_attend_shared_probes_catch_one_token_faults(main_pair):
    """A kernel that loses one prefix key, one tail key, or gives row s the tail of sequence s + 1 would move the probe metric to
    at least 5 x a bound: the mutated float64 references lie that far from what the kernel computes."""
    pre, tail, tp, kv, qs, q, (ro, rl), aimed = main_pair
    out, lse = _run(pre, tail, qs)
    assert AP.signal(out, lse, ro, rl) <= 1.0
    Tp, T, W = 1024, tp["T"], tp["W"]
    assert (T, W) == (192, 30)
    sites = [0, 63, 64, 127, 128, Tp - 1, Tp, Tp + 63, Tp + 64, Tp + T - 1, Tp + T, Tp + T + W - 1]
    assert set(sites) <= aimed
    for p in sites:                                                           # prefix keys, tail keys, window rows
        mo, ml = AP.ref(q, AP.mutate(tp, "M1-drop", p), kv=kv)
        sig = AP.signal(out, lse, mo, ml)
        assert sig >= 5.0, ("M1-drop", p, sig)
    # every sequence with its neighbour's tail (compressed tokens and window)
    K, V = kv
    swap = (np.concatenate([K[:, :, :Tp], np.roll(K[:, :, Tp:], -1, 0)], 2), np.concatenate([V[:, :, :Tp], np.roll(V[:, :, Tp:], -1, 0)], 2))
    mo, ml = AP.ref(q, tp, kv=swap)
    assert AP.signal(out, lse, mo, ml) >= 5.0
    # a prefix row order that mixes the sequences: sequence s's query over the prefix as the row of sequence s + 1 would read it
    # is the same prefix -- what differs per sequence is q, so rolling q must show as well
    mo, ml = AP.ref(np.roll(q, -1, 0), tp, kv=kv)
    assert AP.signal(out, lse, mo, ml) >= 5.0


# ------------------------------------------------------------------------------------------------ C. composition
@pytest.mark.parametrize("method,left", [("gearslKIVI", 0.02), ("gearlKIVI", 0.0)])
def test_shared_composes_to_the_plain_cache(method, left):
    """S = 1: prefix + tail built from the K / V and the seed of a plain cache.  The prefix buffers are the plain cache's segment 0
    bit for bit; attend_shared and attend() are each within the bounds of the same float64 reference."""
    from gear_amd.cache import GearKVCache
    cc = _cc(method, left=left)
    Hkv, Hq, Tp, w0, more = 2, 8, 256, 10, 150
    g = torch.Generator().manual_seed(4)
    k, v = _randn_kv(1, Hkv, Tp + w0 + more, g)
    plain = GearKVCache(1, Hkv, Tp + w0 + more + 128, cc, "cuda", seed=6)
    plain.prefill(k[:, :, :Tp + w0], v[:, :, :Tp + w0])
    state = plain.gen.get_state()
    plain.extend(k[:, :, Tp + w0:], v[:, :, Tp + w0:])
    pre = GearKVCache(1, Hkv, Tp, cc, "cuda", seed=6)
    pre.prefill(k[:, :, :Tp], v[:, :, :Tp])
    tail = GearKVCache(1, Hkv, w0 + more + 128, cc, "cuda", seed=6)
    tail.gen.set_state(state)                                                 # the blocks draw what the plain cache's blocks drew
    tail.extend(k[:, :, Tp:], v[:, :, Tp:])
    assert (plain.seg0, plain.n_comp, plain.n_win) == (Tp, Tp + 128, w0 + more - 128)
    assert (pre.n_comp, pre.kk0) == (Tp, plain.kk0) and (tail.n_comp, tail.n_win) == (128, plain.n_win)
    f, gq = plain.fpi, plain.group
    for name, sl in (("kcode", (Ellipsis, slice(0, Tp // f))), ("kscale", (Ellipsis, slice(0, Tp // gq))), ("kmn", (Ellipsis, slice(0, Tp // gq))),
                     ("vcode", (slice(None), slice(None), slice(0, Tp))), ("vscale", (slice(None), slice(None), slice(0, Tp))),
                     ("vmn", (slice(None), slice(None), slice(0, Tp))), ("kQtok", (slice(None), slice(None), slice(0, Tp))),
                     ("vQtok", (slice(None), slice(None), slice(0, Tp))), ("kPseg", (0,)), ("vPseg", (0,)),
                     ("koidx", (Ellipsis, slice(0, plain.kk0))), ("koval", (Ellipsis, slice(0, plain.kk0))),
                     ("voidx", (slice(None), slice(0, Tp))), ("voval", (slice(None), slice(0, Tp)))):
        if name in plain.bufs:
            assert torch.equal(pre.bufs[name][sl], plain.bufs[name][sl]), name
    parts = AP.decompose(plain)
    rng = np.random.default_rng(3)
    qs, _ = AP.decode_batches(parts, Hq, rng)
    qs.append(AP.f16(rng.standard_normal((1, Hq, 1, AP.D))))
    tp, kv = _joint_keys(pre, tail)
    Kj, Vj = AP.keys(parts)
    assert np.array_equal(Kj, kv[0]) and np.array_equal(Vj, kv[1])            # the joint keys ARE the plain cache's keys
    ro, rl = AP.ref(np.concatenate(qs, 2), parts)
    out, lse = _run(pre, tail, qs)
    _check(f"compose-shared[{method}]", out, lse, ro, rl)
    outs, lses = [], []
    for q in qs:
        o, l = plain.attend(torch.tensor(q, dtype=torch.float16, device="cuda"), return_lse=True)
        outs.append(host(o).astype(np.float64))
        lses.append(host(l).astype(np.float64)[:, :, None])
    _check(f"compose-plain[{method}]", np.concatenate(outs, 2), np.concatenate(lses, 2), ro, rl)


# ------------------------------------------------------------------------------------------------ D. no state change
def test_attend_shared_changes_no_state():
    pre, tail = _pair(_cc(), 3, 2, 256, 100, seed=4)
    before = [{k: t.clone() for k, t in c.bufs.items()} for c in (pre, tail)]
    counters = [(c.n_comp, c.n_win, c.seg0, c.kk0) for c in (pre, tail)]
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        tail.attend_shared(torch.randn(3, 8, 1, 128, generator=g).half().cuda(), pre, return_lse=True)
    tail.attend_shared(torch.randn(3, 8, 1, 128, generator=g).half().cuda(), pre)
    torch.cuda.synchronize()
    assert [(c.n_comp, c.n_win, c.seg0, c.kk0) for c in (pre, tail)] == counters
    for c, b in zip((pre, tail), before):
        for k, t in c.bufs.items():
            assert torch.equal(t, b[k]), k


def test_attend_shared_argument_checks():
    from gear_amd import _lib as L
    from gear_amd.cache import GearKVCache
    pre, tail = _pair(_cc(), 2, 2, 128, 10, seed=2)
    q = torch.zeros(2, 8, 1, 128, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError):
        tail.attend_shared(q, tail)                                           # the prefix must have batch 1
    with pytest.raises(ValueError):
        tail.attend_shared(q[:1], pre)                                        # q rows != sequences
    with pytest.raises(ValueError):
        tail.attend_shared(q, GearKVCache(1, 2, 128, _cc(bits=4), "cuda"))    # another compress config
    with pytest.raises(L.GearError):
        tail.attend_shared(q, GearKVCache(1, 2, 128, _cc(), "cuda"))          # an empty prefix: Tp = 0 is refused by the library
    with pytest.raises(L.GearError):
        tail.attend_shared(torch.zeros(2, 3, 1, 128, dtype=torch.float16, device="cuda"), pre)      # Hq % Hkv


# ------------------------------------------------------------------------------------------------ E. decoder
def _blocks_equal(pc, tc, T0, nb):
    """Layer-0 caches: the tail's nb decode-time blocks equal the plain cache's blocks behind its T0 prompt tokens, bit for bit."""
    f, g, R = pc.fpi, pc.group, pc.R
    n = nb * R
    assert torch.equal(tc.kcode[..., :n // f], pc.kcode[..., T0 // f:(T0 + n) // f])
    for nm in ("kscale", "kmn"):
        assert torch.equal(tc.bufs[nm][..., :n // g], pc.bufs[nm][..., T0 // g:(T0 + n) // g]), nm
    for nm in ("vcode", "vscale", "vmn", "kQtok", "vQtok"):
        assert torch.equal(tc.bufs[nm][:, :, :n], pc.bufs[nm][:, :, T0:T0 + n]), nm
    for nm in ("kPseg", "vPseg"):
        assert torch.equal(tc.bufs[nm][1:1 + nb], pc.bufs[nm][1:1 + nb]), nm
    kb = pc.kk_blk
    assert kb > 0 and tc.kk0 == 0
    assert torch.equal(tc.koidx[..., :nb * kb].int(), pc.koidx[..., pc.kk0:pc.kk0 + nb * kb].int() - T0)
    assert torch.equal(tc.koval[..., :nb * kb], pc.koval[..., pc.kk0:pc.kk0 + nb * kb])
    for nm in ("voidx", "voval"):
        assert torch.equal(tc.bufs[nm][:, :n], pc.bufs[nm][:, T0:T0 + n]), nm


def test_decoder_shared_matches_plain_teacher_forced():
    """S = 1, the same tokens fed to a plain batch-1 decoder and to a shared-prefix one, over three block boundaries."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    P, n = 150, 140                                                            # 128 compressed + 22; boundaries at 192, 256
    ids = torch.randint(0, 1000, (1, P + n), generator=torch.Generator().manual_seed(7)).cuda()
    plain = FastGearDecoder(model, 512, seed=3)
    sh = FastGearDecoder(model, 256, batch=1, seed=3, shared_prefix_tokens=128)
    lp, ls = plain.prefill(ids[:, :P]), sh.prefill_shared(ids[:, :P])
    assert ls.shape == (1, 1000) and torch.equal(lp, ls)
    assert sh.shared_live and sh.pos == P
    p0, t0, x0 = plain.layers[0]["cache"], sh.layers[0]["cache"], sh.layers[0]["prefix"]
    assert (x0.n_comp, x0.n_win, t0.n_comp, t0.n_win) == (128, 0, 0, 22)
    for nm in ("kcode", "vcode", "kscale", "vmn", "kQtok", "vQtok", "voidx"):    # the prefix payload = segment 0 of the plain decoder
        a, b = x0.bufs[nm], p0.bufs[nm]
        assert torch.equal(a, b[tuple(slice(0, s) for s in a.shape)]), nm
    assert torch.equal(x0.kPseg[0], p0.kPseg[0]) and x0.kk0 == p0.kk0
    worst = 1.0
    for i in range(n):
        a, b = plain.step(ids[:, P + i]), sh.step(ids[:, P + i])
        worst = min(worst, _cos(a, b))
        assert torch.equal(t0.kwin[:, :, :t0.n_win], p0.kwin[:, :, :p0.n_win]) and t0.n_win == p0.n_win      # layer 0: no attention upstream
        assert torch.equal(t0.vwin[:, :, :t0.n_win], p0.vwin[:, :, :p0.n_win])
    assert worst > 0.999, worst
    assert (p0.n_comp, t0.n_comp, sh.pos) == (256, 128, P + n) and p0.n_win == t0.n_win == (P + n) % 64
    _blocks_equal(p0, t0, 128, 2)


def test_decoder_shared_greedy_rows_equal_and_match_plain():
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    g = torch.Generator().manual_seed(3)
    P, gen = 120, 80
    ids = torch.randint(0, 1000, (1, P), generator=g).cuda()
    thr = _threshold(model, ids)
    plain, margins = _greedy(model, ids, P + gen)
    dec = FastGearDecoder(model, 256, batch=4, seed=8, shared_prefix_tokens=128)
    out = dec.generate(ids, P + gen, shared_prefix=True)
    assert out.shape == (4, P + gen) and torch.equal(out[:, :P], ids.expand(4, -1))
    for r in range(1, 4):
        assert torch.equal(out[r], out[0]), r
    _compare(out[:1], plain, margins, P, thr, 24)
    assert dec.layers[0]["prefix"].n_comp == 64 and dec.layers[0]["cache"].seq_len == P + gen - 1 - 64


def test_decoder_shared_sampling(left=0.02):
    """S = 8, temperature 1: every emitted token is sample_tokens of that step's own logits at its position; two runs with one seed
    are equal; the rows are not all equal.
    Two runs can only be equal if two identical attention calls are: gear_attn_decode_shared takes the vector kernels' DET
    instantiations, which add the outlier corrections as 64-bit integer sums (csrc/attention.hip, osum_add) -- a float sum through
    LDS atomics depends on the order in which waves run, and a draw that lies that close to a CDF boundary then takes the
    neighbouring token (measured with float sums: one of 8 rows parted after more than 60 equal tokens).
    test_attend_shared_is_bit_reproducible checks the attention call on its own."""
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.sampling import SamplingParams, sample_tokens
    model = _tiny("gearslKIVI" if left else "gearlKIVI", 2, left=left)
    P, gen, S = 100, 70, 8
    ids = torch.randint(0, 1000, (1, P), generator=torch.Generator().manual_seed(5)).cuda()
    sp = SamplingParams(1.0, 0, 1.0, 11)

    def run():
        dec = FastGearDecoder(model, 256, batch=S, seed=8, shared_prefix_tokens=64)
        seen = []
        pre, step = dec.prefill_shared, dec.step

        def rec(fn):
            def f(x):
                lg = fn(x)
                seen.append((lg.clone(), dec.pos))
                return lg
            return f
        dec.prefill_shared, dec.step = rec(pre), rec(step)
        return dec.generate(ids, P + gen, sampling=sp, shared_prefix=True), seen

    out, seen = run()
    assert out.shape == (S, P + gen) and len(seen) == gen
    for i, (lg, pos) in enumerate(seen):
        assert pos == P + i and lg.shape == (S, 1000)
        assert torch.equal(out[:, P + i], sample_tokens(lg, sp, pos=pos)[0]), i
    out2, _ = run()
    assert torch.equal(out, out2)
    assert not all(torch.equal(out[r], out[0]) for r in range(1, S))
    assert len({int(t) for t in out[:, P]}) > 1                               # the first token already differs: one logits row, S draws


def test_decoder_shared_sampling_without_outliers():
    """The same checks on a cache without outliers."""
    test_decoder_shared_sampling(left=0.0)


def test_decoder_shared_refusals():
    from gear_amd import _lib as L
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    with pytest.raises(NotImplementedError):
        FastGearDecoder(model, 256, batch=2, cache_kind="fp16", shared_prefix_tokens=128)
    with pytest.raises(NotImplementedError):
        FastGearDecoder(model, 256, batch=2, tp_rank=0, tp_world=2, shared_prefix_tokens=128)
    ids = torch.randint(0, 1000, (1, 150)).cuda()
    with pytest.raises(ValueError):
        FastGearDecoder(model, 256, batch=2).prefill_shared(ids)              # no prefix cache
    dec = FastGearDecoder(model, 256, batch=2, seed=1, shared_prefix_tokens=128)
    with pytest.raises(NotImplementedError):
        dec.generate(ids, 160, graph=True, shared_prefix=True)
    with pytest.raises(ValueError):
        dec.prefill_shared(ids.expand(2, -1))                                 # [2, T]: one prompt only
    with pytest.raises(ValueError):
        dec.prefill_shared(ids[0])
    snap = [{k: t.clone() for k, t in p.buf.items()} for p in (dec.pool, dec.prefix_pool)]
    with pytest.raises(L.GearError):
        dec.prefill_shared(torch.randint(0, 1000, (1, 200)).cuda())           # 192 compressed > the 128 the prefix cache holds
    assert dec.pos == 0 and not dec.shared_live
    for p, b in zip((dec.pool, dec.prefix_pool), snap):
        for k, t in p.buf.items():
            assert torch.equal(t, b[k]), k
    assert all(lw["cache"].seq_len == 0 and lw["prefix"].seq_len == 0 for lw in dec.layers)
    dec.prefill_shared(ids)
    assert dec.shared_live
    tok = torch.randint(0, 1000, (2, 3)).cuda()
    for call in (lambda: dec.extend(tok), lambda: dec.verify(tok), lambda: dec.accept(1), lambda: dec.step_graph(),
                 lambda: dec.step_graph_sampled(None), lambda: dec.generate_speculative(ids, 160)):
        with pytest.raises(NotImplementedError):
            call()
    assert dec.step(tok[:, :1]).shape == (2, 1000)                            # and the decoder is still usable


# ------------------------------------------------------------------------------------------------ F. allocation
def test_decoder_shared_allocation():
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    S, Tp_cap, tail_cap = 8, 1024, 128
    sh = FastGearDecoder(model, tail_cap, batch=S, shared_prefix_tokens=Tp_cap)
    un = FastGearDecoder(model, Tp_cap + tail_cap, batch=S)
    nbytes = lambda pool: sum(t.numel() * t.element_size() for t in pool.buf.values())
    for name, t in sh.prefix_pool.buf.items():
        assert t.shape[2 if name in ("kPseg", "vPseg") else 1] == 1, name     # [layers, (nseg,) batch = 1, ...]
    for name, t in sh.pool.buf.items():
        assert t.shape[2 if name in ("kPseg", "vPseg") else 1] == S, name
    shared, unshared = nbytes(sh.prefix_pool) + nbytes(sh.pool), nbytes(un.pool)
    print(f"allocated cache bytes: shared {shared} unshared {unshared} ({unshared / shared:.2f} x)")
    assert shared < unshared
