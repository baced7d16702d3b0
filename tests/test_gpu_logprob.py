"""gear_token_logprobs (csrc/logprob.hip) per element against the float64 reference of tests/logprob_ref.py, and the scoring surface
built on it: FastGearDecoder.score(), scoring.compare_caches(), generate(return_logprobs=True).

Tolerances.  lp, lse and top_lp: absolute error <= 1e-4 on finite values.  With |x| <= 32 every exp(x - m) carries a relative error
of at most about (|x - m| + 2) 2^-23 < 8e-6 (the argument's rounding in the multiply by log2(e), v_exp_f32's own ulp); a sum of
positive terms keeps that relative bound, so log(sum) moves by < 8e-6; the fp32 accumulation and the final log (done in fp64 and
rounded once) add less than 1e-6.  1e-4 leaves a factor of about 10.  kl: <= 2e-4 by the same argument (two such sums and the
mass-weighted difference), kl >= -1e-6, and exactly 0.0 when ref_logits is logits.  Only the rows that hold +-65504 produce values
beyond 1024 in magnitude; an fp32 output cannot be closer than half an ulp there, which logprob_ref.tolerance adds (nothing below
1024).  rank, agree and top_idx are exact: the random rows have no ties among their leaders (asserted on the CPU,
tests/test_logprob_ref_cpu.py) and the tie rows follow the lowest-index rule on both sides.  NaN, -inf and ignored outputs:
exactly as specified."""
import functools

import numpy as np
import pytest
import torch

import logprob_ref as R

pytestmark = pytest.mark.gpu


def _dev(a, ld, fill=float("nan")):
    """numpy fp16 [N, V] -> a [N, V] view of a cuda [N, ld] buffer whose pitch gap holds `fill`."""
    N, V = a.shape
    buf = torch.full((N, ld), fill, dtype=torch.float16, device="cuda")
    buf[:, :V] = torch.from_numpy(a).cuda()
    return buf[:, :V]


def _run(x, ids, r=None, k=0):
    from gear_amd.scoring import token_logprobs
    o = token_logprobs(x, ids, r, k)
    torch.cuda.synchronize()
    g = lambda t: None if t is None else t.cpu().numpy()      # noqa: E731
    return dict(lp=g(o.logprobs), lse=g(o.lse), rank=g(o.rank), kl=g(o.kl), agree=g(o.agree), top_idx=g(o.top_idx),
                top_lp=g(o.top_logprobs))


def _close(got, want, base, what):
    """Finite reference values within the bound; NaN / +-inf exactly where the reference has them."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    err = np.abs(got[fin] - want[fin])
    tol = R.tolerance(want[fin], base)
    worst = float((err - tol).max()) if err.size else -1.0
    print(f"{what}: max abs err {float(err.max()) if err.size else 0.0:.3e}")
    assert worst <= 0.0, (what, float(err.max()))


def _check(out, ref, k, has_ref, what):
    _close(out["lp"], ref["lp"], 1e-4, what + " lp")
    _close(out["lse"], ref["lse"], 1e-4, what + " lse")
    assert np.array_equal(out["rank"], ref["rank"]), what + " rank"
    if k:
        assert np.array_equal(out["top_idx"], ref["top_idx"]), what + " top_idx"
        _close(out["top_lp"], ref["top_lp"], 1e-4, what + " top_lp")
    else:
        assert out["top_idx"] is None and out["top_lp"] is None
    if has_ref:
        _close(out["kl"], ref["kl"], 2e-4, what + " kl")
        k_ok = out["kl"][~np.isnan(out["kl"])]
        assert (k_ok >= -1e-6).all(), what + " kl sign"
        assert np.array_equal(out["agree"], ref["agree"]), what + " agree"
    else:
        assert out["kl"] is None and out["agree"] is None


@functools.lru_cache(maxsize=None)
def _uniform_case(V, N):
    x, ids, r = R.uniform_rows(N, V, V + N), R.random_ids(N, V, V + N), R.uniform_rows(N, V, V + N + 50)
    refs = {k: R.reference(x, ids, r, min(k, V)) for k in R.K_TOPS}      # computed once, shared by the three pitches
    return x, ids, r, refs


@pytest.mark.parametrize("pitch", R.PITCHES)
@pytest.mark.parametrize("V,N", R.SHAPES)
def test_kernel_matches_float64_reference(V, N, pitch):
    x, ids, r, refs = _uniform_case(V, N)
    ld = R.pitch_of(pitch, V)
    xd, rd, idd = _dev(x, ld), _dev(r, ld), torch.from_numpy(ids).cuda()
    for k in R.K_TOPS:
        if k > V:                                            # V = 7: k_top = 8 is an argument error, 7 is the most there is
            with pytest.raises(ValueError):
                _run(xd, idd, None, k)
            k = V
            refs = dict(refs)
            refs[k] = R.reference(x, ids, r, k)
        for has_ref in (False, True):
            _check(_run(xd, idd, rd if has_ref else None, k), refs[k], k, has_ref, f"V={V} N={N} ld={ld} k={k} ref={has_ref}")


@pytest.mark.parametrize("V", [7, 64, 1003, 128256])
def test_value_cases(V):
    for name, x, ids, r, _ in R.special_rows(V):
        for ld in (V, V + 1):
            xd, rd, idd = _dev(x, ld), _dev(r, ld), torch.from_numpy(ids).cuda()
            for k in (0, min(8, V)):
                _check(_run(xd, idd, rd, k), R.reference(x, ids, r, k), k, True, f"{name} V={V} ld={ld} k={k}")
    # ignored and out-of-range ids, spelled out
    name, x, ids, r, _ = R.special_rows(V)[-1]
    out = _run(_dev(x, V), torch.from_numpy(ids).cuda())
    assert out["lp"][0] == 0.0 and out["lp"][3] == 0.0 and np.isnan(out["lp"][1]) and np.isnan(out["lp"][2])
    assert out["rank"].tolist() == [-1, -1, -1, -1] and np.isfinite(out["lse"]).all()


def test_sliced_3d_view_needs_no_copy():
    B, n, V = 3, 9, 1003
    x = R.uniform_rows(B * n, V, 11).reshape(B, n, V)
    r = R.uniform_rows(B * n, V, 12).reshape(B, n, V)
    ids = R.random_ids(B * (n - 1), V, 13).reshape(B, n - 1)
    xd, rd = torch.from_numpy(x).cuda(), torch.from_numpy(r).cuda()
    from gear_amd.scoring import token_logprobs
    o = token_logprobs(xd[:, :-1], torch.from_numpy(ids).cuda(), rd[:, :-1], 8)
    assert o.logprobs.shape == (B, n - 1) and o.top_idx.shape == (B, n - 1, 8)
    ref = R.reference(x[:, :-1].reshape(-1, V), ids.reshape(-1), r[:, :-1].reshape(-1, V), 8)
    out = dict(lp=o.logprobs, lse=o.lse, rank=o.rank, kl=o.kl, agree=o.agree, top_idx=o.top_idx, top_lp=o.top_logprobs)
    out = {k: t.cpu().numpy().reshape((-1,) + tuple(t.shape[2:])) for k, t in out.items()}
    _check(out, ref, 8, True, "sliced [B, n, V][:, :-1]")
    # the evenly spaced 3-D case goes in one launch and gives the same bits as its rows one by one
    full = token_logprobs(xd, torch.from_numpy(R.random_ids(B * n, V, 14).reshape(B, n)).cuda())
    rows = token_logprobs(xd.reshape(-1, V), torch.from_numpy(R.random_ids(B * n, V, 14)).cuda())
    assert torch.equal(full.logprobs.reshape(-1), rows.logprobs)


def test_kl_is_exactly_zero_against_itself():
    for V in (1003, 128256):
        x, ids, _, _ = _uniform_case(V, 1 if V > 5000 else 3)
        xd = _dev(x, V + 1)
        out = _run(xd, torch.from_numpy(ids).cuda(), xd, 0)
        assert (out["kl"] == 0.0).all() and (out["agree"] == 1).all()


def _bits(out):
    return {k: (None if v is None else v.view(np.int32) if v.dtype == np.float32 else v) for k, v in out.items()}


def _same_bits(a, b, rows_a, rows_b, what):
    a, b = _bits(a), _bits(b)
    for k in a:
        assert (a[k] is None) == (b[k] is None)
        if a[k] is not None:
            assert np.array_equal(a[k][rows_a], b[k][rows_b]), (what, k)


@pytest.mark.parametrize("V", [1003, 4099, 128256])
def test_row_independence_reproducibility_and_poisoned_padding(V):
    N = 300 if V < 100000 else 5
    x, ids, r, _ = _uniform_case(V, N)
    x, ids, r = x.copy(), ids.copy(), r.copy()
    fixed_x, fixed_r, fixed_id = R.uniform_rows(1, V, 99), R.uniform_rows(1, V, 98), V // 3
    alone = _run(_dev(fixed_x, V), torch.tensor([fixed_id]).cuda(), _dev(fixed_r, V), 8)
    for pos in sorted({0, N // 2, N - 1}):
        xx, rr, ii = x.copy(), r.copy(), ids.copy()
        xx[pos], rr[pos], ii[pos] = fixed_x[0], fixed_r[0], fixed_id
        batch = _run(_dev(xx, V), torch.from_numpy(ii).cuda(), _dev(rr, V), 8)
        _same_bits(alone, batch, slice(0, 1), slice(pos, pos + 1), f"row {pos} of {N}")
    xd, rd, idd = _dev(x, V), _dev(r, V), torch.from_numpy(ids).cuda()
    a, b = _run(xd, idd, rd, 8), _run(xd, idd, rd, 8)
    _same_bits(a, b, slice(None), slice(None), "two identical calls")
    # pitch gaps full of +inf / NaN: no output may change.  (A pitch of V + 8 keeps every row's alignment; V + 1 shifts it, which
    # changes where the 16-byte loads start but never the per-thread column order of a row with the same alignment -- so the
    # comparison is against the same pitch with a harmless gap.)
    for ld in (V + 1, V + 8):
        clean = _run(_dev(x, ld, 0.0), idd, _dev(r, ld, 0.0), 8)
        for fill in (float("inf"), float("nan")):
            _same_bits(clean, _run(_dev(x, ld, fill), idd, _dev(r, ld, fill), 8), slice(None), slice(None), f"gap {fill} ld {ld}")


@pytest.mark.parametrize("V", [1003, 128256])
def test_mutations_move_lse_as_predicted_and_ids_swap_lp(V):
    x = R.uniform_rows(1, V, 21)
    ids = torch.tensor([V // 2]).cuda()
    base = R.reference(x, [V // 2])["lse"][0]
    for col in (0, V - 1, V - 1 - (V % 8)):
        y = x.copy()
        y[0, col] = np.float16(40.0)                          # an entry that outweighs the whole row: the sum must see exactly this column
        want = R.reference(y, [V // 2])["lse"][0]
        assert abs(want - base) > 1.0                         # the mutation is far above the tolerance
        for ld in (V, V + 1):
            got = _run(_dev(y, ld), ids)["lse"][0]
            assert abs(float(got) - want) <= 1e-4, (col, ld, float(got), want)
    x2 = R.uniform_rows(2, V, 22)
    i2 = np.array([3, V - 2])
    a = _run(_dev(np.stack([x2[0], x2[0]]), V), torch.from_numpy(i2).cuda())["lp"]
    b = _run(_dev(np.stack([x2[0], x2[0]]), V), torch.from_numpy(i2[::-1].copy()).cuda())["lp"]
    assert a[0] != a[1] and a.view(np.int32).tolist() == b.view(np.int32).tolist()[::-1]


# ------------------------------------------------------------------------------------------------- the decoders
def _tiny():
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    cfg = LlamaConfigLite(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2,
                          num_attention_heads=4, num_key_value_heads=2, k_bits=2, v_bits=2)
    cc = dict(compress_method="gearslKIVI", group_size=64, residual=64, quantize_bit=2, rank=4, rankv=4, loop=3, left=0.02)
    torch.manual_seed(0)
    return LlamaForCausalLM_GEARKIVI(cfg, cc).half().cuda().eval()


@functools.lru_cache(maxsize=None)
def _model():
    return _tiny()


P_LEN, T_LEN = 150, 291          # 150 prompt + 140 scored tokens (+ the first scored position from the prefill logits): blocks at 192, 256


def _ids(B=2, T=T_LEN, seed=1):
    return torch.randint(0, 1000, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()


def _dec(kind="gear", batch=2, **kw):
    from gear_amd.fast_decode import FastGearDecoder
    return FastGearDecoder(_model(), 512, batch=batch, seed=3, cache_kind=kind, **kw)


def _tap(dec):
    """Record the logits this decoder's prefill / prefill_shared / step / extend / extend_shared calls return, in call order; for
    the graph steps (step_graph / step_graph_sampled) a copy of the graph's static logits buffer taken right after the replay."""
    rec = []
    for name in ("prefill", "prefill_shared", "step", "extend", "extend_shared"):
        def wrap(*a, _f=getattr(dec, name), **kw):
            out = _f(*a, **kw)
            rec.append(out)
            return out
        setattr(dec, name, wrap)
    for name, buf in (("step_graph", "logits_static"), ("step_graph_sampled", "logits_sampled_static")):
        def wrap_g(*a, _f=getattr(dec, name), _buf=buf, **kw):
            out = _f(*a, **kw)
            rec.append(getattr(dec, _buf).clone())
            return out
        setattr(dec, name, wrap_g)
    return rec


def _cross_bound(logits):
    """How far the log-probs of two gear decoders fed the same tokens may lie apart.  Their compressed payloads differ in the last
    bits (float atomics in the compressor's low-rank step, csrc/lowrank.hip); through the layers that flips fp16 roundings, so a
    logit moves by whole fp16 ulps.  The bound allows 4 ulps at the largest logit recorded (the log-sum-exp moves by no more than
    the logits do): 4 * 2^(floor(log2 max|x|) - 10)."""
    m = float(logits.float().abs().max())
    return 4.0 * 2.0 ** (np.floor(np.log2(m)) - 10)


def _record_steps(dec, ids, P):
    """prefill + step by hand: the logits that predict positions P .. T - 1, [B, T - P, V]."""
    lg = [dec.prefill(ids[:, :P])]
    for t in range(P, ids.shape[1] - 1):
        lg.append(dec.step(ids[:, t:t + 1]))
    return torch.stack(lg, 1)


@pytest.mark.parametrize("kind", ["gear", "fp16", "kivi"])
def test_score_step_equals_recorded_logits_and_leaves_the_same_state(kind):
    from gear_amd.scoring import token_logprobs
    ids = _ids()
    a, b = _dec(kind), _dec(kind)
    own = _tap(a)
    res = a.score(ids, P_LEN, mode="step", top_k=3)
    lg = _record_steps(b, ids, P_LEN)
    if kind == "gear":
        # Two gear decoders with one seed are not bit-identical: the low-rank step of the compressor sums with float atomics
        # (csrc/lowrank.hip), so the payload depends on arrival order.  The bit-for-bit comparison therefore runs against the logits
        # this decoder's own prefill / step calls returned; the second decoder gives the state to compare and log-probs that must
        # lie within _cross_bound, as those of a third plain decoder do (their spread is printed: the figure in DESIGN.md).
        lp_b = token_logprobs(lg, ids[:, P_LEN:]).logprobs
        lp_c = token_logprobs(_record_steps(_dec(kind), ids, P_LEN), ids[:, P_LEN:]).logprobs
        bound = _cross_bound(lg)
        print(f"two plain gear decoders, {tuple(lp_b.shape)} log-probs: max |diff| {float((lp_b - lp_c).abs().max()):.3e}, "
              f"{int((lp_b != lp_c).sum())} of {lp_b.numel()} differ; score() vs plain {float((res.logprobs - lp_b).abs().max()):.3e}; "
              f"bound {bound:.3e}")
        assert (lp_b - lp_c).abs().max() <= bound and (res.logprobs - lp_b).abs().max() <= bound
        lg = torch.stack(own, 1)
    want = token_logprobs(lg, ids[:, P_LEN:], top_k=3)
    assert res.logprobs.shape == (2, T_LEN - P_LEN) and res.logprobs.dtype == torch.float32
    assert torch.equal(res.logprobs.view(torch.int32), want.logprobs.view(torch.int32))
    assert torch.equal(res.rank, want.rank) and torch.equal(res.top_idx, want.top_idx)
    assert torch.equal(res.top_logprobs.view(torch.int32), want.top_logprobs.view(torch.int32))
    ref = R.reference(lg.reshape(-1, 1000).cpu().numpy(), ids[:, P_LEN:].reshape(-1).cpu().numpy())
    _close(res.logprobs.cpu().numpy(), ref["lp"], 1e-4, f"score step {kind}")
    assert abs(res.nll + ref["lp"].mean()) < 1e-4 and abs(res.perplexity - np.exp(-ref["lp"].mean())) < 1e-3 * res.perplexity
    assert res.top1 == float((ref["rank"] == 0).mean()) and res.kl is None and res.kl_mean is None
    ca, cb = a.layers[0]["cache"], b.layers[0]["cache"]
    assert a.pos == b.pos == T_LEN - 1
    for name in ("n_comp", "n_win", "seg0", "kk0", "n_tok", "n_kwin", "n_kpacked", "n_vpacked"):
        assert getattr(ca, name, None) == getattr(cb, name, None), name
    nw = getattr(ca, "n_win", None) or getattr(ca, "n_kwin", 0)
    if kind == "gear":                                        # (layer 0's K / V rows depend on the token embeddings only)
        assert nw > 0
    assert torch.equal(ca.kwin[:, :, :nw], cb.kwin[:, :, :nw])
    if hasattr(ca, "vwin"):
        assert torch.equal(ca.vwin[:, :, :nw], cb.vwin[:, :, :nw])
    else:
        assert torch.equal(ca.vring, cb.vring)               # KIVI: the sliding fp16 V ring


@pytest.mark.parametrize("kind", ["gear", "fp16"])
def test_score_extend_equals_extends_own_logits(kind):
    from gear_amd.scoring import token_logprobs
    ids = _ids()
    a, b = _dec(kind), _dec(kind)
    res = a.score(ids, P_LEN, mode="extend", chunk=48)
    pieces = [token_logprobs(b.prefill(ids[:, :P_LEN]), ids[:, P_LEN]).logprobs.view(2, 1)]
    for t in range(P_LEN, T_LEN - 1, 48):
        e = min(t + 48, T_LEN - 1)
        pieces.append(token_logprobs(b.extend(ids[:, t:e]), ids[:, t + 1:e + 1]).logprobs)
    want = torch.cat(pieces, 1)
    assert torch.equal(res.logprobs.view(torch.int32), want.view(torch.int32))
    assert a.pos == b.pos and a.layers[0]["cache"].n_win == b.layers[0]["cache"].n_win


def test_score_refusals():
    from gear_amd._lib import GearError
    ids = _ids()
    k = _dec("kivi")
    with pytest.raises(NotImplementedError):
        k.score(ids, P_LEN, mode="extend")
    assert k.pos == 0
    assert k.score(ids[:, :160], P_LEN, mode="step").logprobs.shape == (2, 10)
    from gear_amd.fast_decode import FastGearDecoder
    small = FastGearDecoder(_model(), 128, batch=2, cache_kind="gear")
    with pytest.raises(GearError, match="do not fit"):
        small.score(ids, P_LEN)
    assert small.pos == 0 and small.layers[0]["cache"].seq_len == 0
    with pytest.raises(ValueError):
        small.score(ids, T_LEN)
    with pytest.raises(ValueError):
        small.score(ids, P_LEN, mode="chunk")


def test_compare_caches():
    from gear_amd.scoring import compare_caches
    ids = _ids(T=230)
    P = 150
    same = compare_caches(_model(), ids, P, kinds=("fp16", "fp16"), max_tokens=512, seed=3)
    assert same[0].kl is None and (same[1].kl == 0).all() and (same[1].agree == 1).all() and same[1].kl_mean == 0.0
    assert torch.equal(same[0].logprobs, same[1].logprobs)
    from gear_amd.fast_decode import FastGearDecoder
    taps = []
    init = FastGearDecoder.__init__

    def tapped(self, *a, **kw):
        init(self, *a, **kw)
        taps.append(_tap(self))

    FastGearDecoder.__init__ = tapped                         # the decoders compare_caches builds record their own logits
    try:
        res = compare_caches(_model(), ids, P, kinds=("fp16", "gear", "kivi"), max_tokens=512, seed=3)
    finally:
        FastGearDecoder.__init__ = init
    kl = res[1].kl
    assert kl.shape == (2, 230 - P) and torch.isfinite(kl).all() and (kl >= -1e-6).all()
    assert len(res) == 3 and res[0].kl is None
    lf, lgr, lkv = (torch.stack(t, 1).reshape(-1, 1000).cpu().numpy() for t in taps)
    for i, (kind, lx) in enumerate((("gear", lgr), ("kivi", lkv)), 1):
        ref = R.reference(lx, ids[:, P:].reshape(-1).cpu().numpy(), lf)
        print(f"compare_caches {kind}: kl_mean {res[i].kl_mean:.6f} (float64 {ref['kl'].mean():.6f}), agree {res[i].agree_rate:.3f}")
        assert torch.isfinite(res[i].kl).all() and (res[i].kl >= -1e-6).all()
        assert abs(res[i].kl_mean - ref["kl"].mean()) <= 2e-4
        assert abs(res[i].agree_rate - float(ref["agree"].mean())) < 1e-12
        _close(res[i].kl.cpu().numpy(), ref["kl"], 2e-4, f"compare_caches {kind} kl")
        _close(res[i].logprobs.cpu().numpy(), ref["lp"], 1e-4, f"compare_caches {kind} lp")
    assert torch.equal(res[0].logprobs, same[0].logprobs)


def _generate_pair(dec_a, dec_b, ids, L, **kw):
    """(tokens, logprobs, the logits dec_b's own calls returned): the tokens equal those of the call without the keyword."""
    toks = dec_a.generate(ids, L, **kw)
    assert isinstance(toks, torch.Tensor)                    # without the keyword: a tensor, as before
    own = _tap(dec_b)
    out = dec_b.generate(ids, L, return_logprobs=True, **kw)
    assert isinstance(out, tuple) and len(out) == 2
    assert torch.equal(out[0], toks)
    return out[0], out[1], own


@pytest.mark.parametrize("how", ["greedy", "sampled"])
def test_generate_return_logprobs(how):
    from gear_amd.sampling import SamplingParams
    from gear_amd.scoring import token_logprobs
    kw = {} if how == "greedy" else dict(sampling=SamplingParams(1.0, 0, 1.0, 11))
    ids = _ids(T=100, seed=4)
    L = 140                                                  # crosses the block boundary at 128
    toks, lps, own = _generate_pair(_dec(), _dec(), ids, L, **kw)
    assert lps.shape == (2, L - 100) and lps.dtype == torch.float32
    # the logits every emitted token was taken from: the emitting decoder's own (a second gear decoder differs in the last bits:
    # float atomics in the compressor's low-rank step)
    want = token_logprobs(torch.stack(own, 1), toks[:, 100:]).logprobs
    assert torch.equal(lps.view(torch.int32), want.view(torch.int32))
    plain = _record_steps(_dec(), toks, 100)
    bound = _cross_bound(plain)
    assert (lps - token_logprobs(plain, toks[:, 100:]).logprobs).abs().max() <= bound
    # graph=True: the kernel runs after each replay on the graph's static logits buffer -- bit for bit against copies of that
    # buffer taken after every replay (and the prefill / warm-up step logits in front of them)
    g = _dec()
    g_own = _tap(g)
    g_toks, g_lps = g.generate(ids, L, graph=True, return_logprobs=True, **kw)
    assert g_lps.shape == lps.shape and torch.equal(g_toks[:, :100], ids) and len(g_own) == L - 100
    assert g.graph is not None or g.graph_sampled is not None
    g_want = token_logprobs(torch.stack(g_own, 1), g_toks[:, 100:]).logprobs
    assert torch.equal(g_lps.view(torch.int32), g_want.view(torch.int32))
    if how == "greedy":
        # same tokens and, up to what separates any two gear decoders, the same log-probs as graph=False
        assert torch.equal(g_toks, toks) and (g_lps - lps).abs().max() <= bound
    else:
        # a draw at temperature 1 over the whole vocabulary can flip on the last-bit differences between two gear decoders, and
        # every later token follows it: the graph run's log-probs are compared on its own tokens, teacher-forced through a plain
        # decoder; the first token comes from the (dense, reproducible) prefill row
        again = token_logprobs(_record_steps(_dec(), g_toks, 100), g_toks[:, 100:]).logprobs
        assert (g_lps - again).abs().max() <= bound
        assert torch.equal(g_toks[:, :101], toks[:, :101])


def test_generate_return_logprobs_shared_prefix():
    from gear_amd.sampling import SamplingParams
    from gear_amd.scoring import token_logprobs
    S = SamplingParams(1.0, 0, 1.0, 11)
    ids = _ids(B=1, T=140, seed=5)
    L = 170
    mk = lambda: _dec(batch=4, shared_prefix_tokens=192)      # noqa: E731
    toks, lps, own = _generate_pair(mk(), mk(), ids, L, shared_prefix=True, sampling=S)
    assert toks.shape == (4, L) and lps.shape == (4, L - 140)
    want = token_logprobs(torch.stack(own, 1), toks[:, 140:]).logprobs
    assert torch.equal(lps.view(torch.int32), want.view(torch.int32))
    # with a suffix per sequence: the first token comes from the last extend_shared() row
    suf = _ids(B=4, T=9, seed=6)
    toks2, lps2, own = _generate_pair(mk(), mk(), ids, L, shared_prefix=True, suffix_ids=suf, sampling=S)
    assert lps2.shape == (4, L - 149)
    lg = [own[1][:, -1]] + own[2:]                           # (own[0]: the prefill_shared row, not sampled from with a suffix)
    want = token_logprobs(torch.stack(lg, 1), toks2[:, 149:]).logprobs
    assert torch.equal(lps2.view(torch.int32), want.view(torch.int32))


def test_score_extend_allocates_no_fp32_copy_of_the_logits():
    B, T, V, c = 2, 600, 1000, 64
    ids = _ids(B=B, T=T, seed=8)
    from gear_amd.fast_decode import FastGearDecoder
    probe = FastGearDecoder(_model(), 1024, batch=B, seed=3)
    P = 64
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    probe.prefill(ids[:, :P])                                # the calls score() makes, without the scoring and with every result
    for t in range(P, T - 1, c):                             # dropped at once: what extend(64) itself needs on a fresh decoder --
        probe.extend(ids[:, t:min(t + c, T - 1)])            # its activations, the returned logits and the per-layer attention
    torch.cuda.synchronize()                                 # workspaces, which a decoder allocates at first use and grows with
    act = torch.cuda.max_memory_allocated() - m0             # the context (score() starts from an empty decoder, so it pays them too)
    del probe
    dec = FastGearDecoder(_model(), 1024, batch=B, seed=3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = dec.score(ids, P, mode="extend", chunk=c)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    budget = 4 * B * c * V * 2 + act
    print(f"score(extend, chunk {c}): peak {peak} bytes over the pre-call figure, budget {budget} (extend({c}) itself {act})")
    assert res.logprobs.shape == (B, T - P)
    assert peak < budget
    assert budget < act + (T - P) * B * V * 4               # a full fp32 log-softmax of the scored positions would not fit it
