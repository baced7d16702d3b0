"""gear_sample_tokens on the GPU against the float64 reference (tests/sample_ref.py): one-token resolution with aimed uniforms, the
Philox stream, the sampled distribution (chi-square), greedy equivalences, determinism and graph capture, speculative rejection
sampling; then the decoders that use it (FastGearDecoder.generate / generate_speculative, the hook model, harness.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sample_ref as R
from gear_amd.sampling import SamplingParams, sample_tokens

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
MARGIN = 2e-6          # aimed uniforms stay this far inside their interval (fp32 u, 32.32 fixed-point masses)


def _chi2_bound(df: int) -> float:
    """1 - 1e-6 quantile of chi-square(df), Wilson-Hilferty (131.4 at df 63, 56.5 at df 15)."""
    z = 4.753424
    return df * (1 - 2 / (9 * df) + z * np.sqrt(2 / (9 * df))) ** 3


def _chi2(counts: np.ndarray, p: np.ndarray) -> tuple:
    """Pearson statistic over the bins of p > 0, bins with expected count < 5 merged into one."""
    N = counts.sum()
    exp = N * p
    big = exp >= 5
    obs = list(counts[big]) + ([counts[~big & (p > 0)].sum()] if (~big & (p > 0)).any() else [])
    ex = list(exp[big]) + ([exp[~big & (p > 0)].sum()] if (~big & (p > 0)).any() else [])
    obs, ex = np.array(obs, np.float64), np.array(ex, np.float64)
    return float(((obs - ex) ** 2 / ex).sum()), len(ex) - 1


def _row(V, dtype, gen, scale=2.0, step=None, ninf=0.0):
    x = torch.randn(V, generator=gen) * scale
    if step:
        x = torch.round(x / step) * step                        # many ties (top-k edge, top-p groups)
    if ninf:                                                     # masked columns; the row keeps its largest value
        m = torch.rand(V, generator=gen) < ninf
        m[int(torch.argmax(x))] = False
        x[m] = float("-inf")
    return x.to(dtype)


def _top_p_clear(x32, top_k, top_p):
    """The top-p decision of every value is at least MARGIN away from the threshold (fixed-point vs float64 masses)."""
    if top_p >= 1:
        return True
    x = np.asarray(x32, np.float64)
    keep = R.kept_mask(x32, top_k, 1.0)
    p = R.probs(x32, keep)
    vals = np.unique(x[keep])[::-1]
    mass = np.array([p[keep & (x == v)].sum() for v in vals])
    above = np.concatenate([[0.0], np.cumsum(mass)[:-1]])
    return bool(np.all(np.abs(above - top_p) > MARGIN))


PARAMS = [(1.0, 0, 1.0), (0.8, 50, 0.95), (1.0, 0, 0.9), (0.7, 5, 1.0), (1.3, 0, 0.5), (0.6, 1000, 0.8)]


# ------------------------------------------------------------------------------------------------- 1. one-token resolution
@pytest.mark.parametrize("V", [1, 7, 1000, 32000, 128256])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_aimed_uniforms_pick_every_kept_token(V, dtype):
    gen = torch.Generator().manual_seed(V + (dtype == torch.float32))
    checked = 0
    for ci, (t, k, p) in enumerate(PARAMS):
        for attempt in range(20):
            raw = _row(V, dtype, gen, scale=2.0 if V < 100000 else 3.0, step=0.25 if ci % 2 else None, ninf=0.05 if ci == 2 else 0.0)
            x32 = R.scaled(raw.float().numpy(), t)
            if _top_p_clear(x32, k, p):
                break
        keep = R.kept_mask(x32, k, p)
        iv = [(i, lo, hi) for i, lo, hi in R.intervals(x32, keep) if hi - lo > 2 * MARGIN]
        idx = sorted(set(np.nonzero(keep)[0].tolist()))
        # the first and last kept tokens, the lowest kept value (top-k tie edge / top-p boundary), and a sample of the rest
        xs = np.asarray(x32, np.float64)
        must = {idx[0], idx[-1]} | {i for i in idx if xs[i] == xs[keep].min()}
        chosen = [c for c in iv if c[0] in must]
        rest = [c for c in iv if c[0] not in must]
        if len(rest) > 200:
            rest = [rest[j] for j in np.linspace(0, len(rest) - 1, 200).astype(int)]
        chosen += rest
        assert chosen, (V, t, k, p)
        u = torch.tensor([[np.float32((lo + hi) / 2), 0.0] for _, lo, hi in chosen], dtype=torch.float32)
        ok = (u[:, 0].double().numpy() > np.array([lo for _, lo, _ in chosen]) + MARGIN / 2) & \
             (u[:, 0].double().numpy() < np.array([hi for _, _, hi in chosen]) - MARGIN / 2)
        rows = raw.to(DEV).unsqueeze(0).repeat(len(chosen), 1)
        tok, acc, lp = sample_tokens(rows, SamplingParams(t, k, p, seed=1), pos=0, u=u.to(DEV))
        tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
        want = np.array([i for i, _, _ in chosen])
        assert np.array_equal(tok[ok], want[ok]), (V, dtype, t, k, p, np.nonzero(tok[ok] != want[ok])[0][:5])
        assert (acc.cpu() == 0).all()
        pr = R.probs(x32, keep)
        assert np.abs(lp - np.log(pr[tok])).max() < 1e-5, (V, t, k, p)
        assert keep[tok].all()
        checked += int(ok.sum())
    assert checked >= 6


# ------------------------------------------------------------------------------------------------- 2. the Philox stream
def test_generator_draws_match_the_reference():
    gen = torch.Generator().manual_seed(5)
    rows, V, nps, pos0, seed = 1200, 1000, 3, 17, 0x1234_5678_9ABC
    prm = SamplingParams(0.9, 40, 0.95, seed)
    raw = torch.randn(rows, V, generator=gen).half()
    pos_dev = torch.tensor([100, 0, 0, 0], dtype=torch.int32, device=DEV)
    tok, acc, lp = sample_tokens(raw.to(DEV), prm, pos=pos0, n_per_seq=nps, pos_dev=pos_dev)
    tok = tok.cpu().numpy()
    skipped = 0
    for r in range(rows):
        P, b = 100 + pos0 + r % nps, r // nps
        u = R.uniform(seed, P, b, 0)
        x32 = R.scaled(raw[r].float().numpy(), prm.temperature)
        keep = R.kept_mask(x32, prm.top_k, prm.top_p)
        iv = R.intervals(x32, keep)
        if not _top_p_clear(x32, prm.top_k, prm.top_p) or min(min(abs(u - lo), abs(u - hi)) for _, lo, hi in iv) < 1e-5:
            skipped += 1
            continue
        want = R.sample_row(raw[r].float().numpy(), prm.temperature, prm.top_k, prm.top_p, u)[0]
        assert tok[r] == want, (r, tok[r], want)
    assert skipped < rows // 100


# ------------------------------------------------------------------------------------------------- 3. the distribution
@pytest.mark.parametrize("t,k,p", [(1.0, 0, 1.0), (0.8, 20, 1.0), (1.0, 0, 0.9), (0.7, 30, 0.95)])
def test_distribution_chi_square(t, k, p):
    gen = torch.Generator().manual_seed(11)
    V, N = 64, 1 << 18
    for _ in range(20):
        raw = torch.randn(V, generator=gen) * 1.5
        x32 = R.scaled(raw.numpy(), t)
        if _top_p_clear(x32, k, p):
            break
    keep = R.kept_mask(x32, k, p)
    pr = R.probs(x32, keep)
    rows = raw.to(DEV).unsqueeze(0).repeat(N, 1)
    tok, _, _ = sample_tokens(rows, SamplingParams(t, k, p, seed=99), pos=3)
    counts = np.bincount(tok.cpu().numpy(), minlength=V)
    assert counts[~keep].sum() == 0
    stat, df = _chi2(counts, pr)
    assert stat < _chi2_bound(df), (stat, df)


# ------------------------------------------------------------------------------------------------- 4. greedy equivalences
@pytest.mark.parametrize("B", [1, 4, 16])
def test_greedy_equivalences(B):
    gen = torch.Generator().manual_seed(B)
    x = (torch.randn(B, 32000, generator=gen) * 3).half().to(DEV)
    x[0, 100] = x[0, 200] = x[0].max() + 1          # a tie at the max: the first index wins
    want = torch.argmax(x, -1)
    assert int(want[0]) == 100
    tok, _, lp = sample_tokens(x, SamplingParams(temperature=0, top_k=7, top_p=0.3), pos=5)
    assert torch.equal(tok, want) and (lp == 0).all()
    xf = torch.randn(B, 32000, generator=gen).to(DEV)    # fp32: no ties
    assert (xf.topk(2, -1).values[:, 0] > xf.topk(2, -1).values[:, 1]).all()
    tok, _, lp = sample_tokens(xf, SamplingParams(temperature=1.0, top_k=1, seed=3), pos=5)
    assert torch.equal(tok, torch.argmax(xf, -1))
    assert lp.abs().max() < 1e-6


# ------------------------------------------------------------------------------------------------- 5. determinism, graphs
def test_determinism_graph_capture_and_stream_keys():
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(16, 32000, generator=gen).half().to(DEV)
    prm = SamplingParams(1.0, 0, 0.9, seed=42)
    a = sample_tokens(x, prm, pos=10)
    b = sample_tokens(x, prm, pos=10)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sample_tokens(x, prm, pos=10)                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        c = sample_tokens(x, prm, pos=10)
    g.replay()
    torch.cuda.synchronize()
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    other_pos = sample_tokens(x, prm, pos=11)[0]
    other_seed = sample_tokens(x, SamplingParams(1.0, 0, 0.9, seed=43), pos=10)[0]
    assert (other_pos != a[0]).sum() > 4 and (other_seed != a[0]).sum() > 4
    # the device-side position: pos_dev[0] + pos == pos
    pd = torch.tensor([7, 0, 0, 0], dtype=torch.int32, device=DEV)
    assert torch.equal(sample_tokens(x, prm, pos=3, pos_dev=pd)[0], a[0])


# ------------------------------------------------------------------------------------------------- 6. rejection sampling
def test_accept_rule_with_aimed_uniforms():
    gen = torch.Generator().manual_seed(8)
    V = 1000
    prm = SamplingParams(0.8, 50, 0.95, seed=0)
    raw = torch.randn(64, V, generator=gen).half()
    us, drafts, want_acc = [], [], []
    for r in range(64):
        x32 = R.scaled(raw[r].float().numpy(), prm.temperature)
        keep = R.kept_mask(x32, prm.top_k, prm.top_p)
        pr = R.probs(x32, keep)
        kept = np.nonzero(keep)[0]
        d = int(kept[r % len(kept)]) if r % 4 else int(np.nonzero(~keep)[0][0])     # every 4th draft lies outside the kept set
        ua = pr[d] * (0.5 if r % 2 else 1.5) if pr[d] > 0 else 0.3
        ua = min(ua, 0.999)
        us.append([float(np.float32(0.37)), ua])
        drafts.append(d)
        want_acc.append(int(ua < pr[d]))
    u = torch.tensor(us, dtype=torch.float32, device=DEV)
    tok, acc, lp = sample_tokens(raw.to(DEV), prm, pos=0, draft=torch.tensor(drafts, device=DEV), u=u)
    tok, acc = tok.cpu().numpy(), acc.cpu().numpy()
    assert acc.tolist() == want_acc
    for r in range(64):
        if acc[r]:
            assert tok[r] == drafts[r]
        else:
            assert tok[r] != drafts[r]
            want = R.sample_row(raw[r].float().numpy(), prm.temperature, prm.top_k, prm.top_p, us[r][0], us[r][1], drafts[r])
            assert (int(tok[r]), 0) == want[:2]


def test_speculative_emission_is_distributed_as_p():
    gen = torch.Generator().manual_seed(21)
    V, N = 64, 1 << 18
    t, k, p = 0.9, 24, 0.97
    for _ in range(20):
        raw = torch.randn(V, generator=gen) * 1.5
        x32 = R.scaled(raw.numpy(), t)
        if _top_p_clear(x32, k, p):
            break
    keep = R.kept_mask(x32, k, p)
    pr = R.probs(x32, keep)
    d = int(np.argsort(-pr)[1])                          # the second most likely token as every row's draft
    rows = raw.to(DEV).unsqueeze(0).repeat(N, 1)
    tok, acc, _ = sample_tokens(rows, SamplingParams(t, k, p, seed=5), pos=0, draft=torch.full((N,), d, device=DEV))
    tok, acc = tok.cpu().numpy(), acc.cpu().numpy()
    counts = np.bincount(tok, minlength=V)
    assert counts[~keep].sum() == 0
    assert (tok[acc == 1] == d).all() and (tok[acc == 0] != d).all()
    stat, df = _chi2(counts, pr)
    assert stat < _chi2_bound(df), (stat, df)
    rate = acc.mean()
    assert abs(rate - pr[d]) < 6 * np.sqrt(pr[d] * (1 - pr[d]) / N)


def test_temperature_zero_reproduces_the_greedy_rule():
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(12, 32000, generator=gen).half().to(DEV)
    am = torch.argmax(x, -1)
    d = am.clone()
    d[1::2] = (d[1::2] + 1) % 32000
    d[0] = -1
    tok, acc, _ = sample_tokens(x, SamplingParams(temperature=0), pos=0, n_per_seq=4, draft=d)
    assert torch.equal(tok, am)
    assert acc.tolist() == [0] + [int(i % 2 == 0) for i in range(1, 12)]


# ------------------------------------------------------------------------------------------------- 7. the decoders
def _tiny(method="gearslKIVI", n_kv=2, left=0.02, layers=2):
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    cfg = LlamaConfigLite(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=layers,
                          num_attention_heads=4, num_key_value_heads=n_kv, k_bits=2, v_bits=2)
    cc = dict(compress_method=method, group_size=64, residual=64, quantize_bit=2, rank=4, rankv=4, loop=3, left=left)
    torch.manual_seed(0)
    return LlamaForCausalLM_GEARKIVI(cfg, cc).half().cuda().eval()


S = SamplingParams(0.8, 50, 0.95, seed=7)


def _near_boundary(logits_row, params, P, b, tol):
    """The draw at (P, b) lies within tol of a CDF boundary of this row (a token another rounding of the logits may flip)."""
    u = R.uniform(params.seed, P, b, 0)
    x32 = R.scaled(logits_row.float().cpu().numpy(), params.temperature)
    iv = R.intervals(x32, R.kept_mask(x32, params.top_k, params.top_p))
    return min(min(abs(u - lo), abs(u - hi)) for _, lo, hi in iv) < tol


@pytest.mark.parametrize("kind", ["gear", "fp16"])
def test_sampled_generate_is_seed_reproducible(kind):
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny()
    ids = torch.randint(0, 1000, (2, 100), generator=torch.Generator().manual_seed(1)).cuda()
    L = 180                                                          # crosses the block boundary at 128

    def run(params, **kw):
        return FastGearDecoder(model, 512, batch=2, seed=3, cache_kind=kind).generate(ids, L, sampling=params, **kw)

    a, b = run(S), run(S)
    assert a.shape == (2, L) and torch.equal(a, b)
    assert torch.equal(a[:, :100], ids) and (a >= 0).all() and (a < 1000).all()
    c = run(SamplingParams(0.8, 50, 0.95, seed=8))
    assert (c[:, 100:] != a[:, 100:]).any()
    greedy = FastGearDecoder(model, 512, batch=2, seed=3, cache_kind=kind).generate(ids, L)
    assert torch.equal(run(SamplingParams(temperature=0)), greedy)
    assert (a[:, 100:] != greedy[:, 100:]).any()


def test_sampled_tokens_follow_the_reference_at_their_positions():
    """Eager sampled decoding: the token at position P is the reference's draw from step()'s logits with the (seed, b, P) uniform."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny()
    ids = torch.randint(0, 1000, (2, 90), generator=torch.Generator().manual_seed(2)).cuda()
    dec = FastGearDecoder(model, 512, batch=2, seed=5)
    lg = dec.prefill(ids)
    checked = 0
    for _ in range(40):
        tok = dec._sample(lg, S)
        for b in range(2):
            x = lg[b].float().cpu().numpy()
            if not _near_boundary(lg[b], S, dec.pos, b, 1e-5):
                want = R.sample_row(x, S.temperature, S.top_k, S.top_p, R.uniform(S.seed, dec.pos, b, 0))[0]
                assert int(tok[b]) == want, (dec.pos, b)
                checked += 1
        lg = dec.step(tok)
    assert checked >= 76


def test_sampled_graph_step_matches_eager_and_leaves_greedy_graph_alone():
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny()
    ids = torch.randint(0, 1000, (2, 90), generator=torch.Generator().manual_seed(3)).cuda()
    fe, fg = FastGearDecoder(model, 512, batch=2, seed=5), FastGearDecoder(model, 512, batch=2, seed=5)
    le = fe.prefill(ids)
    fg.prefill(ids)
    tok = fe._sample(le, S)
    le = fe.step(tok)
    fg.step(tok)
    tok = fe._sample(le, S)
    mism, worst = 0, 1.0
    for i in range(100):                                             # across the block boundaries at 128 and 192
        le = fe.step(tok)
        te = fe._sample(le, S)
        tg = fg.step_graph_sampled(S, tok).clone()
        lg = fg.logits_sampled_static
        worst = min(worst, float(torch.nn.functional.cosine_similarity(le.float(), lg.float()).min()))
        # exact: the graph drew at the right position from its own logits
        assert torch.equal(tg, sample_tokens(lg, S, pos=fe.pos)[0].view(-1, 1)), i
        for b in range(2):
            if int(te[b]) != int(tg[b]):                            # graph / eager logits differ by rounding: only near a boundary
                mism += 1
                assert _near_boundary(le[b], S, fe.pos, b, 2e-2), (i, b)
        tok = te
    assert worst > 0.9995 and mism <= 4, (worst, mism)
    assert fg.pos == fe.pos and fg.state.tolist()[0] == fe.pos
    # params changed: captured again; then the greedy graph after the sampled one is still the argmax of its own (correct) logits
    S2 = SamplingParams(1.0, 0, 0.9, seed=1)
    fe_tok = fe._sample(fe.step(tok), S2)
    assert torch.equal(fg.step_graph_sampled(S2, tok), sample_tokens(fg.logits_sampled_static, S2, pos=fe.pos)[0].view(-1, 1))
    tok = fe_tok
    for i in range(20):
        le = fe.step(tok)
        nxt = fg.step_graph(tok)
        assert torch.equal(nxt, fg.logits_static.argmax(-1, keepdim=True))
        assert float(torch.nn.functional.cosine_similarity(le.float(), fg.logits_static.float()).min()) > 0.9995
        tok = le.argmax(-1, keepdim=True)
    assert fg.graph is not None and fg.graph_sampled is not None


def test_sampled_generate_graph_equals_eager():
    """Full runs: the graph path draws the same tokens as the eager path (each token a function of seed, sequence, position and
    logits; the two paths' logits differ by rounding only -- the teacher-forced test above bounds where that can flip a draw)."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny()
    ids = torch.randint(0, 1000, (2, 100), generator=torch.Generator().manual_seed(4)).cuda()
    eager = FastGearDecoder(model, 512, batch=2, seed=3).generate(ids, 150, sampling=S)
    graph = FastGearDecoder(model, 512, batch=2, seed=3).generate(ids, 150, graph=True, sampling=S)
    assert torch.equal(eager, graph)
    g0 = FastGearDecoder(model, 512, batch=2, seed=3).generate(ids, 150, graph=True)
    assert torch.equal(FastGearDecoder(model, 512, batch=2, seed=3).generate(ids, 150, graph=True,
                                                                             sampling=SamplingParams(temperature=0)), g0)


def test_sampled_speculative_temperature_zero_is_greedy_speculative():
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny()
    pat = torch.randint(0, 1000, (2, 12), generator=torch.Generator().manual_seed(5))
    ids = pat.repeat(1, 12).cuda()
    a, sa = FastGearDecoder(model, 1024, batch=2, seed=8).generate_speculative(ids, 144 + 60, return_stats=True)
    b, sb = FastGearDecoder(model, 1024, batch=2, seed=8).generate_speculative(ids, 144 + 60, return_stats=True,
                                                                               sampling=SamplingParams(temperature=0))
    assert torch.equal(a, b) and sa == sb


def test_sampled_speculative_emits_only_kept_tokens():
    """n-gram drafts at batch 2 through block boundaries: every emitted token lies in the kept set of the verify row it came from."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny()
    pat = torch.randint(0, 1000, (2, 12), generator=torch.Generator().manual_seed(6))
    ids = pat.repeat(1, 12).cuda()
    P, L = ids.shape[1], ids.shape[1] + 100                          # 144 -> 244: boundaries at 192 and 256 - 64
    prm = SamplingParams(0.8, 3, 0.9, seed=11)
    dec = FastGearDecoder(model, 1024, batch=2, seed=8)
    calls = []
    verify = dec.verify

    def spy(x):
        lg = verify(x)
        calls.append((dec.pos, lg.clone()))
        return lg

    dec.verify = spy
    out, st = dec.generate_speculative(ids, L, draft="ngram", n_draft=3, return_stats=True, sampling=prm)
    assert out.shape == (2, L) and st["tokens"] == L - P and st["passes"] == len(calls)
    print(f"sampled ngram: {st}")
    ends = [p for p, _ in calls[1:]] + [L - 1]
    n_checked = 0
    for (p, lg), nxt in zip(calls, ends):
        for i in range(nxt - p):                                     # tokens at positions p + 1 .. nxt came from rows 0 .. nxt - p - 1
            for b in range(2):
                x32 = R.scaled(lg[b, i].float().cpu().numpy(), prm.temperature)
                keep = R.kept_mask(x32, prm.top_k, prm.top_p)
                assert keep[int(out[b, p + 1 + i])], (p, i, b)
                n_checked += 1
    assert n_checked == 2 * (L - P - 1)


def test_hook_model_generate_do_sample():
    model = _tiny()
    ids = torch.randint(0, 1000, (2, 100), generator=torch.Generator().manual_seed(7)).cuda()
    L = 130

    def gen(**kw):
        torch.manual_seed(0)        # the hook's power iteration draws its start basis from torch's generator (as the reference)
        return model.generate(ids, L, **kw)

    a = gen(do_sample=True, temperature=0.8, top_k=50, top_p=0.95, seed=1)
    b = gen(do_sample=True, temperature=0.8, top_k=50, top_p=0.95, seed=1)
    c = gen(do_sample=True, temperature=0.8, top_k=50, top_p=0.95, seed=2)
    g = gen()
    assert a.shape == (2, L) and torch.equal(a, b) and (a[:, 100:] != c[:, 100:]).any()
    assert torch.equal(gen(do_sample=False, temperature=0.8, seed=1), g)
    assert torch.equal(gen(do_sample=True, temperature=0.0), g)


# ------------------------------------------------------------------------------------------------- 8. the harness
def test_harness_do_sample():
    import json
    for extra in (["--model", "gearl", "--fast"], ["--model", "KIVI"]):
        cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "harness.py"), "--layers", "2", "--prompt_len", "200",
               "--max_length", "260", "--batch_size", "2", "--json", "--do_sample", *extra]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=660, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        assert "Peak memory usage on GPU" in p.stdout
        res = json.loads(p.stdout.strip().splitlines()[-1])
        assert len(res) == 1 and res[0]["do_sample"] and res[0]["max_length"] == 260 and res[0]["new_tokens_per_s"] > 0
        assert (res[0]["temperature"], res[0]["top_k"], res[0]["top_p"]) == (0.8, 50, 0.95)
