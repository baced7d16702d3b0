"""GPU tests of speculative verify: gear_attn_verify_cache (GearKVCache.attend_verify) probed at one-token resolution, LSE included
(tests/attn_probe.py, every applicable mutation past 5x a bound) across the cache configurations and the attention options;
causality; no state change; agreement with attend_extend and with append + attend; FastGearDecoder.verify / accept on both cache
kinds (bit-exact commits, continuation through step() / step_graph()); generate_speculative against plain greedy decoding; and the
refusals."""
import numpy as np
import pytest
import torch

import attn_probe as AP
from conftest import rel_fro
from test_gpu_attn_probe import ATTEND_OPTS, _cc, _verify

pytestmark = pytest.mark.gpu


def host(t):
    return t.detach().cpu().numpy()


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


def _filled(cc, B, Hkv, T0, more, seed):
    from gear_amd.cache import GearKVCache
    g = torch.Generator().manual_seed(seed)
    c = GearKVCache(B, Hkv, T0 + more + 128, cc, "cuda", seed=seed)
    c.prefill(torch.randn(B, Hkv, T0, 128, generator=g).half().cuda(), torch.randn(B, Hkv, T0, 128, generator=g).half().cuda())
    if more:
        c.extend(torch.randn(B, Hkv, more, 128, generator=g).half().cuda(), torch.randn(B, Hkv, more, 128, generator=g).half().cuda())
    return c


def _chunk(c, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(c.B, c.H, n, 128, generator=g).half().cuda(), torch.randn(c.B, c.H, n, 128, generator=g).half().cuda())


def _verify_probe(tag, c, Hq, n, seed, opt=None, mutations=True):
    """attend_verify under the options `opt` (ATTEND_OPTS form) against the float64 reference and the mutated references."""
    from gear_amd import _lib as L
    opt = opt or {}
    c.use_tiles = opt.get("_tiles", True)
    c.use_chunk_index = opt.get("_chunk_index", True)
    set_opts = {k: v for k, v in opt.items() if not k.startswith("_")}
    try:
        for k, v in set_opts.items():
            L.set_option(k, v)
        kn, vn = _chunk(c, n, seed)
        parts = AP.decompose(c, kn=kn, vn=vn)
        rng = np.random.default_rng(seed)
        qr, aimed = AP.extend_queries(parts, Hq, rng, max_rounds=64 if mutations else 1)    # (few rows per call: many rounds)
        # + one round of plain Gaussian queries: at draft sizes every row may carry an aimed probe (one dominant key, L ~ 1), and
        # a log-sum-exp without log L (M9) only shows where many keys share the softmax
        qr = qr + [(AP.f16(rng.standard_normal((c.B, Hq, n, 128))), None)]
        rounds = []
        for q, used in qr:
            out, lse = c.attend_verify(torch.tensor(q, dtype=torch.float16, device="cuda"), kn, vn, return_lse=True)
            rounds.append((q, host(out).astype(np.float64), host(lse).astype(np.float64), used))
        _verify(tag, parts, Hq, rounds, aimed, mutations)
    finally:
        for k in set_opts:
            L.set_option(k, 0)
        c.use_tiles = c.use_chunk_index = True


# ------------------------------------------------------------------------------------------------ attend_verify probes
VER = [  # method, bits, group, residual, rank, left, Hq, Hkv, prompt, committed, n
    ("gearslKIVI", 2, 64, 64, 4, 0.02, 8, 2, 200, 150, 1),        # G 4: the decode shape
    ("gearslKIVI", 2, 64, 64, 4, 0.02, 8, 2, 200, 150, 2),        # G n = 8
    ("gearlKIVI", 4, 32, 128, 8, 0.0, 4, 4, 300, 300, 4),         # MHA, group 32, residual 128
    ("KIVI", 2, 32, 64, 0, 0.05, 2, 1, 130, 140, 3),              # G n = 6
    ("gearslKIVI", 4, 64, 128, 16, 0.05, 1, 1, 260, 280, 5),      # rank 16
    ("gearslKIVI", 2, 64, 64, 8, 0.02, 8, 8, 70, 130, 8),         # MHA, G n = 8
    ("gearlKIVI", 2, 64, 64, 4, 0.0, 2, 2, 30, 0, 16),            # T = 0
    ("gearslKIVI", 2, 32, 64, 4, 0.05, 4, 2, 128, 64, 4),         # W = 0
    ("gearslKIVI", 2, 64, 64, 4, 0.03, 3, 1, 200, 100, 5),        # G 3
    ("gearslKIVI", 2, 64, 64, 8, 0.02, 16, 2, 200, 100, 2),       # G 8
    ("gearslKIVI", 2, 64, 64, 4, 0.02, 4, 4, 127, 0, 16),         # W = R - 1, n = 16: W + n > wcap
    ("gearslKIVI", 2, 32, 128, 4, 0.02, 4, 2, 300, 260, 16),      # group 32, residual 128, n = 16
    ("gearslKIVI", 2, 64, 64, 4, 0.02, 8, 2, 3000, 1100, 4),      # long context: many splits
    ("gearslKIVI", 2, 64, 64, 4, 0.02, 8, 1, 8300, 0, 2),         # T > 8192: the generic kernel
]


@pytest.mark.parametrize("case", VER, ids=[f"{c[0]}-b{c[1]}-g{c[2]}-R{c[3]}-r{c[4]}-s{c[5]}-{c[6]}x{c[7]}-{c[8]}+{c[9]}-n{c[10]}"
                                           for c in VER])
def test_attend_verify_probes(case):
    method, bits, group, R, rank, left, Hq, Hkv, T0, more, n = case
    B = 2 if Hkv <= 2 and T0 + more < 4000 else 1
    c = _filled(_cc(method, bits, group, R, rank, left=left), B, Hkv, T0, more, seed=11)
    if T0 == 30:
        assert c.n_comp == 0
    if T0 == 128:
        assert c.n_win == 0
    if T0 == 127:
        assert c.n_win == R - 1
    if T0 == 8300:
        assert c.n_comp > 8192
    _verify_probe(f"attend_verify[G{Hq // Hkv}]", c, Hq, n, seed=n)


@pytest.fixture(scope="module")
def main_cache():
    return _filled(_cc(), 1, 2, 200, 150, seed=21)          # seg0 = 192, four decode-time blocks, W = 30


@pytest.mark.parametrize("opt", list(ATTEND_OPTS))
def test_attend_verify_probes_under_options(main_cache, opt):
    """n = 1, 2, 3 at G = 4: G n = 4 / 8 (the matrix-core kernel's NREP when it runs) and 12 (the vector kernel per row)."""
    c = main_cache
    assert c.seg0 == 192 and c.n_comp == 320 and c.n_win == 30
    for n in (1, 2, 3):
        _verify_probe(f"attend_verify[{opt}]", c, 8, n, seed=5 + n, opt=ATTEND_OPTS[opt])


def test_attend_verify_matrix_core_at_mha(options):
    """MHA with n = 2 / 4 / 8 on the matrix-core kernel (NREP = n), by option and by the default rule (B Hkv splits >= 256)."""
    c = _filled(_cc(), 1, 8, 1000, 100, seed=31)
    options(attn_mfma=1)
    for n in (2, 4, 8):
        _verify_probe("attend_verify[mha-mfma]", c, 8, n, seed=n)
    options(attn_mfma=0)
    big = _filled(_cc(), 1, 32, 4000, 0, seed=32)
    _verify_probe("attend_verify[mha-default]", big, 32, 4, seed=3, mutations=False)


@pytest.mark.parametrize("rk,rv", [(4, 8), (8, 4)])
def test_attend_verify_unequal_ranks(rk, rv):
    c = _filled(_cc(rank=rk, rankv=rv), 1, 2, 130, 140, seed=rk)
    assert (c.rk, c.rv) == (rk, rv)
    for opt in ("default", "mfma", "generic"):
        _verify_probe(f"attend_verify[r{rk}/{rv}]", c, 4, 2, seed=6, opt=ATTEND_OPTS[opt])


def test_attend_verify_overflowed_tiles():
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
    # (seed 7: test_gpu_attn_probe's decode probes of this cache.  The probe set of seed 8 takes the matrix-core kernel to a row
    # error of 1.1e-2, past ROW_BOUND, at n = 1 -- the decode partials of the same queries, so decode alike)
    # Longer drafts: the bounds only -- the 12x keys of the first 100 tokens outweigh what the aimed probes can single out among
    # the chunk rows (M2 signal 0.7 at n = 2)
    for opt in ("mfma", "vector"):
        _verify_probe(f"attend_verify[overflowed-{opt}]", c, 8, 1, seed=7, opt=ATTEND_OPTS[opt])
        for n in (2, 4):
            _verify_probe(f"attend_verify[overflowed-{opt}]", c, 8, n, seed=7, opt=ATTEND_OPTS[opt], mutations=False)


# ------------------------------------------------------------------------------------------------ semantics
@pytest.mark.parametrize("method,left", [("gearlKIVI", 0.0), ("gearslKIVI", 0.02)], ids=["no-outliers", "outliers"])
def test_verify_is_causal(method, left):
    """Changing chunk row j leaves rows < j unchanged and changes row j.  Bit-identical without outliers; with outliers the decode
    kernels add the outlier terms with LDS float atomics (attention.hip), so two identical calls may already differ in the last
    bits: there rows < j are held to that run-to-run difference (measured here) and row j must move far past it."""
    c = _filled(_cc(method, left=left), 1, 2, 200, 70, seed=3)
    g = torch.Generator().manual_seed(5)
    n = 16
    q = torch.randn(1, 8, n, 128, generator=g).half().cuda()
    kn, vn = _chunk(c, n, 6)
    a = c.attend_verify(q, kn, vn)
    noise = float((c.attend_verify(q, kn, vn).float() - a.float()).abs().max())
    if left == 0.0:
        assert noise == 0.0
    for j in (0, 5, 15):
        kn2, vn2 = kn.clone(), vn.clone()
        kn2[:, :, j] += 1.0
        vn2[:, :, j] -= 1.0
        b = c.attend_verify(q, kn2, vn2)
        if left == 0.0:
            assert torch.equal(a[:, :, :j], b[:, :, :j])
        else:
            assert j == 0 or float((a[:, :, :j].float() - b[:, :, :j].float()).abs().max()) <= max(4 * noise, 5e-4)
        assert float((a[:, :, j].float() - b[:, :, j].float()).abs().max()) > max(16 * noise, 2e-3)


def test_verify_changes_no_state():
    c = _filled(_cc(), 2, 2, 200, 100, seed=4)
    before = {k: t.clone() for k, t in c.bufs.items()}
    counters = (c.n_comp, c.n_win, c.seg0, c.kk0)
    g = torch.Generator().manual_seed(1)
    for n in (1, 4, 16):
        q = torch.randn(2, 8, n, 128, generator=g).half().cuda()
        kn, vn = _chunk(c, n, n)
        c.attend_verify(q, kn, vn, return_lse=True)
    torch.cuda.synchronize()
    assert (c.n_comp, c.n_win, c.seg0, c.kk0) == counters
    for k, t in c.bufs.items():
        assert torch.equal(t, before[k]), k


@pytest.mark.parametrize("case", [VER[0], VER[2], VER[4], VER[6], VER[7], VER[10], VER[12]],
                         ids=["G4", "mha-g32", "r16", "T0", "W0", "Wfull", "long"])
def test_verify_agrees_with_extend(case):
    method, bits, group, R, rank, left, Hq, Hkv, T0, more, _ = case
    c = _filled(_cc(method, bits, group, R, rank, left=left), 1, Hkv, T0, more, seed=12)
    g = torch.Generator().manual_seed(2)
    for n in (1, 2, 4, 8, 16):
        q = torch.randn(1, Hq, n, 128, generator=g).half().cuda()
        kn, vn = _chunk(c, n, 3 * n)
        a, la = c.attend_verify(q, kn, vn, return_lse=True)
        b, lb = c.attend_extend(q, kn, vn, return_lse=True)
        assert rel_fro(host(a), host(b)) < 2e-3, n
        assert float((la - lb).abs().max()) < 1e-2, n


@pytest.mark.parametrize("method,left,Hq,Hkv", [("gearslKIVI", 0.02, 8, 2), ("KIVI", 0.0, 4, 4), ("gearlKIVI", 0.05, 2, 1)])
def test_verify_of_one_token_equals_decode(method, left, Hq, Hkv):
    c = _filled(_cc(method, 2, 64, 64, 4, left=left), 2, Hkv, 200, 90, seed=7)
    g = torch.Generator().manual_seed(9)
    q = torch.randn(2, Hq, 1, 128, generator=g).half().cuda()
    k, v = _chunk(c, 1, 10)
    a = c.attend_verify(q, k, v)
    c.append(k, v)
    b = c.attend(q)
    assert rel_fro(host(a), host(b)) < 2e-3


# ------------------------------------------------------------------------------------------------ decoder
def _tiny(method, n_kv, left=0.0, layers=2):
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    cfg = LlamaConfigLite(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=layers,
                          num_attention_heads=4, num_key_value_heads=n_kv, k_bits=2, v_bits=2)
    cc = dict(compress_method=method, group_size=64, residual=64, quantize_bit=2, rank=4, rankv=4, loop=3, left=left)
    torch.manual_seed(0)
    return LlamaForCausalLM_GEARKIVI(cfg, cc).half().cuda().eval()


def _cos(a, b):
    return float(torch.nn.functional.cosine_similarity(a.float().reshape(-1, a.shape[-1]), b.float().reshape(-1, b.shape[-1])).min())


def _state(dec):
    if dec.pool is not None:
        bufs = {k: t.clone() for k, t in dec.pool.buf.items()}
    else:
        bufs = {f"{i}{s}": getattr(lw["cache"], s).clone() for i, lw in enumerate(dec.layers) for s in ("kwin", "vwin")}
    return bufs, [(lw["cache"].n_comp, lw["cache"].n_win) for lw in dec.layers], dec.pos


def _same_state(x, y):
    (bx, cx, px), (by, cy, py) = x, y
    assert bx.keys() == by.keys()
    for k in bx:
        assert torch.equal(bx[k], by[k]), k
    assert cx == cy and px == py


@pytest.mark.parametrize("kind", ["gear", "fp16"])
def test_decoder_verify_matches_extend_and_changes_nothing(kind):
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    P, B = 150, 2
    ids = torch.randint(0, 1000, (B, P + 16)).cuda()
    a = FastGearDecoder(model, 512, batch=B, seed=3, cache_kind=kind)
    b = FastGearDecoder(model, 512, batch=B, seed=3, cache_kind=kind)
    a.prefill(ids[:, :P])
    b.prefill(ids[:, :P])
    before = _state(a)
    for n in (1, 4, 16):
        lv = a.verify(ids[:, P:P + n])
        torch.cuda.synchronize()
        _same_state(_state(a), before)
        assert lv.shape == (B, n, 1000)
        snap = _state(b)
        le = b.extend(ids[:, P:P + n])
        assert _cos(lv, le) > 0.999, n
        # b back to the prompt state: a fresh twin (extend commits)
        b = FastGearDecoder(model, 512, batch=B, seed=3, cache_kind=kind)
        b.prefill(ids[:, :P])
        _same_state(_state(b), snap)


@pytest.mark.parametrize("kind", ["gear", "fp16"])
def test_decoder_accept_is_bit_exact(kind):
    """accept(m) leaves buffers and counters bit-identical to committing the same verify rows 0 .. m - 1 through extend_all
    (Fp16KVCache.extend); P = 190: rows cross the block boundary at 192 for m >= 3."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    P, n = 190, 6
    ids = torch.randint(0, 1000, (1, P + n)).cuda()
    for m in (0, 1, 3, n):
        a = FastGearDecoder(model, 512, seed=4, cache_kind=kind)
        b = FastGearDecoder(model, 512, seed=4, cache_kind=kind)
        a.prefill(ids[:, :P])
        b.prefill(ids[:, :P])
        a.verify(ids[:, P:])
        ks = [k[:, :, :m].clone() for k in a._pending["ks"]]
        vs = [v[:, :, :m].clone() for v in a._pending["vs"]]
        assert a.accept(m) == m
        if m:
            if kind == "gear":
                b.pool.extend_all(ks, vs)
            else:
                for lw, k, v in zip(b.layers, ks, vs):
                    lw["cache"].extend(k, v)
            b.pos += m
        torch.cuda.synchronize()
        _same_state(_state(a), _state(b))
        assert a.pos == P + m
        c0 = a.layers[0]["cache"]
        if kind == "gear":
            assert (c0.n_comp, c0.n_win) == ((192, P + m - 192) if P + m >= 192 else (128, P + m - 128))


def test_accept_then_step_and_graph_continue():
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearlKIVI", 2, left=0.03)
    P = 100
    ids = torch.randint(0, 1000, (1, P + 8)).cuda()
    fe, fg = FastGearDecoder(model, 512, seed=5), FastGearDecoder(model, 512, seed=5)
    for f in (fe, fg):
        f.prefill(ids[:, :P])
        f.verify(ids[:, P:P + 8])
        f.accept(5)
    tok = ids[:, P + 5:P + 6]
    worst = 1.0
    for i in range(80):
        a = fe.step(tok)
        if i % 3 == 2 or i < 2:
            b = fg.step(tok)
        else:
            fg.step_graph(tok)
            b = fg.logits_static
        worst = min(worst, _cos(a, b))
        tok = a.argmax(-1, keepdim=True)
    assert worst > 0.9995, worst
    n = P + 5 + 80
    for f in (fe, fg):
        c = f.layers[0]["cache"]
        assert (f.pos, c.n_comp, c.n_win) == (n, n - n % 64, n % 64)


# ------------------------------------------------------------------------------------------------ generate_speculative
def _greedy(model, ids, max_length, kind="gear"):
    """Plain greedy decoding with step(): tokens [B, max_length] and the top-2 logit margin of every generated token [B, gen]."""
    from gear_amd.fast_decode import FastGearDecoder
    dec = FastGearDecoder(model, 1024, batch=ids.shape[0], seed=8, cache_kind=kind)
    lg = dec.prefill(ids)
    out, margins = [ids], []
    while sum(t.shape[1] for t in out) < max_length:
        top = lg.float().topk(2, -1).values
        margins.append(top[:, 0] - top[:, 1])
        nxt = lg.argmax(-1, keepdim=True)
        out.append(nxt)
        if sum(t.shape[1] for t in out) < max_length:
            lg = dec.step(nxt)
    return torch.cat(out, 1), torch.stack(margins, 1)


def _threshold(model, ids):
    """2 x the largest |verify - step| logit difference measured on this model over 32 positions: where the plain run's top-2
    margin exceeds twice the largest perturbation of a logit, the argmax cannot move."""
    from gear_amd.fast_decode import FastGearDecoder
    B = ids.shape[0]
    x = FastGearDecoder(model, 1024, batch=B, seed=8)
    y = FastGearDecoder(model, 1024, batch=B, seed=8)
    lx, _ = x.prefill(ids), y.prefill(ids)
    tok = lx.argmax(-1, keepdim=True)
    diff = 0.0
    for _ in range(8):
        run, steps = [tok], []
        for _ in range(4):                                         # 4 tokens fed one at a time by step() on x ...
            steps.append(x.step(run[-1]))
            run.append(steps[-1].argmax(-1, keepdim=True))
        lv = y.verify(torch.cat(run[:4], 1))                       # ... and at once by verify() on y
        y.accept(4)
        diff = max(diff, float((lv.float() - torch.stack(steps, 1).float()).abs().max()))
        tok = run[-1]
    return 2.0 * diff


def _compare(out, plain, margins, P, thr, min_tokens):
    """Each row equal to the plain greedy run up to its first generated position with a top-2 margin below thr; at least
    min_tokens generated tokens compared over all rows.  Returns that number."""
    assert out.shape == plain.shape
    low = margins < thr
    total = 0
    for r in range(out.shape[0]):
        j = int(low[r].nonzero()[0]) if bool(low[r].any()) else margins.shape[1]
        assert torch.equal(out[r, :P + j], plain[r, :P + j]), (r, j)
        total += j
    assert total >= min_tokens, (total, thr)
    return total


def test_generate_speculative_matches_greedy():
    model = _tiny("gearslKIVI", 2, left=0.02)
    g = torch.Generator().manual_seed(3)
    P, gen = 120, 80
    ids = torch.randint(0, 1000, (1, P), generator=g).cuda()
    thr = _threshold(model, ids)
    print(f"generate_speculative threshold: 2 x max |verify - step| logit difference = {thr:.4g}")
    plain, margins = _greedy(model, ids, P + gen)
    j = int((margins[0] < thr).nonzero()[0]) if bool((margins[0] < thr).any()) else gen
    assert j >= 24, (j, thr)
    L = P + j                                                       # the stretch where greedy is unambiguous
    from gear_amd.fast_decode import FastGearDecoder

    def oracle(toks, k):
        return plain[:, toks.shape[1]:toks.shape[1] + k]

    def wrong(toks, k):
        return (oracle(toks, k) + 1) % 1000

    for name, drafter, nd in (("oracle", oracle, 3), ("oracle7", oracle, 7), ("wrong", wrong, 3)):
        dec = FastGearDecoder(model, 1024, seed=8)
        out, st = dec.generate_speculative(ids, L, draft=drafter, n_draft=nd, return_stats=True)
        assert out.shape == (1, L)
        assert torch.equal(out, plain[:, :L]), name
        assert st["tokens"] == j
        if name.startswith("oracle"):
            assert st["acceptance_rate"] >= 0.9, st
            assert st["passes"] <= (j - 1 + nd) // (nd + 1) + 1, st
        else:
            assert st["accepted"] == 0 and st["passes"] == j - 1, st
    # and past the unambiguous stretch: equal up to the first low-margin token
    dec = FastGearDecoder(model, 1024, seed=8)
    out = dec.generate_speculative(ids, P + gen, draft=oracle, n_draft=3)
    _compare(out, plain, margins, P, thr, 24)


def test_generate_speculative_ngram_on_repetitive_prompt():
    model = _tiny("gearslKIVI", 2, left=0.02)
    g = torch.Generator().manual_seed(4)
    pat = torch.randint(0, 1000, (3, 12), generator=g)
    ids = pat.repeat(1, 12).cuda()                                 # 144 tokens per row, a 12-token pattern each
    P, gen = ids.shape[1], 64
    thr = _threshold(model, ids)
    plain, margins = _greedy(model, ids, P + gen)
    from gear_amd.fast_decode import FastGearDecoder
    dec = FastGearDecoder(model, 1024, batch=3, seed=8)
    out, st = dec.generate_speculative(ids, P + gen, draft="ngram", n_draft=3, return_stats=True)
    assert out.shape == (3, P + gen) and st["tokens"] == gen
    _compare(out, plain, margins, P, thr, 24)
    print(f"ngram: {st}")


def test_generate_speculative_batch_takes_the_minimum():
    model = _tiny("gearslKIVI", 2, left=0.02)
    g = torch.Generator().manual_seed(5)
    P, gen = 100, 48
    ids = torch.randint(0, 1000, (2, P), generator=g).cuda()
    thr = _threshold(model, ids)
    plain, margins = _greedy(model, ids, P + gen)
    low = (margins < thr).any(0)
    j = int(low.nonzero()[0]) if bool(low.any()) else gen
    assert j >= 8, (j, thr)
    L = P + j
    from gear_amd.fast_decode import FastGearDecoder

    def drafter(toks, k):          # row 0: the greedy continuation; row 1: its second draft is always wrong
        d = plain[:, toks.shape[1]:toks.shape[1] + k].clone()
        if k >= 2:
            d[1, 1] = (d[1, 1] + 1) % 1000
        return d

    dec = FastGearDecoder(model, 1024, batch=2, seed=8)
    out, st = dec.generate_speculative(ids, L, draft=drafter, n_draft=3, return_stats=True)
    assert torch.equal(out, plain[:, :L])
    assert st["accepted"] <= st["passes"]                          # at most one draft (row 1's first) per pass
    assert st["tokens_per_pass"] > 1.5, st


# ------------------------------------------------------------------------------------------------ refusals
def test_verify_refusals(monkeypatch):
    from gear_amd import _lib as L
    from gear_amd.cache import N_MAX_VERIFY
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    dec = FastGearDecoder(model, 192, seed=1)
    with pytest.raises(ValueError):
        dec.verify(torch.randint(0, 1000, (1, 4)).cuda())          # no prefill yet
    with pytest.raises(ValueError):
        dec.accept(0)                                              # no verify
    dec.prefill(torch.randint(0, 1000, (1, 240)).cuda())           # 192 compressed (the capacity) + 48 in the window
    assert dec._room() == 15
    snap = _state(dec)
    with pytest.raises(L.GearError):
        dec.verify(torch.randint(0, 1000, (1, 16)).cuda())         # the 64th window row would need a block past the capacity
    _same_state(_state(dec), snap)
    with pytest.raises(ValueError):
        dec.verify(torch.randint(0, 1000, (1, N_MAX_VERIFY + 1)).cuda())
    dec.verify(torch.randint(0, 1000, (1, 3)).cuda())
    with pytest.raises(ValueError):
        dec.accept(4)                                              # m > n
    assert dec.accept(2) == 2
    with pytest.raises(ValueError):
        dec.accept(1)                                              # the verify was accepted already
    with pytest.raises(ValueError):
        c = dec.layers[0]["cache"]
        q = torch.zeros(1, 4, N_MAX_VERIFY + 1, 128, dtype=torch.float16, device="cuda")
        c.attend_verify(q, q[:, :2], q[:, :2])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(NotImplementedError):
        dec.verify(torch.randint(0, 1000, (1, 2)).cuda())
    monkeypatch.undo()
    dec.tp_world = 2                                               # (a sharded decoder's attribute: the check comes first)
    with pytest.raises(NotImplementedError):
        dec.verify(torch.randint(0, 1000, (1, 2)).cuda())
    dec.tp_world = 1
