"""GPU tests of chunk extend: gear_attn_extend_cache against a float64 reconstruction, causality, n = 1 against the decode kernel,
bit-exact commits (GearKVCache.extend, GearKVCachePool.extend_all), FastGearDecoder.extend on the fp16 and the compressed cache,
continuation through step() / step_graph(), and the capacity refusal."""
import copy

import numpy as np
import pytest
import torch

from conftest import rel_fro
from test_gpu_fast_decode import _reconstruct_cache

pytestmark = pytest.mark.gpu


def host(t):
    return t.detach().cpu().numpy()


def _cc(method, bits, group, R, rank, left):
    return dict(compress_method=method, group_size=group, residual=R, quantize_bit=bits, rank=rank, rankv=rank, loop=3, left=left)


def _filled(cc, B, Hkv, T0, more, seed, cap=None):
    """A cache after a prompt of T0 tokens and `more` committed tokens (several factor segments when more spans blocks)."""
    from gear_amd.cache import GearKVCache
    g = torch.Generator().manual_seed(seed)
    c = GearKVCache(B, Hkv, cap or (T0 + more + 64), cc, "cuda", seed=seed)
    c.prefill(torch.randn(B, Hkv, T0, 128, generator=g).half().cuda(), torch.randn(B, Hkv, T0, 128, generator=g).half().cuda())
    if more:
        c.extend(torch.randn(B, Hkv, more, 128, generator=g).half().cuda(), torch.randn(B, Hkv, more, 128, generator=g).half().cuda())
    return c


def _ref_extend(q, K, V, kw, vw, kn, vn):
    """float64 chunk attention on the GPU: q [B,Hq,n,D]; K, V [B,Hkv,T,D] reconstructed; window; chunk rows; causal offset T + W."""
    dev = "cuda"
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device=dev)
    Kall = torch.cat([t(K), t(kw), t(kn)], 2)
    Vall = torch.cat([t(V), t(vw), t(vn)], 2)
    Hq, Hkv, n = q.shape[1], Kall.shape[1], q.shape[2]
    Kall, Vall = Kall.repeat_interleave(Hq // Hkv, 1), Vall.repeat_interleave(Hq // Hkv, 1)
    s = torch.einsum("bhnd,bhtd->bhnt", t(q), Kall) / np.sqrt(128)
    off = Kall.shape[2] - n
    mask = torch.ones((n, Kall.shape[2]), dtype=torch.bool, device=dev).tril(off)
    s = s.masked_fill(~mask, float("-inf"))
    return torch.einsum("bhnt,bhtd->bhnd", torch.softmax(s, -1), Vall).cpu().numpy()


def _check(c, Hq, n, seed):
    g = torch.Generator().manual_seed(seed)
    B, Hkv = c.B, c.H
    q = torch.randn(B, Hq, n, 128, generator=g).half().cuda()
    kn = torch.randn(B, Hkv, n, 128, generator=g).half().cuda()
    vn = torch.randn(B, Hkv, n, 128, generator=g).half().cuda()
    before = (c.n_comp, c.n_win)
    out = c.attend_extend(q, kn, vn)
    assert (c.n_comp, c.n_win) == before
    K, V = _reconstruct_cache(c)
    ref = _ref_extend(host(q), K, V, host(c.kwin[:, :, :c.n_win]), host(c.vwin[:, :, :c.n_win]), host(kn), host(vn))
    return rel_fro(host(out).astype(np.float64), ref)


# method, bits, group, residual, rank, left, Hq, Hkv, prompt, committed after the prompt, chunk sizes
CASES = [("gearslKIVI", 2, 64, 64, 4, 0.02, 8, 2, 200, 150, (1, 7, 64, 200, 2048)),
         ("gearlKIVI", 4, 32, 128, 8, 0.0, 4, 4, 300, 300, (1, 7, 64, 200)),
         ("KIVI", 2, 32, 64, 0, 0.05, 2, 1, 130, 140, (1, 7, 64, 200)),
         ("gearslKIVI", 4, 64, 128, 16, 0.05, 1, 1, 260, 280, (1, 7, 200, 2048)),
         ("gearslKIVI", 2, 64, 64, 8, 0.02, 8, 8, 70, 130, (1, 64, 200)),
         ("gearlKIVI", 2, 64, 64, 4, 0.0, 2, 2, 30, 0, (1, 7, 64, 200)),        # T = 0: window only
         ("gearslKIVI", 2, 32, 64, 4, 0.05, 4, 2, 128, 64, (1, 7, 64, 2048))]   # W = 0: the commit ends on a boundary


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-b{c[1]}-g{c[2]}-R{c[3]}-r{c[4]}-s{c[5]}-{c[6]}x{c[7]}-{c[8]}+{c[9]}"
                                              for c in CASES])
def test_attend_extend_matches_float64_reconstruction(case):
    method, bits, group, R, rank, left, Hq, Hkv, T0, more, ns = case
    c = _filled(_cc(method, bits, group, R, rank, left), 2 if Hkv <= 2 else 1, Hkv, T0, more, seed=11)
    if T0 == 30:
        assert c.n_comp == 0 and c.n_win == 30
    if T0 == 128:
        assert c.n_win == 0 and c.n_comp == 192
    worst = max(_check(c, Hq, n, seed=n) for n in ns)
    assert worst < 2e-3, worst


def test_extend_is_causal():
    c = _filled(_cc("gearslKIVI", 2, 64, 64, 4, 0.02), 1, 2, 200, 70, seed=3)
    g = torch.Generator().manual_seed(5)
    n, j = 100, 37
    q = torch.randn(1, 4, n, 128, generator=g).half().cuda()
    kn = torch.randn(1, 2, n, 128, generator=g).half().cuda()
    vn = torch.randn(1, 2, n, 128, generator=g).half().cuda()
    a = c.attend_extend(q, kn, vn)
    kn2, vn2 = kn.clone(), vn.clone()
    kn2[:, :, j] += 1.0
    vn2[:, :, j] -= 1.0
    b = c.attend_extend(q, kn2, vn2)
    assert torch.equal(a[:, :, :j], b[:, :, :j])
    assert not torch.equal(a[:, :, j:], b[:, :, j:])
    assert not torch.equal(a[:, :, j], b[:, :, j])


@pytest.mark.parametrize("method,left,Hq,Hkv", [("gearslKIVI", 0.02, 8, 2), ("KIVI", 0.0, 4, 4), ("gearlKIVI", 0.05, 2, 1)])
def test_extend_of_one_token_equals_decode(method, left, Hq, Hkv):
    c = _filled(_cc(method, 2, 64, 64, 4, left), 2, Hkv, 200, 90, seed=7)
    g = torch.Generator().manual_seed(9)
    q = torch.randn(2, Hq, 1, 128, generator=g).half().cuda()
    k = torch.randn(2, Hkv, 1, 128, generator=g).half().cuda()
    v = torch.randn(2, Hkv, 1, 128, generator=g).half().cuda()
    a = c.attend_extend(q, k, v)
    c.append(k, v)
    b = c.attend(q)
    assert rel_fro(host(a), host(b)) < 2e-3


def _bufs_equal(x, y):
    assert x.bufs.keys() == y.bufs.keys()
    for name in x.bufs:
        assert torch.equal(x.bufs[name], y.bufs[name]), name
    assert (x.n_comp, x.n_win, x.seg0, x.kk0) == (y.n_comp, y.n_win, y.seg0, y.kk0)


@pytest.mark.parametrize("R,left,H", [(64, 0.02, 2), (128, 0.05, 4), (64, 0.0, 1)])
def test_cache_extend_commit_is_bit_exact(R, left, H):
    from gear_amd.cache import GearKVCache
    cc = _cc("gearslKIVI", 2, 64, R, 4, left)
    T0 = R + 30
    for n in (5, R - 30, 3 * R + 11):          # no boundary, exactly one (n = R - W), several
        g = torch.Generator().manual_seed(n)
        kp, vp = torch.randn(2, H, T0, 128, generator=g).half().cuda(), torch.randn(2, H, T0, 128, generator=g).half().cuda()
        kn, vn = torch.randn(2, H, n, 128, generator=g).half().cuda(), torch.randn(2, H, n, 128, generator=g).half().cuda()
        a, b = GearKVCache(2, H, 1024, cc, "cuda", seed=4), GearKVCache(2, H, 1024, cc, "cuda", seed=4)
        a.prefill(kp, vp)
        b.prefill(kp, vp)
        a.extend(kn, vn)
        for i in range(n):
            b.append(kn[:, :, i:i + 1], vn[:, :, i:i + 1])
            b.maybe_compress()
        torch.cuda.synchronize()
        _bufs_equal(a, b)
        assert a.seq_len == T0 + n


@pytest.mark.parametrize("R,H", [(64, 4), (64, 2), (128, 2)])
def test_pool_extend_all_is_bit_exact(R, H):
    from gear_amd.cache import GearKVCache, GearKVCachePool
    cc = _cc("gearslKIVI", 2, 64, R, 4, 0.02)
    nl, B, T0 = 3, 1, R + 20

    def mk():
        pool = GearKVCachePool(nl, B, H, 1024, cc, "cuda", seed=6)
        return pool, [GearKVCache(B, H, 1024, cc, "cuda", pool=pool, layer=i, seed=6 + i) for i in range(nl)]

    for n in (7, R - 20, 2 * R + 9):
        g = torch.Generator().manual_seed(n)
        pre = [(torch.randn(B, H, T0, 128, generator=g).half().cuda(), torch.randn(B, H, T0, 128, generator=g).half().cuda())
               for _ in range(nl)]
        new = [(torch.randn(B, H, n, 128, generator=g).half().cuda(), torch.randn(B, H, n, 128, generator=g).half().cuda())
               for _ in range(nl)]
        (pa, ca), (pb, cb) = mk(), mk()
        for cs in (ca, cb):
            for c, (k, v) in zip(cs, pre):
                c.prefill(k, v)
        nb = pa.extend_all([k for k, _ in new], [v for _, v in new])
        want_nb = 0
        for i in range(n):
            for c, (k, v) in zip(cb, new):
                c.append(k[:, :, i:i + 1], v[:, :, i:i + 1])
            if cb[0].n_win == R:
                pb.compress_all()
                want_nb += 1
        torch.cuda.synchronize()
        assert nb == want_nb
        for name in pa.buf:
            assert torch.equal(pa.buf[name], pb.buf[name]), name
        for x, y in zip(ca, cb):
            assert (x.n_comp, x.n_win) == (y.n_comp, y.n_win)


def _tiny(method, n_kv, left=0.0, layers=2):
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    cfg = LlamaConfigLite(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=layers,
                          num_attention_heads=4, num_key_value_heads=n_kv, k_bits=2, v_bits=2)
    cc = dict(compress_method=method, group_size=64, residual=64, quantize_bit=2, rank=4, rankv=4, loop=3, left=left)
    torch.manual_seed(0)
    return LlamaForCausalLM_GEARKIVI(cfg, cc).half().cuda().eval()


def _cos(a, b):
    return float(torch.nn.functional.cosine_similarity(a.float().reshape(-1, a.shape[-1]), b.float().reshape(-1, b.shape[-1])).min())


def test_decoder_extend_on_fp16_cache_matches_prefill():
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("KIVI", 2)
    P, C = 90, 70
    ids = torch.randint(0, 1000, (2, P + C)).cuda()
    a = FastGearDecoder(model, 512, batch=2, cache_kind="fp16")
    a.prefill(ids[:, :P])
    la = a.extend(ids[:, P:])
    assert la.shape == (2, C, 1000) and a.pos == P + C and a.layers[0]["cache"].n_win == P + C
    b = FastGearDecoder(model, 512, batch=2, cache_kind="fp16")
    lb = b.prefill(ids)
    assert _cos(la[:, -1], lb) > 0.9999
    with torch.no_grad():                      # one dense forward of the module: its hidden states at every position
        hidden, _ = model.model(ids, None, True)
        lm = model.lm_head(hidden[:, P:])
    assert _cos(la, lm) > 0.999
    # and the decode continues from the extended cache as from the long prompt
    tok = lb.argmax(-1, keepdim=True)
    assert _cos(a.step(tok), b.step(tok)) > 0.9999


@pytest.mark.parametrize("n_kv", [1, 2, 4])
def test_decoder_extend_on_compressed_cache_matches_float32_restatement(n_kv):
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.modeling_llamagear import apply_rotary_pos_emb
    model = _tiny("gearslKIVI", n_kv, left=0.02)
    P, C, B = 150, 100, 1
    ids = torch.randint(0, 1000, (B, P + C)).cuda()
    dec = FastGearDecoder(model, 512, batch=B, seed=2)
    dec.prefill(ids[:, :P])
    snap = []
    for lw in dec.layers:
        c = lw["cache"]
        K, V = _reconstruct_cache(c)
        snap.append((torch.tensor(K, dtype=torch.float32, device="cuda"), torch.tensor(V, dtype=torch.float32, device="cuda"),
                     c.kwin[:, :, :c.n_win].float(), c.vwin[:, :, :c.n_win].float()))
    got = dec.extend(ids[:, P:])
    assert dec.pos == P + C and dec.layers[0]["cache"].seq_len == P + C
    m32 = copy.deepcopy(model).float()
    Hq, D = 4, 128
    with torch.no_grad():
        h = m32.model.embed_tokens(ids[:, P:])
        pos = torch.arange(P, P + C, device="cuda").unsqueeze(0)
        for layer, (K, V, kw, vw) in zip(m32.model.layers, snap):
            at = layer.self_attn
            x = layer.input_layernorm(h)
            q = at.q_proj(x).view(B, C, Hq, D).transpose(1, 2)
            k = at.k_proj(x).view(B, C, n_kv, D).transpose(1, 2)
            v = at.v_proj(x).view(B, C, n_kv, D).transpose(1, 2)
            cos, sin = at.rotary_emb(v, pos)
            q, k = apply_rotary_pos_emb(q, k, cos, sin)
            Kall = torch.cat([K, kw, k], 2).repeat_interleave(Hq // n_kv, 1)
            Vall = torch.cat([V, vw, v], 2).repeat_interleave(Hq // n_kv, 1)
            s = q @ Kall.transpose(2, 3) / D ** 0.5
            mask = torch.ones((C, Kall.shape[2]), dtype=torch.bool, device="cuda").tril(Kall.shape[2] - C)
            a = torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ Vall
            h = h + at.o_proj(a.transpose(1, 2).reshape(B, C, Hq * D))
            h = h + layer.mlp(layer.post_attention_layernorm(h))
        ref = m32.lm_head(m32.model.norm(h))
    assert _cos(got, ref) > 0.999


def test_extend_then_step_and_graph_continue():
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearlKIVI", 2, left=0.03)
    P, C = 100, 50
    ids = torch.randint(0, 1000, (1, P + C)).cuda()
    fe, fg = FastGearDecoder(model, 512, seed=5), FastGearDecoder(model, 512, seed=5)
    fe.prefill(ids[:, :P])
    fg.prefill(ids[:, :P])
    le, lg = fe.extend(ids[:, P:]), fg.extend(ids[:, P:])
    assert torch.equal(le, lg)
    tok = le[:, -1].argmax(-1, keepdim=True)
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
    n = P + C + 80
    for f in (fe, fg):
        c = f.layers[0]["cache"]
        assert (f.pos, c.n_comp, c.n_win) == (n, n - n % 64, n % 64)


def test_extend_past_capacity_changes_nothing():
    from gear_amd import _lib as L
    from gear_amd.fast_decode import FastGearDecoder
    c = _filled(_cc("gearslKIVI", 2, 64, 64, 4, 0.02), 1, 2, 150, 40, seed=1, cap=256)
    before = {k: t.clone() for k, t in c.bufs.items()}
    state = (c.n_comp, c.n_win)
    kn = torch.randn(1, 2, 200, 128).half().cuda()
    with pytest.raises(L.GearError):
        c.extend(kn, kn)
    assert (c.n_comp, c.n_win) == state
    for k, t in c.bufs.items():
        assert torch.equal(t, before[k]), k
    model = _tiny("gearslKIVI", 2, left=0.02)
    dec = FastGearDecoder(model, 256, seed=1)
    with pytest.raises(ValueError):
        dec.extend(torch.randint(0, 1000, (1, 4)).cuda())          # no prefill yet
    dec.prefill(torch.randint(0, 1000, (1, 200)).cuda())
    snap = {k: t.clone() for k, t in dec.pool.buf.items()}
    with pytest.raises(L.GearError):
        dec.extend(torch.randint(0, 1000, (1, 120)).cuda())
    assert dec.pos == 200 and (dec.layers[0]["cache"].n_comp, dec.layers[0]["cache"].n_win) == (192, 8)
    for k, t in dec.pool.buf.items():
        assert torch.equal(t, snap[k]), k
