"""GPU tests of the fast decode path: pre-allocated GearKVCache + segment-aware fused attention + the per-token glue
kernels (gear_amd/cache.py, gear_amd/fast_decode.py, csrc/decode_ops.hip)."""
import math

import numpy as np
import pytest
import torch

import attn_probe as AP
from conftest import rel_fro
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def host(t):
    return t.detach().cpu().numpy()


def _reconstruct_cache(c):
    """float64 [B,H,n_comp,128] K and V from the cache buffers (dequant + per-segment Q P^T; a stored outlier replaces the
    dequantized value, the low-rank term on top) -- attn_probe's."""
    return AP.reconstruct_cache(c)


def _ref_attn(q, K, V, kw, vw, n_rep):
    K = np.concatenate([K, kw.astype(np.float64)], 2)
    V = np.concatenate([V, vw.astype(np.float64)], 2)
    K, V = np.repeat(K, n_rep, 1), np.repeat(V, n_rep, 1)
    s = np.einsum("bhd,bhtd->bht", q.astype(np.float64)[:, :, 0], K) / math.sqrt(128)
    s -= s.max(-1, keepdims=True)
    a = np.exp(s)
    a /= a.sum(-1, keepdims=True)
    return np.einsum("bht,bhtd->bhd", a, V)[:, :, None]


@pytest.fixture(params=[0, 1], ids=["reduce-launch", "folded-merge"], autouse=True)
def attn_fold(request):
    """Every test of this module also runs with the merge of the attention's partial results folded into the partial launch (option
    attn_fold: the last workgroup of a query head to arrive merges -- same slot partition, same order of additions as the reduce
    kernel, so the same bits)."""
    from gear_amd import _lib as L
    L.load().gear_set_option(b"attn_fold", request.param)
    yield request.param
    L.load().gear_set_option(b"attn_fold", 0)


@pytest.fixture
def attn_option():
    """Select the generic (variable-chunk) decode-attention kernel for one test; always restored."""
    from gear_amd import _lib as L

    def setter(on):
        L.set_option("attn_generic", 1 if on else 0)
    yield setter
    L.set_option("attn_generic", 0)


@pytest.mark.parametrize("method,bits,Hq,Hkv,T0,left", [("gearlKIVI", 2, 4, 4, 200, 0.0), ("gearlKIVI", 4, 4, 2, 64, 0.0),
                                                        ("KIVI", 2, 2, 2, 30, 0.0), ("gearlKIVI", 2, 2, 2, 2304, 0.0),
                                                        ("gearlKIVI", 2, 4, 4, 200, 0.02), ("gearslKIVI", 4, 8, 2, 320, 0.05),
                                                        ("KIVI", 2, 2, 2, 130, 0.02)])
@pytest.mark.parametrize("kernel", ["planned", "lists", "generic"])
def test_cache_attend_matches_reconstruction(attn_option, kernel, method, bits, Hq, Hkv, T0, left):
    """planned = the chunk kernel with the outliers through the sparse tiles, lists = the same kernel walking the sorted lists,
    generic = the any-shape kernel."""
    from gear_amd.cache import GearKVCache
    if kernel == "lists" and not left:
        pytest.skip("no outliers: same launch as planned")
    attn_option(kernel == "generic")
    torch.manual_seed(71)
    cc = dict(compress_method=method, group_size=64, residual=64, quantize_bit=bits, rank=4, rankv=4, loop=3, left=left)
    B, D, steps = 2, 128, 150
    c = GearKVCache(B, Hkv, T0 + steps + 10, cc, "cuda")
    c.use_tiles = kernel == "planned"
    c.prefill(torch.randn(B, Hkv, T0, D).half().cuda(), torch.randn(B, Hkv, T0, D).half().cuda())
    assert c.n_comp == T0 - T0 % 64 and c.n_win == T0 % 64
    worst = 0.0
    for i in range(steps):
        c.append(torch.randn(B, Hkv, 1, D).half().cuda(), torch.randn(B, Hkv, 1, D).half().cuda())
        q = torch.randn(B, Hq, 1, D).half().cuda()
        out = c.attend(q)
        if i % 13 == 0 or c.n_win == 64 or c.n_win == 1:
            K, V = _reconstruct_cache(c)
            ref = _ref_attn(host(q), K, V, host(c.kwin[:, :, :c.n_win]), host(c.vwin[:, :, :c.n_win]), Hq // Hkv)
            worst = max(worst, rel_fro(host(out).astype(np.float64), ref))
        c.maybe_compress()
        assert c.seq_len == T0 + i + 1 and c.n_win < 64
    assert worst < 2e-3, worst
    assert c.n_comp == (T0 + steps) - (T0 + steps) % 64
    if left:   # the tiles hold every list entry of their chunk exactly once (-1: more entries than the tile holds -> list path)
        nblk = (c.n_comp - c.seg0) // 64
        kcnt, vcnt = host(c.kcnt), host(c.vcnt)
        nck = (c.n_comp + 127) // 128
        valid = host(c.koidx)[..., :c.kk0 + nblk * c.kk_blk].astype(np.int64) & 0xFFFF          # [B,H,D,2,n]
        want = np.stack([(valid // 128 == ch).sum(axis=(2, 3, 4)) for ch in range(nck)], axis=-1)      # [B,H,nck]
        got = kcnt[:, :, :nck]
        assert ((got == want) | ((got == -1) & (want > c.dims["ktile_cap"]))).all()
        assert (got >= 0).any()
        assert (vcnt[:, :, :c.n_comp // 64] >= 0).all()
        assert int(vcnt[:, :, :c.n_comp // 64].sum()) == B * c.n_comp * 2 * c.kv


def test_cache_at_its_maximum_length(attn_option):
    """GearKVCache at the longest context it takes (16384 tokens; the chunk kernel stops at 8192, the any-shape kernel takes over):
    prompt of 16200 tokens, decoding across the last block boundaries up to the very last token, attention against the
    reconstruction; a block past the capacity must be refused."""
    from gear_amd.cache import GearKVCache
    torch.manual_seed(73)
    cc = dict(compress_method="gearslKIVI", group_size=64, residual=64, quantize_bit=2, rank=8, rankv=8, loop=3, left=0.02)
    B, Hq, Hkv, D, T0 = 1, 2, 2, 128, 16200
    c = GearKVCache(B, Hkv, 16384, cc, "cuda")
    assert c.Tmax == 16384
    c.prefill(torch.randn(B, Hkv, T0, D).half().cuda(), torch.randn(B, Hkv, T0, D).half().cuda())
    worst = 0.0
    for i in range(16384 - T0):
        c.append(torch.randn(B, Hkv, 1, D).half().cuda(), torch.randn(B, Hkv, 1, D).half().cuda())
        q = torch.randn(B, Hq, 1, D).half().cuda()
        out = c.attend(q)
        if i % 61 == 0 or c.seq_len == 16384:
            K, V = _reconstruct_cache(c)
            ref = _ref_attn(host(q), K, V, host(c.kwin[:, :, :c.n_win]), host(c.vwin[:, :, :c.n_win]), Hq // Hkv)
            worst = max(worst, rel_fro(host(out).astype(np.float64), ref))
        c.maybe_compress()
    assert c.seq_len == 16384 and worst < 2e-3, worst
    for _ in range(64):                                   # the fp16 window still takes a block's worth of tokens ...
        c.append(torch.randn(B, Hkv, 1, D).half().cuda(), torch.randn(B, Hkv, 1, D).half().cuda())
    with pytest.raises(AssertionError):                   # ... which can no longer be compressed into the full cache
        c.maybe_compress()


def _oracle_block(x, layout, k, g, bits):
    """Oracle (fp16-stepwise arithmetic, the fused path's mode) on one block: outlier selection on the block's rows, fill with the
    fp16-rounded row mean, group quantization.  x fp16 [B,H,T,128]; layout "k": rows = channels over T, "v": rows = tokens
    over H*128.  Returns (codes [rows, len], scale, mn, isml, ilrg, rows32)."""
    B, H, T, D = x.shape
    if layout == "k":
        rows = np.ascontiguousarray(x.transpose(0, 1, 3, 2)).reshape(B * H * D, T).astype(np.float32)
    else:
        rows = np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B * T, H * D).astype(np.float32)
    orig = rows.copy()
    isml = ilrg = None
    if k > 0:
        isml, ilrg, mean = orc.outlier_select(rows, k)
        fill = mean.astype(np.float16).astype(np.float32)
        np.put_along_axis(rows, isml, fill[:, None], 1)
        np.put_along_axis(rows, ilrg, fill[:, None], 1)
    q = orc.quant_pack_lastdim(rows.astype(np.float16), g, bits, mode=0)
    return orc.unpack_tensor(q["code"], bits, 1), q["scale"], q["mn"], isml, ilrg, orig


@pytest.mark.parametrize("left,bits,Hkv,count", [(0.0, 2, 2, "nominal"), (0.02, 2, 4, "nominal"), (0.05, 4, 2, "nominal"),
                                                 (0.02, 2, 4, "reference"), (0.05, 4, 2, "reference")])
def test_cache_contents_match_oracle_block_by_block(left, bits, Hkv, count):
    """After a prefill and 150 appended tokens every block of the cache -- packed codes, scale / zero point, outlier lists
    and values -- is what the ORACLE makes of the fp16 K / V of exactly that block (bit-exact: fp16-stepwise arithmetic):
    a block written from the wrong window slice, at the wrong offset or with the wrong list position fails here."""
    from gear_amd.cache import GearKVCache
    torch.manual_seed(73)
    B, D, T0, steps, g, R = 2, 128, 200, 150, 64, 64
    cc = dict(compress_method="gearlKIVI", group_size=g, residual=R, quantize_bit=bits, rank=4, rankv=4, loop=3, left=left,
              block_outlier_count=count)
    c = GearKVCache(B, Hkv, T0 + steps + 10, cc, "cuda")
    if count == "reference" and left:      # the reference's formula on a 64-token row: int(H * D * s / 2), at most half the row
        assert c.kk_blk == min(int(int(B * Hkv * 64 * D * left) / B / 64 / 2), 32) and c.kk_blk > max(1, round(64 * left / 2))
    k_all = torch.randn(B, Hkv, T0 + steps, D).half()
    v_all = torch.randn(B, Hkv, T0 + steps, D).half()
    c.prefill(k_all[:, :, :T0].cuda(), v_all[:, :, :T0].cuda())
    for i in range(T0, T0 + steps):
        c.append(k_all[:, :, i:i + 1].cuda(), v_all[:, :, i:i + 1].cuda())
        c.maybe_compress()
    n = c.n_comp
    assert n == (T0 + steps) // R * R and c.seg0 == T0 // R * R
    fpi = 32 // bits
    kcode = orc.unpack_tensor(host(c.kcode[:, :, :, :n // fpi]), bits, 3)        # [B,H,D,n]
    vcode = orc.unpack_tensor(host(c.vcode[:, :, :n]), bits, 3)                  # [B,H,n,D]
    blocks = [(0, c.seg0, c.kk0)] + [(t, t + R, c.kk_blk) for t in range(c.seg0, n, R)]
    o_off = 0
    for t0, t1, kk in blocks:
        kb, vb = k_all[:, :, t0:t1].numpy(), v_all[:, :, t0:t1].numpy()
        T = t1 - t0
        # ---- K: rows = channels over the block's tokens
        qc, sc, mn, isml, ilrg, rows = _oracle_block(kb, "k", kk, g, bits)
        got = kcode[:, :, :, t0:t1].reshape(B * Hkv * D, T)
        mask = np.ones_like(qc, bool)
        if kk:
            np.put_along_axis(mask, isml, False, 1)
            np.put_along_axis(mask, ilrg, False, 1)
            oi = (host(c.koidx[..., o_off:o_off + kk]).astype(np.int64) & 0xFFFF).reshape(B * Hkv * D, 2, kk) - t0
            assert np.array_equal(oi[:, 0], np.sort(isml, 1)) and np.array_equal(oi[:, 1], np.sort(ilrg, 1)), (t0, "K outlier sets")
            ov = host(c.koval[..., o_off:o_off + kk]).reshape(B * Hkv * D, 2 * kk)
            assert np.array_equal(ov.view(np.uint16), np.take_along_axis(rows, oi.reshape(B * Hkv * D, 2 * kk), 1).astype(np.float16).view(np.uint16))
        assert np.array_equal(got[mask], qc[mask]), (t0, "K codes")
        assert np.array_equal(host(c.kscale[:, :, :, t0 // g:t1 // g]).reshape(sc.shape).view(np.uint16), sc.view(np.uint16)), (t0, "K scale")
        assert np.array_equal(host(c.kmn[:, :, :, t0 // g:t1 // g]).reshape(mn.shape).view(np.uint16), mn.view(np.uint16)), (t0, "K mn")
        o_off += kk
        # ---- V: rows = tokens across the heads
        qc, sc, mn, isml, ilrg, rows = _oracle_block(vb, "v", c.kv, g, bits)
        got = np.ascontiguousarray(vcode[:, :, t0:t1].transpose(0, 2, 1, 3)).reshape(B * T, Hkv * D)
        mask = np.ones_like(qc, bool)
        if c.kv:
            np.put_along_axis(mask, isml, False, 1)
            np.put_along_axis(mask, ilrg, False, 1)
            oi = (host(c.voidx[:, t0:t1]).astype(np.int64) & 0xFFFF).reshape(B * T, 2 * c.kv)
            assert np.array_equal(oi[:, :c.kv], np.sort(isml, 1)) and np.array_equal(oi[:, c.kv:], np.sort(ilrg, 1)), (t0, "V outlier sets")
            ov = host(c.voval[:, t0:t1]).reshape(B * T, 2 * c.kv)
            assert np.array_equal(ov.view(np.uint16), np.take_along_axis(rows, oi, 1).astype(np.float16).view(np.uint16))
        assert np.array_equal(got[mask], qc[mask]), (t0, "V codes")
        vs = np.ascontiguousarray(host(c.vscale[:, :, t0:t1]).transpose(0, 2, 1, 3)).reshape(sc.shape)
        vm = np.ascontiguousarray(host(c.vmn[:, :, t0:t1]).transpose(0, 2, 1, 3)).reshape(mn.shape)
        assert np.array_equal(vs.view(np.uint16), sc.view(np.uint16)) and np.array_equal(vm.view(np.uint16), mn.view(np.uint16)), (t0, "V scale / mn")
    # nothing was written past the compressed tokens
    assert int(c.kcode[:, :, :, n // fpi:].abs().max()) == 0 and int(c.vcode[:, :, n:].abs().max()) == 0
    # the factors of every segment approximate that block's error: reconstruction beats the quantized backbone alone
    K, V = _reconstruct_cache(c)
    ek = np.linalg.norm(K - k_all[:, :, :n].numpy().astype(np.float64))
    c.lowrank = False
    K0, _ = _reconstruct_cache(c)
    c.lowrank = True
    assert ek < np.linalg.norm(K0 - k_all[:, :, :n].numpy().astype(np.float64))


def test_glue_kernels_match_torch():
    from gear_amd import _lib as L
    from gear_amd.cache import GearKVCache
    from gear_amd.modeling_llamagear import LlamaRMSNorm, LlamaRotaryEmbedding, apply_rotary_pos_emb
    torch.manual_seed(72)
    B, Hq, Hkv, D = 2, 4, 2, 128
    cc = dict(compress_method="KIVI", group_size=64, residual=64, quantize_bit=2, rank=0, rankv=0, loop=0)
    c = GearKVCache(B, Hkv, 256, cc, "cuda")
    rot = LlamaRotaryEmbedding(D, 4096, 10000.0).cuda()
    for pos in (0, 1, 777, 4095):
        c.n_win = 5
        qkv = torch.randn(B, (Hq + 2 * Hkv) * D).half().cuda()
        q = c.append_rope(qkv, Hq, pos, 10000.0)
        qq, kk, vv = qkv.split([Hq * D, Hkv * D, Hkv * D], -1)
        qq, kk, vv = qq.view(B, 1, Hq, D).transpose(1, 2), kk.view(B, 1, Hkv, D).transpose(1, 2), vv.view(B, 1, Hkv, D).transpose(1, 2)
        cos, sin = rot(vv, torch.tensor([[pos]], device="cuda"))
        qr, kr = apply_rotary_pos_emb(qq, kk, cos, sin)
        assert float((q.float() - qr.float()).abs().max()) < 4e-3 * max(1.0, float(qr.abs().max()))
        assert float((c.kwin[:, :, 5].float() - kr[:, :, 0].float()).abs().max()) < 4e-3 * max(1.0, float(kr.abs().max()))
        assert torch.equal(c.vwin[:, :, 5], vv[:, :, 0])
    # add + rmsnorm
    lib = L.load()
    H = 512
    res, delta = torch.randn(3, H).half().cuda(), torch.randn(3, H).half().cuda()
    norm = LlamaRMSNorm(H, 1e-5).half().cuda()
    norm.weight.data = torch.randn(H).half().cuda()
    y, ro = torch.empty_like(res), torch.empty_like(res)
    L.check(lib.gear_add_rmsnorm(L.ptr(res), L.ptr(delta), L.ptr(norm.weight), 3, H, 1e-5, L.ptr(ro), L.ptr(y), L.stream_ptr()), "n")
    assert torch.equal(ro, res + delta)
    ref = norm(res + delta)
    assert float((y.float() - ref.float()).abs().max()) <= 2e-3 * float(ref.abs().max())
    # silu * up
    gu = torch.randn(3, 2 * 300).half().cuda()
    out = torch.empty(3, 300).half().cuda()
    L.check(lib.gear_silu_mul(L.ptr(gu), 3, 300, L.ptr(out), L.stream_ptr()), "s")
    ref = torch.nn.functional.silu(gu[:, :300]) * gu[:, 300:]
    assert float((out.float() - ref.float()).abs().max()) <= 2e-3 * float(ref.abs().max())


def _tiny(method, n_kv=2):
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    cfg = LlamaConfigLite(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=3,
                          num_attention_heads=4, num_key_value_heads=n_kv, k_bits=4, v_bits=4)
    cc = dict(compress_method=method, group_size=64, residual=64, quantize_bit=4, rank=4, rankv=4, loop=3)
    torch.manual_seed(0)
    return LlamaForCausalLM_GEARKIVI(cfg, cc).half().cuda().eval()


@pytest.mark.parametrize("n_kv", [2, 4])
def test_fast_decoder_tracks_the_attention_hook_module(n_kv):
    """Quantization-only cache (no random bases): the fast path and the reference-shaped module see the same tokens and
    must produce near-identical logits over a decode run that crosses two block boundaries -- with 2 KV heads through the kernel
    chain, with 4 through the single-launch block compressor (cache.BLOCK_KERNEL_MIN_HEADS)."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("KIVI", n_kv)
    ids = torch.randint(0, 1000, (1, 100)).cuda()
    fast = FastGearDecoder(model, 512)
    with torch.no_grad():
        lf = fast.prefill(ids)
        lm, past = model(ids, None, True)
        cos = torch.nn.functional.cosine_similarity(lf.float(), lm[:, -1].float()).min()
        assert cos > 0.999, cos
        tok = lm[:, -1].argmax(-1, keepdim=True)
        worst = 1.0
        for i in range(100):
            lf = fast.step(tok)
            lm, past = model(tok, past, True)
            worst = min(worst, float(torch.nn.functional.cosine_similarity(lf.float(), lm[:, -1].float()).min()))
            tok = lm[:, -1].argmax(-1, keepdim=True)
        assert worst > 0.995, worst
    assert fast.layers[0]["cache"].n_comp == 192 and fast.layers[0]["cache"].n_win == 8


def _hook_run(model, ids, n, teacher=None):
    model.model._hook_graph = None
    outs, toks = [], []
    with torch.no_grad():
        torch.manual_seed(7)          # (block boundaries draw their power-iteration bases from torch's generator)
        logits, past = model(ids, None, True)
        nxt = logits[:, -1].argmax(-1, keepdim=True)
        for i in range(n):
            if teacher is not None:
                nxt = teacher[i]
            toks.append(nxt)
            logits, past = model(nxt, past, True)
            outs.append(logits[:, -1].clone())
            nxt = logits[:, -1].argmax(-1, keepdim=True)
    return outs, toks, past


@pytest.mark.parametrize("batch", [1, 2])
def test_hook_decode_step_variants_agree(batch):
    """The attention hook's fused decode step: (a) with the norm weights folded into second copies of q/k/v and
    gate/up (the default: 345 against 316 tokens/s at 7B shapes) against the modules' own weights with the norm weight applied
    in the GEMV loop -- fp16 rounding apart; (b) the same step replayed as ONE hipGraph (LlamaModel_GEAR.graph_decode) against
    the eager launches -- the same kernels in the same order: logits equal to an fp16 ulp over 150 tokens and two block
    boundaries, cache counters and slot 8 identical."""
    from gear_amd.modeling_llamagear import LlamaDecoderLayer_GEAR
    model = _tiny("gearlKIVI", 2)
    ids = torch.randint(0, 1000, (batch, 200 if batch == 1 else 70)).cuda()
    n = 150 if batch == 1 else 80
    old = LlamaDecoderLayer_GEAR.fold_norm_weights
    try:
        LlamaDecoderLayer_GEAR.fold_norm_weights = False
        own, toks, _ = _hook_run(model, ids, n)
        LlamaDecoderLayer_GEAR.fold_norm_weights = True
        fold, _, past_e = _hook_run(model, ids, n, teacher=toks)
        worst = min(float(torch.nn.functional.cosine_similarity(a.float(), b.float()).min()) for a, b in zip(own, fold))
        assert worst > 0.999, worst
        # the block boundaries' random bases drawn ahead during the token steps (LlamaModel_GEAR.prefetch_bases) are the bases drawn
        # at the boundary: same values in the same order of torch's CPU generator -> the same logits, bit for bit
        model.model.prefetch_bases = False
        nopf, _, _ = _hook_run(model, ids, n, teacher=toks)
        model.model.prefetch_bases = True
        assert all(torch.equal(a, b) for a, b in zip(fold, nopf)), "prefetched bases changed the result"
        model.model.graph_decode = True
        graph, _, past_g = _hook_run(model, ids, n, teacher=toks)
        assert model.model._hook_graph is not None, "the graph path was not taken"
        diff = max(float((a.float() - b.float()).abs().max()) for a, b in zip(fold, graph))
        scale = max(float(a.float().abs().max()) for a in fold)
        assert diff <= 2e-3 * scale, (diff, scale)
        assert past_g[0][8] == past_e[0][8] == ids.shape[1] + n
        ce, cg = past_e[0].cache, past_g[0].cache
        assert (ce.n_comp, ce.n_win) == (cg.n_comp, cg.n_win)
        assert torch.equal(ce.kcode[..., :ce.n_comp // ce.fpi], cg.kcode[..., :cg.n_comp // cg.fpi])
    finally:
        LlamaDecoderLayer_GEAR.fold_norm_weights = old
        model.model.graph_decode = False
        model.model.prefetch_bases = True


@pytest.mark.parametrize("batch, n_kv", [(1, 2), (2, 4), (6, 2)])
def test_fp16_cache_baseline_decoder(batch, n_kv):
    """cache_kind='fp16' (the uncompressed model "None" of the reference's harness, cuda_supported_gear/test.py:41-62) through the same
    decoder: a token step over the fp16 cache must give the logits of the dense causal forward over prompt + token (the decoder's own
    prefill path: torch SDPA), for the fused GEMV path (batch <= 4) and the library-GEMM path (batch 6), MHA-like and grouped heads."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("KIVI", n_kv)
    torch.manual_seed(batch)
    ids = torch.randint(0, 1000, (batch, 151)).cuda()
    dec = FastGearDecoder(model, 256, batch=batch, cache_kind="fp16")
    ref = FastGearDecoder(model, 256, batch=batch, cache_kind="fp16")
    with torch.no_grad():
        dec.prefill(ids[:, :140])
        for t in range(140, 151):
            ls = dec.step(ids[:, t:t + 1])
        lr = ref.prefill(ids)
    assert dec.layers[0]["cache"].n_win == 151 and dec.pool is None
    cos = torch.nn.functional.cosine_similarity(ls.float(), lr.float()).min()
    assert cos > 0.9995, cos
    assert float((ls.float() - lr.float()).abs().max()) <= 2e-2 * float(lr.float().abs().max())
    with pytest.raises(NotImplementedError):
        dec.step_graph()


def test_fast_decoder_generate_lowrank_deterministic():
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearlKIVI")
    ids = torch.randint(0, 1000, (2, 70)).cuda()
    a = FastGearDecoder(model, 256, batch=2, seed=3).generate(ids, 200)
    b = FastGearDecoder(model, 256, batch=2, seed=3).generate(ids, 200)
    assert a.shape == (2, 200) and torch.equal(a, b) and torch.equal(a[:, :70], ids)


def test_graph_and_eager_steps_interleave():
    """step() after the graph was captured moves the host counters only; the next replay must first bring the device-side
    {pos, slot, T, W} up to date (round-1 advisor finding: it replayed with a stale state).  Teacher-forced against a purely
    eager decoder over a run with outliers in the cache and one block boundary."""
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    cfg = LlamaConfigLite(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2,
                          num_attention_heads=4, num_key_value_heads=2, k_bits=2, v_bits=2)
    cc = dict(compress_method="gearlKIVI", group_size=64, residual=64, quantize_bit=2, rank=4, rankv=4, loop=3, left=0.03)
    torch.manual_seed(0)
    model = LlamaForCausalLM_GEARKIVI(cfg, cc).half().cuda().eval()
    ids = torch.randint(0, 1000, (1, 100)).cuda()
    fe, fg = FastGearDecoder(model, 512, seed=5), FastGearDecoder(model, 512, seed=5)
    tok = fe.prefill(ids).argmax(-1, keepdim=True)
    fg.prefill(ids)
    worst = 1.0
    for i in range(60):
        le = fe.step(tok)
        if i % 3 == 2 or i < 2:
            lg = fg.step(tok)                     # eager step in between
        else:
            fg.step_graph(tok)
            lg = fg.logits_static
        worst = min(worst, float(torch.nn.functional.cosine_similarity(le.float(), lg.float()).min()))
        tok = le.argmax(-1, keepdim=True)
    assert worst > 0.9995, worst
    assert (fe.pos, fe.layers[0]["cache"].n_comp) == (fg.pos, fg.layers[0]["cache"].n_comp) == (160, 128)


def test_graph_replay_matches_eager_decode():
    """The hipGraph-captured token step (device-side pos / slot / T / W) tracks the eager fast path token for token,
    across block compressions (which run eagerly between replays).  The graph plans the attention split for the cache
    capacity, so sums associate differently: compare logits, teacher-forced with the eager path's tokens."""
    from gear_amd.fast_decode import FastGearDecoder
    for method in ("KIVI", "gearlKIVI"):
        model = _tiny(method)
        ids = torch.randint(0, 1000, (2, 90)).cuda()
        fe, fg = FastGearDecoder(model, 512, batch=2, seed=5), FastGearDecoder(model, 512, batch=2, seed=5)
        tok = fe.prefill(ids).argmax(-1, keepdim=True)
        fg.prefill(ids)
        tok2 = fe.step(tok).argmax(-1, keepdim=True)
        fg.step(tok)
        tok = tok2
        worst = 1.0
        for i in range(150):
            le = fe.step(tok)
            nxt_g = fg.step_graph(tok)
            lg = fg.logits_static
            worst = min(worst, float(torch.nn.functional.cosine_similarity(le.float(), lg.float()).min()))
            assert torch.isfinite(lg).all()
            tok = le.argmax(-1, keepdim=True)
        assert worst > 0.9995, (method, worst)
        ce, cg = fe.layers[0]["cache"], fg.layers[0]["cache"]
        assert (ce.n_comp, ce.n_win, fe.pos) == (cg.n_comp, cg.n_win, fg.pos) == (192, 49, 241)   # 90 + 1 + 150 tokens
        assert fg.state.tolist() == [241, 49, 192, 50]


@pytest.mark.parametrize("B,K,N", [(1, 4096, 4096), (1, 11008, 4096), (2, 4096, 12288), (4, 512, 1000), (3, 4096, 32000), (1, 64, 7)])
def test_gemv_f16_matches_library(B, K, N):
    from gear_amd import _lib as L
    torch.manual_seed(81)
    x = torch.randn(B, K).half().cuda()
    w = (torch.randn(N, K) * 0.05).half().cuda()
    y = torch.empty(B, N).half().cuda()
    L.check(L.load().gear_gemv_f16(L.ptr(x), L.ptr(w), B, K, N, L.ptr(y), L.stream_ptr()), "gemv")
    ref = x.double() @ w.double().t()
    assert rel_fro(host(y).astype(np.float64), host(ref)) < 1e-3


@pytest.mark.parametrize("B", [1, 3])
def test_fused_norm_gemv_matches_the_unfused_chain(B):
    """gear_gemv_f16_norm == add -> RMSNorm -> linear (-> SwiGLU) of torch on the same fp16 tensors, to fp16 rounding."""
    from gear_amd import _lib as L
    from gear_amd.modeling_llamagear import LlamaRMSNorm
    lib = L.load()
    K, N = 512, 328
    torch.manual_seed(1)
    res, delta = torch.randn(B, K).half().cuda(), torch.randn(B, K).half().cuda()
    norm = LlamaRMSNorm(K, 1e-5).half().cuda()
    norm.weight.data = (1 + 0.1 * torch.randn(K)).half().cuda()
    W = (torch.randn(N, K) / K ** 0.5).half().cuda()
    for d in (delta, None):
        for swiglu in (0, 1, 2):     # 1: (gate, up) rows interleaved; 2: blocked [gate rows | up rows], as the modules hold them
            y = torch.empty(B, N // 2 if swiglu else N).half().cuda()
            ro = torch.empty_like(res)
            L.check(lib.gear_gemv_f16_norm(L.ptr(res), L.ptr(d), L.ptr(norm.weight), 1e-5, L.ptr(W), B, K, N, swiglu,
                                           L.ptr(ro), L.ptr(y), L.stream_ptr()), "gemv_norm")
            v = res + d if d is not None else res
            if d is not None:
                assert torch.equal(ro, v)
            ref = torch.nn.functional.linear(norm(v).float(), W.float())
            if swiglu == 1:
                ref = torch.nn.functional.silu(ref[:, 0::2]) * ref[:, 1::2]
            elif swiglu == 2:
                ref = torch.nn.functional.silu(ref[:, :N // 2]) * ref[:, N // 2:]
            assert float((y.float() - ref).abs().max()) <= 4e-3 * float(ref.abs().max())
    # blocked == interleaved on the permuted weight, bit for bit (the same pairs, the same arithmetic)
    Wi = torch.stack([W[:N // 2], W[N // 2:]], 1).reshape(N, K).contiguous()
    y1, y2 = torch.empty(B, N // 2).half().cuda(), torch.empty(B, N // 2).half().cuda()
    L.check(lib.gear_gemv_f16_norm(L.ptr(res), None, L.ptr(norm.weight), 1e-5, L.ptr(Wi), B, K, N, 1, None, L.ptr(y1), L.stream_ptr()), "il")
    L.check(lib.gear_gemv_f16_norm(L.ptr(res), None, L.ptr(norm.weight), 1e-5, L.ptr(W), B, K, N, 2, None, L.ptr(y2), L.stream_ptr()), "bl")
    assert torch.equal(y1, y2)
    # norm weight folded into W's columns (norm_w NULL) + the residual-add GEMV, in place
    Wf = (W.float() * norm.weight.float()[None, :]).half()
    y = torch.empty(B, N).half().cuda()
    L.check(lib.gear_gemv_f16_norm(L.ptr(res), None, None, 1e-5, L.ptr(Wf), B, K, N, 0, None, L.ptr(y), L.stream_ptr()), "folded")
    ref = torch.nn.functional.linear(norm(res).float(), W.float())
    assert float((y.float() - ref).abs().max()) <= 4e-3 * float(ref.abs().max())
    for Kd in (K, 8192 + 64):   # the second shape takes the split-K path
        xd, Wd = torch.randn(B, Kd).half().cuda(), (torch.randn(K, Kd) / Kd ** 0.5).half().cuda()
        r0 = torch.randn(B, K).half().cuda()
        ref = (r0.float() + torch.nn.functional.linear(xd.float(), Wd.float()).half().float()).half()
        r1 = r0.clone()
        L.check(lib.gear_gemv_f16_add(L.ptr(xd), L.ptr(Wd), B, Kd, K, L.ptr(r1), L.ptr(r1), L.stream_ptr()), "add")
        assert float((r1.float() - ref.float()).abs().max()) <= 4e-3 * float(ref.abs().max())
    # aliasing the new residual with an input is refused (other workgroups still read it)
    with pytest.raises(L.GearError):
        L.check(lib.gear_gemv_f16_norm(L.ptr(res), L.ptr(delta), L.ptr(norm.weight), 1e-5, L.ptr(W), B, K, N, 0,
                                       L.ptr(res), L.ptr(y), L.stream_ptr()), "alias")


def test_fused_qkv_rope_matches_gemv_plus_rope_append():
    """gear_gemv_qkv_rope == gear_add_rmsnorm -> gear_gemv_f16 -> gear_rope_append (the same rotation arithmetic on GEMV
    outputs that differ by fp16 rounding of the folded norm scale), with host and device-side pos / slot."""
    from gear_amd import _lib as L
    lib = L.load()
    B, K, Hq, Hkv, R = 2, 512, 4, 2, 64
    torch.manual_seed(2)
    res, delta = torch.randn(B, K).half().cuda(), torch.randn(B, K).half().cuda()
    nw = (1 + 0.1 * torch.randn(K)).half().cuda()
    W = (torch.randn((Hq + 2 * Hkv) * 128, K) / K ** 0.5).half().cuda()
    pos, slot = 777, 9
    # unfused chain
    x, ro = torch.empty_like(res), torch.empty_like(res)
    L.check(lib.gear_add_rmsnorm(L.ptr(res), L.ptr(delta), L.ptr(nw), B, K, 1e-5, L.ptr(ro), L.ptr(x), L.stream_ptr()), "n")
    qkv = torch.empty(B, W.shape[0]).half().cuda()
    L.check(lib.gear_gemv_f16(L.ptr(x), L.ptr(W), B, K, W.shape[0], L.ptr(qkv), L.stream_ptr()), "g")
    q0 = torch.empty(B, Hq, 1, 128).half().cuda()
    kw0, vw0 = torch.zeros(B, Hkv, R, 128).half().cuda(), torch.zeros(B, Hkv, R, 128).half().cuda()
    L.check(lib.gear_rope_append(L.ptr(qkv), B, Hq, Hkv, 128, pos, 10000.0, L.ptr(q0), L.ptr(kw0), L.ptr(vw0), slot, R,
                                 L.stream_ptr()), "r")
    state = torch.tensor([pos, slot, 0, slot + 1], dtype=torch.int32).cuda()
    for dyn in (None, state):
        q1 = torch.empty_like(q0)
        kw1, vw1, ro1 = torch.zeros_like(kw0), torch.zeros_like(vw0), torch.empty_like(res)
        L.check(lib.gear_gemv_qkv_rope(L.ptr(res), L.ptr(delta), L.ptr(nw), 1e-5, L.ptr(W), B, K, Hq, Hkv, 128,
                                       0 if dyn is not None else pos, 0 if dyn is not None else slot, R, 10000.0,
                                       L.ptr(dyn), L.ptr(ro1), L.ptr(q1), L.ptr(kw1), L.ptr(vw1), L.stream_ptr()), "f")
        assert torch.equal(ro1, ro)
        for got, ref in ((q1, q0), (kw1, kw0), (vw1, vw0)):
            assert float((got.float() - ref.float()).abs().max()) <= 6e-3 * float(ref.abs().max())
        # only the addressed slot is written
        assert float(kw1[:, :, :slot].abs().max()) == 0 and float(kw1[:, :, slot + 1:].abs().max()) == 0


@pytest.mark.parametrize("left", [0.0, 0.03])
def test_pooled_block_compress_matches_per_layer(left):
    """GearKVCachePool.compress_all (all layers' windows in one compress call) writes exactly what the per-layer
    GearKVCache.maybe_compress path writes (quantization-only cache: no random bases involved), outlier lists included."""
    from gear_amd.cache import GearKVCache, GearKVCachePool
    torch.manual_seed(91)
    cc = dict(compress_method="KIVI", group_size=64, residual=64, quantize_bit=2, rank=0, rankv=0, loop=0, left=left)
    Lyr, B, H, D = 3, 2, 2, 128
    pool = GearKVCachePool(Lyr, B, H, 256, cc, "cuda", D)
    pooled = [GearKVCache(B, H, 256, cc, "cuda", D, pool=pool, layer=i) for i in range(Lyr)]
    single = [GearKVCache(B, H, 256, cc, "cuda", D) for _ in range(Lyr)]
    for blk in range(2):
        for _ in range(64):
            for cp, cs in zip(pooled, single):
                k, v = torch.randn(B, H, 1, D).half().cuda(), torch.randn(B, H, 1, D).half().cuda()
                cp.append(k, v)
                cs.append(k, v)
        pool.compress_all()
        for cs in single:
            cs.maybe_compress()
        for cp, cs in zip(pooled, single):
            assert cp.n_comp == cs.n_comp == 64 * (blk + 1) and cp.n_win == cs.n_win == 0
            for name in ("kcode", "kscale", "kmn", "vcode", "vscale", "vmn") + (("koidx", "koval", "voidx", "voval", "kcnt", "vcnt") if left else ()):
                assert torch.equal(getattr(cp, name), getattr(cs, name)), name
    q = torch.randn(B, 4, 1, D).half().cuda()
    a, b_ = pooled[1].attend(q), single[1].attend(q)
    if left:   # the sparse corrections are added with fp32 LDS atomics: the order of the additions is not fixed
        assert float((a.float() - b_.float()).abs().max()) <= 2e-3 * float(b_.float().abs().max())
    else:
        assert torch.equal(a, b_)


@pytest.mark.parametrize("method,bits,left", [("gearslKIVI", 2, 0.02), ("KIVI", 4, 0.0)])
def test_cache_with_the_kivi_default_residual_of_128(method, bits, left):
    """residual_length = 128 (the KIVI default, cuda_supported_gear/modeling_llama_kivi.py): a 128-token fp16 window, blocks of
    128 tokens compressed in place; attention over compressed + window tokens against the float64 reconstruction."""
    from gear_amd.cache import GearKVCache
    torch.manual_seed(74)
    B, Hq, Hkv, D, T0, steps, R = 1, 4, 2, 128, 300, 280, 128
    cc = dict(compress_method=method, group_size=64, residual=R, quantize_bit=bits, rank=4, rankv=4, loop=3, left=left)
    c = GearKVCache(B, Hkv, T0 + steps + 10, cc, "cuda")
    c.prefill(torch.randn(B, Hkv, T0, D).half().cuda(), torch.randn(B, Hkv, T0, D).half().cuda())
    assert c.n_comp == 256 and c.n_win == 44
    worst, seen_full = 0.0, False
    for i in range(steps):
        c.append(torch.randn(B, Hkv, 1, D).half().cuda(), torch.randn(B, Hkv, 1, D).half().cuda())
        q = torch.randn(B, Hq, 1, D).half().cuda()
        out = c.attend(q)
        if i % 17 == 0 or c.n_win in (1, 65, 127, 128):
            seen_full |= c.n_win == 128
            K, V = _reconstruct_cache(c)
            ref = _ref_attn(host(q), K, V, host(c.kwin[:, :, :c.n_win]), host(c.vwin[:, :, :c.n_win]), Hq // Hkv)
            worst = max(worst, rel_fro(host(out).astype(np.float64), ref))
        c.maybe_compress()
        assert c.n_win < 128
    assert seen_full and worst < 2e-3, worst
    assert c.n_comp == (T0 + steps) // R * R


@pytest.mark.parametrize("case,bits,lowrank", [("gear_kivi_b2", 2, False), ("gear_stance_gearl_b2", 2, True)])
def test_streaming_cache_matches_reference_forward_trace(golden, case, bits, lowrank):
    """FastGearDecoder's data path -- GearKVCache: in-place window append, gear_attn_decode_cache, gear_compress_block at block
    boundaries -- held to the traces made by EXECUTING the reference's LlamaAttention_GEAR.forward (tests/golden/make_f8_ref.py,
    cuda_supported_gear/modeling_llamagear.py:177-484): fed the trace's post-projection q / k / v step by step, the attention output
    of every decode step matches the reference's (1e-3 overall, 2e-3 worst step, the hook module's own tolerance) and the packed K / V
    codes + scale + zero point + fp16 windows are the reference's bit for bit.  With low-rank factors the payload is still
    bit-identical; the factors start from the cache's own random basis (channel side, not the reference's token-side draw), and on
    this fixture's white-noise error matrices -- no dominant directions for three power iterations to find -- two random starts give
    two different rank-4 terms, so the outputs are only loosely comparable there (12 % apart; the hook module, which draws the
    reference's bases, is held to 2e-3 on the same trace in test_gpu_attention.py)."""
    from gear_amd.cache import GearKVCache
    f = golden(f"f8_ref_{case}.npz")
    qkv = torch.from_numpy(f[case + "_qkv"]).cuda()                 # [3, 1, H, T, D]
    ref = f[case + "_out"]                                          # [1, 1 + steps, H*D]
    H, T, D = qkv.shape[2], qkv.shape[3], qkv.shape[4]
    steps = ref.shape[1] - 1
    TP = T - steps
    cc = dict(compress_method="gearlKIVI" if lowrank else "KIVI", group_size=64, residual=64, quantize_bit=bits, rank=4, rankv=4, loop=3)
    c = GearKVCache(1, H, T + 64, cc, "cuda", D, seed=3)
    c.prefill(qkv[1][:, :, :TP].contiguous(), qkv[2][:, :, :TP].contiguous())
    outs = []
    for i in range(steps):
        t = TP + i
        c.append(qkv[1][:, :, t:t + 1].contiguous(), qkv[2][:, :, t:t + 1].contiguous())
        o = c.attend(qkv[0][:, :, t:t + 1].contiguous())          # [1, H, 1, D]
        outs.append(host(o).transpose(0, 2, 1, 3).reshape(1, 1, H * D))
        c.maybe_compress()
    got = np.concatenate(outs, 1)
    want = ref[:, 1:]
    tol_all, tol_step = (1e-3, 2e-3) if not lowrank else (0.25, 0.5)     # (1e-3 / 2e-3 since round 5's fp32-weight fixture stand-in)
    assert rel_fro(got, want) < tol_all, rel_fro(got, want)
    assert max(rel_fro(got[:, i], want[:, i]) for i in range(steps)) < tol_step
    n, fpi = c.n_comp, 32 // bits
    assert c.seq_len == int(f[case + "_seq"][0])
    same = lambda t, a: np.array_equal(host(t).view(np.uint16), a.view(np.uint16)) if a.dtype == np.float16 else np.array_equal(host(t), a)
    assert same(c.kcode[..., :n // fpi], f[case + "_kcode"]) and same(c.vcode[:, :, :n], f[case + "_vcode"])
    assert same(c.kscale[..., :n // 64], f[case + "_kscale"]) and same(c.kmn[..., :n // 64], f[case + "_kmn"])
    assert same(c.vscale[:, :, :n], f[case + "_vscale"]) and same(c.vmn[:, :, :n], f[case + "_vmn"])
    assert same(c.kwin[:, :, :c.n_win], f[case + "_kfull"]) and same(c.vwin[:, :, :c.n_win], f[case + "_vfull"])


@pytest.mark.parametrize("method,bits,Hq,Hkv,T0,left,rank", [("gearslKIVI", 2, 8, 2, 520, 0.02, 8), ("gearslKIVI", 2, 8, 1, 300, 0.05, 16),
                                                             ("gearlKIVI", 4, 4, 2, 200, 0.0, 4), ("KIVI", 2, 2, 2, 190, 0.02, 0),
                                                             ("gearslKIVI", 2, 16, 2, 130, 0.02, 8), ("gearslKIVI", 4, 6, 2, 260, 0.03, 8)])
def test_matrix_core_attention_kernel(method, bits, Hq, Hkv, T0, left, rank):
    """Round 5: attn_decode_partial_mfma -- the chunk's codes once into an LDS tile as exact fp16 integers, scores and outputs as
    v_mfma_f32_32x32x16_f16 with the scaled q / p rows of up to 8 query heads as ONE A operand, outlier corrections scattered into the
    zeroed tile -- against the float64 reconstruction of the cache (2e-3, the vector kernel's tolerance) and against the vector kernel
    (option attn_mfma = -1) on the same cache; 2 / 4 / 8 / 1 (ratio 3) query heads per KV head, ranks 0 / 4 / 8 / 16, 2 and 4 bits,
    ragged last chunk, window, decode-time blocks."""
    from gear_amd import _lib as L
    from gear_amd.cache import GearKVCache
    torch.manual_seed(73)
    cc = dict(compress_method=method, group_size=64, residual=64, quantize_bit=bits, rank=rank, rankv=rank, loop=3, left=left)
    B, D, steps = 2, 128, 140
    c = GearKVCache(B, Hkv, T0 + steps + 10, cc, "cuda")
    c.prefill(torch.randn(B, Hkv, T0, D).half().cuda(), torch.randn(B, Hkv, T0, D).half().cuda())
    worst = worst_ab = 0.0
    try:
        for i in range(steps):
            c.append(torch.randn(B, Hkv, 1, D).half().cuda(), torch.randn(B, Hkv, 1, D).half().cuda())
            q = torch.randn(B, Hq, 1, D).half().cuda()
            L.set_option("attn_mfma", 1)
            out = c.attend(q)
            if i % 11 == 0 or c.n_win in (1, 64):
                L.set_option("attn_mfma", -1)
                out_v = c.attend(q)
                worst_ab = max(worst_ab, rel_fro(host(out).astype(np.float64), host(out_v).astype(np.float64)))
                K, V = _reconstruct_cache(c)
                ref = _ref_attn(host(q), K, V, host(c.kwin[:, :, :c.n_win]), host(c.vwin[:, :, :c.n_win]), Hq // Hkv)
                worst = max(worst, rel_fro(host(out).astype(np.float64), ref))
            c.maybe_compress()
    finally:
        L.set_option("attn_mfma", 0)
    assert worst < 2e-3, worst
    assert worst_ab < 1e-3, worst_ab


def test_matrix_core_attention_with_overflowed_tiles():
    """A chunk / block whose sparse tile overflowed (count -1) sends the matrix-core kernel to the sorted lists: K outliers of every
    channel crowded into the first 128 tokens, V outliers of every row crowded into one head."""
    from gear_amd import _lib as L
    from gear_amd.cache import GearKVCache
    torch.manual_seed(74)
    cc = dict(compress_method="gearslKIVI", group_size=64, residual=64, quantize_bit=2, rank=8, rankv=8, loop=3, left=0.04)
    B, Hq, Hkv, T0, D = 1, 8, 4, 512, 128
    k = torch.randn(B, Hkv, T0, D)
    v = torch.randn(B, Hkv, T0, D)
    k[:, :, :100] *= 12.0                          # every channel's top / bottom-k tokens lie in chunk 0
    v[:, 1] *= 12.0                                # every row's outliers lie in head 1
    c = GearKVCache(B, Hkv, T0 + 128, cc, "cuda")
    c.prefill(k.half().cuda(), v.half().cuda())
    assert int((c.kcnt[:, :, :4] < 0).sum()) > 0 and int((c.vcnt[:, 1, :8] < 0).sum()) > 0      # the case under test
    c.append(torch.randn(B, Hkv, 1, D).half().cuda(), torch.randn(B, Hkv, 1, D).half().cuda())
    q = torch.randn(B, Hq, 1, D).half().cuda()
    try:
        L.set_option("attn_mfma", 1)
        out = c.attend(q)
        L.set_option("attn_mfma", -1)
        out_v = c.attend(q)
    finally:
        L.set_option("attn_mfma", 0)
    K, V = _reconstruct_cache(c)
    ref = _ref_attn(host(q), K, V, host(c.kwin[:, :, :c.n_win]), host(c.vwin[:, :, :c.n_win]), Hq // Hkv)
    assert rel_fro(host(out).astype(np.float64), ref) < 2e-3
    assert rel_fro(host(out).astype(np.float64), host(out_v).astype(np.float64)) < 1e-3
