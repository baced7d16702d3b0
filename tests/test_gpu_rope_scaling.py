"""RoPE scaling on the GPU: the four frequency-table entry points (gear_rope_append_freq, gear_rope_append_dyn_freq,
gear_gemv_qkv_rope_freq, gear_kivi_rope_append_freq) per element against a float64 restatement of the rotation, their agreement
with the theta entry points on the unscaled table, and the decoders / the attention hook on a tiny model whose config scales.

Bound per rotated element (four fp16 roundings: cos or sin, two products, their sum -- each at most 2^-11 relative, the products
bounded by |x1| and |x2| times a factor near 1):  |got - ref| <= 2^-9 (|x1| + |x2|) + 2^-24.
The reference takes the angle as the kernels do -- the fp32 product pos * inv_freq[p], formed in numpy -- and everything after it in
float64."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=64)
YARN = dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=64)
THETA = 10000.0
HQ, HKV, K, R = 4, 2, 256, 64
POSITIONS = (0, 1, 63, 64, 65, 1000, 16383)


def _table(scaling):
    from types import SimpleNamespace
    from gear_amd.rope import rope_parameters
    inv, af = rope_parameters(SimpleNamespace(rope_theta=THETA, rope_scaling=scaling, max_position_embeddings=4096))
    return inv, af


def _plain_table():
    return (1.0 / (THETA ** (torch.arange(0, 128, 2).float() / 128))), 1.0


def _rotate64(x, pos, inv, af):
    """x [..., 128] fp16 values (numpy) -> (float64 rotation, bound) with cos / sin of the fp32 angle times af."""
    inv = inv.numpy().astype(np.float32)
    ang = (np.float32(pos) * inv).astype(np.float32).astype(np.float64)
    c, s = np.cos(ang) * af, np.sin(ang) * af
    x = x.astype(np.float64)
    x1, x2 = x[..., :64], x[..., 64:]
    ref = np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    b = 2.0 ** -9 * (np.abs(x1) + np.abs(x2)) + 2.0 ** -24
    return ref, np.concatenate([b, b], -1)


def _check(got, x, pos, inv, af, what):
    ref, bound = _rotate64(x, pos, inv, af)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bound).max())
    print(f"{what}: pos {pos}: worst error / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, pos, worst)
    return err, bound


def _np(t):
    return t.detach().cpu().numpy()


def _sees_the_bug(got, x, pos, af):
    """Negative control: against the UNSCALED table the same comparison must fail on a low-frequency pair once pos >= 64."""
    ref, bound = _rotate64(x, pos, _plain_table()[0], af)
    bad = np.abs(got.astype(np.float64) - ref) > bound
    return bool(bad[..., 32:64].any() or bad[..., 96:].any())


@pytest.fixture(scope="module")
def lib():
    from gear_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def qkv():
    torch.manual_seed(11)
    return torch.randn(4, (HQ + 2 * HKV) * 128).half().cuda()


def _split(qkv, B):
    a = _np(qkv[:B]).astype(np.float32)
    return (a[:, :HQ * 128].reshape(B, HQ, 128), a[:, HQ * 128:(HQ + HKV) * 128].reshape(B, HKV, 128),
            a[:, (HQ + HKV) * 128:].reshape(B, HKV, 128))


@pytest.mark.parametrize("scaling", [S, YARN], ids=["llama3", "yarn"])
@pytest.mark.parametrize("dyn", [False, True], ids=["host", "dyn"])
def test_rope_append_freq_against_float64(lib, qkv, scaling, dyn):
    from gear_amd import _lib as L
    inv, af = _table(scaling)
    tab = inv.cuda()
    B, slot = 3, 9
    xq, xk, xv = _split(qkv, B)
    seen = False
    for pos in POSITIONS:
        q = torch.zeros(B, HQ, 1, 128).half().cuda()
        kw, vw = torch.zeros(B, HKV, R, 128).half().cuda(), torch.zeros(B, HKV, R, 128).half().cuda()
        if dyn:
            st = torch.tensor([pos, slot, 0, slot + 1], dtype=torch.int32).cuda()
            rc = lib.gear_rope_append_dyn_freq(L.ptr(qkv), B, HQ, HKV, 128, L.ptr(st), L.ptr(tab), af, L.ptr(q), L.ptr(kw), L.ptr(vw),
                                               R, L.stream_ptr())
        else:
            rc = lib.gear_rope_append_freq(L.ptr(qkv), B, HQ, HKV, 128, pos, L.ptr(tab), af, L.ptr(q), L.ptr(kw), L.ptr(vw), slot, R,
                                           L.stream_ptr())
        L.check(rc, "gear_rope_append_freq")
        gq, gk = _np(q)[:, :, 0].astype(np.float32), _np(kw)[:, :, slot].astype(np.float32)
        _check(gq, xq, pos, inv, af, "q")
        _check(gk, xk, pos, inv, af, "k")
        assert np.array_equal(_np(vw)[:, :, slot].astype(np.float32), xv)
        assert float(kw[:, :, :slot].abs().max()) == 0 and float(kw[:, :, slot + 1:].abs().max()) == 0
        if pos >= 64:
            seen = seen or _sees_the_bug(gk, xk, pos, af)
    assert seen, "the comparison cannot tell scaled from unscaled frequencies"


@pytest.mark.parametrize("scaling", [S, YARN], ids=["llama3", "yarn"])
@pytest.mark.parametrize("B", [1, 3, 4])
def test_gemv_qkv_rope_freq_against_float64(lib, scaling, B):
    from gear_amd import _lib as L
    inv, af = _table(scaling)
    tab = inv.cuda()
    torch.manual_seed(B)
    x = torch.randn(B, K).half().cuda()
    W = (torch.randn((HQ + 2 * HKV) * 128, K) / K ** 0.5).half().cuda()
    N = W.shape[0]
    y = torch.empty(B, N).half().cuda()
    L.check(lib.gear_gemv_f16_norm(L.ptr(x), None, None, 1e-5, L.ptr(W), B, K, N, 0, None, L.ptr(y), L.stream_ptr()), "gemv")
    xq, xk, xv = _split(y, B)
    slot, seen = 5, False
    for pos in POSITIONS:
        for dyn in (None, torch.tensor([pos, slot, 0, slot + 1], dtype=torch.int32).cuda()):
            q = torch.zeros(B, HQ, 1, 128).half().cuda()
            kw, vw = torch.zeros(B, HKV, R, 128).half().cuda(), torch.zeros(B, HKV, R, 128).half().cuda()
            rc = lib.gear_gemv_qkv_rope_freq(L.ptr(x), None, None, 1e-5, L.ptr(W), B, K, HQ, HKV, 128, 0 if dyn is not None else pos,
                                             0 if dyn is not None else slot, R, L.ptr(tab), af, L.ptr(dyn), None, L.ptr(q), L.ptr(kw),
                                             L.ptr(vw), L.stream_ptr())
            L.check(rc, "gear_gemv_qkv_rope_freq")
            gq, gk = _np(q)[:, :, 0].astype(np.float32), _np(kw)[:, :, slot].astype(np.float32)
            _check(gq, xq, pos, inv, af, "q")
            _check(gk, xk, pos, inv, af, "k")
            assert np.array_equal(_np(vw)[:, :, slot].astype(np.float32), xv)
            if pos >= 64:
                seen = seen or _sees_the_bug(gk, xk, pos, af)
    assert seen, "the comparison cannot tell scaled from unscaled frequencies"


@pytest.mark.parametrize("scaling", [S, YARN], ids=["llama3", "yarn"])
@pytest.mark.parametrize("bits", [2, 4])
def test_kivi_rope_append_freq_against_float64_and_its_parent(lib, qkv, scaling, bits):
    from gear_amd import _lib as L
    inv, af = _table(scaling)
    tab = inv.cuda()
    B, n, tcap, kslot = 2, 70, 128, 6
    evict = n - (R + 1)
    xq, xk, xv = _split(qkv, B)
    torch.manual_seed(5)
    ring0 = torch.randn(B, HKV, R + 1, 128).half().cuda()
    seen = False

    def run(freq, pos):
        q = torch.zeros(B, HQ, 1, 128).half().cuda()
        kw, ring = torch.zeros(B, HKV, R, 128).half().cuda(), ring0.clone()
        vcode = torch.zeros(B, HKV, tcap, 128 * bits // 32, dtype=torch.int32).cuda()
        vs, vm = torch.zeros(B, HKV, tcap, 2).half().cuda(), torch.zeros(B, HKV, tcap, 2).half().cuda()
        tail = (L.ptr(q), L.ptr(kw), kslot, L.ptr(ring), n, R, evict, L.ptr(vcode), L.ptr(vs), L.ptr(vm), tcap, 64, bits, L.stream_ptr())
        if freq:
            L.check(lib.gear_kivi_rope_append_freq(L.ptr(qkv), B, HQ, HKV, 128, pos, L.ptr(tab), af, *tail), "freq")
        else:
            L.check(lib.gear_kivi_rope_append(L.ptr(qkv), B, HQ, HKV, 128, pos, THETA, *tail), "theta")
        return q, kw, ring, vcode, vs, vm

    for pos in POSITIONS:
        q, kw, ring, vcode, vs, vm = run(True, pos)
        gq, gk = _np(q)[:, :, 0].astype(np.float32), _np(kw)[:, :, kslot].astype(np.float32)
        _check(gq, xq, pos, inv, af, "q")
        _check(gk, xk, pos, inv, af, "k")
        # V does not rotate: the ring row and the evicted row's codes / scale / minimum are the parent's, bit for bit
        _, _, ring_p, vcode_p, vs_p, vm_p = run(False, pos)
        assert np.array_equal(_np(ring)[:, :, n % (R + 1)].astype(np.float32), xv)
        assert torch.equal(ring, ring_p) and torch.equal(vcode, vcode_p) and torch.equal(vs, vs_p) and torch.equal(vm, vm_p)
        assert int((vcode[:, :, evict] != 0).sum()) > 0 and float(vs[:, :, evict].abs().min()) > 0
        if pos >= 64:
            seen = seen or _sees_the_bug(gk, xk, pos, af)
    assert seen, "the comparison cannot tell scaled from unscaled frequencies"


def test_freq_entries_on_the_unscaled_table_agree_with_theta(lib, qkv):
    """Host pow and device exp2f differ in the last place of inv_freq, so the two flavours are compared through the bound (both
    lie within it of the float64 rotation with the table's angles ... the theta flavour up to its own angle error), not bit for bit."""
    from gear_amd import _lib as L
    inv, af = _plain_table()
    tab = inv.cuda()
    B, slot = 2, 3
    xq, xk, _ = _split(qkv, B)
    for pos in POSITIONS:
        outs = []
        for freq in (True, False):
            q = torch.zeros(B, HQ, 1, 128).half().cuda()
            kw, vw = torch.zeros(B, HKV, R, 128).half().cuda(), torch.zeros(B, HKV, R, 128).half().cuda()
            if freq:
                rc = lib.gear_rope_append_freq(L.ptr(qkv), B, HQ, HKV, 128, pos, L.ptr(tab), 1.0, L.ptr(q), L.ptr(kw), L.ptr(vw), slot, R,
                                               L.stream_ptr())
            else:
                rc = lib.gear_rope_append(L.ptr(qkv), B, HQ, HKV, 128, pos, THETA, L.ptr(q), L.ptr(kw), L.ptr(vw), slot, R,
                                          L.stream_ptr())
            L.check(rc, "rope_append")
            outs.append((_np(q)[:, :, 0].astype(np.float64), _np(kw)[:, :, slot].astype(np.float64)))
        for got, ref, x in ((outs[0][0], outs[1][0], xq), (outs[0][1], outs[1][1], xk)):
            bound = 2.0 ** -9 * (np.abs(x[..., :64]) + np.abs(x[..., 64:])) + 2.0 ** -24
            bound = np.concatenate([bound, bound], -1)
            err = np.abs(got - ref)
            print(f"unscaled table against theta: pos {pos}: worst error / bound = {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), pos


# ------------------------------------------------------------------------------------------------------------- decoders
def _tiny(scaling, method="gearlKIVI", n_kv=2, layers=2):
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    cfg = LlamaConfigLite(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=layers,
                          num_attention_heads=4, num_key_value_heads=n_kv, k_bits=2, v_bits=2, rope_theta=THETA, rope_scaling=scaling)
    cc = dict(compress_method=method, group_size=64, residual=64, quantize_bit=2, rank=4, rankv=4, loop=3, left=0.0)
    torch.manual_seed(0)
    return LlamaForCausalLM_GEARKIVI(cfg, cc).half().cuda().eval()


@pytest.fixture(scope="module")
def scaled_model():
    return _tiny(S)


@pytest.fixture(scope="module")
def ids():
    return torch.randint(0, 1000, (2, 160), generator=torch.Generator().manual_seed(3)).cuda()


def _cos(a, b):
    return float(torch.nn.functional.cosine_similarity(a.float().reshape(-1, a.shape[-1]), b.float().reshape(-1, b.shape[-1])).min())


@pytest.mark.parametrize("kind", ["gear", "kivi"])
def test_decoder_k_rows_use_the_scaled_table(scaled_model, ids, kind):
    """Layer 0's K rows of three step()s behind a 70-token prompt: the pre-RoPE projection recomputed from the embedding (float64
    RMS statistics and dot products, rounded once to fp16 as the GEMV rounds its result), rotated in float64 with the scaled table."""
    from gear_amd.fast_decode import FastGearDecoder
    model = scaled_model
    dec = FastGearDecoder(model, 256, batch=2, cache_kind=kind)
    assert dec.rope is not None
    inv, af = _table(S)
    with torch.no_grad():
        dec.prefill(ids[:, :70])
        for t in range(70, 73):
            dec.step(ids[:, t:t + 1])
        lw = dec.layers[0]
        h = model.model.embed_tokens(ids[:, 70:73]).double()                       # [B, 3, hidden]
        x = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + dec.eps)
        kpre = (x @ lw["wqkv"].double().t())[..., HQ * 128:(HQ + HKV) * 128].half()    # the GEMV's fp16 result
    cache = lw["cache"]
    n_kwin = cache.n_win if kind == "gear" else cache.n_kwin
    assert n_kwin == 9                                                              # tokens 64 .. 72 sit in the window
    rows = _np(cache.kwin[:, :, 6:9]).astype(np.float32)                            # [B, Hkv, 3, 128]: tokens 70, 71, 72
    kpre = _np(kpre).astype(np.float32).reshape(2, 3, HKV, 128)
    seen = False
    for i, pos in enumerate((70, 71, 72)):
        _check(rows[:, :, i], kpre[:, i], pos, inv, af, f"{kind} K row")
        seen = seen or _sees_the_bug(rows[:, :, i], kpre[:, i], pos, af)
    assert seen


@pytest.mark.parametrize("kind", ["gear", "fp16", "kivi"])
def test_step_tracks_the_dense_paths_on_a_scaled_model(scaled_model, ids, kind):
    """step() rotates in the kernel, extend() / prefill() through ScaledRotaryEmbedding: teacher-forced over 80 tokens their logits
    stay at cosine > 0.999 (KIVI has no extend(): every step is compared with the prefill of the prompt that ends in its token)."""
    from gear_amd.fast_decode import FastGearDecoder
    P, n = 70, 80
    a = FastGearDecoder(scaled_model, 256, batch=2, seed=4, cache_kind=kind)
    with torch.no_grad():
        a.prefill(ids[:, :P])
        steps = torch.stack([a.step(ids[:, t:t + 1]) for t in range(P, P + n)], 1)
        if kind == "kivi":
            ref = torch.stack([FastGearDecoder(scaled_model, 256, batch=2, cache_kind=kind).prefill(ids[:, :t + 1])
                               for t in range(P, P + n)], 1)
        else:
            b = FastGearDecoder(scaled_model, 256, batch=2, seed=4, cache_kind=kind)
            b.prefill(ids[:, :P])
            ref = b.extend(ids[:, P:P + n])
    worst = min(_cos(steps[:, i], ref[:, i]) for i in range(n))
    print(f"{kind}: worst cosine of step() against the dense path over {n} tokens: {worst:.6f}")
    assert worst > 0.999, worst


def test_step_graph_equals_eager_steps_on_a_scaled_model(scaled_model, ids):
    from gear_amd.fast_decode import FastGearDecoder
    fe, fg = FastGearDecoder(scaled_model, 256, batch=2, seed=5), FastGearDecoder(scaled_model, 256, batch=2, seed=5)
    with torch.no_grad():
        tok = fe.prefill(ids[:, :70]).argmax(-1, keepdim=True)
        fg.prefill(ids[:, :70])
        tg = tok
        for i in range(5):
            tok = fe.step(tok).argmax(-1, keepdim=True)
            tg = fg.step_graph(tg)
            assert torch.equal(tok, tg), i
    assert fg.graph is not None and fe.pos == fg.pos == 75


def test_hook_generate_agrees_with_the_fast_decoder_on_a_scaled_model(ids):
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.rope import ScaledRotaryEmbedding
    model = _tiny(S, method="KIVI")
    assert all(type(layer.self_attn.rotary_emb) is ScaledRotaryEmbedding for layer in model.model.layers)
    with torch.no_grad():
        hook = model.generate(ids[:, :70], 90)
        fast = FastGearDecoder(model, 256, batch=2).generate(ids[:, :70], 90)
    assert hook.shape == fast.shape == (2, 90) and torch.equal(hook, fast)


def test_default_rope_type_is_the_unscaled_model(ids):
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.modeling_llamagear import LlamaRotaryEmbedding
    outs = []
    for scaling in (None, {"rope_type": "default"}):
        model = _tiny(scaling, method="KIVI")
        assert type(model.model.layers[0].self_attn.rotary_emb) is LlamaRotaryEmbedding
        dec = FastGearDecoder(model, 256, batch=2)
        assert dec.rope is None
        with torch.no_grad():
            logits = dec.prefill(ids[:, :70]).clone()
            toks = FastGearDecoder(model, 256, batch=2).generate(ids[:, :70], 100)
        outs.append((logits, toks))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
