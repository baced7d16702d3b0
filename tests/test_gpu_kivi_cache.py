"""The KIVI cache on the fused decode path: cache.KiviKVCache (csrc/kivi.hip) against the KIVI state-machine oracle
(oracle/kivi_oracle.py, pinned by tests/golden/f8_ref_kivi_*.npz), its attention at one-token resolution against a float64
reference (tests/attn_probe.py), FastGearDecoder(cache_kind="kivi") against LlamaForCausalLM_KIVI's own hook decode, and the
harness's KIVI row through the fast decoder."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_probe as AP
from conftest import ROOT, rel_fro
from test_gpu_verify import _cos, _tiny

pytestmark = pytest.mark.gpu

D = 128
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for tag, (r, e) in sorted(WORST.items()):
        print(f"KIVI {tag}: row_err {r:.3e} (bound {AP.ROW_BOUND:g}) lse_err {e:.3e} (bound {AP.LSE_BOUND:g})")


def host(t):
    return t.detach().cpu().numpy()


def _cache(B, Hkv, cap, bits, R):
    from gear_amd.cache import KiviKVCache
    return KiviKVCache(B, Hkv, cap, bits, 64, R, "cuda")


def _rows(B, H, n, g):
    return torch.randn(B, H, n, D, generator=g).half()


def _state(c):
    return ({n: getattr(c, n).clone() for n in ("kcode", "kscale", "kmn", "vcode", "vscale", "vmn", "kwin", "vring")},
            (c.n_tok, c.n_kpacked, c.n_vpacked, c.ring_start))


def _same(x, y):
    return x[1] == y[1] and all(torch.equal(x[0][n], y[0][n]) for n in x[0])


# ------------------------------------------------------------------------------------------------ 1. trace against the oracle
def _check_packed(c, o):
    """Packed K / V of the cache == the oracle's, bit for bit; the ring in token order == the oracle's fp16 V window."""
    oc = o.c
    fpi, Tk, Nv = c.fpi, c.n_kpacked, c.n_vpacked
    assert (oc["kc"].shape[3] * fpi if oc["kc"] is not None else 0) == Tk
    if Tk:
        assert np.array_equal(host(c.kcode[..., :Tk // fpi]), oc["kc"])
        assert np.array_equal(host(c.kscale[..., :Tk // 64]).view(np.uint16), oc["ks"].view(np.uint16))
        assert np.array_equal(host(c.kmn[..., :Tk // 64]).view(np.uint16), oc["km"].view(np.uint16))
    assert (oc["vc"].shape[2] if oc["vc"] is not None else 0) == Nv + c.v_pending
    if Nv:          # (the oracle has quantized the pending row already; its bits are compared once the next append has written them)
        assert np.array_equal(host(c.vcode[:, :, :Nv]), oc["vc"][:, :, :Nv])
        assert np.array_equal(host(c.vscale[:, :, :Nv]).view(np.uint16), oc["vs"][:, :, :Nv].view(np.uint16))
        assert np.array_equal(host(c.vmn[:, :, :Nv]).view(np.uint16), oc["vm"][:, :, :Nv].view(np.uint16))
    ring = host(c.ring_tokens())
    assert np.array_equal(ring[:, :, c.v_pending:].view(np.uint16), np.ascontiguousarray(oc["vfull"]).view(np.uint16))
    if oc["kfull"] is not None:
        assert np.array_equal(host(c.kwin[:, :, :c.n_kwin]).view(np.uint16), np.ascontiguousarray(oc["kfull"]).view(np.uint16))
    else:
        assert c.n_kwin == 0


TRACE = [(2, 2, 2, 1, 40, 64, 140), (4, 4, 2, 2, 130, 64, 140), (2, 2, 2, 1, 200, 64, 140), (2, 4, 2, 1, 64, 64, 140),
         (2, 2, 2, 1, 100, 128, 170)]


@pytest.mark.parametrize("bits,Hq,Hkv,B,Tp,R,steps", TRACE, ids=[f"b{c[0]}-Hq{c[1]}-Hkv{c[2]}-B{c[3]}-Tp{c[4]}-R{c[5]}" for c in TRACE])
def test_kivi_cache_trace_vs_oracle(bits, Hq, Hkv, B, Tp, R, steps):
    """prefill + (append, attend, maybe_compress) x steps with the k / v / q the oracle gets: counters as the hook's tuple, packed
    codes / scales / minima and both fp16 windows equal to the oracle's bit for bit (at every state change of the trace's first
    2 R + 4 steps, then every 16th step and at the end), attention outputs within the hook's bound of the oracle's
    (test_kivi_decode_trace_vs_oracle: worst per-step rel_fro < 5e-3)."""
    from oracle.kivi_oracle import KiviAttentionOracle
    g = torch.Generator().manual_seed(100 * Tp + bits + R)
    k, v, q = _rows(B, Hkv, Tp + steps, g), _rows(B, Hkv, Tp + steps, g), _rows(B, Hq, steps, g)
    kd, vd, qd = k.cuda(), v.cuda(), q.cuda()
    c = _cache(B, Hkv, Tp + steps, bits, R)
    o = KiviAttentionOracle(Hq, Hkv, D, 64, bits, R)
    c.prefill(kd[:, :, :Tp], vd[:, :, :Tp])
    o.prefill(host(q[:, :, :1]), host(k[:, :, :Tp]), host(v[:, :, :Tp]))
    assert c.seq_len == Tp and c.hook_counters() == (Tp - Tp % R, Tp % R, max(0, Tp - R), min(Tp, R))
    _check_packed(c, o)
    worst = 0.0
    for i in range(steps):
        t = Tp + i
        c.append(kd[:, :, t:t + 1], vd[:, :, t:t + 1])
        out = c.attend(qd[:, :, i:i + 1])
        c.maybe_compress()
        ref = o.decode(host(q[:, :, i:i + 1]), host(k[:, :, t:t + 1]), host(v[:, :, t:t + 1]))
        worst = max(worst, rel_fro(host(out), ref))
        L = t + 1
        assert c.seq_len == L and c.hook_counters() == (L - L % R, L % R, max(0, L - R), min(L, R)), (i, c.hook_counters())
        assert c.n_vpacked == max(0, L - (R + 1), min(Tp, L) - R) and c.ring_start == c.n_vpacked % (R + 1)
        if i < 2 * R + 4 or i % 16 == 0 or i == steps - 1:
            _check_packed(c, o)
    print(f"KIVI trace b{bits} Hq{Hq} Hkv{Hkv} B{B} Tp{Tp} R{R}: worst rel_fro {worst:.3e} (bound 5e-3)")
    assert worst < 5e-3, worst


def test_kivi_append_rope_equals_rope_append_then_append():
    """gear_kivi_rope_append == gear_rope_append's rotation followed by gear_kivi_append: same q, same cache bits (over an
    eviction and a K flush)."""
    from gear_amd import _lib as L
    B, Hq, Hkv, R = 2, 4, 2, 64
    g = torch.Generator().manual_seed(3)
    k, v = _rows(B, Hkv, 60, g).cuda(), _rows(B, Hkv, 60, g).cuda()
    a, b = _cache(B, Hkv, 200, 2, R), _cache(B, Hkv, 200, 2, R)
    a.prefill(k, v)
    b.prefill(k, v)
    kw, vw = torch.zeros(B, Hkv, 1, D, dtype=torch.float16, device="cuda"), torch.zeros(B, Hkv, 1, D, dtype=torch.float16, device="cuda")
    for i in range(12):
        qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).half().cuda()
        qa = a.append_rope(qkv, Hq, 60 + i, 10000.0)
        qb = torch.empty_like(qa)
        L.check(L.load().gear_rope_append(L.ptr(qkv), B, Hq, Hkv, D, 60 + i, 10000.0, L.ptr(qb), L.ptr(kw), L.ptr(vw), 0, 1,
                                          L.stream_ptr(qkv)), "gear_rope_append")
        b.append(kw, vw)
        assert torch.equal(qa, qb)
        a.maybe_compress()
        b.maybe_compress()
        assert _same(_state(a), _state(b)), i
    assert a.n_kpacked == 64 and a.n_vpacked == 72 - 65


# ------------------------------------------------------------------------------------------------ 2. probes at one-token resolution
def _reference_keys(c):
    """float64 K-hat, V-hat [B, Hkv, L, 128] of the cache: dequantized codes where a token is packed, the fp16 rows elsewhere."""
    g, b, fpi, Tk, Nv = c.group, c.bits, c.fpi, c.n_kpacked, c.n_vpacked
    Kd = (AP._unpack(host(c.kcode[..., :Tk // fpi]), b, 3) * np.repeat(host(c.kscale[..., :Tk // g]).astype(np.float64), g, 3)
          + np.repeat(host(c.kmn[..., :Tk // g]).astype(np.float64), g, 3)).transpose(0, 1, 3, 2)
    Vd = (AP._unpack(host(c.vcode[:, :, :Nv]), b, 3) * np.repeat(host(c.vscale[:, :, :Nv]).astype(np.float64), g, 3)
          + np.repeat(host(c.vmn[:, :, :Nv]).astype(np.float64), g, 3))
    K = np.concatenate([Kd, host(c.kwin[:, :, :c.n_kwin]).astype(np.float64)], 2)
    V = np.concatenate([Vd, host(c.ring_tokens()).astype(np.float64)], 2)
    assert K.shape[2] == V.shape[2] == c.seq_len
    return K, V


def _filled(bits, R, B, Hkv, Tp, more, seed):
    g = torch.Generator().manual_seed(seed)
    k, v = _rows(B, Hkv, Tp + more, g).cuda(), _rows(B, Hkv, Tp + more, g).cuda()
    c = _cache(B, Hkv, Tp + more + 8, bits, R)
    c.prefill(k[:, :, :Tp], v[:, :, :Tp])
    for t in range(Tp, Tp + more):
        c.maybe_compress()
        c.append(k[:, :, t:t + 1], v[:, :, t:t + 1])
    return c


def _sites(c):
    return sorted({p for p in (0, c.n_vpacked - 1, c.n_vpacked, c.n_kpacked - 1, c.n_kpacked, c.seq_len - 1,
                               (c.n_vpacked & ~63) - 1, c.n_vpacked & ~63) if 0 <= p < c.seq_len})


def _probe_queries(K, Hq, sites, rng):
    """q [B, Hq, n, 128]: one row per site (every query head aimed at that token of its KV head), one per neighbouring pair of
    sites, two Gaussian rows; and the sites that every head could aim at."""
    B, Hkv = K.shape[:2]
    G = Hq // Hkv
    rows, aimed = [], []
    for targets in [[p] for p in sites] + [[p, p + 1] for p in sites if p + 1 in sites]:
        q = np.zeros((B, Hq, 1, D))
        ok = True
        for b in range(B):
            for hq in range(Hq):
                a = AP.aim(K[b, hq // G], targets)
                ok = ok and a is not None
                q[b, hq, 0] = a if a is not None else AP.f16(rng.standard_normal(D))
        rows.append(q)
        if ok and len(targets) == 1:
            aimed.append(targets[0])
    for _ in range(2):
        rows.append(AP.f16(rng.standard_normal((B, Hq, 1, D))))
    return rows, aimed


def _run(c, rows):
    outs, lses = [], []
    for q in rows:
        o, l = c.attend(torch.tensor(q, dtype=torch.float16, device="cuda"), return_lse=True)
        outs.append(host(o).astype(np.float64))
        lses.append(host(l).astype(np.float64)[:, :, None])
    return np.concatenate(outs, 2), np.concatenate(lses, 2)


# (bits, R, B, Hq, Hkv, prompt, appended): L = 270: Tk 256, Nv 205, seam [192, 270) behind three partial chunks | 4-bit, R 128:
# L = 400: Tk 384, Nv 271, seam [256, 400) with a packed K group in it | L = 100: no partial launch at all (Nv = 35)
PROBE = [(2, 64, 2, 4, 2, 150, 120), (4, 128, 1, 4, 1, 300, 100), (2, 64, 1, 2, 2, 30, 70)]


@pytest.fixture(scope="module", params=PROBE, ids=[f"b{c[0]}-R{c[1]}-L{c[5] + c[6]}" for c in PROBE])
def probed(request):
    bits, R, B, Hq, Hkv, Tp, more = request.param
    c = _filled(bits, R, B, Hkv, Tp, more, seed=Tp + more)
    K, V = _reference_keys(c)
    parts = AP.window_parts(K, V)
    sites = _sites(c)
    rows, aimed = _probe_queries(K, Hq, sites, np.random.default_rng(Tp))
    q = np.concatenate(rows, 2)
    return c, parts, (K, V), rows, q, AP.ref(q, parts, kv=(K, V)), sites, aimed


def test_kivi_attend_probes(probed):
    """Rows and LSE of attend() against float64 attention over the dequantized cache, with queries aimed at the tokens on both
    sides of every seam (Nv, Tk, the first seam token, token 0, the newest token): test_gpu_shared's bounds, rows 1e-2, LSE 4e-2."""
    c, parts, kv, rows, q, (ro, rl), sites, aimed = probed
    out, lse = _run(c, rows)
    assert np.isfinite(out).all() and np.isfinite(lse).all()
    r, e = AP.row_err(out, ro), AP.lse_err(lse, rl)
    tag = f"attend b{c.bits} R{c.R} L{c.seq_len} (Tk {c.n_kpacked}, Nv {c.n_vpacked})"
    WORST[tag] = (r, e)
    print(f"KIVI probe {tag}: row_err {r:.3e} lse_err {e:.3e}")
    assert r <= AP.ROW_BOUND and e <= AP.LSE_BOUND, (tag, r, e)


def test_kivi_attend_probes_catch_one_token_faults(probed):
    """A kernel that drops one token, or reads a zero V row for it, at Nv - 1, Nv, Tk - 1, Tk, L - 1 or token 0 would move the
    probe metric to at least 5 x a bound: the mutated float64 references lie that far from what the kernel computes."""
    c, parts, (K, V), rows, q, (ro, rl), sites, aimed = probed
    out, lse = _run(c, rows)
    assert AP.signal(out, lse, ro, rl) <= 1.0
    want = {p for p in (0, c.n_vpacked - 1, c.n_vpacked, c.n_kpacked - 1, c.n_kpacked, c.seq_len - 1) if 0 <= p < c.seq_len}
    assert want <= set(aimed), (sorted(want), aimed)
    for p in sorted(want):
        mo, ml = AP.ref(q, AP.mutate(parts, "M1-drop", p), kv=(K, V))
        assert AP.signal(out, lse, mo, ml) >= 5.0, ("drop", p, AP.signal(out, lse, mo, ml))
        Vz = V.copy()
        Vz[:, :, p] = 0.0
        mo, ml = AP.ref(q, parts, kv=(K, Vz))
        assert AP.signal(out, lse, mo, ml) >= 5.0, ("zero V", p, AP.signal(out, lse, mo, ml))
        Kz = K.copy()
        Kz[:, :, p] = 0.0
        mo, ml = AP.ref(q, parts, kv=(Kz, V))
        assert AP.signal(out, lse, mo, ml) >= 5.0, ("zero K", p, AP.signal(out, lse, mo, ml))


# ------------------------------------------------------------------------------------------------ 3. no state change, equal bits
@pytest.mark.parametrize("flushed", [False, True])
def test_kivi_attend_changes_no_state_and_repeats(flushed):
    """attend() twice: equal bits (no sum in the call depends on the order in which waves run), no buffer and no counter moved.
    flushed: right after a K flush -- an empty K window and R + 1 ring rows, the widest seam (64 + 128 tokens at R = 128)."""
    R = 128
    c = _filled(4, R, 2, 2, 200, 184 if flushed else 150, seed=8)
    if flushed:
        c.maybe_compress()
        assert (c.seq_len, c.n_kwin, c.n_vwin) == (384, 0, R + 1) and c.seq_len - (c.n_vpacked & ~63) == 192
    before = _state(c)
    q = torch.randn(2, 4, 1, D, generator=torch.Generator().manual_seed(2)).half().cuda()
    a, la = c.attend(q, return_lse=True)
    b, lb = c.attend(q, return_lse=True)
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert torch.equal(c.attend(q), a)
    assert _same(before, _state(c))
    K, V = _reference_keys(c)
    ro, rl = AP.ref(host(q).astype(np.float64), AP.window_parts(K, V), kv=(K, V))
    assert AP.row_err(host(a).astype(np.float64), ro) <= AP.ROW_BOUND and AP.lse_err(host(la)[:, :, None], rl) <= AP.LSE_BOUND


def test_kivi_cache_refuses_what_is_not_built():
    from gear_amd import _lib as L
    from gear_amd.cache import KiviKVCache
    for kw in (dict(bits=3), dict(group=32), dict(residual=96), dict(head_dim=64)):
        args = dict(bits=2, group=64, residual=64, head_dim=128)
        args.update(kw)
        with pytest.raises(L.GearError):
            KiviKVCache(1, 2, 256, args["bits"], args["group"], args["residual"], "cuda", args["head_dim"])
    c = _cache(1, 1, 64, 2, 64)
    g = torch.Generator().manual_seed(1)
    k, v = _rows(1, 1, 130, g).cuda(), _rows(1, 1, 130, g).cuda()
    c.prefill(k[:, :, :60], v[:, :, :60])
    for t in range(60, 64):
        c.append(k[:, :, t:t + 1], v[:, :, t:t + 1])
    with pytest.raises(L.GearError, match="maybe_compress"):
        c.append(k[:, :, 64:65], v[:, :, 64:65])                      # the K window is full
    c.maybe_compress()
    for t in range(64, 127):
        c.append(k[:, :, t:t + 1], v[:, :, t:t + 1])
    st = _state(c)
    with pytest.raises(L.GearError, match="capacity"):
        c.append(k[:, :, 127:128], v[:, :, 127:128])                  # a second block would not fit 64 packed tokens
    assert _same(st, _state(c))


# ------------------------------------------------------------------------------------------------ 4. decoder
def _hook_of(model):
    from gear_amd.modeling_llama_kivi import LlamaForCausalLM_KIVI
    cc = dict(model.model.layers[0].self_attn.compress_config)
    hook = LlamaForCausalLM_KIVI(model.config, cc).half().cuda().eval()
    hook.load_state_dict(model.state_dict())
    return hook


@pytest.mark.parametrize("n_kv,batch", [(2, 2), (4, 2), (2, 6)], ids=["gqa-b2", "mha-b2", "gqa-b6-library-gemm"])
def test_kivi_decoder_matches_the_hook_teacher_forced(n_kv, batch):
    """FastGearDecoder(cache_kind="kivi") against LlamaForCausalLM_KIVI's own hook decode on the same weights and tokens: prompt
    90, 150 tokens (both windows fill, two K flushes, the ring wraps).  Logits cosine > 0.999 at every step
    (test_decoder_shared_matches_plain_teacher_forced's figure), finite everywhere; the final counters are the hook's tuple's."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("KIVI", n_kv)
    hook = _hook_of(model)
    P, n = 90, 150
    ids = torch.randint(0, 1000, (batch, P + n), generator=torch.Generator().manual_seed(11)).cuda()
    dec = FastGearDecoder(model, P + n + 8, batch=batch, cache_kind="kivi")
    with torch.no_grad():
        lh, past = hook(ids[:, :P], None, True)
    lf = dec.prefill(ids[:, :P])
    worst = _cos(lf, lh[:, -1])
    assert torch.isfinite(lf).all()
    for i in range(n):
        with torch.no_grad():
            lh, past = hook(ids[:, P + i:P + i + 1], past, True)
        lf = dec.step(ids[:, P + i])
        assert torch.isfinite(lf).all(), i
        worst = min(worst, _cos(lf, lh[:, -1]))
    print(f"KIVI decoder n_kv {n_kv} batch {batch}: worst logits cosine {worst:.6f}")
    assert worst > 0.999, worst
    T = P + n
    assert dec.pos == T
    for lw, tup in zip(dec.layers, past):
        c = lw["cache"]
        assert c.seq_len == T == tup[8]
        assert c.hook_counters() == (T - T % 64, T % 64, T - 64, 64)
        assert tup[0].shape[-1] * c.fpi == T - T % 64 and tup[1].shape[2] == T % 64
        assert tup[4].shape[2] == T - 64 and tup[5].shape[2] == 64


def test_kivi_decoder_generate_repeats_and_refuses():
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.sampling import SamplingParams
    model = _tiny("KIVI", 2)
    ids = torch.randint(0, 1000, (2, 70), generator=torch.Generator().manual_seed(5)).cuda()
    sp = SamplingParams(0.8, 50, 0.95, 7)
    a = FastGearDecoder(model, 160, batch=2, cache_kind="kivi").generate(ids, 150, sampling=sp)
    b = FastGearDecoder(model, 160, batch=2, cache_kind="kivi").generate(ids, 150, sampling=sp)
    assert a.shape == (2, 150) and torch.equal(a, b) and torch.equal(a[:, :70], ids)
    g1 = FastGearDecoder(model, 160, batch=2, cache_kind="kivi").generate(ids, 150)
    g2 = FastGearDecoder(model, 160, batch=2, cache_kind="kivi").generate(ids, 150)
    assert g1.shape == (2, 150) and torch.equal(g1, g2)
    with pytest.raises(ValueError, match="'gear', 'fp16' or 'kivi'"):
        FastGearDecoder(model, 160, cache_kind="int8")
    for kw in (dict(shared_prefix_tokens=64), dict(tp_world=2)):
        with pytest.raises(NotImplementedError, match="cache_kind='kivi'"):
            FastGearDecoder(model, 160, batch=2, cache_kind="kivi", **kw)
    dec = FastGearDecoder(model, 200, batch=2, cache_kind="kivi")
    dec.prefill(ids)
    tok = ids[:, :1]
    ref = dec.step(tok).clone()
    par = torch.tensor([-1, 0, 0])
    refused = [lambda: dec.step_graph(), lambda: dec.step_graph_sampled(sp), lambda: dec.extend(ids[:, :4]),
               lambda: dec.verify(ids[:, :3]), lambda: dec.verify_tree(ids[:, :3], par), lambda: dec.accept(1),
               lambda: dec.accept_path(torch.tensor([0])), lambda: dec.generate_speculative(ids, 100),
               lambda: dec.reorder([1, 0]), lambda: dec.snapshot(), lambda: dec.restore(None), lambda: dec.load_prefix(None),
               lambda: dec.generate(ids, 100, graph=True), lambda: dec.generate(ids[:1], 100, shared_prefix=True)]
    state = [_state(lw["cache"]) for lw in dec.layers]
    for i, fn in enumerate(refused):
        with pytest.raises(NotImplementedError, match="cache_kind='kivi'"):
            fn()
        assert dec.pos == 71 and all(_same(s, _state(lw["cache"])) for s, lw in zip(state, dec.layers)), i
    nxt = dec.step(tok)                                               # the decoder still steps afterwards
    assert torch.isfinite(nxt).all() and dec.pos == 72 and nxt.shape == ref.shape


# ------------------------------------------------------------------------------------------------ 5. harness
def _harness(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "harness.py"), "--layers", "2", "--prompt_len", "200", "--max_length", "330",
           "--batch_size", "2", "--json", *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stdout


def test_harness_kivi_through_the_fast_decoder():
    res, _ = _harness("--model", "KIVI", "--fast")
    assert len(res) == 1 and res[0]["variant"] == "KIVI" and res[0]["fast"] is True
    assert res[0]["max_length"] == 330 and res[0]["new_tokens_per_s"] > 0 and res[0]["cache_bytes"] > 0


def test_harness_all_fast_prints_three_fast_rows():
    res, text = _harness("--all", "--fast")
    assert [r["variant"] for r in res] == ["gearl", "KIVI", "None"]
    assert all(r["fast"] is True and r["new_tokens_per_s"] > 0 and r["max_length"] == 330 for r in res)
    assert text.count("(fast path)") == 3
