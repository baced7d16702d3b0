"""Shared-prefix decode timing (GPU box), one JSON line:
  layer: the Llama-2-7B attention shape (32 query / 32 KV heads), gearslKIVI 2-bit, rank 8, 2 % outliers, a 4096-token prompt and
         64 compressed + 32 window tokens per sequence.  For S in {1, 2, 4, 8, 16}: GearKVCache.attend_shared over (one prefix
         cache, S tails) beside attend() on an unshared batch-S cache of the same total length and beside S x attend() at batch 1;
         the shared call also with attn_mfma = 1 / -1 (the option acts on the prefix AND the tail dispatch: "off" against the
         default shows where the prefix's matrix-core grouping starts to win, "on" also moves the one-row tails to that kernel).
         diff_vs_unshared_cache: the two caches compress the prompt with different random start bases, so this is the distance
         between two valid compressions, not a kernel error (tests/test_gpu_shared.py holds the kernel to float64).
         Warm = median of 7 back-to-back calls; cold = median of 5 calls each behind a 512 MiB write.  Event times.
  decoder: random-weight 7B-shaped FastGearDecoder, 4096-token prompt, 256 generated tokens, S = 16 greedy: prefill ms, decode
         tokens/s (all sequences) and allocated cache bytes, shared against unshared batch 16; whether the greedy rows are equal.
usage: python tools/shared_timing.py [--quick]   (--quick: the layer part only)"""
import gc
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

dev = torch.device("cuda")
CC = dict(compress_method="gearslKIVI", group_size=64, residual=64, quantize_bit=2, rank=8, rankv=8, loop=3, left=0.02)


def timed(fn, flush=None):
    if flush is not None:
        flush.fill_(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3          # us


def measure(fn, flush):
    for _ in range(3):
        fn()
    return dict(warm=round(statistics.median(timed(fn) for _ in range(7)), 1),
                cold=round(statistics.median(timed(fn, flush) for _ in range(5)), 1))


def layer_part():
    from gear_amd import _lib as L
    from gear_amd.cache import GearKVCache
    H, Tp, T, W = 32, 4096, 64, 32
    torch.manual_seed(0)
    flush = torch.empty((512 << 20) // 4, dtype=torch.float32, device=dev)
    kp, vp = (torch.randn(1, H, Tp, 128, device=dev).half() for _ in range(2))
    pre = GearKVCache(1, H, Tp, CC, dev)
    pre.prefill(kp, vp)
    one = GearKVCache(1, H, Tp + T + 128, CC, dev)          # the batch-1 cache of the S x attend() column
    one.prefill(kp, vp)
    one.extend(*(torch.randn(1, H, T + W, 128, device=dev).half() for _ in range(2)))
    q1 = torch.randn(1, H, 1, 128, device=dev).half()
    res = {"shape": dict(Hq=H, Hkv=H, Tp=Tp, T=T, W=W, method="gearslKIVI 2-bit g64 rank 8, 2 % outliers")}
    res["attend_b1_us"] = measure(lambda: one.attend(q1), flush)
    res["by_S"] = {}
    for S in (1, 2, 4, 8, 16):
        kt, vt = (torch.randn(S, H, T + W, 128, device=dev).half() for _ in range(2))
        tail = GearKVCache(S, H, T + 128, CC, dev)
        tail.extend(kt, vt)
        un = GearKVCache(S, H, Tp + T + 128, CC, dev)
        un.prefill(kp.expand(S, -1, -1, -1).contiguous(), vp.expand(S, -1, -1, -1).contiguous())
        un.extend(kt, vt)
        assert (tail.n_comp, tail.n_win, un.n_comp, un.n_win) == (T, W, Tp + T, W)
        q = torch.randn(S, H, 1, 128, device=dev).half()
        r = dict(shared=measure(lambda: tail.attend_shared(q, pre), flush), unshared=measure(lambda: un.attend(q), flush))

        def s_times():
            for _ in range(S):
                one.attend(q1)
        r["S_x_batch1"] = measure(s_times, flush)
        for name, val in (("shared_mfma_on", 1), ("shared_mfma_off", -1)):
            L.set_option("attn_mfma", val)
            try:
                r[name] = measure(lambda: tail.attend_shared(q, pre), flush)
            finally:
                L.set_option("attn_mfma", 0)
        r["shared_vs_unshared"] = dict(warm=round(r["shared"]["warm"] / r["unshared"]["warm"], 3),
                                       cold=round(r["shared"]["cold"] / r["unshared"]["cold"], 3))
        a, b = tail.attend_shared(q, pre).float(), un.attend(q).float()
        r["diff_vs_unshared_cache"] = round(float((a - b).abs().max()), 5)
        res["by_S"][S] = r
        del tail, un
        gc.collect()
        torch.cuda.empty_cache()
    r16 = res["by_S"][16]["shared_vs_unshared"]
    res["target_S16_ratio_le_1"] = dict(warm="met" if r16["warm"] <= 1.0 else "missed", cold="met" if r16["cold"] <= 1.0 else "missed")
    del flush
    return res


def decoder_part():
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    P, N, S = 4096, 256, 16
    mcfg = LlamaConfigLite(num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=32, hidden_size=4096,
                           intermediate_size=11008, max_position_embeddings=8192, k_bits=2, v_bits=2, group_size=64,
                           residual_length=64)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        torch.manual_seed(0)
        with torch.device(dev):
            model = LlamaForCausalLM_GEARKIVI(mcfg, CC).eval()
    finally:
        torch.set_default_dtype(old)
    ids = torch.randint(0, mcfg.vocab_size, (1, P), device=dev)
    L = P + N
    nbytes = lambda pool: sum(t.numel() * t.element_size() for t in pool.buf.values())
    res = dict(prompt=P, generated=N, S=S)
    for name in ("shared", "unshared"):
        if name == "shared":
            make = lambda: FastGearDecoder(model, N + 64, batch=S, shared_prefix_tokens=P)
            size = lambda d: nbytes(d.pool) + nbytes(d.prefix_pool)
            prompt = ids
            pre = lambda d: d.prefill_shared(prompt)
        else:
            make = lambda: FastGearDecoder(model, L + 64, batch=S)
            size = lambda d: nbytes(d.pool)
            prompt = ids.expand(S, -1).contiguous()
            pre = lambda d: d.prefill(prompt)
        dec = make()
        pre(dec)                                          # warm-up of the prefill's GEMM / SDPA shapes on a decoder of its own
        del dec
        gc.collect()
        torch.cuda.empty_cache()
        dec = make()
        cache_bytes = size(dec)
        box = {}
        t_pre = timed(lambda: box.__setitem__("lg", pre(dec))) / 1e3
        nxt = box["lg"].argmax(-1, keepdim=True)
        out = [nxt]
        nxt = dec.step(nxt).argmax(-1, keepdim=True)      # one step outside the timed stretch warms up the library handles
        out.append(nxt)

        def loop():
            t = out[-1]
            for _ in range(N - 2):
                t = dec.step(t).argmax(-1, keepdim=True)
                out.append(t)
        t_dec = timed(loop) / 1e3
        dec.check_block_kernel()
        toks = torch.cat(out, 1)
        res[name] = dict(prefill_ms=round(t_pre, 1), decode_ms=round(t_dec, 1), tokens_per_s=round(S * (N - 2) / (t_dec / 1e3), 1),
                         cache_bytes=cache_bytes, cache_GiB=round(cache_bytes / 2 ** 30, 2),
                         greedy_rows_equal=bool(all(torch.equal(toks[r], toks[0]) for r in range(1, S))))
        del dec
        gc.collect()
        torch.cuda.empty_cache()
    res["speedup_tokens_per_s"] = round(res["shared"]["tokens_per_s"] / res["unshared"]["tokens_per_s"], 2)
    res["prefill_ratio"] = round(res["unshared"]["prefill_ms"] / res["shared"]["prefill_ms"], 2)
    res["cache_ratio"] = round(res["unshared"]["cache_bytes"] / res["shared"]["cache_bytes"], 2)
    return res


if __name__ == "__main__":
    from gear_amd import _lib
    _lib.load()
    out = {"tool": "shared_timing", "gpu": torch.cuda.get_device_name(0), "layer": layer_part()}
    if "--quick" not in sys.argv:
        out["decoder"] = decoder_part()
    print(json.dumps(out))
