"""KIVI-cache timing (GPU box), one JSON line:
  layer: the Llama-2-7B attention shape (32 query / 32 KV heads), 2-bit, group 64, R = 64, L = 4096 + 37 tokens, batch 1, 4 and 16.
         Three calls in the same run: KiviKVCache.attend (packed K to 4096 + a 37-row K window, 4068 packed V rows + 65 ring rows),
         GearKVCache.attend with compress_method="KIVI" (the same packed bytes: 4096 compressed + 37 window tokens) and
         Fp16KVCache.attend.  ratio_vs_gear_cache = the KIVI call over the GEAR-cache call: measured against existing code.
         Warm = median of 7 back-to-back calls; cold = median of 5 calls each behind a 512 MiB write.  Event times.
  decoder: random-weight 7B-shaped model, 4096-token prompt, 256 generated tokens, batch 1, greedy eager steps: tokens/s and
         allocated cache bytes of FastGearDecoder with cache_kind "gear" (on the KIVI model: the KIVI quantizer under GEAR's window
         discipline), "kivi" and "fp16", and tokens/s of LlamaForCausalLM_KIVI's own hook decode.
usage: python tools/kivi_timing.py [--quick]   (--quick: the layer part only)"""
import gc
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

dev = torch.device("cuda")
CC = dict(compress_method="KIVI", group_size=64, residual=64, quantize_bit=2, rank=0, rankv=0, loop=3, left=0.0)


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
    from gear_amd.cache import Fp16KVCache, GearKVCache, KiviKVCache
    H, Tp, more, R = 32, 4096, 37, 64
    L = Tp + more
    torch.manual_seed(0)
    flush = torch.empty((512 << 20) // 4, dtype=torch.float32, device=dev)
    res = {"shape": dict(Hq=H, Hkv=H, L=L, bits=2, group=64, R=R), "by_batch": {}}
    for B in (1, 4, 16):
        k, v = (torch.randn(B, H, L, 128, device=dev).half() for _ in range(2))
        kivi = KiviKVCache(B, H, L + 64, 2, 64, R, dev)
        kivi.prefill(k[:, :, :Tp], v[:, :, :Tp])
        for t in range(Tp, L):
            kivi.maybe_compress()
            kivi.append(k[:, :, t:t + 1], v[:, :, t:t + 1])
        gear = GearKVCache(B, H, L + 64, CC, dev)
        gear.prefill(k[:, :, :Tp], v[:, :, :Tp])
        gear.extend(k[:, :, Tp:], v[:, :, Tp:])
        f16 = Fp16KVCache(B, H, L + 64, dev)
        f16.prefill(k, v)
        assert (kivi.seq_len, kivi.n_kpacked, kivi.n_vpacked) == (L, Tp, L - R - 1) and (gear.n_comp, gear.n_win) == (Tp, more)
        q = torch.randn(B, H, 1, 128, device=dev).half()
        r = dict(kivi=measure(lambda: kivi.attend(q), flush), gear_cache_kivi_method=measure(lambda: gear.attend(q), flush),
                 fp16=measure(lambda: f16.attend(q), flush))
        r["ratio_vs_gear_cache"] = dict(warm=round(r["kivi"]["warm"] / r["gear_cache_kivi_method"]["warm"], 3),
                                        cold=round(r["kivi"]["cold"] / r["gear_cache_kivi_method"]["cold"], 3))
        # the two caches hold the same K codes; their V differs in the 27 rows that KIVI keeps in fp16 and GEAR's discipline packed
        r["diff_vs_gear_cache"] = round(float((kivi.attend(q).float() - gear.attend(q).float()).abs().max()), 5)
        res["by_batch"][B] = r
        del kivi, gear, f16, k, v
        gc.collect()
        torch.cuda.empty_cache()
    del flush
    return res


def decoder_part():
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.modeling_llama_kivi import LlamaForCausalLM_KIVI
    from gear_amd.modeling_llamagear import LlamaConfigLite
    P, N = 4096, 256
    mcfg = LlamaConfigLite(num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=32, hidden_size=4096,
                           intermediate_size=11008, max_position_embeddings=8192, k_bits=2, v_bits=2, group_size=64,
                           residual_length=64)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        torch.manual_seed(0)
        with torch.device(dev):
            model = LlamaForCausalLM_KIVI(mcfg, CC).eval()
    finally:
        torch.set_default_dtype(old)
    ids = torch.randint(0, mcfg.vocab_size, (1, P), device=dev)
    res = dict(prompt=P, generated=N, batch=1)

    def cache_bytes(dec):
        if dec.pool is not None:
            return sum(t.numel() * t.element_size() for t in dec.pool.buf.values())
        return sum(t.numel() * t.element_size() for lw in dec.layers for t in vars(lw["cache"]).values()
                   if isinstance(t, torch.Tensor) and t.dim() == 4)

    for kind in ("gear", "kivi", "fp16"):
        dec = FastGearDecoder(model, P + N + 64, batch=1, cache_kind=kind)
        nbytes = cache_bytes(dec)
        nxt = dec.prefill(ids).argmax(-1, keepdim=True)
        nxt = dec.step(nxt).argmax(-1, keepdim=True)      # one step outside the timed stretch warms up the library handles
        box = [nxt]

        def loop():
            t = box[0]
            for _ in range(N - 2):
                t = dec.step(t).argmax(-1, keepdim=True)
        t_dec = timed(loop) / 1e3
        res[kind] = dict(decode_ms=round(t_dec, 1), tokens_per_s=round((N - 2) / (t_dec / 1e3), 1), cache_bytes=nbytes,
                         cache_MiB=round(nbytes / 2 ** 20, 1))
        del dec
        gc.collect()
        torch.cuda.empty_cache()
    with torch.no_grad():
        logits, past = model(ids, None, True)
        nxt = logits[:, -1].argmax(-1, keepdim=True)
        logits, past = model(nxt, past, True)
        box = [logits[:, -1].argmax(-1, keepdim=True), past]

        def hook_loop():
            t, p = box
            for _ in range(N - 2):
                lg, p = model(t, p, True)
                t = lg[:, -1].argmax(-1, keepdim=True)
        t_hook = timed(hook_loop) / 1e3
    res["kivi_hook"] = dict(decode_ms=round(t_hook, 1), tokens_per_s=round((N - 2) / (t_hook / 1e3), 1))
    res["kivi_fast_vs_hook"] = round(res["kivi"]["tokens_per_s"] / res["kivi_hook"]["tokens_per_s"], 2)
    return res


if __name__ == "__main__":
    from gear_amd import _lib
    _lib.load()
    out = {"tool": "kivi_timing", "gpu": torch.cuda.get_device_name(0), "layer": layer_part()}
    if "--quick" not in sys.argv:
        out["decoder"] = decoder_part()
    print(json.dumps(out))
