"""Shared-prefix chunk extend timing (GPU box), one JSON line:
  layer: the Llama-2-7B attention shape (32 query / 32 KV heads), gearslKIVI 2-bit, rank 8, 2 % outliers, a 4096-token prompt and
         64 compressed + 32 window tokens per sequence.  For S in {1, 4, 16} and n in {16, 64, 256}:
         GearKVCache.attend_extend_shared over (one prefix cache, S tails) beside attend_extend on an unshared batch-S cache of the
         same total length and beside n x attend_shared (what n decode steps spend in attention; the window does not grow here).
         Warm = median of 7 back-to-back calls; cold = median of 5 calls each behind a 512 MiB write.  Event times.
  decoder: random-weight 7B-shaped FastGearDecoder, 4096-token prompt, S = 16, n = 64: prefill_shared + extend_shared against the
         unshared batch-16 prefill of 4096 + 64 tokens and against 64 shared step() calls; synchronised event times.
usage: python tools/extend_shared_timing.py [--quick]   (--quick: the layer part only)"""
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.shared_timing import CC, measure, timed

dev = torch.device("cuda")


def layer_part():
    from gear_amd.cache import GearKVCache
    H, Tp, T, W = 32, 4096, 64, 32
    torch.manual_seed(0)
    flush = torch.empty((512 << 20) // 4, dtype=torch.float32, device=dev)
    kp, vp = (torch.randn(1, H, Tp, 128, device=dev).half() for _ in range(2))
    pre = GearKVCache(1, H, Tp, CC, dev)
    pre.prefill(kp, vp)
    res = {"shape": dict(Hq=H, Hkv=H, Tp=Tp, T=T, W=W, method="gearslKIVI 2-bit g64 rank 8, 2 % outliers"), "by_S_n": {}}
    for S in (1, 4, 16):
        kt, vt = (torch.randn(S, H, T + W, 128, device=dev).half() for _ in range(2))
        tail = GearKVCache(S, H, T + 128, CC, dev)
        tail.extend(kt, vt)
        un = GearKVCache(S, H, Tp + T + 128, CC, dev)
        un.prefill(kp.expand(S, -1, -1, -1).contiguous(), vp.expand(S, -1, -1, -1).contiguous())
        un.extend(kt, vt)
        assert (tail.n_comp, tail.n_win, un.n_comp, un.n_win) == (T, W, Tp + T, W)
        q1 = torch.randn(S, H, 1, 128, device=dev).half()
        for n in (16, 64, 256):
            q, k, v = (torch.randn(S, H, n, 128, device=dev).half() for _ in range(3))
            r = dict(shared=measure(lambda: tail.attend_extend_shared(q, k, v, pre), flush),
                     unshared=measure(lambda: un.attend_extend(q, k, v), flush))

            def n_steps():
                for _ in range(n):
                    tail.attend_shared(q1, pre)
            r["n_x_attend_shared"] = measure(n_steps, flush)
            r["shared_vs_unshared"] = dict(warm=round(r["shared"]["warm"] / r["unshared"]["warm"], 3),
                                           cold=round(r["shared"]["cold"] / r["unshared"]["cold"], 3))
            r["shared_vs_n_steps_warm"] = round(r["shared"]["warm"] / r["n_x_attend_shared"]["warm"], 4)
            res["by_S_n"][f"S{S}_n{n}"] = r
        del tail, un
        gc.collect()
        torch.cuda.empty_cache()
    r = res["by_S_n"]["S16_n64"]["shared_vs_unshared"]
    res["target_S16_n64_ratio_le_1"] = dict(warm="met" if r["warm"] <= 1.0 else "missed", cold="met" if r["cold"] <= 1.0 else "missed")
    del flush
    return res


def decoder_part():
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    P, n, S = 4096, 64, 16
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
    suf = torch.randint(0, mcfg.vocab_size, (S, n), device=dev)
    res = dict(prompt=P, n=n, S=S)
    dec = FastGearDecoder(model, 3 * n + 64, batch=S, shared_prefix_tokens=P)
    dec.prefill_shared(ids)
    dec.extend_shared(suf)                            # warm-up of both paths' GEMM shapes and library handles
    dec.step(suf[:, :1])
    del dec
    gc.collect()
    torch.cuda.empty_cache()
    dec = FastGearDecoder(model, 3 * n + 64, batch=S, shared_prefix_tokens=P)
    res["prefill_shared_ms"] = round(timed(lambda: dec.prefill_shared(ids)) / 1e3, 1)
    res["extend_shared_ms"] = round(timed(lambda: dec.extend_shared(suf)) / 1e3, 1)
    dec.reset_shared()
    res["extend_shared_after_reset_ms"] = round(timed(lambda: dec.extend_shared(suf)) / 1e3, 1)
    dec.reset_shared()

    def steps():
        for i in range(n):
            dec.step(suf[:, i])
    res["shared_steps_ms"] = round(timed(steps) / 1e3, 1)
    dec.check_block_kernel()
    del dec
    gc.collect()
    torch.cuda.empty_cache()
    full = torch.cat([ids.expand(S, -1), suf], 1).contiguous()
    un = FastGearDecoder(model, P + n + 128, batch=S)
    un.prefill(full)                                  # warm-up on a decoder of its own
    del un
    gc.collect()
    torch.cuda.empty_cache()
    un = FastGearDecoder(model, P + n + 128, batch=S)
    res["unshared_prefill_ms"] = round(timed(lambda: un.prefill(full)) / 1e3, 1)
    res["shared_total_ms"] = round(res["prefill_shared_ms"] + res["extend_shared_ms"], 1)
    res["speedup_vs_unshared_prefill"] = round(res["unshared_prefill_ms"] / res["shared_total_ms"], 2)
    res["speedup_next_batch_vs_unshared_prefill"] = round(res["unshared_prefill_ms"] / res["extend_shared_after_reset_ms"], 2)
    res["speedup_vs_shared_steps"] = round(res["shared_steps_ms"] / res["extend_shared_ms"], 2)
    return res


if __name__ == "__main__":
    from gear_amd import _lib
    _lib.load()
    out = {"tool": "extend_shared_timing", "gpu": torch.cuda.get_device_name(0), "layer": layer_part()}
    if "--quick" not in sys.argv:
        out["decoder"] = decoder_part()
    print(json.dumps(out))
