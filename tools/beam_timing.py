"""Beam-search timing (GPU box), one JSON line:
  pool:    the Llama-2-7B cache shape (32 layers, 32 KV heads), gearslKIVI 2-bit, rank 8, 2 % outliers, tails of a shared-prefix
           decoder (no prompt segment) holding 17, 64 + 17 and 256 + 17 tokens, S in {4, 16} sequences.  GearKVCachePool.reorder
           (gear_cache_reorder: the live ranges, twice, in two launches) with a full permutation beside the whole-slab torch
           gather over the same pool (index_select into a temporary, then a copy back, per buffer).  moved_MB = the workspace =
           the live bytes of all sequences; slab_MB = the pool's allocated bytes.
           Warm = median of 7 back-to-back calls; cold = median of 5 calls each behind a 512 MiB write.  Event times.
  decoder: random-weight 7B-shaped FastGearDecoder, 1024-token prompt, 128 generated tokens: generate_beam (S beams) beside
           generate(shared_prefix=True, sampling=...) at the same S; tokens/s of the decode part (S x steps / (call - prefill)).
usage: python tools/beam_timing.py [--quick]   (--quick: the pool part only)"""
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


def pool_part():
    from gear_amd.cache import GearKVCache, GearKVCachePool
    Lyr, H, cap = 32, 32, 256 + 64
    flush = torch.empty((512 << 20) // 4, dtype=torch.float32, device=dev)
    res = {"shape": dict(layers=Lyr, Hkv=H, tail_capacity=cap, method="gearslKIVI 2-bit g64 rank 8, 2 % outliers"), "by_S": {}}
    for S in (4, 16):
        res["by_S"][S] = {}
        for n in (17, 64 + 17, 256 + 17):
            torch.manual_seed(n + S)
            pool = GearKVCachePool(Lyr, S, H, cap, CC, dev)
            caches = [GearKVCache(S, H, cap, CC, dev, pool=pool, layer=i) for i in range(Lyr)]
            k, v = (torch.randn(S, H, n, 128, device=dev).half() for _ in range(2))
            pool.extend_all([k] * Lyr, [v] * Lyr)
            assert (caches[0].n_comp, caches[0].n_win) == (n - n % 64, n % 64)
            idx = torch.tensor([(b + 1) % S for b in range(S)], device=dev)

            def gather_torch():
                for name, t in pool.buf.items():
                    t.copy_(t.index_select(2 if name in ("kPseg", "vPseg") else 1, idx))

            r = dict(reorder_us=measure(lambda: pool.reorder(idx), flush), torch_gather_us=measure(gather_torch, flush),
                     moved_MB=round(pool._rws.numel() / 1e6, 2),
                     slab_MB=round(sum(t.numel() * t.element_size() for t in pool.buf.values()) / 1e6, 2), torch_launches=2 * len(pool.buf))
            r["reorder_GBps_warm"] = round(4 * pool._rws.numel() / r["reorder_us"]["warm"] / 1e3, 1)      # read + write, twice
            r["speedup"] = dict(warm=round(r["torch_gather_us"]["warm"] / r["reorder_us"]["warm"], 2),
                                cold=round(r["torch_gather_us"]["cold"] / r["reorder_us"]["cold"], 2))
            res["by_S"][S][n] = r
            del pool, caches, k, v
            gc.collect()
            torch.cuda.empty_cache()
    del flush
    return res


def decoder_part():
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    from gear_amd.sampling import SamplingParams
    P, N = 1024, 128
    mcfg = LlamaConfigLite(num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=32, hidden_size=4096,
                           intermediate_size=11008, max_position_embeddings=4096, k_bits=2, v_bits=2, group_size=64,
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
    sp = SamplingParams(0.8, 50, 0.95, 1)
    res = dict(prompt=P, generated=N, by_S={})
    for S in (4, 16):
        make = lambda: FastGearDecoder(model, N + 64, batch=S, shared_prefix_tokens=P)
        make().generate_beam(ids, P + 8)                    # warm-up: prefill shapes, sort, library handles
        t_pre = timed(lambda: make().prefill_shared(ids)) / 1e3
        runs = {}
        for name, call in (("beam", lambda d: d.generate_beam(ids, P + N)),
                           ("sampled", lambda d: d.generate(ids, P + N, sampling=sp, shared_prefix=True))):
            dec = make()
            t = timed(lambda: call(dec)) / 1e3
            runs[name] = dict(call_ms=round(t, 1), tokens_per_s=round(S * (N - 1) / ((t - t_pre) / 1e3), 1))
            del dec
            gc.collect()
            torch.cuda.empty_cache()
        runs["prefill_ms"] = round(t_pre, 1)
        runs["beam_vs_sampled"] = round(runs["beam"]["tokens_per_s"] / runs["sampled"]["tokens_per_s"], 3)
        res["by_S"][S] = runs
    return res


if __name__ == "__main__":
    from gear_amd import _lib
    _lib.load()
    out = {"tool": "beam_timing", "gpu": torch.cuda.get_device_name(0), "pool": pool_part()}
    if "--quick" not in sys.argv:
        out["decoder"] = decoder_part()
    print(json.dumps(out))
