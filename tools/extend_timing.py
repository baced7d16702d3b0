"""Chunk extend timing (GPU box), one JSON line:
  layer: per-layer GearKVCache.attend_extend at the Llama-2-7B attention shape (32 query / 32 KV heads, batch 1) over a 4096-token
         gearslKIVI 2-bit cache (rank 8, 2 % outliers, 32 window tokens) for n in {1, 16, 64, 256, 1024}, beside attend() for one
         token on the same cache.  Warm = median of 7 back-to-back calls; cold = median of 5 calls each behind a 512 MiB write
         (larger than the last-level cache).  Event times.
  decoder: random-weight 7B-shaped FastGearDecoder after a 4096-token prompt: extend(512) wall time (two passes: the second one
         at 4.6k context) against 512 step() calls; synchronised event times around the whole call.
usage: python tools/extend_timing.py [--quick]   (--quick: the layer part only)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

dev = torch.device("cuda")


def timed(fn, flush=None):
    if flush is not None:
        flush.fill_(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3          # us


def layer_part():
    from gear_amd.cache import GearKVCache
    B, H, T = 1, 32, 4096
    cc = dict(compress_method="gearslKIVI", group_size=64, residual=64, quantize_bit=2, rank=8, rankv=8, loop=3, left=0.02)
    torch.manual_seed(0)
    c = GearKVCache(B, H, T + 1200, cc, dev)
    c.prefill(torch.randn(B, H, T + 32, 128, device=dev).half(), torch.randn(B, H, T + 32, 128, device=dev).half())
    flush = torch.empty((512 << 20) // 4, dtype=torch.float32, device=dev)
    q1 = torch.randn(B, H, 1, 128, device=dev).half()
    res = {"cache": dict(T=c.n_comp, W=c.n_win, Hq=H, Hkv=H, method="gearslKIVI 2-bit g64 rank 8, 2 % outliers")}
    for _ in range(3):
        c.attend(q1)
    res["attend_us"] = dict(warm=statistics.median(timed(lambda: c.attend(q1)) for _ in range(7)),
                            cold=statistics.median(timed(lambda: c.attend(q1), flush) for _ in range(5)))
    res["attend_extend_us"] = {}
    for n in (1, 16, 64, 256, 1024):
        q = torch.randn(B, H, n, 128, device=dev).half()
        k = torch.randn(B, H, n, 128, device=dev).half()
        v = torch.randn(B, H, n, 128, device=dev).half()
        for _ in range(2):
            c.attend_extend(q, k, v)
        warm = statistics.median(timed(lambda: c.attend_extend(q, k, v)) for _ in range(7))
        cold = statistics.median(timed(lambda: c.attend_extend(q, k, v), flush) for _ in range(5))
        res["attend_extend_us"][n] = dict(warm=round(warm, 1), cold=round(cold, 1),
                                          vs_attend_warm=round(warm / res["attend_us"]["warm"], 2),
                                          vs_n_attend_warm=round(warm / (n * res["attend_us"]["warm"]), 4))
    res["attend_us"] = {k: round(x, 1) for k, x in res["attend_us"].items()}
    # roofline of the n = 64 call: compressed bytes read once per KV head and M-tile + the matrix-core FLOPs
    comp_bytes = sum(t.numel() * t.element_size() for n_, t in c.bufs.items() if n_ not in ("kwin", "vwin")) * c.n_comp / c.Tmax
    flops = 4 * H * 64 * (c.seq_len + 64) * 128
    res["roofline_n64"] = dict(compressed_MB=round(comp_bytes / 1e6, 2), mfma_GFLOP=round(flops / 1e9, 3),
                               hbm_floor_us=round(comp_bytes / 8e12 * 1e6, 2), mfma_floor_us=round(flops / 2.5e15 * 1e6, 2))
    del flush
    return res


def decoder_part():
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    P, N = 4096, 512
    mcfg = LlamaConfigLite(num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=32, hidden_size=4096,
                           intermediate_size=11008, max_position_embeddings=8192, k_bits=2, v_bits=2, group_size=64,
                           residual_length=64)
    cc = dict(compress_method="gearslKIVI", group_size=64, residual=64, quantize_bit=2, rank=8, rankv=8, loop=3, left=0.02)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        torch.manual_seed(0)
        with torch.device(dev):
            model = LlamaForCausalLM_GEARKIVI(mcfg, cc).eval()
    finally:
        torch.set_default_dtype(old)
    dec = FastGearDecoder(model, P + 3 * N + 256)
    ids = torch.randint(0, mcfg.vocab_size, (1, P + 2 * N + 64), device=dev)
    dec.prefill(ids[:, :P])
    dec.extend(ids[:, P:P + 64])                     # warm-up (library handles, GEMM shapes of the chunk path)
    t1 = timed(lambda: dec.extend(ids[:, P + 64:P + 64 + N]))
    t2 = timed(lambda: dec.extend(ids[:, P + 64 + N:P + 64 + 2 * N]))
    tok = ids[:, -1:]
    dec.step(tok)
    torch.cuda.synchronize()

    def steps():
        for _ in range(N):
            dec.step(tok)
    ts = timed(steps)
    dec.check_block_kernel()
    return dict(prompt=P, n=N, extend_ms=[round(t1 / 1e3, 2), round(t2 / 1e3, 2)], steps_ms=round(ts / 1e3, 2),
                ms_per_step=round(ts / 1e3 / N, 3), speedup=round(ts / min(t1, t2), 2))


if __name__ == "__main__":
    from gear_amd import _lib
    _lib.load()
    out = {"tool": "extend_timing", "gpu": torch.cuda.get_device_name(0), "layer": layer_part()}
    if "--quick" not in sys.argv:
        out["decoder"] = decoder_part()
    print(json.dumps(out))
