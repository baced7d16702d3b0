"""Speculative verify timing (GPU box), one JSON line:
  layer: per-layer GearKVCache.attend_verify at the Llama-2-7B attention shape (32 query / 32 KV heads, batch 1) over a 4096-token
         gearslKIVI 2-bit cache (rank 8, 2 % outliers, 32 window tokens) for n in {1, 2, 4, 8, 16}, beside attend() for one token
         and attend_extend at the same n on the same cache.  Warm = median of 7 back-to-back calls; cold = median of 5 calls each
         behind a 512 MiB write (larger than the last-level cache).  Event times.
  decoder: random-weight 7B-shaped FastGearDecoder, 4096-token prompt, 256 generated tokens: tokens/s of generate() eager and with
         graph=True, and of generate_speculative with an oracle drafter (replays the eager greedy run) at n_draft 3 and 7 and with an
         always-wrong drafter.  Decode time = the whole call minus the prompt's prefill (timed on its own); synchronised events.
usage: python tools/spec_timing.py [--quick]   (--quick: the layer part only)"""
import gc
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
    att = dict(warm=statistics.median(timed(lambda: c.attend(q1)) for _ in range(7)),
               cold=statistics.median(timed(lambda: c.attend(q1), flush) for _ in range(5)))
    res["attend_us"] = {k: round(x, 1) for k, x in att.items()}
    res["verify_us"], res["extend_us"] = {}, {}
    for n in (1, 2, 4, 8, 16):
        q = torch.randn(B, H, n, 128, device=dev).half()
        k = torch.randn(B, H, n, 128, device=dev).half()
        v = torch.randn(B, H, n, 128, device=dev).half()
        for name, fn in (("verify_us", lambda: c.attend_verify(q, k, v)), ("extend_us", lambda: c.attend_extend(q, k, v))):
            for _ in range(2):
                fn()
            warm = statistics.median(timed(fn) for _ in range(7))
            cold = statistics.median(timed(fn, flush) for _ in range(5))
            res[name][n] = dict(warm=round(warm, 1), cold=round(cold, 1), vs_attend_warm=round(warm / att["warm"], 2),
                                vs_attend_cold=round(cold / att["cold"], 2))
        res["verify_us"][n]["vs_extend_warm"] = round(res["verify_us"][n]["warm"] / res["extend_us"][n]["warm"], 2)
    del flush
    return res


def decoder_part():
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    P, N = 4096, 256
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
    ids = torch.randint(0, mcfg.vocab_size, (1, P), device=dev)
    L = P + N

    def fresh():
        gc.collect()
        torch.cuda.empty_cache()
        return FastGearDecoder(model, L + 64)

    d = fresh()
    d.prefill(ids)
    d.verify(ids[:, :4])                              # warm-up of the chunk path's GEMM shapes
    d.accept(4)
    del d
    d = fresh()
    t_pre = timed(lambda: d.prefill(ids)) / 1e3       # ms
    del d
    res = dict(prompt=P, generated=N, prefill_ms=round(t_pre, 1))
    box = {}

    def run(name, fn):
        dec = fresh()
        t = timed(lambda: box.__setitem__(name, fn(dec))) / 1e3
        dec.check_block_kernel()
        res[name] = dict(ms=round(t, 1), tokens_per_s=round((N - 1) / ((t - t_pre) / 1e3), 1))

    run("generate_eager", lambda dec: dec.generate(ids, L))
    plain = box["generate_eager"]
    run("generate_graph", lambda dec: dec.generate(ids, L, graph=True))
    res["graph_equals_eager"] = bool(torch.equal(box["generate_graph"], plain))

    def oracle(toks, k):
        return plain[:, toks.shape[1]:toks.shape[1] + k]

    def wrong(toks, k):
        return (oracle(toks, k) + 1) % mcfg.vocab_size

    for name, drafter, nd in (("spec_oracle_k3", oracle, 3), ("spec_oracle_k7", oracle, 7), ("spec_wrong_k3", wrong, 3)):
        run(name, lambda dec: dec.generate_speculative(ids, L, draft=drafter, n_draft=nd, return_stats=True))
        out, st = box[name]
        res[name].update(passes=st["passes"], tokens_per_pass=round(st["tokens_per_pass"], 2),
                         acceptance_rate=round(st["acceptance_rate"], 3), equals_eager=bool(torch.equal(out, plain)),
                         vs_eager=round(res[name]["tokens_per_s"] / res["generate_eager"]["tokens_per_s"], 2))
    return res


if __name__ == "__main__":
    from gear_amd import _lib
    _lib.load()
    out = {"tool": "spec_timing", "gpu": torch.cuda.get_device_name(0), "layer": layer_part()}
    if "--quick" not in sys.argv:
        out["decoder"] = decoder_part()
    print(json.dumps(out))
