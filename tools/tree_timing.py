"""Tree-verify timing (GPU box), one JSON line:
  layer: GearKVCache.attend_verify_tree against attend_verify at the Llama-2-7B attention shape (32 query / 32 KV heads, batch 1)
         over a 4096-token gearslKIVI 2-bit cache (rank 8, 2 % outliers, 32 window tokens) for n in {4, 8, 16}; the tree is two
         chains under one root (the chain mask as well: the same keys as attend_verify).  Per n the three calls are timed in
         interleaved rounds -- 5 warm-up rounds, then 30 rounds of one call each, event times -- and reported as medians with the
         spread (max - min over three blocks of 10 rounds) of attend_verify, which is the resolution of the comparison.
  decoder: random-weight 7B-shaped FastGearDecoder, a prompt of 4096 tokens that repeats a 48-token pattern in which every 12th
         token alternates between two values (so the trailing n-gram has earlier occurrences with two continuations), 256 generated
         tokens: tokens per pass and tokens/s of generate_speculative(n_draft=7) at tree_width 1 and 2.
usage: python tools/tree_timing.py [--quick]   (--quick: the layer part only)"""
import gc
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

dev = torch.device("cuda")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3          # us


def layer_part():
    from gear_amd.cache import GearKVCache
    from gear_amd.speculative import tree_layout
    B, H, T = 1, 32, 4096
    cc = dict(compress_method="gearslKIVI", group_size=64, residual=64, quantize_bit=2, rank=8, rankv=8, loop=3, left=0.02)
    torch.manual_seed(0)
    c = GearKVCache(B, H, T + 1200, cc, dev)
    c.prefill(torch.randn(B, H, T + 32, 128, device=dev).half(), torch.randn(B, H, T + 32, 128, device=dev).half())
    res = {"cache": dict(T=c.n_comp, W=c.n_win, Hq=H, Hkv=H, method="gearslKIVI 2-bit g64 rank 8, 2 % outliers")}
    for n in (4, 8, 16):
        q = torch.randn(B, H, n, 128, device=dev).half()
        k = torch.randn(B, H, n, 128, device=dev).half()
        v = torch.randn(B, H, n, 128, device=dev).half()
        two = torch.tensor(([-1, 0, 0] + list(range(1, n - 2)))[:n])
        masks = {name: tree_layout(p)[0].view(torch.int32)[0].to(dev) for name, p in (("chain", torch.arange(-1, n - 1)), ("tree", two))}
        fns = dict(verify=lambda: c.attend_verify(q, k, v), tree_chain_mask=lambda: c.attend_verify_tree(q, k, v, masks["chain"]),
                   tree=lambda: c.attend_verify_tree(q, k, v, masks["tree"]))
        t = {name: [] for name in fns}
        for r in range(35):
            for name, fn in fns.items():
                x = timed(fn)
                if r >= 5:
                    t[name].append(x)
        med = {name: statistics.median(x) for name, x in t.items()}
        blocks = [statistics.median(t["verify"][i:i + 10]) for i in (0, 10, 20)]
        res[n] = dict({name + "_us": round(x, 1) for name, x in med.items()}, verify_spread_us=round(max(blocks) - min(blocks), 2),
                      tree_vs_verify=round(med["tree"] / med["verify"], 3),
                      chain_mask_vs_verify=round(med["tree_chain_mask"] / med["verify"], 3))
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
    g = torch.Generator().manual_seed(4)
    pat = torch.randint(0, mcfg.vocab_size, (48,), generator=g)
    ids = pat.repeat((P + 47) // 48)[:P].clone()
    alt = torch.arange(11, P, 12)
    ids[alt[1::2]] = (ids[alt[1::2]] + 1) % mcfg.vocab_size
    ids = ids.view(1, P).to(dev)
    L = P + N

    def fresh():
        gc.collect()
        torch.cuda.empty_cache()
        return FastGearDecoder(model, L + 64)

    d = fresh()
    d.prefill(ids)
    d.verify(ids[:, :8])                              # warm-up of the pass's GEMM shapes
    d.accept(8)
    del d
    d = fresh()
    t_pre = timed(lambda: d.prefill(ids)) / 1e3       # ms
    del d
    res = dict(prompt=P, generated=N, n_draft=7, prefill_ms=round(t_pre, 1))
    box = {}
    for width in (1, 2, 1, 2):                        # (each width twice: the second run is reported, the first shows the spread)
        dec = fresh()
        t = timed(lambda: box.__setitem__(width, dec.generate_speculative(ids, L, draft="ngram", n_draft=7, return_stats=True,
                                                                          tree_width=width))) / 1e3
        dec.check_block_kernel()
        out, st = box[width]
        prev = res.get(f"tree_width_{width}", {}).get("tokens_per_s")
        res[f"tree_width_{width}"] = dict(ms=round(t, 1), tokens_per_s=round((N - 1) / ((t - t_pre) / 1e3), 1), passes=st["passes"],
                                          tokens_per_pass=round(st["tokens_per_pass"], 2),
                                          acceptance_rate=round(st["acceptance_rate"], 3), first_run_tokens_per_s=prev)
    res["same_tokens"] = bool(torch.equal(box[1][0], box[2][0]))
    return res


if __name__ == "__main__":
    from gear_amd import _lib
    _lib.load()
    out = {"tool": "tree_timing", "gpu": torch.cuda.get_device_name(0), "layer": layer_part()}
    if "--quick" not in sys.argv:
        out["decoder"] = decoder_part()
    print(json.dumps(out))
