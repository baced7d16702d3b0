"""Token sampling timing (GPU box), one JSON line:
  sampler: gear_sample_tokens on random fp16 logits at V = 32000 and 128256, B in {1, 4, 16, 64}, for (temperature, top_k, top_p) =
         (0.8, 50, 0.95), (1.0, 0, 0.9) and temperature 0, beside the torch-composed HF warper chain (temperature -> topk mask ->
         sort / softmax / cumsum top-p mask -> softmax -> multinomial; argmax for temperature 0) on the same logits.  Warm = median
         of 9 single eager calls (host launch cost included: the GPU waits for the Python call); cold = median of 5 such calls each
         behind a 512 MiB write (larger than the last-level cache).  Event times, microseconds.  (Device time of the kernel alone:
         run the tool under rocprofv3 --kernel-trace --stats.)
  decoder: random-weight 7B-shaped FastGearDecoder, 4096-token prompt, 256 generated tokens, batch 1 and 16: tokens/s of greedy and
         sampled (0.8, 50, 0.95) generate(), eager and graph=True.  Decode time = the whole call minus the prompt's prefill (timed
         on its own); synchronised events.
  speculative: sampled generate_speculative with the n-gram drafter (n_draft 3) on a repetitive prompt (a 16-token pattern
         repeated to 4096 tokens), batch 1: tokens/s and acceptance rate, beside sampled generate() on the same prompt.
usage: python tools/sample_timing.py [--quick]   (--quick: the sampler part only)"""
import gc
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

dev = torch.device("cuda")
PARAMS = {"t0.8_k50_p0.95": (0.8, 50, 0.95), "t1.0_k0_p0.9": (1.0, 0, 0.9), "t0": (0.0, 0, 1.0)}


def timed(fn, flush=None):
    if flush is not None:
        flush.fill_(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3          # us


def torch_chain(logits, t, k, p):
    """HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> softmax -> multinomial, in torch ops."""
    if t == 0:
        return logits.argmax(-1)
    x = logits.float() / t
    if k:
        x = x.masked_fill(x < torch.topk(x, k, -1).values[:, -1:], float("-inf"))
    if p < 1:
        s, idx = torch.sort(x, -1)
        remove = s.softmax(-1).cumsum(-1) <= 1 - p
        remove[:, -1] = False
        x = x.scatter(1, idx, s.masked_fill(remove, float("-inf")))
    return torch.multinomial(x.softmax(-1), 1)


def sampler_part():
    from gear_amd.sampling import SamplingParams, sample_tokens
    flush = torch.empty((512 << 20) // 4, dtype=torch.float32, device=dev)
    res = {}
    for V in (32000, 128256):
        for B in (1, 4, 16, 64):
            x = torch.randn(B, V, device=dev).half() * 3
            for name, (t, k, p) in PARAMS.items():
                prm = SamplingParams(t, k, p, seed=1)
                row = {}
                for impl, fn in (("gear", lambda: sample_tokens(x, prm, pos=5)), ("torch", lambda: torch_chain(x, t, k, p))):
                    for _ in range(3):
                        fn()
                    row[impl] = dict(warm=round(statistics.median(timed(fn) for _ in range(9)), 1),
                                     cold=round(statistics.median(timed(fn, flush) for _ in range(5)), 1))
                row["speedup_warm"] = round(row["torch"]["warm"] / row["gear"]["warm"], 1)
                res[f"V{V}_B{B}_{name}"] = row
    del flush
    return res


def _model():
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
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
    return model, mcfg


def decoder_part(model, mcfg):
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.sampling import SamplingParams
    P, N = 4096, 256
    S = SamplingParams(0.8, 50, 0.95, seed=1)
    res = dict(prompt=P, generated=N, sampling=[S.temperature, S.top_k, S.top_p])
    for B in (1, 16):
        ids = torch.randint(0, mcfg.vocab_size, (B, P), device=dev)
        L = P + N

        def fresh():
            gc.collect()
            torch.cuda.empty_cache()
            return FastGearDecoder(model, L + 64, batch=B)

        d = fresh()
        d.generate(ids, P + 4)                          # warm-up of the prefill / step shapes
        del d
        d = fresh()
        t_pre = timed(lambda: d.prefill(ids)) / 1e3     # ms
        del d
        r = dict(prefill_ms=round(t_pre, 1))
        box = {}
        for name, kw in (("greedy_eager", {}), ("greedy_graph", dict(graph=True)), ("sampled_eager", dict(sampling=S)),
                         ("sampled_graph", dict(graph=True, sampling=S))):
            dec = fresh()
            t = timed(lambda: box.__setitem__(name, dec.generate(ids, L, **kw))) / 1e3
            r[name] = dict(ms=round(t, 1), tokens_per_s=round(B * (N - 1) / ((t - t_pre) / 1e3), 1),
                           ms_per_step=round((t - t_pre) / (N - 1), 3))
            del dec
        r["sampled_graph_equals_eager"] = bool(torch.equal(box["sampled_graph"], box["sampled_eager"]))
        r["sampled_vs_greedy_graph"] = round(r["sampled_graph"]["tokens_per_s"] / r["greedy_graph"]["tokens_per_s"], 3)
        res[f"B{B}"] = r
    return res


def speculative_part(model, mcfg):
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.sampling import SamplingParams
    P, N = 4096, 256
    S = SamplingParams(0.8, 50, 0.95, seed=1)
    pat = torch.randint(0, mcfg.vocab_size, (1, 16), generator=torch.Generator().manual_seed(3))
    ids = pat.repeat(1, P // 16).to(dev)
    L = P + N

    def fresh():
        gc.collect()
        torch.cuda.empty_cache()
        return FastGearDecoder(model, L + 64)

    d = fresh()
    t_pre = timed(lambda: d.prefill(ids)) / 1e3
    del d
    res = dict(prompt="16-token pattern x 256", generated=N, prefill_ms=round(t_pre, 1))
    box = {}
    dec = fresh()
    t = timed(lambda: box.__setitem__("g", dec.generate(ids, L, sampling=S))) / 1e3
    res["sampled_eager"] = dict(tokens_per_s=round((N - 1) / ((t - t_pre) / 1e3), 1))
    dec = fresh()
    t = timed(lambda: box.__setitem__("s", dec.generate_speculative(ids, L, draft="ngram", n_draft=3, return_stats=True,
                                                                    sampling=S))) / 1e3
    st = box["s"][1]
    res["sampled_spec_ngram_k3"] = dict(tokens_per_s=round((N - 1) / ((t - t_pre) / 1e3), 1), passes=st["passes"],
                                        tokens_per_pass=round(st["tokens_per_pass"], 2),
                                        acceptance_rate=round(st["acceptance_rate"], 3))
    return res


if __name__ == "__main__":
    from gear_amd import _lib
    _lib.load()
    out = {"tool": "sample_timing", "gpu": torch.cuda.get_device_name(0), "sampler_us": sampler_part()}
    if "--quick" not in sys.argv:
        model, mcfg = _model()
        out["decoder"] = decoder_part(model, mcfg)
        out["speculative"] = speculative_part(model, mcfg)
    print(json.dumps(out))
