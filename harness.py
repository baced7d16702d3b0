#!/usr/bin/env python3
"""harness.py -- counterpart of the reference's timing harness cuda_supported_gear/test.py (:25-102): generate with a Llama-2-7B
shaped model through the GEAR cache, the KIVI cache or a plain fp16 cache and print wall time, peak GPU memory and tokens/s.

Same knobs as the reference (--batch_size, --model with "gearl" / "KIVI" / "None" in it; prompt 1000 tokens, generation up to
1500 -- test.py:25-28), plus what the reference hard-codes: --prompt_len, --max_length, the compress_config fields, --layers to
shrink the model, --all to run the three variants back to back.  There is no network here: weights are random (Llama shapes) and
the prompt is synthetic token ids, which does not change the timing of a greedy decode.

    python harness.py --model gearl --batch_size 8            # the reference's default run
    python harness.py --all --batch_size 1 --fast             # all three variants through the fast decode path
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build(variant, mcfg, cc, dev):
    from gear_amd.modeling_llama_kivi import LlamaForCausalLM_KIVI
    from gear_amd.modeling_llamagear import LlamaAttention_GEAR, LlamaForCausalLM_GEARKIVI, _rep, apply_rotary_pos_emb
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        torch.manual_seed(0)
        with torch.device(dev):
            if variant == "gearl":
                return LlamaForCausalLM_GEARKIVI(mcfg, cc).eval()
            if variant == "KIVI":
                return LlamaForCausalLM_KIVI(mcfg, cc).eval()

            class LlamaAttention_FP16(LlamaAttention_GEAR):
                """The uncompressed baseline (transformers' LlamaForCausalLM in the reference, test.py:56-60): fp16 K / V cache."""

                def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_value=None,
                            output_attentions=False, use_cache=False, **kw):
                    b, q, _ = hidden_states.shape
                    qs = self.q_proj(hidden_states).view(b, q, self.num_heads, self.head_dim).transpose(1, 2)
                    ks = self.k_proj(hidden_states).view(b, q, self.num_key_value_heads, self.head_dim).transpose(1, 2)
                    vs = self.v_proj(hidden_states).view(b, q, self.num_key_value_heads, self.head_dim).transpose(1, 2)
                    past = 0 if past_key_value is None else past_key_value[8]
                    if position_ids is None:
                        position_ids = torch.arange(past, past + q, device=hidden_states.device).unsqueeze(0)
                    cos, sin = self.rotary_emb(vs, position_ids)
                    qs, ks = apply_rotary_pos_emb(qs, ks, cos, sin)
                    if past_key_value is not None:
                        ks, vs = torch.cat([past_key_value[0], ks], 2), torch.cat([past_key_value[1], vs], 2)
                    n = self.num_key_value_groups
                    o = F.scaled_dot_product_attention(qs, _rep(ks, n), _rep(vs, n), is_causal=past_key_value is None and q > 1)
                    o = self.o_proj(o.transpose(1, 2).reshape(b, q, self.num_heads * self.head_dim))
                    return o, None, ((ks, vs, None, None, None, None, None, None, past + q) if use_cache else None)

            m = LlamaForCausalLM_GEARKIVI(mcfg, cc)
            for i, layer in enumerate(m.model.layers):
                a = LlamaAttention_FP16(i, mcfg, cc)
                a.load_state_dict(layer.self_attn.state_dict())
                layer.self_attn = a
            return m.eval()
    finally:
        torch.set_default_dtype(old)


def run(variant, args, dev):
    from gear_amd.modeling_llamagear import LlamaConfigLite
    mcfg = LlamaConfigLite(num_hidden_layers=args.layers, max_position_embeddings=max(4096, args.max_length + 64),
                           k_bits=args.bits, v_bits=args.bits, group_size=args.group_size, residual_length=args.residual,
                           rope_scaling=args.rope_scaling)
    cc = dict(compress_method=args.compress_method, group_size=args.group_size, residual=args.residual, quantize_bit=args.bits,
              rank=args.rank, rankv=args.rank, loop=args.loop, left=args.left)
    model = build(variant, mcfg, cc, dev)
    torch.manual_seed(1)
    ids = torch.randint(0, mcfg.vocab_size, (args.batch_size, args.prompt_len), device=dev)
    torch.cuda.reset_peak_memory_stats(dev)
    torch.cuda.synchronize()
    t0 = time.time()
    # --do_sample: HF's generate(do_sample=True, temperature, top_k, top_p) through gear_sample_tokens; without it the greedy path
    sampling = None
    hook_kw = {}
    if args.do_sample:
        from gear_amd.sampling import SamplingParams
        sampling = SamplingParams(args.temperature, args.top_k, args.top_p, args.seed)
        hook_kw = dict(do_sample=True, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, seed=args.seed)
    fast_kw = {} if sampling is None else dict(sampling=sampling)
    # --repetition_penalty / --no_repeat_ngram_size / --min_new_tokens / --stop_at_eos: HF's generate() kwargs of those names through
    # gear_logits_process and gear_eos_update (random weights: the EOS id is whatever --stop_at_eos names)
    eos = None if args.stop_at_eos < 0 else args.stop_at_eos
    if args.repetition_penalty != 1.0 or args.no_repeat_ngram_size or args.min_new_tokens or eos is not None:
        from gear_amd.logits import LogitsParams
        fast_kw["logits"] = LogitsParams(args.repetition_penalty, args.no_repeat_ngram_size, args.min_new_tokens, eos)
        if args.graph:
            fast_kw["graph"] = True
        hook_kw.update(repetition_penalty=args.repetition_penalty, no_repeat_ngram_size=args.no_repeat_ngram_size,
                       min_new_tokens=args.min_new_tokens, eos_token_id=eos)
    elif args.graph:
        fast_kw["graph"] = True
    cache_bytes = None
    if variant == "gearl" and args.fast and args.shared_prefix:
        # the batch continues ONE prompt (row 0) stored once: a batch-1 prefix cache + per-sequence tails (gear_attn_decode_shared)
        from gear_amd.fast_decode import FastGearDecoder
        # --num_beams N: beam search with N beams over that prompt (generate_beam: one beam per sequence, the tails follow the
        # beams through gear_cache_reorder); the reference's evaluation scripts hand num_beams to generate() the same way
        bs = args.num_beams or args.batch_size
        dec = FastGearDecoder(model, args.max_length - args.prompt_len + args.residual + 8, batch=bs,
                              shared_prefix_tokens=args.prompt_len)
        if args.num_beams:
            out, beam_scores = dec.generate_beam(ids[:1], args.max_length, num_beams=bs, length_penalty=args.length_penalty,
                                                 num_return_sequences=bs)
        else:
            out = dec.generate(ids[:1], args.max_length, shared_prefix=True, **fast_kw)
        cache_bytes = sum(t.numel() * t.element_size() for pool in (dec.pool, dec.prefix_pool) for t in pool.buf.values())
    elif variant == "gearl" and args.fast:
        from gear_amd.fast_decode import FastGearDecoder
        dec = FastGearDecoder(model, args.max_length + 8, batch=args.batch_size)
        if args.tree_width:
            # speculative decoding with prompt-lookup drafts: chains (1) or draft trees of this width (verify_tree / accept_path)
            out = dec.generate_speculative(ids, args.max_length, draft="ngram", n_draft=7, tree_width=args.tree_width, **fast_kw)
        else:
            out = dec.generate(ids, args.max_length, **fast_kw)
        cache_bytes = sum(t.numel() * t.element_size() for t in dec.pool.buf.values())
        del dec
    elif variant == "None" and args.fast:
        # the control through the SAME decoder (fused GEMVs, gear_attn_decode_f16 over cache.Fp16KVCache): gearl and None then
        # differ in the cache only
        from gear_amd.fast_decode import FastGearDecoder
        out = FastGearDecoder(model, args.max_length + 8, batch=args.batch_size, cache_kind="fp16").generate(ids, args.max_length,
                                                                                                             **fast_kw)
    elif variant == "KIVI" and args.fast:
        # the KIVI baseline through the SAME decoder too (cache.KiviKVCache on csrc/kivi.hip): the three rows differ in the cache only
        from gear_amd.fast_decode import FastGearDecoder
        dec = FastGearDecoder(model, args.max_length + 8, batch=args.batch_size, cache_kind="kivi")
        out = dec.generate(ids, args.max_length, **fast_kw)
        cache_bytes = sum(t.numel() * t.element_size() for lw in dec.layers for t in vars(lw["cache"]).values()
                          if isinstance(t, torch.Tensor) and t.dim() == 4)
        del dec
    else:
        out = model.generate(ids, args.max_length, **hook_kw)
    torch.cuda.synchronize()
    dt = time.time() - t0
    peak = torch.cuda.max_memory_allocated(dev) / 2 ** 20
    beams = args.num_beams if variant == "gearl" and args.num_beams else 0
    new = (out.shape[1] - args.prompt_len) * (beams or args.batch_size)
    print(f"[{variant}{' (fast path)' if args.fast else ''}] Peak memory usage on GPU: {peak:.1f} MB")
    if cache_bytes is not None:
        print(f"[{variant}] allocated cache: {cache_bytes / 2 ** 20:.1f} MB{' (shared prefix)' if args.shared_prefix else ''}")
    print(f"[{variant}] time {dt:.3f}   ({new / dt:.1f} new tokens/s, {f'{beams} beams' if beams else f'batch {args.batch_size}'}, prompt {args.prompt_len} -> {out.shape[1]})")
    del model
    torch.cuda.empty_cache()
    return dict(variant=variant, fast=bool(args.fast), batch_size=args.batch_size, prompt_len=args.prompt_len,
                max_length=int(out.shape[1]), time_s=dt, new_tokens_per_s=new / dt, peak_mem_MiB=peak, layers=args.layers,
                rope_scaling=args.rope_scaling,
                **(dict(cache_bytes=cache_bytes) if cache_bytes is not None else {}),
                **(dict(shared_prefix=True) if args.shared_prefix and variant == "gearl" else {}),
                **(dict(num_beams=beams, length_penalty=args.length_penalty, best_score=float(beam_scores[0])) if beams else {}),
                **(dict(do_sample=True, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, seed=args.seed)
                   if args.do_sample else {}))


def score(args, dev):
    """--score --fast: the harness's synthetic text (prompt_len prompt tokens, scored up to max_length) teacher-forced through the
    three cache kinds of FastGearDecoder in lockstep, one step() per token (scoring.compare_caches): mean NLL, perplexity and
    top-1 share per kind, mean KL and argmax agreement of the compressed kinds against the fp16 row."""
    from gear_amd.modeling_llamagear import LlamaConfigLite
    from gear_amd.scoring import compare_caches
    mcfg = LlamaConfigLite(num_hidden_layers=args.layers, max_position_embeddings=max(4096, args.max_length + 64),
                           k_bits=args.bits, v_bits=args.bits, group_size=args.group_size, residual_length=args.residual,
                           rope_scaling=args.rope_scaling)
    cc = dict(compress_method=args.compress_method, group_size=args.group_size, residual=args.residual, quantize_bit=args.bits,
              rank=args.rank, rankv=args.rank, loop=args.loop, left=args.left)
    model = build("gearl", mcfg, cc, dev)
    torch.manual_seed(1)
    ids = torch.randint(0, mcfg.vocab_size, (args.batch_size, args.max_length), device=dev)
    kinds = ("fp16", "gear", "kivi")
    res = compare_caches(model, ids, args.prompt_len, kinds=kinds, max_tokens=args.max_length + 8)
    print(f"scoring {args.max_length - args.prompt_len} positions x batch {args.batch_size} after a {args.prompt_len}-token prompt "
          f"({args.layers} layers, mode step)")
    print(f"{'cache':6s} {'mean NLL':>10s} {'perplexity':>12s} {'top-1':>7s} {'mean KL vs fp16':>16s} {'argmax agree':>13s}")
    out = []
    for kind, r in zip(kinds, res):
        kl = "" if r.kl_mean is None else f"{r.kl_mean:.6f}"
        ag = "" if r.agree_rate is None else f"{r.agree_rate:.4f}"
        print(f"{kind:6s} {r.nll:10.5f} {r.perplexity:12.3f} {r.top1:7.4f} {kl:>16s} {ag:>13s}")
        out.append(dict(cache_kind=kind, nll=r.nll, perplexity=r.perplexity, top1=r.top1, kl_mean=r.kl_mean, agree=r.agree_rate))
    return out


def main():
    ap = argparse.ArgumentParser(description="GEAR / KIVI / fp16 generation timing (cuda_supported_gear/test.py)")
    ap.add_argument("--batch_size", type=int, default=8, help="Batch size.")                       # test.py:22
    ap.add_argument("--model", type=str, default="gearl", help='variant: contains "gearl", "KIVI" or "None"')   # test.py:23, :41-60
    ap.add_argument("--all", action="store_true", help="run gearl, KIVI and None back to back")
    ap.add_argument("--prompt_len", type=int, default=1000)                                         # max_token, test.py:26
    ap.add_argument("--max_length", type=int, default=1500)                                         # max_generation_length, :27
    ap.add_argument("--compress_method", default="gearlKIVI")                                       # test.py:31
    ap.add_argument("--group_size", type=int, default=64)
    ap.add_argument("--residual", type=int, default=64)
    ap.add_argument("--bits", type=int, default=2)
    ap.add_argument("--rank", type=int, default=2)
    ap.add_argument("--loop", type=int, default=3)
    ap.add_argument("--left", type=float, default=0.0, help="outlier fraction (fast path only: the hook's fused path stores none)")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--fast", action="store_true", help="every variant through FastGearDecoder (pre-allocated cache, fused kernels): cache kinds gear / kivi / fp16")
    ap.add_argument("--shared_prefix", action="store_true",
                    help="with --fast: the batch continues ONE prompt stored once (shared-prefix decoding) instead of batch_size copies")
    ap.add_argument("--num_beams", type=int, default=0,
                    help="with --fast --shared_prefix: beam search with this many beams over the one prompt (generate_beam)")
    ap.add_argument("--length_penalty", type=float, default=1.0, help="beam scores are divided by length ** length_penalty")
    ap.add_argument("--tree_width", type=int, default=0,
                    help="with --fast: generate_speculative with n-gram drafts (n_draft 7); 1: draft chains, N > 1: draft trees of "
                         "up to N continuations per pass (greedy only)")
    ap.add_argument("--rope_scaling", type=json.loads, default=None,
                    help="the config's rope_scaling as JSON, e.g. '{\"rope_type\": \"llama3\", \"factor\": 8, \"low_freq_factor\": 1, "
                         "\"high_freq_factor\": 4, \"original_max_position_embeddings\": 8192}' (linear / llama3 / yarn; default: none)")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--score", action="store_true",
                    help="with --fast: score the synthetic text through the fp16 / gear / kivi caches (mean NLL, perplexity, top-1; "
                         "KL and argmax agreement against the fp16 row) instead of timing a generation")
    # sampling, with the defaults of GenerationBench/GenerationTest/evaluation_bbh_cot.py:381-390
    ap.add_argument("--do_sample", action="store_true", help="sample (temperature / top-k / top-p) instead of greedy decoding")
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--top_k", type=int, default=50)
    ap.add_argument("--top_p", type=float, default=0.95)
    ap.add_argument("--seed", type=int, default=0, help="key of the sampler's random stream")
    # logits processors and EOS stopping (HF's generate() kwargs; the reference evaluates through them: evaluation_bbh_cot.py:374-392)
    ap.add_argument("--repetition_penalty", type=float, default=1.0, help="HF's repetition_penalty (1: off)")
    ap.add_argument("--no_repeat_ngram_size", type=int, default=0, help="HF's no_repeat_ngram_size (0: off)")
    ap.add_argument("--min_new_tokens", type=int, default=0, help="EOS is held back for this many tokens (needs --stop_at_eos)")
    ap.add_argument("--stop_at_eos", type=int, default=-1, metavar="EOS_ID",
                    help="stop a row at this token id and pad it from there; generation ends once every row stopped (-1: off)")
    ap.add_argument("--graph", action="store_true", help="with --fast --model gearl: captured token steps (generate(graph=True))")
    args = ap.parse_args()
    if args.graph and (not args.fast or args.shared_prefix or args.tree_width or args.all or "gearl" not in args.model):
        raise SystemExit("--graph needs --fast --model gearl without --shared_prefix / --tree_width / --all (graph steps run on the "
                         "compressed cache)")
    if (args.tree_width or args.num_beams) and (args.repetition_penalty != 1.0 or args.no_repeat_ngram_size or args.min_new_tokens
                                                or args.stop_at_eos >= 0):
        raise SystemExit("the logits processors / --stop_at_eos run in generate() only (not with --tree_width or --num_beams)")
    if args.shared_prefix and not args.fast:
        raise SystemExit("--shared_prefix needs --fast (shared-prefix decoding lives in FastGearDecoder)")
    if args.num_beams and not (args.fast and args.shared_prefix):
        raise SystemExit("--num_beams needs --fast --shared_prefix (beam search runs over a shared prefix)")
    if args.num_beams and args.do_sample:
        raise SystemExit("--num_beams and --do_sample exclude each other (beam search is deterministic)")
    if args.num_beams < 0:
        raise SystemExit("--num_beams must be positive")
    if args.tree_width < 0 or (args.tree_width and (not args.fast or args.shared_prefix)):
        raise SystemExit("--tree_width needs --fast without --shared_prefix (speculative decoding lives in FastGearDecoder)")
    if args.tree_width > 1 and args.do_sample:
        raise SystemExit("--tree_width > 1 and --do_sample exclude each other (sampling over a draft tree is not implemented)")
    if args.score and not args.fast:
        raise SystemExit("--score needs --fast (scoring lives in FastGearDecoder)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.score:
        res = score(args, dev)
        if args.json:
            print(json.dumps(res))
        return
    variants = ["gearl", "KIVI", "None"] if args.all else [v for v in ("gearl", "KIVI", "None") if v in args.model]
    if not variants:
        raise SystemExit('--model must contain "gearl", "KIVI" or "None"')
    res = [run(v, args, dev) for v in variants]
    if args.json:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
