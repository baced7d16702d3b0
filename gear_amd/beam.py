"""Beam search over a shared prefix: the bookkeeping of FastGearDecoder.generate_beam.

The S = `batch` hypotheses continue ONE stored prompt (prefill_shared); after every token hypothesis b continues from the history of
hypothesis beam_idx[b], which the decoder follows with reorder(beam_idx) -- gear_cache_reorder gathers the per-sequence tails of all
layers in place, the prefix pool never moves.  The rule ("Beam search"):

  start   beam scores [0, -1e9, ..., -1e9]: the S rows hold the same prompt, so the first step picks S distinct tokens
  step    lp = log_softmax(logits.float(), -1); cand = score[:, None] + lp, flattened to [S V]; the best 2 S candidates by
          descending value, ties to the lower flat index (a stable descending sort)
  select  walking the 2 S candidates in order: an EOS candidate of rank < S becomes a finished hypothesis with score
          cand / len ** length_penalty (len = its length in tokens, prompt and EOS included), an EOS candidate of rank >= S is
          dropped; the first S other candidates become the live beams (beam_idx, token, score)
  advance reorder(beam_idx), step(tokens); the token histories are gathered by the same index
  stop    at max_length; earlier once at least S hypotheses have finished and the worst of the best S finished scores is >= the
          best live score / cur_len ** length_penalty
  end     the live beams join the finished pool with the same normalisation; the best num_return_sequences are returned, padded

The normalisation runs on the host in double precision (the fp32 candidate value divided by len ** length_penalty) and is rounded
to fp32 once, when the scores are returned.  Without an EOS token a step needs no host synchronisation: candidates, indices and
tokens stay on the device and reorder() reads the index there.  With one, the 2 S candidates of a step are read back once.
"""
from __future__ import annotations

import torch

from . import _lib as L


def check_request(dec, input_ids, max_length, num_beams, num_return_sequences):
    """Refuse, before anything changes, what generate_beam cannot run; returns (S, prompt length)."""
    if not dec.shared_prefix_tokens:
        raise ValueError("generate_beam(): construct the decoder with shared_prefix_tokens > 0 (the beams continue one stored prompt)")
    S = dec.batch
    if num_beams is not None and num_beams != S:
        raise ValueError(f"generate_beam(): num_beams = {num_beams}, the decoder was built with batch = {S} (one sequence per beam)")
    if input_ids.dim() != 2 or input_ids.shape[0] != 1 or input_ids.shape[1] < 1:
        raise ValueError(f"generate_beam(): input_ids must be [1, T >= 1] (one prompt), got {list(input_ids.shape)}")
    if not 1 <= num_return_sequences <= S:
        raise ValueError(f"generate_beam(): num_return_sequences = {num_return_sequences}, must lie in [1, {S}]")
    P = input_ids.shape[1]
    if max_length <= P:
        raise ValueError(f"generate_beam(): max_length = {max_length} does not exceed the prompt's {P} tokens")
    c0 = dec.layers[0]["cache"]
    fed = P % c0.R + max_length - 1 - P              # rows a tail holds in the end: the prompt's remainder + the tokens stepped
    if fed // c0.R * c0.R > c0.Tmax:
        raise L.GearError(f"generate_beam(): max_length = {max_length} would compress {fed // c0.R * c0.R} tokens per tail, the "
                          f"tails hold {c0.Tmax}: capacity exceeded")
    return S, P


@torch.no_grad()
def beam_search(dec, input_ids, max_length, num_beams=None, eos_token_id=None, length_penalty=1.0, num_return_sequences=1,
                pad_token_id=0):
    """-> (sequences [n, max_length] long, scores [n] fp32), best first (see the module docstring for the rule)."""
    S, P = check_request(dec, input_ids, max_length, num_beams, num_return_sequences)
    dev = input_ids.device
    logits = dec.prefill_shared(input_ids)
    V = logits.shape[-1]
    seqs = input_ids.expand(S, -1)
    score = torch.full((S,), -1e9, dtype=torch.float32, device=dev)
    score[0] = 0.0
    finished = []                                    # (normalised score, tokens [len] on the device), in the order they finished
    cur_len = P
    while True:
        cand = (score[:, None] + torch.log_softmax(logits.float(), -1)).view(-1)
        vals, flat = torch.sort(cand, descending=True, stable=True)
        vals, flat = vals[:2 * S], flat[:2 * S]
        cur_len += 1                                 # the length of a hypothesis that takes one of these candidates
        if eos_token_id is None:
            beam_idx, tok, score = flat[:S] // V, flat[:S] % V, vals[:S]
        else:
            live = []
            for rank, (v, i) in enumerate(zip(vals.tolist(), flat.tolist())):
                b, t = divmod(i, V)
                if t == eos_token_id:
                    if rank < S:
                        hyp = torch.cat([seqs[b], torch.tensor([t], dtype=seqs.dtype, device=dev)])
                        finished.append((v / cur_len ** length_penalty, hyp))
                    continue
                live.append((b, t, v))
                if len(live) == S:
                    break
            beam_idx = torch.tensor([x[0] for x in live], dtype=torch.long, device=dev)
            tok = torch.tensor([x[1] for x in live], dtype=torch.long, device=dev)
            score = torch.tensor([x[2] for x in live], dtype=torch.float32, device=dev)
        seqs = torch.cat([seqs[beam_idx], tok[:, None]], 1)
        if cur_len >= max_length:
            break
        if eos_token_id is not None and len(finished) >= S:
            best = sorted((f[0] for f in finished), reverse=True)[:S]
            if best[-1] >= live[0][2] / cur_len ** length_penalty:
                break
        dec.reorder(beam_idx)
        logits = dec.step(tok)
    pool = finished + [(v / cur_len ** length_penalty, seqs[b]) for b, v in enumerate(score.tolist())]
    pool.sort(key=lambda f: -f[0])                   # stable: equal scores keep the order in which they entered the pool
    pool = pool[:num_return_sequences]
    out = torch.full((len(pool), max_length), pad_token_id, dtype=torch.long, device=dev)
    for r, (_, hyp) in enumerate(pool):
        out[r, :hyp.numel()] = hyp
    dec.check_block_kernel()
    return out, torch.tensor([f[0] for f in pool], dtype=torch.float32, device=dev)
