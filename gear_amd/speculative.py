"""Greedy speculative decoding helpers (plain torch, CPU or GPU): prompt-lookup drafting and the acceptance rule.

FastGearDecoder.generate_speculative drafts k tokens, checks [last token, d1 .. dk] in one verify() pass and keeps the longest
prefix of drafts the model agrees with, plus the model's own next token."""
from __future__ import annotations

import torch


def ngram_draft(tokens: torch.Tensor, k: int, max_ngram: int = 3) -> torch.Tensor:
    """Prompt-lookup drafting: tokens [B, L] -> drafts [B, k] (long, on tokens' device).

    Per row, the trailing n-gram (n = max_ngram down to 1, longest first) is looked up among the row's earlier positions; the most
    recent earlier occurrence that is followed by at least one token wins, and the (up to) k tokens that followed it are the draft.
    A draft shorter than k is padded with its last token.  No match at any n: the row's last token, k times."""
    if tokens.dim() != 2 or k < 0 or max_ngram < 1:
        raise ValueError(f"ngram_draft: tokens [B, L], k >= 0, max_ngram >= 1 (got {list(tokens.shape)}, {k}, {max_ngram})")
    rows = tokens.detach().cpu().tolist()
    out = []
    for row in rows:
        L = len(row)
        prop = None
        for n in range(min(max_ngram, L - 1), 0, -1):
            tail = row[L - n:]
            for s in range(L - n - 1, -1, -1):          # occurrence [s, s + n) ends before the last position
                if row[s:s + n] == tail:
                    prop = row[s + n:s + n + k]
                    break
            if prop is not None:
                break
        if not prop:
            prop = [row[-1]] if L else [0]
        out.append((prop + [prop[-1]] * k)[:k])
    return torch.tensor(out, dtype=torch.long, device=tokens.device).view(len(rows), k)


def accepted_lengths(drafts: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """Greedy acceptance: drafts [B, k], logits [B, k + 1, V] of the verify pass over [last token, d1 .. dk] -> [B] long, the
    number of leading drafts equal to the model's argmax at the position before them.  The pass then yields those drafts and the
    model's token after them (logits[:, a].argmax): a + 1 tokens, each what plain greedy decoding would have produced."""
    B, k = drafts.shape
    if logits.dim() != 3 or logits.shape[0] != B or logits.shape[1] != k + 1:
        raise ValueError(f"accepted_lengths: drafts [B, k] and logits [B, k + 1, V], got {list(drafts.shape)} / {list(logits.shape)}")
    if k == 0:
        return torch.zeros(B, dtype=torch.long, device=drafts.device)
    match = logits[:, :k].argmax(-1) == drafts.to(logits.device)
    return match.long().cumprod(1).sum(1).to(drafts.device)
