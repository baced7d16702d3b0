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


# ------------------------------------------------------------------------------------------------ draft trees
N_MAX_TREE = 16          # nodes per draft tree (the root included): cache.N_MAX_VERIFY, one uint32 mask bit per node


def tree_layout(parents: torch.Tensor):
    """Draft tree -> what verify_tree() / attend_verify_tree() need.  parents: long [n] or [B, n]; node 0 is the root (the last
    committed token, parent -1), every other node's parent index is smaller than its own (a topological order).  Returns
    (anc uint32 [B or 1, n], depth long [B or 1, n]): bit j of anc[b, i] is set iff node j is node i or one of its ancestors;
    depth is the number of edges up to the root.  ValueError: n > 16, parents[0] != -1, a parent index >= its node (or < 0)."""
    if parents.dim() not in (1, 2) or parents.shape[-1] < 1 or parents.dtype != torch.long:
        raise ValueError(f"tree_layout: parents must be long [n] or [B, n] with n >= 1, got {list(parents.shape)} {parents.dtype}")
    n = parents.shape[-1]
    if n > N_MAX_TREE:
        raise ValueError(f"tree_layout: n = {n} nodes, at most {N_MAX_TREE}")
    p = parents.reshape(-1, n)
    node = torch.arange(n, device=p.device)
    if bool((p[:, 0] != -1).any()):
        raise ValueError("tree_layout: node 0 is the root, parents[0] must be -1")
    if bool(((p[:, 1:] < 0) | (p[:, 1:] >= node[1:])).any()):
        raise ValueError("tree_layout: every node after the root needs a parent index in [0, its own index)")
    anc = torch.ones_like(p)
    depth = torch.zeros_like(p)
    for i in range(1, n):
        anc[:, i] = anc.gather(1, p[:, i:i + 1])[:, 0] | (1 << i)
        depth[:, i] = depth.gather(1, p[:, i:i + 1])[:, 0] + 1
    return anc.to(torch.uint32), depth


def tree_accept(tokens: torch.Tensor, parents: torch.Tensor, logits: torch.Tensor):
    """Greedy acceptance over a draft tree: tokens [B, n] (node 0 = the last committed token), parents long [n] or [B, n]
    (tree_layout's form), logits [B, n, V] of the verify_tree() pass.  From the root: at node u take t = logits[b, u].argmax(); if
    a child of u carries t move to it (the lowest-index child among duplicates), otherwise stop.  Returns (path long [B, n]: the
    nodes visited, root first, padded with -1; length long [B]: nodes on the path, >= 1 -- length - 1 drafts were accepted;
    next_token long [B]: the argmax at the last node of the path).  The pass then yields the path's drafts and next_token, each
    what plain greedy decoding would have produced."""
    if tokens.dim() != 2 or logits.dim() != 3 or tuple(logits.shape[:2]) != tuple(tokens.shape):
        raise ValueError(f"tree_accept: tokens [B, n] and logits [B, n, V], got {list(tokens.shape)} / {list(logits.shape)}")
    B, n = tokens.shape
    dev = logits.device
    par = parents.to(dev).reshape(-1, n).expand(B, n)
    tok = tokens.to(dev)
    best = logits.argmax(-1)                                    # [B, n]
    node = torch.arange(n, device=dev).expand(B, n)
    path = torch.full((B, n), -1, dtype=torch.long, device=dev)
    path[:, 0] = 0
    cur = torch.zeros(B, dtype=torch.long, device=dev)
    length = torch.ones(B, dtype=torch.long, device=dev)
    alive = torch.ones(B, dtype=torch.bool, device=dev)
    for j in range(1, n):
        t = best.gather(1, cur[:, None])
        hit = (par == cur[:, None]) & (tok == t)
        child = torch.where(hit, node, n).min(1).values         # the lowest-index matching child, n: none
        alive = alive & (child < n)
        cur = torch.where(alive, child, cur)
        path[:, j] = torch.where(alive, child, -1)
        length = length + alive.long()
    out_dev = tokens.device
    return path.to(out_dev), length.to(out_dev), best.gather(1, cur[:, None])[:, 0].to(out_dev)


def _continuations(row, k, width, max_ngram):
    """ngram_draft's lookup, keeping up to `width` continuations (<= k tokens each) that differ, most recent occurrence first."""
    L = len(row)
    for n in range(min(max_ngram, L - 1), 0, -1):
        tail = row[L - n:]
        found = []
        for s in range(L - n - 1, -1, -1):
            if row[s:s + n] == tail:
                cont = row[s + n:s + n + k]
                if cont and cont not in found:
                    found.append(cont)
                    if len(found) == width:
                        break
        if found:
            return found
    return [[row[-1]] if L else [0]]


def ngram_tree_draft(tokens: torch.Tensor, n_nodes: int, width: int = 2, max_ngram: int = 3):
    """Prompt-lookup drafting of a tree: tokens [B, L] -> (drafts long [B, n_nodes - 1], parents long [B, n_nodes]); node 0 is the
    root (the row's last token, not among the drafts), node i >= 1 carries drafts[:, i - 1].

    ngram_draft's lookup, but the (up to) `width` most recent occurrences of the trailing n-gram whose continuations differ are
    all kept and merged into a trie under the root (common prefixes are shared).  The n_nodes - 1 draft nodes are split evenly
    between the continuations, the remainder going to the most recent one, which therefore gets the longest branch; nodes a short
    continuation leaves unused extend the first branch, in the end with its last token repeated (ngram_draft's padding rule).
    The parents are always valid for tree_layout; width = 1 gives exactly ngram_draft(tokens, n_nodes - 1, max_ngram) as a chain."""
    if tokens.dim() != 2 or n_nodes < 1 or n_nodes > N_MAX_TREE or width < 1 or max_ngram < 1:
        raise ValueError(f"ngram_tree_draft: tokens [B, L], 1 <= n_nodes <= {N_MAX_TREE}, width >= 1, max_ngram >= 1 "
                         f"(got {list(tokens.shape)}, {n_nodes}, {width}, {max_ngram})")
    k = n_nodes - 1
    drafts, parents = [], []
    for row in tokens.detach().cpu().tolist():
        tok, par = [None], [-1]                                 # the trie, nodes in creation order (parents first)
        conts = _continuations(row, k, width, max_ngram) if k else []
        for j, cont in enumerate(conts):
            _insert(tok, par, cont, k // len(conts) + (k % len(conts) if j == 0 else 0))
        if k:
            tip = _insert(tok, par, conts[0], k + 1 - len(tok))  # what the other branches left unused: the first branch, further
            while len(tok) < n_nodes:
                tip = _child(tok, par, tip, conts[0][-1], 1)
        drafts.append(tok[1:])
        parents.append(par)
    dev = tokens.device
    return (torch.tensor(drafts, dtype=torch.long, device=dev).view(len(drafts), k),
            torch.tensor(parents, dtype=torch.long, device=dev).view(len(parents), n_nodes))


def _child(tok, par, u, t, budget):
    """The child of node u that carries token t; created (budget > 0) when there is none, else None."""
    for c in range(1, len(tok)):
        if par[c] == u and tok[c] == t:
            return c
    if budget <= 0:
        return None
    tok.append(t)
    par.append(u)
    return len(tok) - 1


def _insert(tok, par, cont, budget):
    """Follow the tokens `cont` down from the root, creating at most `budget` nodes -> the last node reached."""
    u = 0
    for t in cont:
        n0 = len(tok)
        c = _child(tok, par, u, t, budget)
        if c is None:
            break
        budget -= len(tok) - n0
        u = c
    return u
