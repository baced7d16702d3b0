"""Scoring: per-token log-probs, perplexity, rank and the KL divergence between two caches' distributions, read from fp16 logits in
place by one launch per call (csrc/logprob.hip, gear_token_logprobs) -- no fp32 copy of [rows, vocab] is ever made.

token_logprobs() is the operator; FastGearDecoder.score() teacher-forces a text through one cache, compare_caches() runs several
caches over the same tokens in lockstep and measures every non-reference cache against the first, step by step."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib as L

K_TOP_MAX = 8


@dataclass
class TokenLogprobs:
    """What one gear_token_logprobs call returns, shaped like `ids` ([N] or [B, n]); kl / agree only with ref_logits, top_* only with
    top_k > 0 (one more axis of length top_k)."""
    logprobs: torch.Tensor
    lse: torch.Tensor
    rank: torch.Tensor
    kl: Optional[torch.Tensor] = None
    agree: Optional[torch.Tensor] = None
    top_idx: Optional[torch.Tensor] = None
    top_logprobs: Optional[torch.Tensor] = None


@dataclass
class ScoreResult:
    """Scores of the positions prompt_len .. T - 1 of a teacher-forced text: logprobs / rank [B, T - prompt_len] (rank 0 = the token
    was the argmax), their summaries, and -- when a comparison ran (compare_caches) -- kl / agree [B, T - prompt_len] against the
    reference cache with kl_mean and agree_rate.  top_idx / top_logprobs [B, T - prompt_len, top_k] when top_k > 0."""
    logprobs: torch.Tensor
    rank: torch.Tensor
    nll: float
    perplexity: float
    top1: float
    kl: Optional[torch.Tensor] = None
    kl_mean: Optional[float] = None
    agree: Optional[torch.Tensor] = None
    agree_rate: Optional[float] = None
    top_idx: Optional[torch.Tensor] = None
    top_logprobs: Optional[torch.Tensor] = None


def _rows(t: torch.Tensor):
    """[N, V] or [B, n, V] with contiguous columns -> list of (2-D view with one row pitch, rows) covering it in order: one view
    when the rows are evenly spaced, one per batch entry otherwise (logits[:, :-1] of an extend result)."""
    if t.dim() == 2:
        return [t]
    B, n, _ = t.shape
    if B == 1 or n == 0 or t.stride(0) == n * t.stride(1):
        return [t.as_strided((B * n, t.shape[2]), (t.stride(1), 1), t.storage_offset())]
    return [t[b] for b in range(B)]


def _launch(x2, r2, ids1, top_k, out, lo):
    """One launch over the rows of x2 [n, V] (pitch x2.stride(0)); results into out[...][lo : lo + n]."""
    n, V = x2.shape
    if n == 0:
        return
    ld = x2.stride(0) if n > 1 else max(x2.stride(0), V)
    sl = lambda t: None if t is None else t[lo:lo + n].data_ptr()      # noqa: E731  (rows of contiguous outputs)
    rc = L.load().gear_token_logprobs(x2.data_ptr(), None if r2 is None else r2.data_ptr(), ids1[lo:lo + n].data_ptr(), n, V, ld,
                                      int(top_k), sl(out["lp"]), sl(out["lse"]), sl(out["rank"]), sl(out.get("kl")),
                                      sl(out.get("agree")), sl(out.get("top_idx")), sl(out.get("top_lp")), L.stream_ptr(x2))
    L.check(rc, "gear_token_logprobs")


def _run(logits, ref_logits, ids1, top_k, out):
    """Every row of logits ([N, V] / [B, n, V]) in order, results into out[...][0 : rows]."""
    xs = _rows(logits)
    rs = [None] * len(xs) if ref_logits is None else _rows(ref_logits)
    lo = 0
    for x2, r2 in zip(xs, rs):
        _launch(x2, r2, ids1, top_k, out, lo)
        lo += x2.shape[0]


def _alloc(N, dev, ref, top_k):
    out = dict(lp=torch.empty(N, dtype=torch.float32, device=dev), lse=torch.empty(N, dtype=torch.float32, device=dev),
               rank=torch.empty(N, dtype=torch.int32, device=dev))
    if ref:
        out["kl"] = torch.empty(N, dtype=torch.float32, device=dev)
        out["agree"] = torch.empty(N, dtype=torch.int32, device=dev)
    if top_k:
        out["top_idx"] = torch.empty((N, top_k), dtype=torch.int32, device=dev)
        out["top_lp"] = torch.empty((N, top_k), dtype=torch.float32, device=dev)
    return out


def _check(logits, ids, ref_logits, top_k):
    if not isinstance(logits, torch.Tensor) or logits.dim() not in (2, 3):
        raise ValueError("token_logprobs: logits must be a [N, V] or [B, n, V] tensor")
    for t in (logits, ids, ref_logits):
        if t is not None and not t.is_cuda:
            raise L.GearError("gear_amd operators run on the GPU only (tensor is on %s); there is no CPU fallback" % t.device)
    if logits.dtype != torch.float16:
        raise ValueError(f"token_logprobs: logits must be fp16, got {logits.dtype}")
    if ids.dtype != torch.int64 or tuple(ids.shape) != tuple(logits.shape[:-1]):
        raise ValueError(f"token_logprobs: ids must be int64 {list(logits.shape[:-1])}, got {ids.dtype} {list(ids.shape)}")
    V = logits.shape[-1]
    if V < 1 or logits.stride(-1) != 1 and V > 1:
        raise L.GearError("token_logprobs: logits columns must be contiguous (V >= 1)")
    if any(st < V for st, n in zip(logits.stride()[:-1], logits.shape[:-1]) if n > 1):
        raise L.GearError(f"token_logprobs: logits rows overlap (strides {logits.stride()})")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 0 <= top_k <= K_TOP_MAX or top_k > V:
        raise ValueError(f"token_logprobs: top_k must be an int in [0, min({K_TOP_MAX}, V)], got {top_k!r}")
    if ref_logits is not None:
        if ref_logits.dtype != torch.float16 or ref_logits.shape != logits.shape or ref_logits.stride() != logits.stride():
            raise ValueError("token_logprobs: ref_logits must be fp16 with the shape and strides of logits")
        if ref_logits.device != logits.device:
            raise L.GearError(f"gear_amd operators need all tensors on one device (got {logits.device} and {ref_logits.device})")
    if ids.device != logits.device:
        raise L.GearError(f"gear_amd operators need all tensors on one device (got {logits.device} and {ids.device})")
    if logits.device.index is not None and logits.device.index != torch.cuda.current_device():
        raise L.GearError(f"tensors live on {logits.device} but the current device is cuda:{torch.cuda.current_device()}")


def token_logprobs(logits: torch.Tensor, ids: torch.Tensor, ref_logits: torch.Tensor = None, top_k: int = 0) -> TokenLogprobs:
    """logits fp16 [N, V] or [B, n, V] (rows may be strided views: logits[:, :-1] needs no copy; columns contiguous), ids int64
    [N] / [B, n] = the target token of each row (< 0: ignored row, logprob 0 and rank -1; >= V: NaN and -1).  ref_logits: the
    same tokens' logits through another cache, same shape and strides -- adds kl = KL(softmax(ref) || softmax(logits)) in nats and
    agree (same argmax).  top_k <= 8: the largest log-probs of every row, descending.  One launch per evenly spaced block of rows,
    no synchronisation, no host reads; the only allocations are the outputs."""
    _check(logits, ids, ref_logits, top_k)
    shape = tuple(ids.shape)
    N = ids.numel()
    out = _alloc(N, logits.device, ref_logits is not None, top_k)
    ids1 = ids.reshape(N) if ids.is_contiguous() else ids.contiguous().view(N)
    _run(logits, ref_logits, ids1, top_k, out)
    v = lambda t: None if t is None else t.view(shape + tuple(t.shape[1:]))      # noqa: E731
    return TokenLogprobs(v(out["lp"]), v(out["lse"]), v(out["rank"]), v(out.get("kl")), v(out.get("agree")), v(out.get("top_idx")),
                         v(out.get("top_lp")))


class _Collector:
    """Per-position results of a teacher-forced run, written by the kernel into [positions, B] buffers (a step's B rows are
    contiguous there) and handed out as [B, positions]."""

    def __init__(self, B, n, dev, ref, top_k):
        self.B, self.n, self.top_k = B, n, top_k
        self.out = _alloc(n * B, dev, ref, top_k)
        self.i = 0

    def add(self, logits, ids, ref_logits=None):
        """logits [B, V] (one position) or [B, c, V] (c positions) with their targets ids [B] / [B, c]."""
        if logits.dim() == 2:
            logits, ids = logits.unsqueeze(1), ids.reshape(-1, 1)
            ref_logits = None if ref_logits is None else ref_logits.unsqueeze(1)
        _check(logits, ids, ref_logits, self.top_k)
        B, c, _ = logits.shape
        if c == 1:             # the step layout: row (position i, sequence b) at i * B + b
            x2 = logits[:, 0]
            _launch(x2, None if ref_logits is None else ref_logits[:, 0], ids.reshape(B).contiguous(), self.top_k,
                    {k: t[self.i * B:] for k, t in self.out.items()}, 0)
        else:                  # a piece of c positions: rows in (sequence, position) order into a staging block, then scattered
            tmp = _alloc(B * c, logits.device, ref_logits is not None, self.top_k)
            _run(logits, ref_logits, ids.contiguous().view(B * c), self.top_k, tmp)
            for k, t in tmp.items():
                dst = self.out[k][self.i * B:(self.i + c) * B]
                dst.view((c, B) + tuple(t.shape[1:])).copy_(t.view((B, c) + tuple(t.shape[1:])).transpose(0, 1))
        self.i += c

    def result(self) -> ScoreResult:
        assert self.i == self.n, (self.i, self.n)
        g = lambda k: (None if k not in self.out else                                # noqa: E731
                       self.out[k].view((self.n, self.B) + tuple(self.out[k].shape[1:])).transpose(0, 1).contiguous())
        lp, rank = g("lp"), g("rank")
        nll = float(-lp.double().mean())
        res = ScoreResult(lp, rank, nll, math.exp(nll) if nll < 700 else float("inf"), float((rank == 0).double().mean()),
                          top_idx=g("top_idx"), top_logprobs=g("top_lp"))
        if "kl" in self.out:
            res.kl, res.agree = g("kl"), g("agree")
            res.kl_mean = float(res.kl.double().mean())
            res.agree_rate = float(res.agree.double().mean())
        return res


def check_score_args(dec, input_ids, prompt_len, mode, chunk, top_k, what="score()"):
    """The argument and capacity checks of FastGearDecoder.score(): everything is refused here, before any state changes."""
    if mode not in ("step", "extend"):
        raise ValueError(f"{what}: mode {mode!r}: 'step' or 'extend'")
    if input_ids.dim() != 2 or input_ids.shape[0] != dec.batch or input_ids.dtype != torch.int64:
        raise ValueError(f"{what}: input_ids must be int64 [{dec.batch}, T], got {input_ids.dtype} {list(input_ids.shape)}")
    T = input_ids.shape[1]
    if isinstance(prompt_len, bool) or not isinstance(prompt_len, int) or not 1 <= prompt_len < T:
        raise ValueError(f"{what}: prompt_len must be an int in [1, T - 1 = {T - 1}], got {prompt_len!r}")
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"{what}: chunk must be an int >= 1, got {chunk!r}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 0 <= top_k <= min(K_TOP_MAX, dec.cfg.vocab_size):
        raise ValueError(f"{what}: top_k must be an int in [0, {K_TOP_MAX}], got {top_k!r}")
    if dec.tp_world > 1 or dec.shared_prefix_tokens:
        raise NotImplementedError(f"{what}: not implemented for head-sharded or shared-prefix decoders")
    if mode == "extend":
        dec._kivi_refused(f"{what} with mode='extend' (extend())")
    c0 = dec.layers[0]["cache"]
    if dec.pos != 0 or c0.seq_len != 0:
        raise ValueError(f"{what}: the decoder already holds {dec.pos} tokens; scoring starts from an empty cache")
    P, F = prompt_len, T - 1          # tokens prefilled, tokens fed in all (the last token is only a target)
    if dec.cache_kind == "fp16":
        fits, cap = F <= c0.R, c0.R
    elif dec.cache_kind == "kivi":
        fits, cap = P <= c0.Tmax and F // c0.R * c0.R <= c0.Tmax, c0.Tmax
    else:
        fits, cap = P - P % c0.R + (P % c0.R + F - P) // c0.R * c0.R <= c0.Tmax, c0.Tmax
    if not fits:
        raise L.GearError(f"{what}: {F} tokens do not fit the cache (capacity {cap}): nothing was changed")


@torch.no_grad()
def score(dec, input_ids, prompt_len, mode="step", chunk=512, top_k=0) -> ScoreResult:
    """FastGearDecoder.score(): see there."""
    check_score_args(dec, input_ids, prompt_len, mode, chunk, top_k)
    B, T = input_ids.shape
    P = prompt_len
    col = _Collector(B, T - P, input_ids.device, False, top_k)
    col.add(dec.prefill(input_ids[:, :P]), input_ids[:, P])
    if mode == "step":
        for t in range(P, T - 1):
            col.add(dec.step(input_ids[:, t:t + 1]), input_ids[:, t + 1])
    else:
        for t in range(P, T - 1, chunk):
            e = min(t + chunk, T - 1)
            col.add(dec.extend(input_ids[:, t:e]), input_ids[:, t + 1:e + 1])
    return col.result()


@torch.no_grad()
def compare_caches(model, input_ids, prompt_len, kinds=("fp16", "gear"), **decoder_kwargs):
    """Score input_ids [B, T] through one FastGearDecoder per cache kind, all fed the same tokens in lockstep (prefill of the first
    prompt_len tokens, then one step() per token: every prediction sees the cache a decoder would see there).  Returns the kinds'
    ScoreResults in the order of `kinds`; every kind after the first also carries kl / agree against the first kind's
    distribution, computed step by step from the two decoders' live [B, vocab] logits -- no [T, vocab] matrix is kept.
    decoder_kwargs go to FastGearDecoder (max_tokens defaults to T + 8)."""
    from .fast_decode import FastGearDecoder
    if len(kinds) < 1:
        raise ValueError("compare_caches(): at least one cache kind")
    B, T = input_ids.shape
    kw = dict(decoder_kwargs)
    max_tokens = kw.pop("max_tokens", T + 8)
    decs = [FastGearDecoder(model, max_tokens, batch=B, cache_kind=k, **kw) for k in kinds]
    for d in decs:
        check_score_args(d, input_ids, prompt_len, "step", 1, 0, what="compare_caches()")
    P = prompt_len
    cols = [_Collector(B, T - P, input_ids.device, i > 0, 0) for i in range(len(decs))]
    for t in range(P - 1, T - 1):
        ref = None
        for i, (d, c) in enumerate(zip(decs, cols)):
            lg = d.prefill(input_ids[:, :P]) if t == P - 1 else d.step(input_ids[:, t:t + 1])
            c.add(lg, input_ids[:, t + 1], ref_logits=ref)
            if i == 0:
                ref = lg
    return [c.result() for c in cols]
