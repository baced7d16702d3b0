"""Logits processors and EOS stopping for the decoders: logit bias / token bans, repetition penalty, n-gram ban and the minimum
length, in HF's processor order, in one launch per step (csrc/logits.hip, gear_logits_process), and the per-sequence "finished"
state (gear_eos_update).

The processors read each sequence's token history from an int32 device buffer (TokenHistory).  The launch appends the token just fed
to it by itself (`cur`), so a captured token step grows the history without a launch of its own.  Nothing here synchronises or reads
the device from the host: both launches are capturable in a graph."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L

N_EOS_MAX = 8
V_MAX = 262144


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def eos_ids(eos_token_id) -> tuple:
    """None / int / sequence of ints -> a tuple of at most 8 ids >= 0 (HF's generate() takes either form)."""
    if eos_token_id is None:
        return ()
    ids = (eos_token_id,) if _is_int(eos_token_id) else tuple(eos_token_id) if isinstance(eos_token_id, (tuple, list)) else None
    if ids is None or not all(_is_int(e) and 0 <= e < 2 ** 31 for e in ids):
        raise ValueError(f"eos_token_id must be an int >= 0 or a tuple of them, got {eos_token_id!r}")
    if len(ids) > N_EOS_MAX:
        raise ValueError(f"eos_token_id: at most {N_EOS_MAX} ids, got {len(ids)}")
    return ids


@dataclass(frozen=True)
class LogitsParams:
    """repetition_penalty 1 = off; no_repeat_ngram_size 0 = off; min_new_tokens bans every eos_token_id (an int or a tuple of up to
    8) until that many tokens were generated; logit_bias {token: bias} is added to the logits first (a bias of -inf bans the token);
    bad_token_ids is sugar for a bias of -inf."""
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_new_tokens: int = 0
    eos_token_id: object = None
    logit_bias: object = None
    bad_token_ids: object = None

    def __post_init__(self):
        p, g, m = self.repetition_penalty, self.no_repeat_ngram_size, self.min_new_tokens
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not p > 0 or p == float("inf"):
            raise ValueError(f"LogitsParams: repetition_penalty must be a finite number > 0, got {p!r}")
        if not _is_int(g) or g < 0:
            raise ValueError(f"LogitsParams: no_repeat_ngram_size must be an int >= 0, got {g!r}")
        if not _is_int(m) or m < 0:
            raise ValueError(f"LogitsParams: min_new_tokens must be an int >= 0, got {m!r}")
        try:
            eos_ids(self.eos_token_id)
        except ValueError as e:
            raise ValueError(f"LogitsParams: {e}") from None
        if m > 0 and not eos_ids(self.eos_token_id):
            raise ValueError("LogitsParams: min_new_tokens needs an eos_token_id to hold back")
        lb = self.logit_bias
        if lb is not None:
            if not isinstance(lb, dict):
                raise ValueError(f"LogitsParams: logit_bias must be a dict token -> float, got {type(lb).__name__}")
            for t, b in lb.items():
                if not _is_int(t) or not 0 <= t < 2 ** 31:
                    raise ValueError(f"LogitsParams: logit_bias token {t!r} must be an int >= 0")
                if isinstance(b, bool) or not isinstance(b, (int, float)) or math.isnan(b) or b == float("inf"):
                    raise ValueError(f"LogitsParams: logit_bias[{t}] = {b!r} must be a number < inf (-inf bans the token)")
        bad = self.bad_token_ids
        if bad is not None:
            if not isinstance(bad, (tuple, list)) or not all(_is_int(t) and 0 <= t < 2 ** 31 for t in bad):
                raise ValueError(f"LogitsParams: bad_token_ids must be a tuple of ints >= 0, got {bad!r}")

    @property
    def eos_ids(self) -> tuple:
        return eos_ids(self.eos_token_id)

    @property
    def bias_items(self) -> tuple:
        """The bias table: unique tokens in ascending order, bad_token_ids as -inf (they win over a finite bias)."""
        d = dict(self.logit_bias or {})
        for t in self.bad_token_ids or ():
            d[t] = float("-inf")
        return tuple(sorted((int(t), float(b)) for t, b in d.items()))

    @property
    def active(self) -> bool:
        """False when no processor would change a logit (the launch can be left out)."""
        return bool(self.repetition_penalty != 1 or self.no_repeat_ngram_size > 0 or self.min_new_tokens > 0 or self.bias_items)

    def __hash__(self):
        return hash((self.repetition_penalty, self.no_repeat_ngram_size, self.min_new_tokens, self.eos_ids, self.bias_items))

    def c_struct(self, device) -> L.LogitsParamsC:
        eos = self.eos_ids
        items = self.bias_items
        tab = _bias_table(items, device) if items else None
        return L.LogitsParamsC(float(self.repetition_penalty), int(self.no_repeat_ngram_size), int(self.min_new_tokens), len(eos),
                               (C.c_int * 8)(*eos), len(items), 0, L.ptr(tab))


_bias_tables = {}     # (items, device) -> the device table; kept for good: captured graphs hold the pointer, and a table is tiny


def _bias_table(items, device):
    key = (items, str(device))
    tab = _bias_tables.get(key)
    if tab is None:
        a = np.zeros(len(items), dtype=np.dtype([("tok", "<i4"), ("bias", "<f4")]))
        a["tok"] = [t for t, _ in items]
        a["bias"] = [b for _, b in items]
        tab = torch.from_numpy(a.view(np.uint8).copy()).to(device)
        _bias_tables[key] = tab
    return tab


class TokenHistory:
    """int32 [batch, cap] on `device`: prompt + generated tokens per sequence, what the processors read."""

    def __init__(self, batch: int, cap: int, device):
        if batch < 1 or cap < 1:
            raise ValueError(f"TokenHistory: batch = {batch}, cap = {cap}")
        self.batch, self.cap = int(batch), int(cap)
        self.buf = torch.zeros((self.batch, self.cap), dtype=torch.int32, device=device)

    def load(self, ids: torch.Tensor) -> int:
        """ids [batch, T] (any integer type, any device) become entries 0 .. T - 1 of every row; returns T."""
        if ids.dim() != 2 or ids.shape[0] != self.batch or ids.shape[1] > self.cap:
            raise ValueError(f"TokenHistory.load: ids must be [{self.batch}, T <= {self.cap}], got {list(ids.shape)}")
        self.buf[:, :ids.shape[1]] = ids.to(device=self.buf.device, dtype=torch.int32)
        return int(ids.shape[1])


def _same_device(name, ref, *tensors):
    L.require_gpu(*tensors)
    for t in tensors:
        if t is not None and t.device != ref.device:
            raise L.GearError(f"{name}: gear_amd operators need all tensors on one device (got {ref.device} and {t.device})")


def process_logits(logits: torch.Tensor, params: LogitsParams, hist, n: int, prompt_len: int, cur: torch.Tensor = None,
                   pos_dev: torch.Tensor = None, out: torch.Tensor = None) -> torch.Tensor:
    """logits [B, V] fp16 / fp32 (rows may be strided, columns contiguous) -> the processed logits, same type, in `out` (a new
    tensor when None; `out is logits` processes in place).

    hist: a TokenHistory or its int32 [B, cap] buffer; the live history length is n (+ pos_dev[0] when pos_dev, a device int32
    tensor, is given -- the decoders pass their device-side state).  cur int64 [B]: the token just fed, appended as entry n - 1 by
    the launch itself.  prompt_len: the length of the prompt part (min_new_tokens counts from there).  One launch, no
    synchronisation, no host reads: capturable in a graph."""
    if not isinstance(params, LogitsParams):
        raise TypeError(f"process_logits: params must be a LogitsParams, got {type(params).__name__}")
    if logits.dim() != 2:
        raise ValueError(f"process_logits: logits must be [rows, V], got {list(logits.shape)}")
    if logits.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"process_logits: logits must be fp16 or fp32, got {logits.dtype}")
    B, V = logits.shape
    if not logits.is_cuda:
        raise L.GearError("gear_amd operators run on the GPU only (tensor is on %s); there is no CPU fallback" % logits.device)
    if logits.stride(1) != 1:
        raise L.GearError("process_logits: logits columns must be contiguous")
    hbuf = hist.buf if isinstance(hist, TokenHistory) else hist
    if hbuf.dtype != torch.int32 or hbuf.dim() != 2 or hbuf.shape[0] != B:
        raise ValueError(f"process_logits: hist must be int32 [{B}, cap]")
    if out is None:
        out = torch.empty((B, V), dtype=logits.dtype, device=logits.device)
    elif out.dtype != logits.dtype or tuple(out.shape) != (B, V) or not out.is_cuda or out.device != logits.device:
        raise ValueError(f"process_logits: out must be {logits.dtype} [{B}, {V}] on {logits.device}")
    elif out.stride(1) != 1:
        raise L.GearError("process_logits: out columns must be contiguous")
    elif out.data_ptr() == logits.data_ptr() and out.stride(0) != logits.stride(0):
        raise ValueError("process_logits: out aliases logits with another row stride")
    if cur is not None:
        if cur.dtype != torch.int64 or cur.numel() != B:
            raise ValueError(f"process_logits: cur must be int64 with {B} entries")
        cur = cur.reshape(B)
    if pos_dev is not None and (pos_dev.dtype != torch.int32 or pos_dev.numel() < 1):
        raise ValueError("process_logits: pos_dev must be a device int32 tensor")
    if not _is_int(n) or n < 0 or (pos_dev is None and n > hbuf.shape[1]):
        raise ValueError(f"process_logits: history length n = {n!r} outside [0, {hbuf.shape[1]}]")
    _same_device("process_logits", logits, hbuf, cur, pos_dev)
    p = params.c_struct(logits.device)
    rc = L.load().gear_logits_process(L.ptr(logits), L.ptr(out), int(logits.dtype == torch.float32), B, V, logits.stride(0),
                                      out.stride(0), L.ptr(hbuf), hbuf.shape[1], L.ptr(pos_dev), int(n), L.ptr(cur),
                                      int(prompt_len), C.byref(p), L.stream_ptr(logits))
    L.check(rc, "gear_logits_process")
    return out


def eos_update(tok: torch.Tensor, done: torch.Tensor, eos_token_id, pad_token_id: int, n_done: torch.Tensor):
    """After the token choice: tok int64 [B] (or [B, 1]) and done int32 [B], both updated in place -- a finished row's token becomes
    pad_token_id, a row that just emitted an EOS id keeps it and is finished from now on; n_done int32 [1] receives the number of
    finished rows.  One launch, capturable."""
    ids = eos_ids(eos_token_id)
    B = done.numel()
    if tok.dtype != torch.int64 or tok.numel() != B or done.dtype != torch.int32 or n_done.dtype != torch.int32 or n_done.numel() < 1:
        raise ValueError(f"eos_update: tok int64 [{B}], done int32 [{B}], n_done int32 [1]")
    if not tok.is_cuda:
        raise L.GearError("gear_amd operators run on the GPU only (tensor is on %s); there is no CPU fallback" % tok.device)
    _same_device("eos_update", tok, tok, done, n_done)
    arr = (C.c_int * max(len(ids), 1))(*ids)
    rc = L.load().gear_eos_update(L.ptr(tok), L.ptr(done), B, C.cast(arr, C.c_void_p), len(ids), int(pad_token_id), L.ptr(n_done),
                                  L.stream_ptr(tok))
    L.check(rc, "gear_eos_update")
