"""Token sampling for the decoders: temperature, top-k, top-p (HF's warper order) and the accept / residual rule of speculative
sampling, in one launch per call (csrc/sample.hip, gear_sample_tokens).

The draws come from Philox4x32-10 keyed by the seed and counted by (position, sequence, purpose): a token is a pure function of
(seed, sequence, position, logits).  Graph replays and eager steps therefore draw the same tokens, head-sharded ranks that hold the
same logits agree without talking, and a rerun with the same seed reproduces a generation."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib as L


@dataclass(frozen=True)
class SamplingParams:
    """temperature 0 = greedy (argmax, first index); top_k 0 (or >= vocab) = off; top_p 1 = off; seed keys the random stream."""
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0

    def __post_init__(self):
        t, k, p, s = self.temperature, self.top_k, self.top_p, self.seed
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not t >= 0 or t == float("inf"):
            raise ValueError(f"SamplingParams: temperature must be a finite number >= 0, got {t!r}")
        if isinstance(k, bool) or not isinstance(k, int) or k < 0:
            raise ValueError(f"SamplingParams: top_k must be an int >= 0, got {k!r}")
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0 < p <= 1:
            raise ValueError(f"SamplingParams: top_p must be in (0, 1], got {p!r}")
        if isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < 2 ** 64:
            raise ValueError(f"SamplingParams: seed must be an int in [0, 2^64), got {s!r}")

    @property
    def greedy(self) -> bool:
        return self.temperature == 0

    def c_struct(self) -> L.SampleParamsC:
        return L.SampleParamsC(float(self.temperature), int(self.top_k), float(self.top_p), 0, int(self.seed))


def sample_tokens(logits: torch.Tensor, params: SamplingParams, pos: int = 0, n_per_seq: int = 1, draft: torch.Tensor = None,
                  u: torch.Tensor = None, pos_dev: torch.Tensor = None):
    """logits [R, V] fp16 / fp32 (rows may be strided, columns contiguous) -> (tokens int64 [R], accepted int32 [R],
    logprobs float32 [R]).

    Row r is sequence r // n_per_seq at position pos + r % n_per_seq (+ pos_dev[0] when pos_dev, a device int32 tensor, is given --
    the decoders pass their device-side state).  draft int64 [R] (-1 = none): the row's drafted token, accepted with probability
    p(d), else the row draws from p without d.  u float32 [R, 2]: (draw, accept) uniforms instead of the generator (tests).
    One launch, no synchronisation, no host reads: capturable in a graph."""
    if not isinstance(params, SamplingParams):
        raise TypeError(f"sample_tokens: params must be a SamplingParams, got {type(params).__name__}")
    if logits.dim() != 2:
        raise ValueError(f"sample_tokens: logits must be [rows, V], got {list(logits.shape)}")
    if logits.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"sample_tokens: logits must be fp16 or fp32, got {logits.dtype}")
    R, V = logits.shape
    if not logits.is_cuda:
        raise L.GearError("gear_amd operators run on the GPU only (tensor is on %s); there is no CPU fallback" % logits.device)
    if logits.stride(1) != 1:
        raise L.GearError("sample_tokens: logits columns must be contiguous")
    if draft is not None:
        if draft.dtype != torch.int64 or draft.numel() != R:
            raise ValueError(f"sample_tokens: draft must be int64 with {R} entries")
        draft = draft.reshape(R)
    if u is not None:
        if u.dtype != torch.float32 or tuple(u.shape) != (R, 2):
            raise ValueError(f"sample_tokens: u must be float32 [{R}, 2]")
    if pos_dev is not None and (pos_dev.dtype != torch.int32 or pos_dev.numel() < 1):
        raise ValueError("sample_tokens: pos_dev must be a device int32 tensor")
    L.require_gpu(draft, u, pos_dev)
    for t in (draft, u, pos_dev):
        if t is not None and t.device != logits.device:
            raise L.GearError(f"gear_amd operators need all tensors on one device (got {logits.device} and {t.device})")
    tokens = torch.empty(R, dtype=torch.int64, device=logits.device)
    accepted = torch.empty(R, dtype=torch.int32, device=logits.device)
    logprobs = torch.empty(R, dtype=torch.float32, device=logits.device)
    p = params.c_struct()
    rc = L.load().gear_sample_tokens(L.ptr(logits), int(logits.dtype == torch.float32), R, V, logits.stride(0), int(n_per_seq),
                                     C.byref(p), L.ptr(pos_dev), int(pos), L.ptr(draft), L.ptr(u), L.ptr(tokens), L.ptr(accepted),
                                     L.ptr(logprobs), L.stream_ptr(logits))
    L.check(rc, "gear_sample_tokens")
    return tokens, accepted, logprobs
