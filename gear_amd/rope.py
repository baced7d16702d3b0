"""RoPE scaling (config.rope_scaling) for every RoPE path: the inverse-frequency table of the scaled types whose table does not
depend on the running length -- "linear", "llama3" (Llama-3.1 / 3.2) and "yarn" -- computed in fp32 the way transformers'
modeling_rope_utils does, and the rotary module that serves the dense paths (prefill, extend, verify) from that table.  The token
step reads the same table on the device (the gear_*_freq entry points, include/gear_hip.h).  Pure host code: no GPU needed."""
from __future__ import annotations

import math

import torch
from torch import nn

SUPPORTED = ("default", "linear", "llama3", "yarn")


def _number(rs: dict, key: str, kind: str, default=None, positive: bool = True) -> float:
    v = rs.get(key, default)
    if v is None:
        raise ValueError(f"rope_scaling type {kind!r}: {key!r} is missing")
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (positive and v <= 0):
        raise ValueError(f"rope_scaling type {kind!r}: {key!r} must be a positive number (got {v!r})")
    return float(v)


def rope_parameters(config, head_dim: int = 128):
    """(inv_freq fp32 [head_dim / 2] | None, attention_factor) of config.rope_theta / config.rope_scaling.

    (None, 1.0) for no scaling or the type "default": the callers then keep the theta code path.  "linear", "llama3" and "yarn"
    give transformers' table (fp32 arithmetic); "dynamic", "longrope" and unknown types raise ValueError (their table depends on
    the running length), as do missing or non-positive parameters."""
    rs = getattr(config, "rope_scaling", None)
    if rs is None:
        return None, 1.0
    if not isinstance(rs, dict):
        raise ValueError(f"rope_scaling must be a dict or None (got {type(rs).__name__})")
    kind = rs.get("rope_type", rs.get("type"))
    if kind is None or kind == "default":
        return None, 1.0
    if kind not in SUPPORTED:
        raise ValueError(f"rope_scaling type {kind!r} is not supported (supported: {', '.join(SUPPORTED)}): 'dynamic' and 'longrope' "
                         "tables depend on the running length")
    base = getattr(config, "rope_theta", None)
    if base is None or not math.isfinite(base) or base <= 0:
        raise ValueError(f"rope_scaling type {kind!r}: rope_theta must be positive (got {base!r})")
    D = int(head_dim)
    if D <= 0 or D % 2:
        raise ValueError(f"rope_scaling type {kind!r}: head_dim must be a positive even number (got {head_dim})")
    factor = _number(rs, "factor", kind)
    inv = 1.0 / (float(base) ** (torch.arange(0, D, 2, dtype=torch.int64, device="cpu").float() / D))
    if kind == "linear":
        return inv / factor, 1.0
    if kind == "llama3":
        orig = _number(rs, "original_max_position_embeddings", kind)
        lo = _number(rs, "low_freq_factor", kind)
        hi = _number(rs, "high_freq_factor", kind)
        if hi <= lo:
            raise ValueError(f"rope_scaling type 'llama3': high_freq_factor ({hi}) must exceed low_freq_factor ({lo})")
        wl = 2 * math.pi / inv
        out = torch.where(wl > orig / lo, inv / factor, inv)
        s = (orig / wl - lo) / (hi - lo)
        smoothed = (1 - s) * inv / factor + s * inv
        medium = ~(wl < orig / hi) & ~(wl > orig / lo)
        return torch.where(medium, smoothed, out), 1.0
    # yarn
    for k in ("mscale", "mscale_all_dim"):
        if rs.get(k) is not None:
            raise ValueError(f"rope_scaling type 'yarn': {k!r} is not supported (give 'attention_factor')")
    orig = _number(rs, "original_max_position_embeddings", kind, getattr(config, "max_position_embeddings", None))
    beta_fast = _number(rs, "beta_fast", kind, 32)
    beta_slow = _number(rs, "beta_slow", kind, 1)
    if rs.get("attention_factor") is not None:
        attention_factor = _number(rs, "attention_factor", kind)
    else:
        attention_factor = 0.1 * math.log(factor) + 1.0
        if attention_factor <= 0:
            raise ValueError(f"rope_scaling type 'yarn': factor {factor} gives the attention factor {attention_factor}")

    def cd(n):
        return D * math.log(orig / (2 * math.pi * n)) / (2 * math.log(base))

    low, high = max(math.floor(cd(beta_fast)), 0), min(math.ceil(cd(beta_slow)), D - 1)
    if low == high:
        high += 0.001
    ramp = torch.clamp((torch.arange(D // 2, dtype=torch.float32, device="cpu") - low) / (high - low), 0, 1)
    return (inv / factor) * ramp + inv * (1 - ramp), float(attention_factor)


class ScaledRotaryEmbedding(nn.Module):
    """LlamaRotaryEmbedding's forward over a given table: cos / sin of position x inv_freq, times the attention factor in fp32,
    then the cast (transformers' order).  The table is no buffer: model.half() must not round it to fp16.  It is kept in fp32 on
    the host, with one copy per device made at first use (table())."""

    def __init__(self, dim, inv_freq, attention_factor: float = 1.0):
        super().__init__()
        inv_freq = torch.as_tensor(inv_freq, dtype=torch.float32).detach().cpu().clone()
        if inv_freq.shape != (dim // 2,):
            raise ValueError(f"inv_freq must hold dim / 2 = {dim // 2} values (got {list(inv_freq.shape)})")
        self.dim, self.attention_factor = dim, float(attention_factor)
        self.inv_freq = inv_freq
        self._on = {}

    def table(self, device) -> torch.Tensor:
        """The fp32 table on `device` (what the gear_*_freq entry points read; a captured graph keeps this tensor's pointer)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.inv_freq.to(device).contiguous()
        return t

    @torch.no_grad()
    def forward(self, x, position_ids):
        freqs = position_ids[:, :, None].float() * self.table(x.device)[None, None, :]
        emb = torch.cat((freqs, freqs), dim=-1)
        return (emb.cos() * self.attention_factor).to(x.dtype), (emb.sin() * self.attention_factor).to(x.dtype)


def rotary_embedding(config, head_dim: int, plain):
    """The rotary module of an attention layer: `plain()` (the unscaled module) when the config does not scale, the scaled one
    otherwise."""
    inv_freq, attention_factor = rope_parameters(config, head_dim)
    if inv_freq is None:
        return plain()
    return ScaledRotaryEmbedding(head_dim, inv_freq, attention_factor)


def device_table(rotary, device):
    """(fp32 device table, attention factor) for the gear_*_freq entry points, or None for an unscaled module."""
    if not isinstance(rotary, ScaledRotaryEmbedding):
        return None
    return rotary.table(device), rotary.attention_factor
