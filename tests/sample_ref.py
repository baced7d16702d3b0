"""Float64 reference of gear_sample_tokens (include/gear_hip.h): Philox4x32-10, HF's warper order (temperature, top-k, top-p), the
index-order draw and the one-hot-drafter accept / residual rule.  numpy only (no GPU, no scipy)."""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Random123's Philox4x32 with 10 rounds: counter 4 x uint32, key 2 x uint32 -> 4 x uint32."""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform(seed: int, P: int, b: int, purpose: int) -> float:
    """The sampler's uniform: (out[0] >> 8) 2^-24 of counter (P, b, purpose, 0), key (seed lo, seed hi); purpose 0 = draw, 1 = accept."""
    o = philox4x32_10((P, b, purpose, 0), (seed & M32, (seed >> 32) & M32))
    return (o[0] >> 8) * 2.0 ** -24


def scaled(logits_row, temperature: float) -> np.ndarray:
    """x = fp32(logit) / temperature, correctly rounded in fp32."""
    return np.asarray(logits_row, dtype=np.float32) / np.float32(temperature)


def kept_mask(x: np.ndarray, top_k: int, top_p: float) -> np.ndarray:
    """The filtered set: finite x; top-k keeps x >= the k-th largest (edge ties kept); top-p keeps x_i iff the softmax mass (over the
    set kept so far) of the values strictly greater than x_i is < top_p."""
    x = np.asarray(x, dtype=np.float64)
    keep = np.isfinite(x)
    V = x.shape[0]
    if 0 < top_k < V and keep.sum() > top_k:
        kth = np.sort(x[keep])[::-1][top_k - 1]
        keep &= x >= kth
    if top_p < 1.0:
        e = np.where(keep, np.exp(x - x[keep].max()), 0.0)
        p = e / e.sum()
        vals = np.unique(x[keep])[::-1]                          # distinct kept values, descending
        mass = np.array([p[keep & (x == v)].sum() for v in vals])
        above = np.concatenate([[0.0], np.cumsum(mass)[:-1]])    # mass of the values strictly greater
        ok = {float(v) for v, a in zip(vals, above) if a < top_p}
        keep &= np.array([float(v) in ok for v in x])
    return keep


def probs(x: np.ndarray, keep: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    e = np.where(keep, np.exp(x - x[keep].max()), 0.0)
    return e / e.sum()


def intervals(x: np.ndarray, keep: np.ndarray, exclude: int = -1):
    """(index, lo, hi) per kept token (minus `exclude`) with positive mass: the draw u in [lo, hi) picks that token."""
    x = np.asarray(x, dtype=np.float64)
    e = np.where(keep, np.exp(x - x[keep].max()), 0.0)
    if 0 <= exclude < e.shape[0]:
        e[exclude] = 0.0
    Z = e.sum()
    c = np.cumsum(e) / Z
    out, lo = [], 0.0
    for i in np.nonzero(e > 0)[0]:
        out.append((int(i), lo, float(c[i])))
        lo = float(c[i])
    return out


def sample_row(logits_row, temperature: float, top_k: int, top_p: float, u_draw: float, u_acc: float = 0.0, draft: int = -1):
    """-> (token, accepted, logprob) of one row, the semantics of gear_sample_tokens in float64."""
    raw = np.asarray(logits_row, dtype=np.float32)
    if temperature == 0:
        tok = int(np.argmax(raw))
        return tok, int(draft >= 0 and draft == tok), 0.0
    x = scaled(raw, temperature)
    keep = kept_mask(x, top_k, top_p)
    p = probs(x, keep)
    if draft >= 0:
        pd = p[draft] if draft < p.shape[0] else 0.0
        if u_acc < pd:
            return int(draft), 1, float(np.log(pd))
    xd = np.asarray(x, dtype=np.float64)
    e = np.where(keep, np.exp(xd - xd[keep].max()), 0.0)
    if 0 <= draft < e.shape[0]:
        e[draft] = 0.0
    c = np.cumsum(e)
    tok = int(np.argmax(c > u_draw * e.sum()))
    return tok, 0, float(np.log(p[tok]))
