"""numpy restatement of gear_logits_process (include/gear_hip.h): bias, repetition penalty, n-gram ban and the minimum-length EOS ban
of ONE row, in HF's processor order.  For every entry it returns the admissible set {round(fp32 path), round(float64-exact result)}:
the kernel computes in fp32 and rounds once, so its value must be the first; the second is allowed where fp32 arithmetic followed by
the rounding to fp16 lands on the other neighbour (double rounding)."""
import numpy as np


def seen_tokens(hist, n, V):
    """distinct in-range tokens of hist[0 .. n)"""
    h = np.asarray(hist[:n], dtype=np.int64)
    return np.unique(h[(h >= 0) & (h < V)])


def ngram_banned(hist, n, g, V):
    """HF NoRepeatNGramLogitsProcessor: tokens that would complete an n-gram already in hist[0 .. n)."""
    if g <= 0 or n < g:
        return np.zeros(0, dtype=np.int64)
    h = [int(t) for t in hist[:n]]
    tail = h[n - g + 1:n]
    out = {h[i + g - 1] for i in range(n - g + 1) if h[i:i + g - 1] == tail}
    return np.array(sorted(t for t in out if 0 <= t < V), dtype=np.int64)


def process_row(x, hist, n, prompt_len, penalty=1.0, ngram=0, min_new=0, eos=(), bias=()):
    """x: one row, float16 or float32.  hist: ints, n of them live.  bias: (token, bias) pairs, unique tokens.
    -> (a, b, touched): a = the fp32 path rounded once to x.dtype, b = the float64 result rounded once, touched = bool mask of the
    entries some processor addresses (every other entry must come out with the bits of x)."""
    x = np.asarray(x)
    V = x.shape[0]
    touched = np.zeros(V, dtype=bool)
    v32, v64 = x.astype(np.float32), x.astype(np.float64)
    p32 = np.float32(penalty)
    with np.errstate(all="ignore"):
        for t, b in bias:
            if 0 <= t < V:
                v32[t] = v32[t] + np.float32(b)
                v64[t] = v64[t] + np.float64(np.float32(b))
                touched[t] = True
        if penalty != 1.0:
            s = seen_tokens(hist, n, V)
            v32[s] = np.where(v32[s] < 0, v32[s] * p32, v32[s] / p32)
            v64[s] = np.where(v64[s] < 0, v64[s] * np.float64(p32), v64[s] / np.float64(p32))
            touched[s] = True
        banned = [ngram_banned(hist, n, ngram, V)]
        if n - prompt_len < min_new:
            banned.append(np.array([e for e in eos if 0 <= e < V], dtype=np.int64))
        for bn in banned:
            v32[bn] = -np.inf
            v64[bn] = -np.inf
            touched[bn] = True
        return v32.astype(x.dtype), v64.astype(x.dtype), touched


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def check_row(got, x, a, b, touched):
    """None when `got` is admissible, else a message naming the first bad entry."""
    g, xb, ab, bb = bits(got), bits(x), bits(a), bits(b)
    bad = np.where(touched, (g != ab) & (g != bb), g != xb)
    if not bad.any():
        return None
    j = int(np.flatnonzero(bad)[0])
    return (f"entry {j}: got {got[j]!r} (bits {int(g[j]):#x}), input {x[j]!r}, admissible {a[j]!r} / {b[j]!r}, "
            f"touched {bool(touched[j])}; {int(bad.sum())} bad entries")
