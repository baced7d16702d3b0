"""Attention probes: a float64 reference of the decode / extend attention kernels with the reconstruction's parts kept apart, the
mutations of that reference that stand for one-token kernel bugs, and queries aimed so that each such bug moves the output or the
LSE far past rounding noise.

Gaussian q over a Gaussian cache gives a nearly flat softmax: one dropped token, one outlier on the wrong head or one piece with
its neighbour's factors barely moves the whole output.  An aimed query makes one (or two) keys outweigh all others by e^12: the
output row then reads that key's V-hat row and the LSE reads its score, so an error at that key is an O(1) error of the row.

Parts (decompose): float64 numpy arrays, nothing added up yet --
  Kd, Vd       [B,H,T,D]  dequantized backbone
  kQ, vQ       [B,H,T,r]  token-side factors; kP, vP [nseg,B,H,D,r] channel-side factors per segment (None: no low-rank term)
  seg          [T]        factor segment of each token (segment 0 = tokens [0, seg0), then one per `seglen` tokens)
  ko_t, ko_v   [B,H,D,2,L] K outlier token (-1: unused slot) and stored value per (channel, side) list
  vo_c, vo_v   [B,T,2,L]  V outlier column h * D + d (-1: unused) and stored value per (token row, side) list
  ko_lr, vo_lr            1.0 where the low-rank term goes on top of a stored outlier (as the kernels do)
  kw, vw       [B,H,W,D]  fp16 window;  kn, vn [B,H,n,D] chunk rows of an extend call (n = 0: decode)
  T, W, n, seg0, seglen
and the softmax plan the mutations act on: drop (key positions left out), causal (shift of the causal edge), gqa ("div" / "mod"),
norescale (a key range merged without its max rescale), lse ("exact" / "no_logL" / "log2").

Keys are numbered 0 .. T-1 (compressed), T .. T+W-1 (window), T+W .. T+W+n-1 (chunk rows); query row i of an extend call sees
keys < T + W + i + 1, a decode query (n = 0) sees all T + W.
"""
from __future__ import annotations

import math

import numpy as np

D = 128
QSCALE = 1.0 / math.sqrt(D)

# Bounds of the probe metrics (row_err: relative to the row's max-norm; lse_err: absolute, natural log).  Set between the
# fp16-shaped reference (K-hat, V-hat, P and the output rounded where a kernel rounds them: test_attn_probe_sensitivity holds it
# at <= BOUND / 3) and the one-token mutations (>= 5 x BOUND on the same probes).
ROW_BOUND = 1e-2
LSE_BOUND = 4e-2
ROW_FLOOR = 1e-2          # row_err denominator floor (a row that is all but zero)
DOMINANCE = 12.0          # an aimed key outweighs all others by at least e^12
Q_MAX = 48.0              # largest element of an aimed q (the scores' fp16 rounding noise grows with it)


def f16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def _host(t):
    if t is None:
        return None
    if hasattr(t, "detach"):
        return t.detach().cpu().numpy()
    return np.asarray(t)


def _unpack(code, bits, dim):
    from oracle import oracle as orc
    return orc.unpack_tensor(code, bits, dim).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------- decompose
def _payload_side(p):
    """One gear_amd.compress.Payload -> (deq [B,H,T,D], Q [B,H,T,r] | None, P [1,B,H,D,r] | None, outlier arrays)."""
    B, H, T, Dd = p.shape
    code, scale, mn = _host(p.code), _host(p.scale).astype(np.float64), _host(p.mn).astype(np.float64)
    q = _unpack(code, p.bits, 3)
    deq = q * np.repeat(scale, p.group, axis=3) + np.repeat(mn, p.group, axis=3)
    if p.kind == "k":
        deq = deq.transpose(0, 1, 3, 2)
    Q = P = None
    if p.P is not None:
        Q, P = _host(p.Q).astype(np.float64), _host(p.P).astype(np.float64)[None]
    o_i = o_v = None
    if p.oidx is not None and p.k_out:
        oi = _host(p.oidx).astype(np.int64) & 0xFFFF
        ov = _host(p.oval).astype(np.float64)
        if p.kind == "k":        # [B,H,D,2k] token indices, side 0 then side 1
            o_i, o_v = oi.reshape(B, H, Dd, 2, -1), ov.reshape(B, H, Dd, 2, -1)
        else:                    # [B,T,2k] columns h * D + d
            o_i, o_v = oi.reshape(B, T, 2, -1), ov.reshape(B, T, 2, -1)
            o_i = np.where(o_i < H * Dd, o_i, -1)
    return deq, Q, P, o_i, o_v


def _empty_lists(shape):
    return np.full(shape + (0,), -1, np.int64), np.zeros(shape + (0,))


def _finish(parts):
    B, H, T = parts["Kd"].shape[:3]
    if parts["ko_t"] is None:
        parts["ko_t"], parts["ko_v"] = _empty_lists((B, H, D, 2))
    if parts["vo_c"] is None:
        parts["vo_c"], parts["vo_v"] = _empty_lists((B, T, 2))
    parts["ko_lr"] = np.ones(parts["ko_t"].shape)
    parts["vo_lr"] = np.ones(parts["vo_c"].shape)
    for nm in ("kw", "vw", "kn", "vn"):
        if parts.get(nm) is None:
            parts[nm] = np.zeros((B, H, 0, D))
        parts[nm] = np.asarray(parts[nm], np.float64)
    parts.update(T=T, W=parts["kw"].shape[2], n=parts["kn"].shape[2], drop=(), causal=0, gqa="div", norescale=None,
                 lse="exact")
    return parts


def window_parts(kw, vw):
    """parts of a plain fp16 cache (no compressed tokens): every key a window row."""
    kw, vw = _host(kw).astype(np.float64), _host(vw).astype(np.float64)
    B, H = kw.shape[:2]
    z = np.zeros((B, H, 0, D))
    return _finish(dict(Kd=z, Vd=z, kQ=None, kP=None, vQ=None, vP=None, seg=np.zeros(0, np.int64), seg0=0, seglen=0, ko_t=None,
                        ko_v=None, vo_c=None, vo_v=None, kw=kw, vw=vw, kn=None, vn=None))


def decompose(src, kw=None, vw=None, kn=None, vn=None):
    """(pk, pv) plain payloads or a GearKVCache -> parts (see the module docstring).  kw / vw: the window of a plain-payload call
    (a cache brings its own); kn / vn: chunk rows of an extend call."""
    if isinstance(src, tuple):
        pk, pv = src
        Kd, kQ, kP, ko_t, ko_v = _payload_side(pk)
        Vd, vQ, vP, vo_c, vo_v = _payload_side(pv)
        T = Kd.shape[2]
        parts = dict(Kd=Kd, Vd=Vd, kQ=kQ, kP=kP, vQ=vQ, vP=vP, seg=np.zeros(T, np.int64), seg0=T, seglen=0,
                     ko_t=ko_t, ko_v=ko_v, vo_c=vo_c, vo_v=vo_v, kw=_host(kw), vw=_host(vw), kn=_host(kn), vn=_host(vn))
        return _finish(parts)
    c = src
    n, g, b = c.n_comp, c.group, c.bits
    fpi = 32 // b
    Kd = (_unpack(_host(c.kcode[:, :, :, :n // fpi]), b, 3) * np.repeat(_host(c.kscale[:, :, :, :n // g]).astype(np.float64), g, 3)
          + np.repeat(_host(c.kmn[:, :, :, :n // g]).astype(np.float64), g, 3)).transpose(0, 1, 3, 2)
    Vd = (_unpack(_host(c.vcode[:, :, :n]), b, 3) * np.repeat(_host(c.vscale[:, :, :n]).astype(np.float64), g, 3)
          + np.repeat(_host(c.vmn[:, :, :n]).astype(np.float64), g, 3))
    seg = np.array([c._segment_of(t) for t in range(n)], np.int64)
    parts = dict(Kd=Kd, Vd=Vd, kQ=None, kP=None, vQ=None, vP=None, seg=seg, seg0=c.seg0, seglen=c.R, ko_t=None, ko_v=None,
                 vo_c=None, vo_v=None, kw=_host(c.kwin[:, :, :c.n_win]), vw=_host(c.vwin[:, :, :c.n_win]), kn=_host(kn),
                 vn=_host(vn))
    if c.lowrank:
        nseg = int(seg.max()) + 1 if n else 1
        parts.update(kQ=_host(c.kQtok[:, :, :n]).astype(np.float64), kP=_host(c.kPseg[:nseg]).astype(np.float64),
                     vQ=_host(c.vQtok[:, :, :n]).astype(np.float64), vP=_host(c.vPseg[:nseg]).astype(np.float64))
    if c.kk_blk and n:
        klen = c.kk0 + ((n - c.seg0) // c.R) * c.kk_blk
        parts["ko_t"] = _host(c.koidx[..., :klen]).astype(np.int64) & 0xFFFF
        parts["ko_v"] = _host(c.koval[..., :klen]).astype(np.float64)
    if c.kv and n:
        oi = _host(c.voidx[:, :n]).astype(np.int64) & 0xFFFF
        parts["vo_c"] = np.where(oi < c.H * D, oi, -1).reshape(c.B, n, 2, -1)
        parts["vo_v"] = _host(c.voval[:, :n]).astype(np.float64).reshape(c.B, n, 2, -1)
    return _finish(parts)


# ------------------------------------------------------------------------------------------------------------ assemble
def lowrank_term(parts, side):
    """[B,H,T,D] low-rank term, each token with the channel factors of its own segment (parts["seg"])."""
    Q, P = parts[side + "Q"], parts[side + "P"]
    out = np.zeros(parts[side.upper() + "d"].shape)
    if Q is None or Q.shape[-1] == 0:
        return out
    for s in np.unique(parts["seg"]):
        m = parts["seg"] == s
        out[:, :, m] = Q[:, :, m] @ P[s].transpose(0, 1, 3, 2)
    return out


def _k_entries(parts):
    t = parts["ko_t"]
    b, h, d, s, i = np.nonzero(t >= 0)
    return b, h, t[b, h, d, s, i], d, parts["ko_v"][b, h, d, s, i], parts["ko_lr"][b, h, d, s, i]


def _v_entries(parts):
    c = parts["vo_c"]
    b, t, s, i = np.nonzero(c >= 0)
    col = c[b, t, s, i]
    return b, col // D, t, col % D, parts["vo_v"][b, t, s, i], parts["vo_lr"][b, t, s, i]


def assemble(parts, fp16=False):
    """K-hat, V-hat [B,H,T,D]: dequant + low-rank term; a stored outlier replaces the dequantized value, the low-rank term on top.
    fp16=True: what the kernels' tiles hold -- every element rounded to fp16; an outlier element either rounded to fp16 (the extend
    kernel's tile) or as deq + lr + fp16(value - deq) (the decode kernels' sparse-tile delta), whichever lies farther off."""
    return _assemble_side(parts, "k", fp16), _assemble_side(parts, "v", fp16)


def _assemble_side(parts, side, fp16=False):
    entries = _k_entries if side == "k" else _v_entries
    deq = parts[side.upper() + "d"]
    lr = lowrank_term(parts, side)
    x = deq + lr
    b, h, t, d, val, onlr = entries(parts)
    exact = val + onlr * lr[b, h, t, d]
    if fp16:
        x = f16(x)
        tile = f16(exact)                                                    # the extend kernel's fp16 tile element
        delta = deq[b, h, t, d] + onlr * lr[b, h, t, d] + f16(val - deq[b, h, t, d])   # decode: fp16 sparse-tile delta
        x[b, h, t, d] = np.where(np.abs(tile - exact) >= np.abs(delta - exact), tile, delta)
    else:
        x[b, h, t, d] = exact
    return x


def reconstruct_payload(p):
    """One plain Payload -> float64 [B,H,T,D]: dequant + Q P^T, an outlier entry = its stored value + Q P^T."""
    deq, Q, P, oi, ov = _payload_side(p)
    B, H, T, _ = deq.shape
    side = p.kind
    parts = {side.upper() + "d": deq, side + "Q": Q, side + "P": P, "seg": np.zeros(T, np.int64)}
    if side == "k":
        parts["ko_t"], parts["ko_v"] = (oi, ov) if oi is not None else _empty_lists((B, H, D, 2))
        parts["ko_lr"] = np.ones(parts["ko_t"].shape)
    else:
        parts["vo_c"], parts["vo_v"] = (oi, ov) if oi is not None else _empty_lists((B, T, 2))
        parts["vo_lr"] = np.ones(parts["vo_c"].shape)
    return _assemble_side(parts, side)


def reconstruct_cache(c):
    """A GearKVCache -> float64 K-hat, V-hat [B,H,n_comp,D] of its compressed tokens (per-segment factors)."""
    return assemble(decompose(c))


def keys(parts, fp16=False):
    """All keys / values of the call: [B,H,T+W+n,D] (compressed, window, chunk rows)."""
    K, V = assemble(parts, fp16)
    return (np.concatenate([K, parts["kw"], parts["kn"]], 2), np.concatenate([V, parts["vw"], parts["vn"]], 2))


# ----------------------------------------------------------------------------------------------------------- reference
def head_map(parts, Hq, Hkv):
    G = Hq // Hkv
    return np.arange(Hq) % Hkv if parts["gqa"] == "mod" else np.arange(Hq) // G


def ref(q, parts, fp16=False, rows=None, kv=None):
    """float64 attention of q [B,Hq,nq,D] over the parts -> (out [B,Hq,nq,D], lse [B,Hq,nq]).  nq = n for an extend call (query
    row i sees keys < T + W + i + 1) or 1 for decode (n = 0: every key).  rows: the query rows of the call the nq rows of q are
    (default 0 .. nq-1).  fp16=True: the noise model -- K-hat / V-hat as the tiles hold them, P and the output rounded to fp16.
    kv: keys(parts, fp16) when the caller already has it."""
    q = np.asarray(q, np.float64)
    B, Hq, nq, _ = q.shape
    Kall, Vall = kv if kv is not None else keys(parts, fp16)
    Hkv, S = Kall.shape[1], Kall.shape[2]
    T, W, n = parts["T"], parts["W"], parts["n"]
    rows = np.arange(nq) if rows is None else np.asarray(rows)
    vis = np.ones((nq, S), bool)
    if n:
        vis = np.arange(S)[None, :] < (T + W + rows + 1 + parts["causal"])[:, None]
    if len(parts["drop"]):
        vis[:, list(parts["drop"])] = False
    hm = head_map(parts, Hq, Hkv)
    out = np.zeros((B, Hq, nq, D))
    lse = np.zeros((B, Hq, nq))
    step = max(1, (1 << 22) // max(1, S * Hq))
    for b in range(B):
        Kb, Vb = Kall[b, hm], Vall[b, hm]                                    # [Hq,S,D]
        for r0 in range(0, nq, step):
            r1 = min(nq, r0 + step)
            s = np.matmul(q[b, :, r0:r1], Kb.transpose(0, 2, 1)) * QSCALE     # [Hq,r,S]
            s = np.where(vis[None, r0:r1], s, -np.inf)
            M = s.max(-1, keepdims=True)
            if parts["norescale"] is not None:                  # one split merged as if its max were the global one
                a, e = parts["norescale"]
                Ms = s[..., a:e].max(-1, keepdims=True)
                Ms = np.where(np.isfinite(Ms), Ms, M)
                shift = np.broadcast_to(M, s.shape).copy()
                shift[..., a:e] = np.broadcast_to(Ms, shift[..., a:e].shape)
                p = np.exp(s - shift)
            else:
                p = np.exp(s - M)
            L = p.sum(-1, keepdims=True)
            if fp16:
                p = f16(p)
            o = np.matmul(p, Vb) / L
            out[b, :, r0:r1] = f16(o) if fp16 else o
            l = (M + np.log(L))[..., 0]
            if parts["lse"] == "no_logL":
                l = M[..., 0]
            elif parts["lse"] == "log2":
                l = l / math.log(2.0)
            lse[b, :, r0:r1] = l
    return out, lse


# ----------------------------------------------------------------------------------------------------------- mutations
MUTATIONS = ("M1-drop", "M2-lose-own", "M2-gain-next", "M3-k-outlier", "M4-v-ignored", "M4-v-head+1", "M4-v-head-1",
             "M5-seg+1", "M5-seg-1", "M6-k-no-lr", "M6-v-no-lr", "M7-no-rescale", "M8-gqa-mod", "M9-no-logL", "M9-log2")


def mutate(parts, kind, where=None):
    """A changed copy of the reference's inputs standing for one kernel bug (see MUTATIONS):
    M1-drop: key position `where` left out of the softmax.  M2-lose-own / -gain-next: the causal edge one key early / late.
    M3-k-outlier: K list entry `where` = (b, h, d, side, i) keeps the dequantized value.  M4-v-*: V list entry (b, t, side, i)
    ignored or applied to head hkv +- 1.  M5-seg+-1: 64-token piece `where` takes the factors of the neighbouring segment.
    M6-k/v-no-lr: list entry `where` without the low-rank term on top.  M7-no-rescale: key range `where` = (a, e) merged without
    its max rescale.  M8-gqa-mod: query head hq reads KV head hq % Hkv.  M9-*: LSE without log L / in base 2."""
    m = dict(parts)
    if kind == "M1-drop":
        m["drop"] = tuple(parts["drop"]) + (int(where),)
    elif kind == "M2-lose-own":
        m["causal"] = -1
    elif kind == "M2-gain-next":
        m["causal"] = 1
    elif kind == "M3-k-outlier":
        m["ko_t"] = parts["ko_t"].copy()
        m["ko_t"][tuple(where)] = -1
    elif kind.startswith("M4-v"):
        b, t, s, i = where
        col = int(parts["vo_c"][b, t, s, i])
        m["vo_c"] = parts["vo_c"].copy()
        if kind == "M4-v-ignored":
            m["vo_c"][b, t, s, i] = -1
        else:
            m["vo_c"][b, t, s, i] = col + (D if kind.endswith("+1") else -D)
    elif kind.startswith("M5-seg"):
        m["seg"] = parts["seg"].copy()
        m["seg"][64 * where:64 * where + 64] += 1 if kind.endswith("+1") else -1
    elif kind == "M6-k-no-lr":
        m["ko_lr"] = parts["ko_lr"].copy()
        m["ko_lr"][tuple(where)] = 0.0
    elif kind == "M6-v-no-lr":
        m["vo_lr"] = parts["vo_lr"].copy()
        m["vo_lr"][tuple(where)] = 0.0
    elif kind == "M7-no-rescale":
        m["norescale"] = tuple(where)
    elif kind == "M8-gqa-mod":
        m["gqa"] = "mod"
    elif kind == "M9-no-logL":
        m["lse"] = "no_logL"
    elif kind == "M9-log2":
        m["lse"] = "log2"
    else:
        raise ValueError(kind)
    return m


# ------------------------------------------------------------------------------------------------------------- metrics
def row_err(out, ref_out, floor=ROW_FLOOR):
    out, ref_out = np.asarray(out, np.float64), np.asarray(ref_out, np.float64)
    den = np.maximum(np.abs(ref_out).max(-1), floor)
    return float((np.abs(out - ref_out).max(-1) / den).max())


def lse_err(lse, ref_lse):
    return float(np.abs(np.asarray(lse, np.float64) - np.asarray(ref_lse, np.float64)).max())


def signal(out, lse, ref_out, ref_lse):
    """max(row_err / ROW_BOUND, lse_err / LSE_BOUND): how far past the bounds a result lies."""
    return max(row_err(out, ref_out) / ROW_BOUND, lse_err(lse, ref_lse) / LSE_BOUND)


# -------------------------------------------------------------------------------------------------------------- probes
def probe_positions(parts, b=0, h=0):
    """Key positions worth aiming at: every 64k-1 / 64k pair below T, the segment edges, the first and last window row, the
    chunk rows, a sample of every K list side (prompt segment, decode-time blocks) and the rows whose V outliers fall in head h."""
    T, W, n, seg = parts["T"], parts["W"], parts["n"], parts["seg"]
    pos = {0, T - 1} if T else set()
    for k in range(1, (T + W + n + 63) // 64):
        pos |= {64 * k - 1, 64 * k}
    for s in np.unique(seg) if T else ():
        ts = np.nonzero(seg == s)[0]
        pos |= {int(ts[0]), int(ts[-1])}
    if W:
        pos |= {T, T + W - 1}
    if n:
        pos |= {T + W, T + W + n // 2, T + W + n - 1}
    pos |= {int(t) for t, _ in k_outlier_sample(parts, b, h)}
    pos |= {int(t) for t, _ in v_outlier_sample(parts, b, h)}
    return sorted(p for p in pos if 0 <= p < T + W + n)


def k_outlier_sample(parts, b, h, per_class=3):
    """[(token, (b, h, d, side, i))]: up to per_class entries of each list side in the prompt segment and in the decode blocks,
    the ones whose value lies farthest from the dequantized one."""
    t = parts["ko_t"][b, h]
    out = []
    for side in (0, 1):
        for prompt in (True, False):
            d, i = np.nonzero(t[:, side] >= 0)
            tok = t[d, side, i]
            m = (tok < parts["seg0"]) == prompt
            d, i, tok = d[m], i[m], tok[m]
            if not len(d):
                continue
            gap = np.abs(parts["ko_v"][b, h, d, side, i] - parts["Kd"][b, h, tok, d])
            lr = np.abs(_lr_at(parts, "k", b, h, tok, d))
            for j in dict.fromkeys(list(np.argsort(-gap)[:per_class]) + list(np.argsort(-lr)[:per_class])):
                out.append((int(tok[j]), (b, h, int(d[j]), side, int(i[j]))))
    return out


def _lr_at(parts, side, b, h, t, d):
    """low-rank term at elements (t[j], d[j]) of head (b, h)."""
    Q, P = parts[side + "Q"], parts[side + "P"]
    if Q is None or Q.shape[-1] == 0:
        return np.zeros(len(t))
    return np.einsum("jr,jr->j", Q[b, h, t], P[parts["seg"][t], b, h, d])


def v_outlier_sample(parts, b, h, count=4):
    """[(token, (b, t, side, i))]: V list entries that fall into head h, largest |value - dequant| first."""
    c = parts["vo_c"][b]
    t, s, i = np.nonzero((c >= 0) & (c // D == h))
    if not len(t):
        return []
    d = c[t, s, i] % D
    gap = np.abs(parts["vo_v"][b, t, s, i] - parts["Vd"][b, h, t, d])
    lr = np.abs(_lr_at(parts, "v", b, h, t, d)) / np.maximum(np.abs(parts["vo_v"][b, t, s, i]), 1.0)     # against the row's scale
    pick = dict.fromkeys(list(np.argsort(-gap)[:count]) + list(np.argsort(-lr)[:count]))
    return [(int(t[j]), (b, int(t[j]), int(s[j]), int(i[j]))) for j in pick]


def aim(Kbh, targets, extra=None, limit=None):
    """A query that makes the target keys (equal scores) outweigh every other key of Kbh [S,D] by e^DOMINANCE: the minimal-norm q
    with q . K[t] = 1 for every target (plus `extra` [D] added to the direction) -- and q . K[j] = 0 for the competitors j that
    came closest, added a few at a time until the targets lead --, scaled.  limit: only keys < limit compete.  Returns the
    fp16-rounded q, or None when no scale reaches the margin within Q_MAX."""
    S = Kbh.shape[0] if limit is None else limit
    targets = list(targets)
    others = np.ones(S, bool)
    others[targets] = False
    if not others.any():
        return f16(Kbh[targets[0]] * 0.5)
    comp = []
    for _ in range(6):
        A = Kbh[targets + comp]
        rhs = np.r_[np.ones(len(targets)), np.zeros(len(comp))]
        u = A.T @ np.linalg.solve(A @ A.T + 1e-9 * np.eye(len(A)), rhs)
        if extra is not None:
            u = u + extra
        c = Kbh[:S] @ u * QSCALE
        cs = c[targets]
        gap = cs.min() - c[others].max()
        if gap > 0.25 * cs.min():
            break
        rank = np.argsort(-np.where(others, c, -np.inf))
        comp += [int(j) for j in rank[:16] if int(j) not in comp][:16]
    if gap <= 1e-3:
        return None

    def margin(al):
        x = al * c
        return np.log(np.exp(x[targets] - x.max()).sum()) - np.log(np.exp(x[others] - x.max()).sum())
    lo, hi = 0.0, (DOMINANCE + math.log(others.sum()) + 2.0 + (cs.max() - cs.min())) / gap
    for _ in range(40):                      # the smallest scale with the margin (+ 0.5 for the fp16 rounding of q): small scores
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if margin(mid) < DOMINANCE + 0.5 else (lo, mid)
    q = f16(hi * u)
    if not np.isfinite(q).all() or np.abs(q).max() > Q_MAX:
        return None
    s = Kbh[:S] @ q * QSCALE
    top = np.log(np.exp(s[targets] - s.max()).sum())
    rest = np.log(np.exp(s[others] - s.max()).sum())
    return q if top - rest >= DOMINANCE else None


def make_probes(parts, b, h, rng, Kall=None, n_flat=2, n_channel=4):
    """Probe queries for KV head h of batch b: [(q [D], label, min_row)] -- token probes at probe_positions, aimed outlier probes
    (the target token with its outlier channel boosted), two-peak probes over every piece / window / chunk boundary pair, channel
    probes +-beta e_d, flat Gaussian probes.  min_row: the first extend query row that sees every target (0: any row)."""
    if Kall is None:
        Kall, _ = keys(parts)
    K = Kall[b, h]
    T, W = parts["T"], parts["W"]
    base = T + W
    probes = []

    def add(targets, label, extras=(None,)):
        for extra in extras:                 # (every key competes, chunk rows past the target included: any later row may carry it)
            q = aim(K, targets, extra)
            if q is not None:
                probes.append((q, label, max(0, max(targets) - base)))
                return

    for p in probe_positions(parts, b, h):
        add([p], f"token@{p}")
    for t, (_, _, d, _, _) in k_outlier_sample(parts, b, h):
        # the outlier's own channel boosted: its stored value (and the low-rank term on top) then weighs in the score
        nk = max(float(np.linalg.norm(K[t])), 1e-6)
        ext = []
        for lam in (2.0, 1.0, 0.5, 0.0):
            e = np.zeros(D)
            e[d] = math.copysign(lam, K[t, d]) / nk
            ext.append(e)
        add([t], f"k-outlier@{t}.{d}", ext)
    S = base + parts["n"]
    for a in [64 * k - 1 for k in range(1, (S + 63) // 64)] + ([T - 1] if T and W else []) + ([base - 1] if parts["n"] and W else []):
        if 0 <= a and a + 1 < S:
            add([a, a + 1], f"pair@{a}|{a + 1}")
    for d in rng.choice(D, size=min(n_channel, D), replace=False):
        for sgn in (1.0, -1.0):
            q = np.zeros(D)
            q[d] = 8.0 * sgn
            probes.append((f16(q), f"channel{'+' if sgn > 0 else '-'}{d}", 0))
    for _ in range(n_flat):
        probes.append((f16(rng.standard_normal(D)), "flat", 0))
    return probes


def edge_probes(parts, b, h, Kall=None):
    """Extend only: [(q, label, row)] -- row i aimed at its own chunk row (T + W + i), and row i aimed at chunk row i + 1 (which
    it must not see)."""
    if Kall is None:
        Kall, _ = keys(parts)
    K = Kall[b, h]
    base, n = parts["T"] + parts["W"], parts["n"]
    out = []
    for i in sorted({0, n // 3, n - 1}):
        q = aim(K, [base + i], None, base + i + 1)
        if q is not None:
            out.append((q, f"own@{i}", i))
    for i in sorted({0, n // 2, n - 2}):
        if 0 <= i < n - 1:
            q = aim(K, [base + i + 1], None, base + i + 2)
            if q is not None:
                out.append((q, f"next@{i}", i))
    return out


def decode_batches(parts, Hq, rng, Kall=None, **kw):
    """Decode (n = 0): the probes as a list of q [B,Hq,1,D]; query head hq carries the probes of its KV head hq // G, one per call
    (heads that run out get flat probes).  Returns (list, the key positions aimed at)."""
    B, Hkv = parts["Kd"].shape[:2]
    G = Hq // Hkv
    if Kall is None:
        Kall, _ = keys(parts)
    per = {}
    aimed = set()
    for b in range(B):
        for h in range(Hkv):
            made = make_probes(parts, b, h, rng, Kall, **kw)
            aimed |= _targets(made)
            pr = [q for q, _, _ in made]
            for g in range(G):       # the G query heads of a KV head share its probes round-robin
                per[b, h * G + g] = pr[g::G] if len(pr) >= G else pr
    nb = max(len(v) for v in per.values())
    out = []
    for j in range(nb):
        q = np.zeros((B, Hq, 1, D))
        for (b, hq), pr in per.items():
            q[b, hq, 0] = pr[j] if j < len(pr) else f16(rng.standard_normal(D))
        out.append(q)
    return out, aimed


def _targets(probes):
    """key positions the labelled probes aim at (token / outlier / pair / own / next probes)."""
    out = set()
    for _, label, _ in probes:
        if "@" in label:
            out |= {int(x) for x in label.split("@")[1].split(".")[0].split("|")}
    return out


def extend_queries(parts, Hq, rng, Kall=None, max_rounds=16, **kw):
    """Extend: rounds of q [B,Hq,n,D] (one extend call each) with the probes of every (b, KV head) spread over the query rows that
    see their targets, as many rounds as the probes need (a short chunk has few rows); rows left over get flat probes.
    Returns ([(q, probe_rows [B,Hq,n] bool)], the key positions aimed at by a placed probe)."""
    B, Hkv = parts["Kd"].shape[:2]
    n = parts["n"]
    G = Hq // Hkv
    if Kall is None:
        Kall, _ = keys(parts)
    todo = {}
    aimed = set()
    for b in range(B):
        for h in range(Hkv):
            e = [(q, lab, row, row + 1) for q, lab, row in edge_probes(parts, b, h, Kall)]      # (q, label, first row, end row)
            todo[b, h] = e + [(q, lab, lo, n) for q, lab, lo in make_probes(parts, b, h, rng, Kall, **kw)]
    rounds = []
    while any(todo.values()) and len(rounds) < max_rounds:
        q = f16(rng.standard_normal((B, Hq, n, D)))
        used = np.zeros((B, Hq, n), bool)
        for (b, h), pr in todo.items():
            heads = [h * G + g for g in range(G)]
            left = []
            for qv, lab, lo, hi in pr:
                free = [(x, i) for i in range(lo, hi) for x in heads if not used[b, x, i]]
                if free:
                    x, i = free[int(rng.integers(len(free)))]
                    q[b, x, i], used[b, x, i] = qv, True
                    aimed |= _targets([(qv, lab, lo)])
                else:
                    left.append((qv, lab, lo, hi))
            todo[b, h] = left
        rounds.append((q, used))
    return rounds, aimed


# ----------------------------------------------------------------------------------------------------------- mutation sites
def mutation_sites(parts, Hq, aimed=None):
    """[(kind, where)] for every mutation that applies to this reference's structure, at sites the probes aim at (aimed: the key
    positions that have a probe -- a key no query can single out, such as a small key among much longer ones, is no M1 site)."""
    T, W, n, seg = parts["T"], parts["W"], parts["n"], parts["seg"]
    B, Hkv = parts["Kd"].shape[:2]
    S = T + W + n
    out = []
    for p in sorted({0, 63, 64, T - 64, T - 65, T - 1, T, T + W - 1, S - 1}):
        if 0 <= p < S and (aimed is None or p in aimed) and not (p >= T + W and n and p != S - 1):
            out.append(("M1-drop", p))
    if n >= 1:
        out.append(("M2-lose-own", None))
    if n >= 2:
        out.append(("M2-gain-next", None))
    h = Hkv - 1
    ks = k_outlier_sample(parts, 0, h, per_class=1)
    for _, where in ks[::2]:                  # (each class's entry farthest from its dequantized value)
        out.append(("M3-k-outlier", where))
    if ks and parts["kQ"] is not None and parts["kQ"].shape[-1]:
        lr = [abs(_lr_at(parts, "k", 0, h, [t], [w[2]])[0]) for t, w in ks]
        out.append(("M6-k-no-lr", ks[int(np.argmax(lr))][1]))
    vs = v_outlier_sample(parts, 0, h, count=1)
    for _, where in vs[:1]:
        out.append(("M4-v-ignored", where))
        if Hkv > 1:
            out.append(("M4-v-head-1" if h > 0 else "M4-v-head+1", where))
    if len(vs) > 1 and parts["vQ"] is not None and parts["vQ"].shape[-1]:
        out.append(("M6-v-no-lr", vs[-1][1]))
    if Hkv > 1:
        vs0 = v_outlier_sample(parts, 0, 0, count=1)
        for _, where in vs0:
            out.append(("M4-v-head+1", where))
    if parts["kQ"] is not None and T and seg.max() > 0:
        for piece in sorted({0, (parts["seg0"] - 1) // 64 if parts["seg0"] else 0, parts["seg0"] // 64, T // 64 - 1}):
            if 0 <= piece < T // 64:
                s = seg[64 * piece]
                out.append(("M5-seg+1" if s < seg.max() else "M5-seg-1", piece))
    if S >= 192:
        out.append(("M7-no-rescale", (64, 128)))
    if T >= 128:
        out.append(("M7-no-rescale", (T - 64, T)))
    if W >= 2 and (T or n):
        out.append(("M7-no-rescale", (T, T + W)))
    if Hkv > 1 and Hq // Hkv > 1:
        out.append(("M8-gqa-mod", None))
    out.append(("M9-no-logL", None))
    out.append(("M9-log2", None))
    return out
