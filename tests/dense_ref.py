"""float64 reference of the dense decode-step kernels (csrc/gemv_f16.hip, csrc/decode_ops.hip) that yields, for every output
element, the SET of fp16 bit patterns a correct kernel may produce.  numpy only.

What is bit-determined is modelled bit-exactly: the sum and the product of two fp16 values are exact in float64, float64 -> fp16
is one correct rounding, and an fp32 add of two fp16 values followed by an fp16 rounding equals the direct rounding
(24 >= 2 * 11 + 2) -- so x + delta, v * w_norm, x * cos and the rotation adds carry no tolerance at all.

What is not bit-determined gets an interval derived from the code, never from kernel output:
  fp32 dot product   |err| <= d * 2^-24 * sum_k |w_k x_k|,  d = roundings on the longest path = 2 per fdot2 * 4 fdot2 per chunk *
                     ceil(nchunk / (64 SK)) chunks per lane + 6 shuffle adds + SK LDS adds           (dot_roundings)
  norm prologue      the same bound on sum v^2 (all terms positive: relative d * 2^-24), pushed through rsqrt(ss / K + eps);
                     rsqrtf, the divide, the add and the multiply: 4 fp32 ulps relative on the scaled result
  add_rmsnorm        sum v^2 by up to 32 fmaf per thread + 6 shuffle adds + 3 LDS adds = 41 roundings; divide, add: one
                     rounding each; rsqrtf MATH_ULPS; v * inv one rounding
  expf / exp2f / cosf / sinf / rsqrtf   MATH_ULPS = 2 fp32 ulps.  The ROCm installation carries no HIP math accuracy table
                     (searched its include/hip headers and share/doc/hip for "ulp": nothing), so the fallback of 2 ulps is used.
  RoPE angle         log2f(theta) on the host <= 1 ulp (glibc), exponent product one rounding: the exponent E = 2p/128 * log2(theta)
                     is off by |E| * (2^-23 + 2^-24), which exp2 turns into a relative ln2 * |dE|; exp2f MATH_ULPS; pos * inv_freq
                     one rounding.  delta(pos, p, theta) = ang * (ln2 * E * 1.5 * 2^-23 + MATH_ULPS * 2^-23 + 2^-24); p == 0 has
                     E == 0 and inv_freq == 1 exactly: delta == 0.
An interval of an fp32 value becomes the run of fp16 values between the roundings of its ends (rounding is monotone).  The epilogues
(residual add, SwiGLU, RoPE) are monotone in each input, so they are evaluated at the corners of their inputs' candidate runs: with
one or two candidates per input the corners ARE all combinations and the set is the discrete list of results; an input with a longer
run (cos / sin at large positions) makes the set the run between the smallest and the largest corner.
+0 and -0 count as one value (a sum's zero has no derivable sign); NaN is its own value, whatever its payload."""
import math

import numpy as np

U = 2.0 ** -24            # fp32 unit roundoff: one correctly rounded operation, relative
ULP = 2.0 ** -23          # one fp32 ulp, relative (upper bound)
MATH_ULPS = 2             # device math functions (see the module docstring)
NANKEY = 1 << 20
EMPTY = 1 << 21
SENTINEL = 0x7DDA         # fp16 NaN payload the GPU tests pre-fill outputs with


def f16(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float16)


def rnd(x):
    """float64 -> fp16 -> float64: one correct rounding."""
    return f16(x).astype(np.float64)


def key(h):
    """fp16 -> ordered integer (monotone in the value; +-0 -> 0; NaN -> NANKEY)."""
    b = np.asarray(h, np.float16).view(np.uint16).astype(np.int64)
    mag = b & 0x7FFF
    return np.where(mag > 0x7C00, NANKEY, np.where(b & 0x8000, -mag, mag))


def unkey(k):
    k = np.asarray(k, np.int64)
    bits = np.where(k < 0, 0x8000 | -k, k)
    bits = np.where((k == NANKEY) | (k == EMPTY), 0x7E00, bits)
    return bits.astype(np.uint16).view(np.float16).astype(np.float64)


def _nunique(keys):
    s = np.sort(keys, -1)
    new = np.concatenate([np.ones(s.shape[:-1] + (1,), bool), s[..., 1:] != s[..., :-1]], -1)
    return (new & (s != EMPTY)).sum(-1)


class Sets:
    """Admissible fp16 values per element: the run of keys lo..hi (empty when hi < lo) plus the discrete keys[..., M]."""

    def __init__(self, ref, lo, hi, keys=None):
        self.ref, self.lo, self.hi = np.asarray(ref, np.float64), np.asarray(lo, np.int64), np.asarray(hi, np.int64)
        self.keys = np.full(self.lo.shape + (1,), EMPTY, np.int64) if keys is None else keys
        self.shape = self.lo.shape

    @staticmethod
    def interval(ref, lo, hi):
        ref, lo, hi = np.broadcast_arrays(np.asarray(ref, np.float64), lo, hi)
        nan = np.isnan(lo) | np.isnan(hi)
        klo, khi = key(f16(np.where(nan, 0.0, lo))), key(f16(np.where(nan, 0.0, hi)))
        keys = np.where(nan, NANKEY, EMPTY)[..., None]
        return Sets(ref, np.where(nan, 1, klo), np.where(nan, 0, khi), keys)

    @staticmethod
    def exact(h):
        k = key(h)
        nan = k == NANKEY
        return Sets(np.asarray(h, np.float16).astype(np.float64), np.where(nan, 1, k), np.where(nan, 0, k), np.where(nan, NANKEY, EMPTY)[..., None])

    def size(self):
        return np.maximum(self.hi - self.lo + 1, 0) + _nunique(self.keys)

    def contains(self, got):
        k = key(got)
        return ((k >= self.lo) & (k <= self.hi)) | (self.keys == k[..., None]).any(-1)

    def bounds(self):
        """(lowest candidate, highest candidate, at most two candidates) of run-only sets, values as float64."""
        assert (self.keys == EMPTY).all() or ((self.keys == NANKEY) == (self.hi < self.lo)[..., None]).all()
        nan = self.hi < self.lo
        return np.where(nan, np.nan, unkey(self.lo)), np.where(nan, np.nan, unkey(self.hi)), (self.hi - self.lo <= 1)

    def _map(self, f, fk):
        return Sets(f(self.ref), f(self.lo), f(self.hi), fk(self.keys))

    def reshape(self, *shape):
        return self._map(lambda a: a.reshape(shape), lambda a: a.reshape(tuple(shape) + (a.shape[-1],)))

    def __getitem__(self, idx):
        idx = idx if isinstance(idx, tuple) else (idx,)
        assert Ellipsis not in idx
        return self._map(lambda a: a[idx], lambda a: a[idx])

    @staticmethod
    def concat(parts, axis):
        assert axis >= 0
        m = max(p.keys.shape[-1] for p in parts)
        pad = lambda a: np.concatenate([a, np.full(a.shape[:-1] + (m - a.shape[-1],), EMPTY, np.int64)], -1)
        cat = lambda name: np.concatenate([getattr(p, name) for p in parts], axis)
        return Sets(cat("ref"), cat("lo"), cat("hi"), np.concatenate([pad(p.keys) for p in parts], axis))

    def describe(self, idx):
        run = [] if self.hi[idx] < self.lo[idx] else [self.lo[idx], self.hi[idx]]
        ks = sorted(set(int(k) for k in self.keys[idx] if k != EMPTY))
        fmt = lambda k: "nan" if k == NANKEY else "%r(0x%04x)" % (float(unkey(k)), int(f16(unkey(k)).view(np.uint16)))
        txt = ("run " + " .. ".join(fmt(k) for k in run) + " ") if run else ""
        return txt + ("{" + ", ".join(fmt(k) for k in ks) + "}" if ks else "")


def corners(fn, ref, *inputs):
    """Sets of fn(*inputs) for an fn that is monotone in every input (fp16-rounded products and sums): fn at every corner of the
    inputs' candidate runs.  inputs: (lo, hi, small) as Sets.bounds() gives them.  fn maps float64 arrays to fp16."""
    n = len(inputs)
    outs = []
    for c in range(1 << n):
        with np.errstate(invalid="ignore", over="ignore"):
            outs.append(key(fn(*[inp[(c >> i) & 1] for i, inp in enumerate(inputs)])))
    ks = np.stack(np.broadcast_arrays(*outs), -1)
    small = np.ones(ks.shape[:-1], bool)
    for inp in inputs:
        small = small & inp[2]
    nan = ks == NANKEY
    lo = np.where(nan, EMPTY, ks).min(-1)
    hi = np.where(nan, -EMPTY, ks).max(-1)
    run = ~small & (hi >= lo)
    keys = np.where(small[..., None] | nan, ks, EMPTY)
    return Sets(np.broadcast_to(ref, small.shape), np.where(run, lo, 1), np.where(run, hi, 0), keys)


def mismatches(got, sets, limit=6):
    got = np.asarray(got, np.float16)
    assert got.shape == sets.shape, (got.shape, sets.shape)
    bad = np.argwhere(~sets.contains(got))
    lines = []
    for idx in map(tuple, bad[:limit]):
        lines.append("  %s: got %r (0x%04x), admissible %s, float64 value %r" % (
            idx, float(got[idx]), int(got[idx].view(np.uint16)), sets.describe(idx), float(sets.ref[idx])))
    return len(bad), lines


def assert_admissible(got, sets, what=""):
    n, lines = mismatches(got, sets)
    if n:
        raise AssertionError("%s: %d of %d elements outside their admissible set\n%s" % (what, n, sets.lo.size, "\n".join(lines)))


def assert_bits(got, want, what=""):
    g, w = np.asarray(got, np.float16).view(np.uint16), np.asarray(want, np.float16).view(np.uint16)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, "%s: %d elements differ bit for bit, first at %s: got 0x%04x, want 0x%04x" % (
        what, len(bad), tuple(bad[0]), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


# ---------------------------------------------------------------------------------------------------------------- gemv_f16.hip
def pick_sk(K, N, max_sk):
    """pick_sk of gemv_f16.hip: the K dimension over 2 waves, over 4 for N <= 8192 and K >= 8192, capped by the entry point."""
    return min(4 if (N <= 8192 and K >= 8192) else 2, max_sk)


def dot_roundings(K, sk):
    return 2 * 4 * math.ceil((K // 8) / (64 * sk)) + 6 + sk


def _dot(x, W, sk):
    """float64 x W^T of fp16-exact operands and the bound of the kernel's fp32 evaluation (plus float64's own error)."""
    K = x.shape[-1]
    ref, S = x @ W.T, np.abs(x) @ np.abs(W).T
    return ref, dot_roundings(K, sk) * U * S + K * 2.0 ** -53 * S


def _h(a):
    return None if a is None else np.asarray(a, np.float16).astype(np.float64)


def gemv_f16(x, W, res_in=None):
    """gear_gemv_f16 / gear_gemv_f16_add: y = fp16(x W^T), then fp16(y + res_in)."""
    x, W = _h(x), _h(W)
    ref, tau = _dot(x, W, pick_sk(x.shape[1], W.shape[0], 4))
    s = Sets.interval(ref, ref - tau, ref + tau)
    if res_in is not None:
        r = _h(res_in)
        s = corners(lambda v: f16(v + r), ref + r, s.bounds())
    return s


def norm_values(x, delta, norm_w, eps, W, max_sk):
    """The val() of a NORM instantiation: (res_out fp16, Sets of fp16(inv * sum_k W[n,k] (w_norm[k] v[k])))."""
    x, delta, nw, W = _h(x), _h(delta), _h(norm_w), _h(W)
    K, N = x.shape[1], W.shape[0]
    sk = pick_sk(K, N, max_sk)
    v = rnd(x + delta) if delta is not None else x
    vw = rnd(v * nw) if nw is not None else v
    dot, tau = _dot(vw, W, sk)
    ss = (v * v).sum(-1, keepdims=True)
    es = dot_roundings(K, sk) * U + K * 2.0 ** -53
    eps32 = float(np.float32(eps))
    inv = lambda s: 1.0 / np.sqrt(s / K + eps32)
    i_lo, i_hi = inv(ss * (1 + es)), inv(ss * (1 - es))
    d_lo, d_hi = dot - tau, dot + tau
    lo = np.minimum(d_lo * i_lo, d_lo * i_hi)
    hi = np.maximum(d_hi * i_lo, d_hi * i_hi)
    lo, hi = _widen(lo, hi, 4 * ULP)
    return f16(v), Sets.interval(dot * inv(ss), lo, hi)


def _widen(lo, hi, rel):
    """[lo, hi] grown by a relative amount at each end (an infinite end stays)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isinf(lo), lo, lo - rel * np.abs(lo)), np.where(np.isinf(hi), hi, hi + rel * np.abs(hi))


def silu_interval(g):
    """The fp32 value g / (1 + expf(-g)) before its fp16 rounding: (ref, lo, hi)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(-g)
        q1 = g / ((1 + e * (1 - MATH_ULPS * ULP)) * (1 - U))
        q2 = g / ((1 + e * (1 + MATH_ULPS * ULP)) * (1 + U))
        lo, hi = np.minimum(q1, q2), np.maximum(q1, q2)
        return (g / (1 + e),) + _widen(lo, hi, U)


def _swiglu(gs, us):
    """fp16(fp16(silu(g)) * u) over the candidates of g and u."""
    glo, ghi, gsmall = gs.bounds()
    assert gsmall.all(), "SwiGLU reference: a gate with more than two candidates (silu is not monotone: choose other inputs)"
    parts = []
    for g in (glo, ghi):
        ref, lo, hi = silu_interval(g)
        sg = Sets.interval(ref, lo, hi)
        parts.append(corners(lambda a, b: f16(a * b), ref * us.ref, sg.bounds(), us.bounds()))
    a, b = parts
    ok = (a.hi < a.lo) & (b.hi < b.lo)      # discrete on both sides: union of the lists
    lo = np.where(ok, 1, np.minimum(np.where(a.hi < a.lo, EMPTY, a.lo), np.where(b.hi < b.lo, EMPTY, b.lo)))
    hi = np.where(ok, 0, np.maximum(np.where(a.hi < a.lo, -EMPTY, a.hi), np.where(b.hi < b.lo, -EMPTY, b.hi)))
    return Sets(_silu_ref(gs.ref) * us.ref, lo, hi, np.concatenate([a.keys, b.keys], -1))


def _silu_ref(g):
    with np.errstate(over="ignore", invalid="ignore"):
        return rnd(g / (1 + np.exp(-g)))


def gemv_f16_norm(x, delta, norm_w, eps, W, swiglu=0):
    """gear_gemv_f16_norm -> (res_out fp16 [B, K], Sets of y).  swiglu 1: rows interleaved (gate, up); 2: [gate rows | up rows]."""
    res_out, val = norm_values(x, delta, norm_w, eps, W, 2 if swiglu else 4)
    if not swiglu:
        return res_out, val
    N = val.shape[1]
    g, u = (val[:, 0::2], val[:, 1::2]) if swiglu == 1 else (val[:, :N // 2], val[:, N // 2:])
    return res_out, _swiglu(g, u)


# ---------------------------------------------------------------------------------------------------------------------- RoPE
def rope_angle(pos, theta):
    """(ang, delta) float64 [64] for pair index p = 0..63 (the derivation is in the module docstring)."""
    p = np.arange(64, dtype=np.float64)
    E = 2 * p / 128 * math.log2(theta)
    rel = np.where(p == 0, 0.0, math.log(2) * E * 1.5 * ULP + MATH_ULPS * ULP)
    ang = pos * 2.0 ** -E
    return ang, ang * np.where(p == 0, 0.0, rel + U)


def _trig_range(a_lo, a_hi, shift):
    """range of cos(a - shift) over [a_lo, a_hi], widened by the device function's ulps."""
    lo, hi = a_lo - shift, a_hi - shift
    v = np.stack([np.cos(lo), np.cos(hi)])
    mn, mx = v.min(0), v.max(0)
    k = np.ceil(lo / np.pi)                     # first multiple of pi at or above lo: an extremum (-1)^k inside?
    inside = k * np.pi <= hi
    ext = np.where(k % 2 == 0, 1.0, -1.0)
    mx = np.where(inside & (ext > 0), 1.0, mx)
    mn = np.where(inside & (ext < 0), -1.0, mn)
    inside2 = (k + 1) * np.pi <= hi             # an interval longer than pi holds both
    mx, mn = np.where(inside2, 1.0, mx), np.where(inside2, -1.0, mn)
    w = MATH_ULPS * ULP
    return mn - w * np.abs(mn), mx + w * np.abs(mx)


def rope_cos_sin(pos, theta):
    """Candidate runs of fp16(cosf(ang)), fp16(sinf(ang)) per pair index: two Sets of shape [64]."""
    ang, d = rope_angle(pos, theta)
    c_lo, c_hi = _trig_range(ang - d, ang + d, 0.0)
    s_lo, s_hi = _trig_range(ang - d, ang + d, np.pi / 2)
    if pos == 0:
        s_lo, s_hi = np.zeros(64), np.zeros(64)     # sinf(0) == 0 exactly (pi / 2 is not exact in float64)
    return Sets.interval(np.cos(ang), c_lo, c_hi), Sets.interval(np.sin(ang), s_lo, s_hi)


def rope_rotate(x1, x2, pos, theta, partner_bug=False, sin_sign_bug=False):
    """fp16 op by op like the kernels: lo = fp16(fp16(x1 c) + fp16(-x2 s)), hi = fp16(fp16(x2 c) + fp16(x1 s)); x1, x2 bounds
    triples of shape [..., 64] -> Sets [..., 128]."""
    c, s = rope_cos_sin(pos, theta)
    cb, sb = c.bounds(), s.bounds()
    f_lo = lambda a, b, cc, sn: f16(rnd(a * cc) + rnd(-b * sn))
    f_hi = lambda a, b, cc, sn: f16(rnd(b * cc) + rnd(a * sn))
    r_lo = rnd(rnd(x1[0] * c.ref) + rnd(-x2[0] * s.ref))
    r_hi = rnd(rnd(x2[0] * c.ref) + rnd(x1[0] * s.ref))
    return Sets.concat([corners(f_lo, r_lo, x1, x2, cb, sb), corners(f_hi, r_hi, x1, x2, cb, sb)], x1[0].ndim - 1)


def _split_heads(val, B, Hq, Hkv):
    v = val.reshape(B, Hq + 2 * Hkv, 128)
    return v[:, :Hq], v[:, Hq:Hq + Hkv], v[:, Hq + Hkv:]


def rope_append(qkv, Hq, Hkv, pos, theta):
    """gear_rope_append -> (Sets q [B, Hq, 128], Sets k [B, Hkv, 128], v fp16 [B, Hkv, 128] -- a plain copy)."""
    qkv = np.asarray(qkv, np.float16)
    B = qkv.shape[0]
    s = Sets.exact(qkv)
    q, k, _ = _split_heads(s, B, Hq, Hkv)
    rot = lambda t: rope_rotate(t[:, :, :64].bounds(), t[:, :, 64:].bounds(), pos, theta)
    return rot(q), rot(k), qkv.reshape(B, Hq + 2 * Hkv, 128)[:, Hq + Hkv:]


def gemv_qkv_rope(x, delta, norm_w, eps, W, Hq, Hkv, pos, theta):
    """gear_gemv_qkv_rope -> (res_out, Sets q, Sets k, Sets v)."""
    res_out, val = norm_values(x, delta, norm_w, eps, W, 2)
    q, k, v = _split_heads(val, np.asarray(x).shape[0], Hq, Hkv)
    rot = lambda t: rope_rotate(t[:, :, :64].bounds(), t[:, :, 64:].bounds(), pos, theta)
    return res_out, rot(q), rot(k), v


# ------------------------------------------------------------------------------------------------------------ decode_ops.hip
def add_rmsnorm(res_in, delta, weight, eps):
    """gear_add_rmsnorm -> (res_out fp16, Sets y): y = fp16(weight * fp16(v * rsqrt(mean(v^2) + eps))), v = fp16(res_in + delta)."""
    x, d, w = _h(res_in), _h(delta), _h(weight)
    H = x.shape[-1]
    v = rnd(x + d) if d is not None else x
    ss = (v * v).sum(-1, keepdims=True)
    es = 41 * U + H * 2.0 ** -53
    eps32 = float(np.float32(eps))
    inv = lambda s, e: (1.0 / np.sqrt((s / H * (1 + e) + eps32) * (1 + e))) * (1 - e * 2 * MATH_ULPS)
    i_lo, i_hi, i_ref = inv(ss * (1 + es), U), inv(ss * (1 - es), -U), 1.0 / np.sqrt(ss / H + eps32)
    a, b = v * i_lo, v * i_hi
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    n = Sets.interval(v * i_ref, lo - U * np.abs(lo), hi + U * np.abs(hi))
    return f16(v), corners(lambda t: f16(w * t), w * rnd(v * i_ref), n.bounds())


def silu_mul(gate_up):
    """gear_silu_mul: out = fp16(fp16(silu(gate)) * up), gate_up = [B, 2 I] = [gate | up]."""
    gu = _h(gate_up)
    I = gu.shape[1] // 2
    g, u = gu[:, :I], gu[:, I:]
    ref, lo, hi = silu_interval(g)
    sg = Sets.interval(ref, lo, hi)
    with np.errstate(invalid="ignore"):
        return corners(lambda a: f16(a * u), rnd(ref) * u, sg.bounds())


# ---------------------------------------------------------------------------------------------------------------- the cases
RHO = 1.0 / 32     # |ref| / sum |w x| of the near-cancelling output: far below the old max-norm checks' sight, and above
#                    2 * d * 2^-24 * 2^11 = 0.0122 for the largest d (50 at K = 8264), so that its set still holds at most 2 values

GEMV_SHAPES = [(8, 1), (64, 7), (520, 5), (2056, 6), (8184, 3), (8192, 3), (8264, 5)]
NORM_SHAPES = [(8, 4, (0, 1, 2)), (520, 12, (0, 1, 2)), (2056, 328, (0, 1, 2)), (8264, 4, (0,))]
EPS = 1e-5


def make_case(seed, B, K, N, delta=False, norm_w=False, special_rows=False):
    """Seeded inputs of one GEMV case.  Activations share their channel signs and the weights follow them (10 % flipped), so that
    every output has |ref| ~ 0.8 sum |w x| and its set one member, seldom two.  Row B - 1 is heavy-tailed (four channels at 50 - 2000
    x the rest).  Output (0, N - 1) nearly cancels: |ref| = RHO * sum |w x| (the odd channels of weight row N - 1 oppose the even
    ones, scaled to balance batch row 0; the other batch rows are 16 x smaller on the odd channels and do not cancel).
    special_rows (B == 4): row 1 is row 0 * 2^-11 (mean square far below eps), row 2 is all zero.
    No operand of the dot product is an fp16 subnormal.  Returns a dict of fp16 arrays (delta / norm_w None when absent)."""
    rng = np.random.default_rng(seed)
    sgn = rng.choice([-1.0, 1.0], K)
    a = 0.25 + 0.75 * rng.random((B, K))
    odd = np.arange(K) % 2 == 1
    a[1:, odd] /= 16
    heavy = rng.choice(K, min(4, K // 2), replace=False)
    a[B - 1, heavy] *= np.array([2000.0, 400.0, 50.0, 50.0])[:len(heavy)]
    v = rnd(sgn * a)
    special = special_rows and B == 4
    if special:
        v[1], v[2] = v[0] * 2.0 ** -11, 0.0
    d = nw = None
    x = v
    if delta:
        d = rnd(v * rng.uniform(0.05, 0.2, (B, K)) * rng.choice([-1.0, 1.0], (B, K)))
        x = rnd(v - d)
        if special:
            x[1], d[1] = x[0] * 2.0 ** -11, d[0] * 2.0 ** -11
        v = rnd(x + d)
    if norm_w:
        nw = rnd(0.75 + 0.75 * rng.random(K))
    act = rnd(v * nw) if norm_w else v
    mag = 0.02 + 0.06 * rng.random((N, K))
    flip = rng.random((N, K)) < 0.1
    flip[:, heavy] = False
    W = sgn * mag * np.where(flip, -1.0, 1.0)
    W[N - 1] = sgn * mag[N - 1] * np.where(odd, -1.0, 1.0)
    t = np.abs(W[N - 1] * act[0])
    P, M = t[~odd].sum(), t[odd].sum()
    W[N - 1, odd] *= P * (1 - RHO) / (M * (1 + RHO))
    W = rnd(W)
    for arr in (act, v, W):
        nz = np.abs(arr[arr != 0])
        assert nz.min() >= 2.0 ** -14 and nz.max() < 60000, "case generator: subnormal or overflowing dot-product operand"
    ratio = np.abs(act @ W.T) / np.maximum(np.abs(act) @ np.abs(W).T, 1e-300)
    if special:
        ratio[2] = 1.0
    return dict(x=f16(x), delta=None if d is None else f16(d), norm_w=None if nw is None else f16(nw), W=f16(W), ratio=ratio,
                special=special)


def norm_variants():
    """(delta, norm_w) presence -> NORM template value: folded 1, addend 2 (with or without the weight), weight only 3."""
    return [((False, False), 1), ((True, False), 2), ((True, True), 2), ((False, True), 3)]


def swiglu_weight(W, swiglu):
    """The weight as swiglu mode 2 wants it ([gate rows | up rows]) from the interleaved one."""
    return np.concatenate([W[0::2], W[1::2]], 0) if swiglu == 2 else W


def subnormal_case(seed, B, K, N):
    """Activations that are all fp16 subnormals (m * 2^-24, m = 1 .. 1023) against weights of +-2^14: every product is m * 2^-10 and
    every partial sum of up to 16384 of them is exact in fp32, so the full result is ONE fp16 value -- and 0 when the dot-product
    instruction flushes subnormal operands."""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 1024, (B, K)).astype(np.uint16).view(np.float16)
    W = f16(2.0 ** 14 * np.where(rng.random((N, K)) < 0.3, -1.0, 1.0))
    return x, W


def gemv_case(K, N, B):
    c = make_case(1000 + K + B, B, K, N)
    c["res"] = f16(np.random.default_rng(K + B).uniform(-4, 4, (B, N)))
    return c


def silu_tail_case():
    return f16(np.random.default_rng(5).standard_normal((3, 600)) * 3)


def rope_qkv(rc):
    """A plain fp16 qkv row for gear_rope_append: Gaussian, a few entries at 50 - 2000 x."""
    Hq, Hkv = rc["heads"]
    rng = np.random.default_rng(4000 + rc["pos"] + rc["K"])
    q = rng.standard_normal((rc["B"], (Hq + 2 * Hkv) * 128))
    q[:, rng.choice(q.shape[1], 6, replace=False)] *= [2000.0, -400.0, 50.0, 50.0, 1e-3, 1e-6]
    return f16(q)

def norm_cases():
    for K, N, modes in NORM_SHAPES:
        for B in (1, 2, 3, 4):
            for (has_d, has_w), norm in norm_variants():
                yield K, N, modes, B, has_d, has_w, make_case(2000 + K + B + 10 * has_d + 20 * has_w, B, K, N, has_d, has_w, True)

def rope_cases():
    heads, ks, poss, thetas, slots = [(1, 1), (4, 2), (8, 1)], [8, 520], [0, 1, 777, 4095, 32767], [1e4, 5e5], [(0, 1), (0, 64), (63, 64)]
    for (has_d, has_w), norm in norm_variants():
        for i in range(5):
            yield dict(has_d=has_d, has_w=has_w, heads=heads[i % 3], B=1 + i % 4, K=ks[i % 2], pos=poss[i],
                       theta=thetas[(i // 2) % 2], slot=slots[i % 3])

def rope_case_inputs(rc):
    Hq, Hkv = rc["heads"]
    return make_case(3000 + rc["pos"] + rc["K"] + 10 * rc["has_d"] + 20 * rc["has_w"], rc["B"], rc["K"], (Hq + 2 * Hkv) * 128,
                       rc["has_d"], rc["has_w"], True)

def all_gate_patterns():
    g = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    ups = np.array([1.0, -3.140625, 65504.0, 2.0 ** -24], np.float16)
    return np.concatenate([np.broadcast_to(g, (4, 65536)), np.repeat(ups[:, None], 65536, 1)], 1)

def rmsnorm_cases():
    for H in (8, 2056, 8192):
        for rows in (1, 5):
            rng = np.random.default_rng(H + rows)
            x = rng.standard_normal((rows, H))
            x[rows - 1, rng.choice(H, 3, replace=False)] *= [2000.0, 300.0, 50.0]      # heavy-tailed row
            if rows > 1:
                x[1] *= 2.0 ** -10                                                    # mean square far below eps
                x[2] = 0.0
            d = rng.standard_normal((rows, H)) * 0.3 * np.abs(x).mean(-1, keepdims=True)
            yield H, rows, f16(x), f16(d), f16(0.75 + 0.75 * rng.random(H))

def all_patterns_qkv():
    """Every fp16 bit pattern once in an x1 position (first half of a q / k head); x2 and the V heads ordinary values."""
    B, Hq, Hkv = 4, 224, 32
    rng = np.random.default_rng(11)
    h = f16(rng.uniform(0.5, 2.0, (B, Hq + 2 * Hkv, 128)) * rng.choice([-1.0, 1.0], (B, Hq + 2 * Hkv, 128)))
    h[:, :Hq + Hkv, :64] = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).reshape(B, Hq + Hkv, 64)
    return h.reshape(B, -1), Hq, Hkv
