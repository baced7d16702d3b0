"""float64 reference of gear_token_logprobs (csrc/logprob.hip) and the case list of its tests.

The fp16 logits are exact inputs; every statistic is computed in float64 with the kernel's rules: -inf entries carry no mass, an
all -inf row is NaN, ignored ids (< 0) give (0, rank -1), out-of-range ids give (NaN, rank -1), equal values are ordered by index
(lowest first) in the argmax and in the top-k, rank counts the entries STRICTLY greater than the target's logit."""
import numpy as np

F16_MAX = 65504.0


def reference(logits, ids, ref_logits=None, k_top=0):
    """logits fp16 [N, V] (numpy), ids int64 [N] -> dict of numpy arrays: lp, lse (float64), rank (int32), top_idx (int32 [N, k]),
    top_lp (float64 [N, k]) and, with ref_logits, kl (float64) and agree (int32)."""
    x = np.asarray(logits).astype(np.float64)
    N, V = x.shape
    ids = np.asarray(ids).astype(np.int64)

    def lse_of(a):
        m = a.max(1)
        dead = np.isneginf(m)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.exp(a - np.where(dead, 0.0, m)[:, None]).sum(1)
            out = m + np.log(s)
        out[dead] = np.nan
        return out

    lse = lse_of(x)
    lp = np.zeros(N)
    rank = np.full(N, -1, np.int32)
    for i in range(N):
        t = ids[i]
        if t < 0:
            lp[i] = 0.0
        elif t >= V:
            lp[i] = np.nan
        else:
            xt = x[i, t]
            rank[i] = int((x[i] > xt).sum())
            lp[i] = np.nan if np.isnan(lse[i]) else (-np.inf if np.isneginf(xt) else xt - lse[i])
    out = dict(lp=lp, lse=lse, rank=rank)
    # value descending, index ascending: a stable sort of the negated values
    order = np.argsort(-x, axis=1, kind="stable")
    if k_top:
        idx = order[:, :k_top]
        v = np.take_along_axis(x, idx, 1)
        with np.errstate(invalid="ignore"):
            tlp = np.where(np.isneginf(v), -np.inf, v - lse[:, None])
        tlp[np.isnan(lse)] = np.nan
        out["top_idx"], out["top_lp"] = idx.astype(np.int32), tlp
    if ref_logits is not None:
        r = np.asarray(ref_logits).astype(np.float64)
        lse_r = lse_of(r)
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.exp(r - lse_r[:, None])
            d = r - x                                    # ref -inf: no mass, contributes 0; x -inf under a finite ref: +inf
            term = np.where(np.isneginf(r), 0.0, np.where(np.isneginf(x), np.inf, p * d))
            kl = term.sum(1) - lse_r + lse
        kl[np.isnan(lse) | np.isnan(lse_r)] = np.nan
        out["kl"] = kl
        out["agree"] = (order[:, 0] == np.argsort(-r, axis=1, kind="stable")[:, 0]).astype(np.int32)
    return out


def uniform_rows(N, V, seed, lo=-30.0, hi=30.0):
    """fp16 [N, V] uniform in [lo, hi].  fp16 has few values there, so a large row repeats many; to keep the reference's top-k free of
    ties (an exact index comparison is then legitimate) the 16 largest entries of every row are made distinct: descending steps of
    1/64 (fp16's spacing between 16 and 32) down from hi + 2, at the positions the row's own largest values occupied."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo, hi, size=(N, V)).astype(np.float16)
    k = min(16, V)
    pos = np.argsort(-x.astype(np.float64), axis=1, kind="stable")[:, :k]
    vals = (hi + 2.0 - np.arange(k) / 64.0).astype(np.float16)
    np.put_along_axis(x, pos, np.broadcast_to(vals, (N, k)).copy(), 1)
    return x


def random_ids(N, V, seed):
    return np.random.default_rng(seed + 1000).integers(0, V, size=N).astype(np.int64)


# (V, N) of the kernel-against-reference cases: the smallest shapes at which it can still go wrong -- under one vector, one exact
# vector row, V % 8 != 0, both workgroup sizes (V <= 8192: 256 threads, beyond: 1024), more rows than one wave of workgroups
SHAPES = [(V, N) for V in (7, 64, 1000, 1003, 4099) for N in (1, 3, 300)] + [(128256, 1), (128256, 5)]
PITCHES = ("V", "V+1", "V+8")
K_TOPS = (0, 1, 8)


def pitch_of(name, V):
    return {"V": V, "V+1": V + 1, "V+8": V + 8}[name]


def special_rows(V, seed=7):
    """The value cases as (name, logits fp16 [n, V], ids int64 [n], ref fp16 [n, V], hand_made_ties).  Rows are built from
    uniform_rows (no ties among the leaders) unless the case is a tie case."""
    NEG = np.float16(-np.inf)
    cases = []

    def base(n, s):
        return uniform_rows(n, V, seed + s), random_ids(n, V, seed + s), uniform_rows(n, V, seed + s + 50)

    x, ids, r = base(2, 1)
    x[0, V // 2] = np.float16(F16_MAX)                        # fp16's largest finite value: exp(x - max) must not overflow
    ids[0] = V // 2
    x[1, 0] = np.float16(F16_MAX)
    x[1, V - 1] = np.float16(-F16_MAX)                        # ... and the widest difference must not either
    ids[1] = V - 1
    cases.append(("f16_max", x, ids, r, False))

    x, ids, r = base(2, 2)
    lead = min(9, V // 2)                                     # the leaders stay finite and distinct
    for row, step in ((0, 3), (1, 2)):
        mask = np.zeros(V, bool)
        mask[::step] = True
        mask[np.argsort(-x[row].astype(np.float64), kind="stable")[:lead]] = False
        x[row, mask] = NEG
        r[row, mask] = NEG                                    # a masked vocabulary entry is masked in both caches
        ids[row] = int(np.flatnonzero(mask if row else ~mask)[0])      # row 0: a live target, row 1: a masked target (lp = -inf)
    cases.append(("neg_inf_entries_and_target", x, ids, r, V < 40))

    x, ids, r = base(2, 3)
    x[0, :] = NEG                                             # nothing finite at all
    x[1, :] = NEG
    r[1, :] = NEG
    cases.append(("all_neg_inf", x, ids, r, True))

    x, ids, r = base(1, 4)
    x[0, :] = np.float16(1.5)
    cases.append(("all_equal", x, ids, r, True))

    x, ids, r = base(2, 5)
    ids[0] = int(np.argmax(x[0].astype(np.float64)))          # the target is the argmax: rank 0
    a = int(np.argmax(x[1].astype(np.float64)))
    b = (a + V // 2 + 1) % V
    b = b if b != a else (a + 1) % V
    x[1, b] = x[1, a]                                         # the target ties with the argmax: rank 0 for both, argmax = lower index
    ids[1] = max(a, b)
    cases.append(("target_is_argmax_and_tied", x, ids, r, True))

    x, ids, r = base(4, 6)
    ids[:] = [-100, V, V + 5, -1]
    cases.append(("ignored_and_out_of_range_ids", x, ids, r, False))
    return cases


def topk_has_ties(x, k):
    """True when the reference's first k (value descending) hold two equal values, or the k-th equals the (k+1)-th."""
    v = -np.sort(-np.asarray(x).astype(np.float64), axis=1, kind="stable")[:, :k + 1]
    return bool((v[:, 1:] == v[:, :-1]).any())


def tolerance(ref, base):
    """The absolute bound on an fp32 output whose float64 reference is `ref`: `base` (1e-4 for lp / lse / top_lp, 2e-4 for kl: the
    derivation in tests/test_gpu_logprob.py, made for |x| <= 32) wherever fp32 can hold it, i.e. up to |ref| = 1024 (half an fp32
    ulp there is 6.1e-5); beyond -- only the rows that hold +-65504 get there -- the fp32 result cannot be closer to the reference
    than half an ulp, |ref| 2^-24, which is added."""
    a = np.abs(np.asarray(ref, np.float64))
    return base + np.where(a > 1024.0, a * 2.0 ** -24, 0.0)
