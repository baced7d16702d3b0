"""GPU parity tests of what k_select_kernel (csrc/kfused.hip) does once the candidates are in LDS: the k-th value of a list, the
ties at the cut ("lower token first", both sides), the sorted lists + bitmap, and the hand-over of a list whose candidate count is
outside [k, capacity] to k_select_fix_kernel.  compress_key(path="fused", mode="fp32") against the CPU oracle with the criterion of
test_gpu_kfused.py (_check_payload: lists, values, scale, mn exact; codes exact but for the fill codes it explains).

Every input is built to land on one decision point, and says so BEFORE the GPU is asked: the oracle's own selection must show the
intended ties, and a replica of the kernel's threshold guess (mean +- z sd of the token sample, which is every token up to
T = 1024) must count the intended number of candidates, so that a mis-built input cannot pass vacuously."""
import math
import os
import re
from statistics import NormalDist

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from test_gpu_kfused import _check_payload, bits_eq, host

pytestmark = pytest.mark.gpu



def _kernel_constant(name):
    """A `constexpr int` of csrc/kfused.hip, read from the source the library is built from: the edge cases below sit on the
    kernel's own capacity, not on a copy of it."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gear_amd", "csrc", "kfused.hip")
    with open(src) as f:
        m = re.search(r"constexpr int %s = (\d+);" % name, f.read())
    assert m, f"{name} not found in {src}"
    return int(m.group(1))


KS_CAP = _kernel_constant("KS_CAP")                    # candidate slots per (channel, side) list
KS_TARGET_MAX = _kernel_constant("KS_TARGET_MAX")      # the host guesses thresholds while k + 5 sqrt(k) + 8 is at most this


@pytest.fixture(scope="module")
def C():
    from gear_amd import compress
    return compress


def _rows(xn):
    """[1, BH, T, D] -> the oracle's rows [BH * D, T] (float32)."""
    B, H, T, D = xn.shape
    return np.ascontiguousarray(xn.transpose(0, 1, 3, 2)).reshape(B * H * D, T).astype(np.float32)


def _candidate_counts(rows, k):
    """Replica of the threshold guess: per row the number of elements above mean + z sd and below mean - z sd -- or None where the
    count depends on the last bits of the guess (the kernel sums in fp32 and rounds the thresholds to fp16: both counts are taken
    with the threshold moved by 2^-8 of its size either way and must agree)."""
    T = rows.shape[1]
    assert T <= 1024, "beyond 1024 tokens the kernel samples"
    target = k + 5.0 * math.sqrt(k) + 8.0
    assert target <= KS_TARGET_MAX, "no guess at this k: every list takes the exact path"
    z = -NormalDist().inv_cdf(min(target / T, 0.5))
    r = rows.astype(np.float64)
    mean = r.mean(1)
    sd = np.sqrt(np.maximum((r * r).mean(1) - mean * mean, 0.0))
    out = []
    for sign in (1.0, -1.0):
        th = mean + sign * z * sd
        d = np.abs(th) * 2.0 ** -8 + 1e-6
        if sign > 0:
            a, b = (r > (th - d)[:, None]).sum(1), (r > (th + d)[:, None]).sum(1)
        else:
            a, b = (r < (th + d)[:, None]).sum(1), (r < (th - d)[:, None]).sum(1)
        out.append(np.where(a == b, a, -1))
    return out[0], out[1]          # (large side, small side); -1: not decided by the replica


def _cut_is_tied(rows, k):
    """Per row and side: the k-th and the (k+1)-th element in value order are equal (the selection has to choose among ties)."""
    s = np.sort(rows, 1)
    T = rows.shape[1]
    assert k < T
    return s[:, T - k] == s[:, T - k - 1], s[:, k - 1] == s[:, k]


def _expect_lower_token_first(rows, k, isml, ilrg):
    """The tie rule, stated independently of the oracle's code: among equal values the lower token index is taken first."""
    T = rows.shape[1]
    order_l = np.lexsort((np.arange(T)[None, :].repeat(rows.shape[0], 0), -rows), axis=1)[:, :k]
    order_s = np.lexsort((np.arange(T)[None, :].repeat(rows.shape[0], 0), rows), axis=1)[:, :k]
    assert np.array_equal(np.sort(order_l, 1), np.sort(ilrg, 1)) and np.array_equal(np.sort(order_s, 1), np.sort(isml, 1))


def _narrow(seed, shape):
    """A narrow Gaussian body (sd 0.01, clipped at 3 sd): nothing of it comes near a threshold that extreme values set."""
    torch.manual_seed(seed)
    return (torch.randn(shape) * 0.01).clamp_(-0.03, 0.03)


def _distinct_halves(gen, n, lo=1.0, hi=1.125):
    """n distinct fp16 values in [lo, hi), shuffled."""
    grid = torch.arange(lo, hi, 2.0 ** -10)[: int((hi - lo) * 1024)]
    assert n <= grid.numel()
    return grid[torch.randperm(grid.numel(), generator=gen)[:n]]


def _place(x, head, ch, n, sign, gen, equal=False):
    """n values of size 1 .. 1.125 (or all 1.0625) with the given sign at random tokens of column (head, ch) that hold body values."""
    free = torch.nonzero(x[0, head, :, ch].abs() < 0.5).flatten()
    tok = free[torch.randperm(free.numel(), generator=gen)[:n]]
    x[0, head, tok, ch] = sign * (torch.full((n,), 1.0625) if equal else _distinct_halves(gen, n))


def _run(C, x, k, bits, group):
    p = C.compress_key(x.cuda(), bits, group, k_out=k, mode="fp32", path="fused")
    return p, _check_payload(p, x.numpy(), k, group, bits)


# ---------------------------------------------------------------------------------------------------------------- ties
def test_ties_few_valued_data(C):
    """fp16 data of 8 distinct values, the outer ones rare: nearly every list's k-th value is shared by elements on both sides of
    the cut, the lists stay inside [k, capacity] (the candidate path, not the exact one, resolves the ties) and more than four
    ties are taken (the bisection inside the tie range) as well as fewer (the walk)."""
    BH, T, k = 8, 1024, 20
    vals = torch.tensor([-3.0, -2.0, -1.0, -0.5, 0.5, 1.0, 2.0, 3.0])
    prob = torch.tensor([0.012, 0.04, 0.2, 0.248, 0.248, 0.2, 0.04, 0.012])
    torch.manual_seed(101)
    x = vals[torch.multinomial(prob, BH * T * 128, replacement=True)].reshape(1, BH, T, 128).half()
    rows = _rows(x.numpy())
    tl, ts = _cut_is_tied(rows, k)
    assert tl.mean() > 0.95 and ts.mean() > 0.95
    cl, cs = _candidate_counts(rows, k)
    fastl, fasts = (cl >= k) & (cl <= KS_CAP), (cs >= k) & (cs <= KS_CAP)
    assert fastl.mean() > 0.9 and fasts.mean() > 0.9, "the ties must be resolved by the candidate path"
    n3 = (rows == 3.0).sum(1)                                   # beyond the tie value 2.0 on the large side
    assert ((k - n3 > 4) & fastl & tl).any() and ((k - n3 >= 1) & (k - n3 <= 4) & fastl & tl).any()
    isml, ilrg, _ = orc.outlier_select(rows, k)
    _expect_lower_token_first(rows, k, isml, ilrg)
    _run(C, x, k, 2, 64)


# ---------------------------------------------------------------------------------------------------------------- constant, one extreme, one-sided
@pytest.mark.parametrize("BH,T,k,bits,group", [(1, 128, 3, 4, 32), (8, 128, 6, 2, 64)])
def test_constant_single_extreme_and_one_sided_columns(C, BH, T, k, bits, group):
    """Columns of head BH - 1 (channels in three quarters of the head): constant (no candidate: the exact path, every element ties);
    a narrow body with k + 2 EQUAL values above and k + 2 below it (every candidate equals the k-th value, none is beyond it, the k
    lowest tokens win; both sides, so that the row mean -- the fill value -- stays inside the body and is no group's extreme, whose
    last bits would depend on the summation order); exactly one extreme value on either side; negative-only and positive-only columns."""
    torch.manual_seed(102)
    gen = torch.Generator().manual_seed(1020)
    x = torch.randn(1, BH, T, 128)
    h = BH - 1
    x[0, h, :, 0] = 0.5
    x[0, h, :, 33] = _narrow(1, (T,))
    _place(x, h, 33, k + 2, 1.0, gen, equal=True)
    _place(x, h, 33, k + 2, -1.0, gen, equal=True)
    x[0, h, :, 70] = _narrow(2, (T,))
    x[0, h, 17, 70] = 4.0
    x[0, h, 90, 70] = -4.0
    x[0, h, :, 71] = -torch.randn(T).abs() - 0.5
    x[0, h, :, 127] = torch.randn(T).abs() + 0.5
    x = x.half()
    rows = _rows(x.numpy())
    r0 = h * 128
    cl, cs = _candidate_counts(rows, k)
    assert np.unique(rows[r0 + 0]).size == 1, "constant column: sd = 0, nothing is strictly beyond the guess"
    assert cl[r0 + 33] == k + 2 and np.unique(rows[r0 + 33][rows[r0 + 33] > 0.5]).size == 1
    assert cs[r0 + 33] == k + 2 and np.unique(rows[r0 + 33][rows[r0 + 33] < -0.5]).size == 1
    assert (rows[r0 + 70] > 1).sum() == 1 and (rows[r0 + 70] < -1).sum() == 1
    assert rows[r0 + 71].max() < 0 and rows[r0 + 127].min() > 0
    isml, ilrg, _ = orc.outlier_select(rows, k)
    _expect_lower_token_first(rows, k, isml, ilrg)
    assert np.array_equal(np.sort(ilrg[r0 + 33]), np.sort(np.nonzero(rows[r0 + 33] > 0.5)[0])[:k])
    assert np.array_equal(np.sort(ilrg[r0 + 0]), np.arange(k)) and np.array_equal(np.sort(isml[r0 + 0]), np.arange(k))
    assert 17 in ilrg[r0 + 70] and 90 in isml[r0 + 70]
    _run(C, x, k, bits, group)


# ---------------------------------------------------------------------------------------------------------------- counts at the edges
@pytest.mark.parametrize("BH", [1, 8])
def test_candidate_counts_at_the_edges(C, BH):
    """A narrow Gaussian with n_hi values of size 1 .. 1.125 above and n_lo below it in a column: the guessed thresholds fall between
    the body and those values, so the two lists' candidate counts are n_hi and n_lo.  Counts: k - 1 (below: exact path), k (every
    candidate is taken), the capacity (the last slot of the list is used) and capacity + 1 (overflow: exact path), with distinct
    values and with all-equal ones.  The two sides of a column differ by at most one value, so that the row mean -- the fill value
    -- stays well inside the body and is no group's minimum or maximum (its last bits depend on the summation order)."""
    T, k = 1024, 20
    x = _narrow(103, (1, BH, T, 128))
    gen = torch.Generator().manual_seed(1030)
    h = BH - 1
    pairs = [(k - 1, k), (k, k - 1), (k, k), (k - 1, k - 1), (KS_CAP, KS_CAP + 1), (KS_CAP + 1, KS_CAP), (KS_CAP, KS_CAP),
             (KS_CAP + 1, KS_CAP + 1)]
    plan = {}                                                   # channel -> (n_hi, n_lo, equal)
    for i, (nh, nl) in enumerate(pairs):
        plan[2 + i] = (nh, nl, False)                           # quarter 0
        plan[72 + i] = (nh, nl, True)                           # quarter 2
        plan[127 - i] = (nh, nl, i % 2 == 1)                    # quarter 3
    for ch, (nh, nl, equal) in plan.items():
        _place(x, h, ch, nh, 1.0, gen, equal)
        _place(x, h, ch, nl, -1.0, gen, equal)
    x = x.half()
    rows = _rows(x.numpy())
    cl, cs = _candidate_counts(rows, k)
    for ch, (nh, nl, equal) in plan.items():
        r = h * 128 + ch
        assert cl[r] == nh and cs[r] == nl, (ch, nh, nl, cl[r], cs[r])
        assert abs(rows[r].mean()) < 0.005 and (np.abs(rows[r]) < 0.5).sum() == T - nh - nl
    isml, ilrg, _ = orc.outlier_select(rows, k)
    _expect_lower_token_first(rows, k, isml, ilrg)
    _run(C, x, k, 2, 64)


# ---------------------------------------------------------------------------------------------------------------- k at the edges
@pytest.mark.parametrize("BH,T,k", [(1, 64, 1), (8, 64, 1), (1, 64, 32), (8, 64, 32)])
def test_k_at_the_edges(C, BH, T, k):
    """k = 1 (one tile; a column with two equal maxima and two equal minima: the lower token of each pair) and 2k = T (every element
    of a column is an outlier on one side or the other; threshold guess at the mean itself)."""
    x = torch.randn(1, BH, T, 128, generator=torch.Generator().manual_seed(104))
    h = BH - 1
    x[0, h, :, 37] = _narrow(3, (T,))
    x[0, h, [9, 50], 37] = 2.0
    x[0, h, [21, 40], 37] = -2.0
    x[0, h, :, 38] = 0.25
    x = x.half()
    rows = _rows(x.numpy())
    assert 2 * k <= T
    isml, ilrg, _ = orc.outlier_select(rows, k)
    _expect_lower_token_first(rows, k, isml, ilrg)
    if k == 1:
        cl, cs = _candidate_counts(rows, k)
        assert cl[h * 128 + 37] == 2 and cs[h * 128 + 37] == 2
        assert ilrg[h * 128 + 37, 0] == 9 and isml[h * 128 + 37, 0] == 21
    else:
        distinct = np.array([np.unique(r).size == T for r in rows])          # (equal values may be taken by both sides)
        assert distinct.sum() > rows.shape[0] // 2
        assert np.array_equal(np.sort(np.concatenate([isml, ilrg], 1), 1)[distinct], np.arange(T)[None, :].repeat(distinct.sum(), 0))
    p = C.compress_key(x.cuda(), 2, 64, k_out=k, mode="fp32", path="fused")
    if k == 1:
        _check_payload(p, x.numpy(), k, 64, 2)
    else:
        # every element is an outlier: the dense part holds nothing but the fill value (test_gpu_kfused.py compares the selection
        # alone beyond k = T / 4, for that reason)
        oi = host(p.oidx).astype(np.int64).reshape(-1, 2 * k)
        assert np.array_equal(oi[:, :k], np.sort(isml, 1)) and np.array_equal(oi[:, k:], np.sort(ilrg, 1))
        bits_eq(host(p.oval).reshape(-1, 2 * k), np.take_along_axis(rows, oi, 1).astype(np.float16), "outlier values")


# ---------------------------------------------------------------------------------------------------------------- ordinary data
def test_random_data_and_decompressed_key(C):
    """Normal data at the 2 % setting: payload == oracle, and the decompressed K == gears_channelQ bit for bit (the criterion of
    test_fused_key_payload_vs_oracle)."""
    BH, T, s = 8, 1024, 0.02
    k = C.outlier_count(1, BH, T, 128, s)
    torch.manual_seed(105)
    x = torch.randn(1, BH, T, 128).half()
    p, _ = _run(C, x, k, 2, 64)
    bits_eq(host(C.decompress(p)), orc.gears_channelQ(x.numpy(), 2, 64, s), "decompressed K")
