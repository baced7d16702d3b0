"""CPU checks of tests/logprob_ref.py, the float64 reference gear_token_logprobs is tested against on the GPU: it agrees with
torch.log_softmax(x.double()), torch.topk and a direct KL sum on every case, applies the tie rules on hand-made rows, and its
random cases have no ties among the first k_top + 1 values -- so the GPU test may compare top_idx exactly."""
import numpy as np
import pytest
import torch

import logprob_ref as R


def _cases():
    for V, N in R.SHAPES:
        if V * N > 400000:
            N = 1                      # the reference is the same code at any N; keep the CPU suite quick
        yield f"uniform_{V}x{N}", R.uniform_rows(N, V, V + N), R.random_ids(N, V, V + N), R.uniform_rows(N, V, V + N + 50), False
    for V in (7, 64, 1003):
        for name, x, ids, r, ties in R.special_rows(V):
            yield f"{name}_{V}", x, ids, r, ties


CASES = list(_cases())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_matches_torch(case):
    name, x, ids, r, ties = case
    N, V = x.shape
    k = min(8, V)
    out = R.reference(x, ids, r, k)
    xd, rd = torch.from_numpy(x).double(), torch.from_numpy(r).double()
    ls = torch.log_softmax(xd, -1).numpy()
    lse = torch.logsumexp(xd, -1).numpy()
    dead = np.isneginf(xd.numpy().max(1))
    for i in range(N):
        if dead[i]:
            assert np.isnan(out["lse"][i])
            assert np.isnan(out["lp"][i]) or ids[i] < 0
            assert np.isnan(out["top_lp"][i]).all() and np.array_equal(out["top_idx"][i], np.arange(k))
            assert np.isnan(out["kl"][i])
            continue
        assert abs(out["lse"][i] - lse[i]) <= 1e-9 * max(1.0, abs(lse[i]))
        t = ids[i]
        if t < 0:
            assert out["lp"][i] == 0.0 and out["rank"][i] == -1
        elif t >= V:
            assert np.isnan(out["lp"][i]) and out["rank"][i] == -1
        else:
            want = ls[i, t]
            assert (np.isneginf(want) and np.isneginf(out["lp"][i])) or abs(out["lp"][i] - want) <= 1e-9 * max(1.0, abs(want))
            assert out["rank"][i] == int((xd[i] > xd[i, t]).sum())
        tv, ti = torch.topk(xd[i], k)
        got = out["top_lp"][i]
        want = ls[i][out["top_idx"][i]]
        fin = np.isfinite(want)
        assert np.array_equal(np.isneginf(want), np.isneginf(got)) and np.allclose(got[fin], want[fin], rtol=1e-9, atol=1e-9)
        assert np.array_equal(xd[i].numpy()[out["top_idx"][i]], tv.numpy())          # the same values as torch.topk, in order
        if not ties:
            assert np.array_equal(out["top_idx"][i], ti.numpy())
        if np.isneginf(rd[i].numpy().max()):
            assert np.isnan(out["kl"][i])
            continue
        p = torch.softmax(rd[i], -1).numpy()
        lr = torch.log_softmax(rd[i], -1).numpy()
        live = p > 0
        with np.errstate(invalid="ignore"):
            direct = np.sum(p[live] * (lr[live] - ls[i][live]))
        assert (np.isinf(direct) and np.isinf(out["kl"][i])) or abs(out["kl"][i] - direct) <= 1e-8 * max(1.0, abs(direct))
        assert out["agree"][i] == int(int(np.argmax(xd[i].numpy())) == int(np.argmax(rd[i].numpy())))


@pytest.mark.parametrize("case", [c for c in CASES if not c[4]], ids=[c[0] for c in CASES if not c[4]])
def test_random_cases_have_no_ties_among_the_leaders(case):
    name, x, ids, r, _ = case
    k = min(8, x.shape[1] - 1)
    assert not R.topk_has_ties(x, k), name
    assert not R.topk_has_ties(r, 1), name


def test_tie_rules_on_hand_made_rows():
    f = np.float16
    # all entries equal: the argmax is index 0, the top-k is 0, 1, 2, ..., nothing is strictly greater than the target
    x = np.full((1, 12), 2.0, f)
    out = R.reference(x, np.array([5]), x.copy(), 8)
    assert np.array_equal(out["top_idx"][0], np.arange(8)) and out["rank"][0] == 0 and out["agree"][0] == 1
    assert abs(out["lp"][0] + np.log(12.0)) < 1e-12 and out["kl"][0] == 0.0
    # two equal maxima: the lower index is the argmax, the other one follows it; both have rank 0
    x = np.array([[0.0, 3.0, 1.0, 3.0, -1.0]], f)
    for t in (1, 3):
        out = R.reference(x, np.array([t]), None, 3)
        assert out["rank"][0] == 0 and list(out["top_idx"][0]) == [1, 3, 2]
    # agreement resolves ties to the lowest index in BOTH rows
    r = np.array([[0.0, 3.0, 1.0, 2.0, -1.0]], f)
    assert R.reference(x, np.array([0]), r, 0)["agree"][0] == 1
    r = np.array([[0.0, 2.0, 1.0, 3.0, -1.0]], f)
    assert R.reference(x, np.array([0]), r, 0)["agree"][0] == 0
    # a target equal to another (non-maximal) entry: rank counts strictly greater entries only
    x = np.array([[5.0, 1.0, 4.0, 1.0]], f)
    assert R.reference(x, np.array([3]), None, 0)["rank"][0] == 2
    # -0.0 and +0.0 are equal values
    x = np.array([[-0.0, 0.0, -1.0]], f)
    assert list(R.reference(x, np.array([1]), None, 2)["top_idx"][0]) == [0, 1]


def test_tolerance_is_the_issue_bound_where_fp32_can_hold_it():
    assert R.tolerance(np.array([0.0, -50.0, 1024.0]), 1e-4).tolist() == [1e-4, 1e-4, 1e-4]
    assert abs(R.tolerance(np.array([-131008.0]), 1e-4)[0] - (1e-4 + 131008.0 * 2.0 ** -24)) < 1e-12
