"""CPU checks of token sampling: the float64 reference (tests/sample_ref.py) against Philox known answers and hand-built rows, the
gear_sample_tokens entry point (bound, exported, argument errors before any launch) and SamplingParams validation."""
import ctypes

import numpy as np
import pytest
import torch

import sample_ref as R
from gear_amd import _lib
from gear_amd.sampling import SamplingParams, sample_tokens

NINF = -np.inf


# ------------------------------------------------------------------------------------------------- Philox
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(counter, key, want):
    assert R.philox4x32_10(counter, key) == want


def test_uniform_stream():
    u = R.uniform(0, 0, 0, 0)
    assert u == (0x6627E8D5 >> 8) * 2.0 ** -24
    assert 0 <= u < 1
    draws = {R.uniform(7, P, b, s) for P in range(20) for b in range(3) for s in range(2)}
    assert len(draws) == 120                             # position, sequence and purpose all change the draw
    assert R.uniform(7, 3, 1, 0) != R.uniform(8, 3, 1, 0)
    assert R.uniform(1 << 32, 3, 1, 0) != R.uniform(0, 3, 1, 0)


# ------------------------------------------------------------------------------------------------- semantics
def test_top_k_keeps_edge_ties():
    x = np.array([1.0, 3.0, 2.0, 2.0, 0.5, 2.0], np.float32)
    assert R.kept_mask(x, 2, 1.0).tolist() == [False, True, True, True, False, True]
    assert R.kept_mask(x, 1, 1.0).tolist() == [False, True, False, False, False, False]
    assert R.kept_mask(x, 6, 1.0).all() and R.kept_mask(x, 0, 1.0).all()
    # fewer finite values than k: all finite ones stay, -inf never
    y = np.array([NINF, 1.0, NINF, 0.0], np.float32)
    assert R.kept_mask(y, 3, 1.0).tolist() == [False, True, False, True]


def test_top_p_boundary_and_ties():
    # p = [0.5, 0.25, 0.125, 0.125] (x = log p): masses above = 0, 0.5, 0.75, 0.75 (the last two are tied)
    x = np.log(np.array([0.5, 0.25, 0.125, 0.125])).astype(np.float32)
    assert R.kept_mask(x, 0, 0.6).tolist() == [True, True, False, False]     # boundary token kept (0.5 < 0.6), the next dropped
    assert R.kept_mask(x, 0, 0.5).tolist() == [True, False, False, False]    # "< top_p" is strict
    assert R.kept_mask(x, 0, 0.76).tolist() == [True, True, True, True]      # the tied pair is kept together
    assert R.kept_mask(x, 0, 0.01).tolist() == [True, False, False, False]   # the top token always stays
    # top-p applies to the softmax over the top-k set
    z = np.log(np.array([0.4, 0.3, 0.2, 0.1])).astype(np.float32)
    assert R.kept_mask(z, 0, 0.5).tolist() == [True, True, False, False]      # over all four: 0.4 above token 1
    assert R.kept_mask(z, 2, 0.58).tolist() == [True, True, False, False]     # over {0.4, 0.3}: 4/7 = 0.571 above token 1
    assert R.kept_mask(z, 2, 0.55).tolist() == [True, False, False, False]


def test_minus_inf_is_masked():
    x = np.array([NINF, 0.0, NINF, 0.0], np.float32)
    keep = R.kept_mask(x, 0, 1.0)
    assert keep.tolist() == [False, True, False, True]
    assert [i for i, _, _ in R.intervals(x, keep)] == [1, 3]
    for u in (0.0, 0.3, 0.49, 0.51, 0.999):
        t, _, lp = R.sample_row(x, 1.0, 0, 1.0, u)
        assert t == (1 if u < 0.5 else 3) and abs(lp - np.log(0.5)) < 1e-12


def test_temperature_zero_is_argmax_first_index():
    x = np.array([0.0, 5.0, -1.0, 5.0], np.float32)
    assert R.sample_row(x, 0.0, 50, 0.1, 0.9) == (1, 0, 0.0)
    assert R.sample_row(x, 0.0, 0, 1.0, 0.9, draft=1) == (1, 1, 0.0)
    assert R.sample_row(x, 0.0, 0, 1.0, 0.9, draft=3) == (1, 0, 0.0)


def test_draw_walks_the_index_order_cdf():
    x = np.log(np.array([0.1, 0.2, 0.3, 0.4])).astype(np.float32)
    keep = R.kept_mask(x, 0, 1.0)
    iv = R.intervals(x, keep)
    assert [i for i, _, _ in iv] == [0, 1, 2, 3]
    assert np.allclose([h for _, _, h in iv], [0.1, 0.3, 0.6, 1.0], atol=1e-6)
    for i, lo, hi in iv:
        assert R.sample_row(x, 1.0, 0, 1.0, (lo + hi) / 2)[0] == i


def test_draft_rule():
    x = np.log(np.array([0.1, 0.2, 0.3, 0.4])).astype(np.float32)
    # accepted iff u_acc < p(d)
    assert R.sample_row(x, 1.0, 0, 1.0, 0.0, u_acc=0.29, draft=2)[:2] == (2, 1)
    t, a, lp = R.sample_row(x, 1.0, 0, 1.0, 0.0, u_acc=0.31, draft=2)
    assert a == 0 and t == 0 and abs(lp - np.log(0.1)) < 1e-6
    # rejected: the residual draws over the kept set without d (0.1, 0.2, 0.4) / 0.7
    for u, want in ((0.1 / 0.7 - 1e-3, 0), (0.1 / 0.7 + 1e-3, 1), (0.3 / 0.7 + 1e-3, 3), (0.999, 3)):
        assert R.sample_row(x, 1.0, 0, 1.0, u, u_acc=0.99, draft=2)[:2] == (want, 0)
    # a draft outside the kept set is never accepted and never drawn
    for ua in (0.0, 0.5):
        t, a, _ = R.sample_row(x, 1.0, 2, 1.0, 0.3, u_acc=ua, draft=0)
        assert a == 0 and t in (2, 3)
    # p(d) = 1: always accepted
    y = np.array([NINF, 0.0, NINF], np.float32)
    assert R.sample_row(y, 1.0, 0, 1.0, 0.5, u_acc=1 - 2 ** -24, draft=1)[:2] == (1, 1)
    assert R.sample_row(x, 1.0, 1, 1.0, 0.5, u_acc=0.999, draft=3)[:2] == (3, 1)


def test_residual_keeps_the_distribution_exact():
    """Sum over the accept / reject branches: P(emit i) = p(d) [i == d] + (1 - p(d)) p(i) / (1 - p(d)) [i != d] = p(i)."""
    x = np.log(np.array([0.1, 0.2, 0.3, 0.4])).astype(np.float32)
    keep = R.kept_mask(x, 0, 1.0)
    p = R.probs(x, keep)
    for d in range(4):
        emit = np.zeros(4)
        emit[d] += p[d]
        for i, lo, hi in R.intervals(x, keep, exclude=d):
            emit[i] += (1 - p[d]) * (hi - lo)
        assert np.allclose(emit, p, atol=1e-12)


# ------------------------------------------------------------------------------------------------- the entry point
def test_sample_entry_is_bound_and_exported():
    assert "gear_sample_tokens" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "gear_sample_tokens")
    lib = _lib.load()
    assert lib.gear_abi_version() == _lib.ABI_VERSION == 5
    assert ctypes.sizeof(_lib.SampleParamsC) == 24


def _call(temperature=1.0, top_k=0, top_p=1.0, rows=4, V=100, ld=100, n_per_seq=1, logits=4096, tok=4096, params=True):
    lib = _lib.load()
    p = _lib.SampleParamsC(temperature, top_k, top_p, 0, 0)
    fake = 4096                  # never dereferenced: every case below fails its argument check before a launch
    return lib.gear_sample_tokens(logits, 0, rows, V, ld, n_per_seq, ctypes.byref(p) if params else None, None, 0, None, None,
                                  tok, fake, fake, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(params=False), b"null params"),
    (dict(logits=None), b"null logits"),
    (dict(tok=None), b"token_out"),
    (dict(V=0, ld=0), b"V = 0"),
    (dict(V=262145, ld=262145), b"V = 262145"),
    (dict(rows=0), b"rows = 0"),
    (dict(ld=99), b"row stride"),
    (dict(n_per_seq=0), b"n_per_seq = 0"),
    (dict(temperature=-0.5), b"temperature"),
    (dict(temperature=float("inf")), b"temperature"),
    (dict(top_k=-1), b"top_k = -1"),
    (dict(top_p=0.0), b"top_p"),
    (dict(top_p=1.5), b"top_p"),
])
def test_argument_errors_without_gpu(kw, msg):
    assert _call(**kw) < 0
    assert msg in _lib.load().gear_last_error()


def test_sample_tokens_refuses_cpu_tensors():
    with pytest.raises(_lib.GearError):
        sample_tokens(torch.zeros(2, 10), SamplingParams())
    with pytest.raises(ValueError):
        sample_tokens(torch.zeros(10), SamplingParams())


# ------------------------------------------------------------------------------------------------- SamplingParams
def test_sampling_params_validation():
    p = SamplingParams()
    assert (p.temperature, p.top_k, p.top_p, p.seed) == (1.0, 0, 1.0, 0)
    assert SamplingParams(temperature=0).greedy and not p.greedy
    SamplingParams(0.8, 50, 0.95, 2 ** 64 - 1)
    for kw in (dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(temperature="1"),
               dict(top_k=-1), dict(top_k=2.5), dict(top_k=True), dict(top_p=0.0), dict(top_p=1.01), dict(top_p=float("nan")),
               dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.0)):
        with pytest.raises(ValueError):
            SamplingParams(**kw)
    with pytest.raises(TypeError):
        sample_tokens(torch.zeros(2, 10), dict(temperature=1.0))
