"""CPU checks of tests/logits_ref.py, the reference gear_logits_process is tested against on the GPU: on fp32 rows it agrees with the
installed transformers' processors (sequence bias, repetition penalty, n-gram ban, minimum new tokens, in that order) -- equal
where they leave a value finite, -inf exactly where they write -inf -- and the LogitsParams validation cases."""
import numpy as np
import pytest
import torch

import logits_ref as R
from gear_amd.logits import LogitsParams, eos_ids


def _hf(x, hist, prompt_len, penalty, ngram, min_new, eos, bias):
    from transformers import (LogitsProcessorList, MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                              RepetitionPenaltyLogitsProcessor, SequenceBiasLogitsProcessor)
    procs = LogitsProcessorList()
    if bias:
        procs.append(SequenceBiasLogitsProcessor(sequence_bias={(int(t),): float(b) for t, b in bias}))
    if penalty != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=float(penalty)))
    if ngram:
        procs.append(NoRepeatNGramLogitsProcessor(ngram))
    if min_new:
        procs.append(MinNewTokensLengthLogitsProcessor(prompt_len, min_new, list(eos), device="cpu"))
    return procs(torch.from_numpy(hist.astype(np.int64)), torch.from_numpy(x.copy())).numpy()


CASES = [
    # penalty, ngram, min_new, eos, bias, n, prompt_len
    (1.3, 0, 0, (), (), 40, 10),
    (0.8, 0, 0, (), (), 40, 10),
    (1.0, 1, 0, (), (), 12, 3),
    (1.0, 2, 0, (), (), 40, 10),
    (1.0, 4, 0, (), (), 64, 10),
    (1.0, 4, 0, (), (), 3, 1),
    (1.0, 4, 0, (), (), 4, 1),
    (1.0, 0, 5, (7, 11), (), 14, 10),
    (1.0, 0, 5, (7, 11), (), 15, 10),
    (1.0, 0, 0, (), ((3, 2.5), (9, float("-inf")), (0, -1.25), (96, 0.5)), 20, 5),
    (1.3, 3, 8, (2,), ((3, 2.5), (9, float("-inf")), (5, -4.0)), 30, 25),
    (1.1, 2, 2, (1, 96), ((0, 1.0),), 1, 0),
]


@pytest.mark.parametrize("case", CASES, ids=[f"c{i}" for i in range(len(CASES))])
def test_reference_matches_transformers(case):
    penalty, ngram, min_new, eos, bias, n, prompt_len = case
    rng = np.random.default_rng(3)
    B, V = 3, 97
    x = (rng.standard_normal((B, V)) * 4).astype(np.float32)
    x[:, 5] = -np.inf                                       # a masked entry stays -inf under every processor
    x[0, 6] = -0.0
    # a small alphabet: repeats, overlapping n-grams, and a match that ends at the last token (the history ends in a repeat)
    hist = rng.integers(0, 12, size=(B, n))
    if n >= 8:
        hist[:, -3:] = hist[:, 2:5]
    hist[0, 0], hist[1, -1] = 0, V - 1
    want = _hf(x, hist, prompt_len, penalty, ngram, min_new, eos, bias)
    for r in range(B):
        a, b, touched = R.process_row(x[r], hist[r], n, prompt_len, penalty, ngram, min_new, eos, bias)
        w = want[r]
        inf = np.isneginf(w)
        assert np.array_equal(np.isneginf(a), inf), (r, np.flatnonzero(np.isneginf(a) != inf))
        # (values, not bits: HF adds a dense bias vector, so its -0 + 0 is +0 where the kernel leaves an untouched -0 alone)
        assert np.array_equal(a[~inf], w[~inf]), r
        # untouched entries are the input's bits, and both members of the admissible set agree on fp32 rows up to one rounding
        assert np.array_equal(a[~touched].view(np.uint32), x[r][~touched].view(np.uint32))
        fin = np.isfinite(a)
        assert np.all(np.abs(a[fin].astype(np.float64) - b[fin].astype(np.float64)) <= np.spacing(np.abs(a[fin])))


def test_reference_exactly_once_and_fp16_rounding():
    """One token filling the history is penalised once; the fp16 result is the fp32 value rounded once."""
    x = np.array([2.0, -2.0, 1.0, -0.0, -np.inf, 3.0], dtype=np.float16)
    hist = [1] * 500 + [0, 3, 4, 99, -7]
    a, b, touched = R.process_row(x, hist, len(hist), 0, penalty=1.3)
    assert a[0] == np.float16(np.float32(2.0) / np.float32(1.3)) and a[1] == np.float16(np.float32(-2.0) * np.float32(1.3))
    assert a[2] == x[2] and a[5] == x[5] and not touched[2] and not touched[5]
    assert np.signbit(a[3]) and a[3] == 0 and a[4] == -np.inf
    assert R.check_row(a, x, a, b, touched) is None
    bad = a.copy()
    bad[2] = np.float16(1.001)
    assert "entry 2" in R.check_row(bad, x, a, b, touched)
    # n-gram: the history's last g - 1 tokens matched at every earlier place, overlapping ones included
    assert R.ngram_banned([5, 5, 5, 5], 4, 3, 10).tolist() == [5]
    assert R.ngram_banned([1, 2, 3, 1, 2], 5, 3, 10).tolist() == [3]
    assert R.ngram_banned([1, 2], 2, 3, 10).tolist() == [] and R.ngram_banned([4, 6, 4], 3, 1, 5).tolist() == [4]


def test_logits_params_validation():
    p = LogitsParams()
    assert not p.active and p.eos_ids == () and p.bias_items == ()
    assert LogitsParams(repetition_penalty=1.3).active and LogitsParams(no_repeat_ngram_size=2).active
    assert LogitsParams(min_new_tokens=3, eos_token_id=2).active and not LogitsParams(eos_token_id=2).active
    assert LogitsParams(eos_token_id=[2, 5]).eos_ids == (2, 5) and eos_ids(7) == (7,)
    q = LogitsParams(logit_bias={9: 1.5, 3: -2}, bad_token_ids=(4, 9))
    assert q.active and q.bias_items == ((3, -2.0), (4, float("-inf")), (9, float("-inf")))
    assert LogitsParams(1.3, 2) == LogitsParams(1.3, 2) and LogitsParams(1.3, 2) != LogitsParams(1.3, 3)
    assert hash(q) == hash(LogitsParams(logit_bias={3: -2, 9: 1.5}, bad_token_ids=(4, 9)))
    with pytest.raises(Exception):
        p.repetition_penalty = 2.0                          # frozen
    for kw in (dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
               dict(repetition_penalty=float("inf")), dict(repetition_penalty=True), dict(repetition_penalty="1"),
               dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5), dict(no_repeat_ngram_size=True),
               dict(min_new_tokens=-1), dict(min_new_tokens=2), dict(min_new_tokens=2.0, eos_token_id=1),
               dict(eos_token_id=-1), dict(eos_token_id=1.0), dict(eos_token_id=tuple(range(9))), dict(eos_token_id=(1, "a")),
               dict(logit_bias=[(1, 2.0)]), dict(logit_bias={-1: 1.0}), dict(logit_bias={1: float("nan")}),
               dict(logit_bias={1: float("inf")}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={1: "x"}),
               dict(bad_token_ids=5), dict(bad_token_ids=(-2,)), dict(bad_token_ids=(1.0,))):
        with pytest.raises(ValueError):
            LogitsParams(**kw)


def test_cpu_tensors_are_refused():
    from gear_amd import _lib
    from gear_amd.logits import TokenHistory, eos_update, process_logits
    x = torch.zeros(2, 16, dtype=torch.float16)
    h = torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(_lib.GearError):
        process_logits(x, LogitsParams(1.3), h, 1, 0)
    with pytest.raises(TypeError):
        process_logits(x, None, h, 1, 0)
    with pytest.raises(ValueError):
        process_logits(x[0], LogitsParams(1.3), h, 1, 0)
    with pytest.raises(ValueError):
        process_logits(x.double(), LogitsParams(1.3), h, 1, 0)
    with pytest.raises(_lib.GearError):
        eos_update(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), 1, 1, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        eos_update(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 1, 1, torch.zeros(1, dtype=torch.int32))
    t = TokenHistory(2, 8, "cpu")
    assert t.load(torch.tensor([[1, 2, 3], [4, 5, 6]])) == 3 and t.buf[1, :4].tolist() == [4, 5, 6, 0]
    with pytest.raises(ValueError):
        t.load(torch.zeros(2, 9, dtype=torch.long))
