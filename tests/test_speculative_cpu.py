"""CPU checks of gear_amd.speculative: prompt-lookup drafting and the greedy acceptance rule."""
import pytest
import torch

from gear_amd.speculative import accepted_lengths, ngram_draft


def _t(*rows):
    return torch.tensor(rows, dtype=torch.long)


def test_ngram_longest_match_wins():
    # trailing 3-gram (1 2 3) occurs at 0 -> 9 9; the trailing 1-gram (3) occurs more recently at 6 -> 7
    toks = _t([1, 2, 3, 9, 9, 8, 3, 7, 5, 1, 2, 3])
    assert ngram_draft(toks, 2).tolist() == [[9, 9]]
    assert ngram_draft(toks, 2, max_ngram=1).tolist() == [[7, 5]]


def test_ngram_most_recent_occurrence_wins():
    toks = _t([4, 5, 1, 4, 5, 2, 4, 5])
    assert ngram_draft(toks, 1).tolist() == [[2]]          # (4 5) at 3 beats (4 5) at 0
    assert ngram_draft(toks, 3).tolist() == [[2, 4, 5]]


def test_ngram_short_continuation_is_padded():
    toks = _t([6, 7, 8, 6, 7])
    assert ngram_draft(toks, 4).tolist() == [[8, 6, 7, 7]]


def test_ngram_no_match_fallback():
    toks = _t([1, 2, 3, 4])
    assert ngram_draft(toks, 3).tolist() == [[4, 4, 4]]
    assert ngram_draft(_t([5]), 2).tolist() == [[5, 5]]
    assert tuple(ngram_draft(toks, 0).shape) == (1, 0)


def test_ngram_batch_rows_independent():
    a, b = [1, 2, 3, 1, 2], [7, 8, 9, 10, 11]
    both = ngram_draft(_t(a, b), 2)
    assert both.tolist() == [ngram_draft(_t(a), 2)[0].tolist(), ngram_draft(_t(b), 2)[0].tolist()]
    assert both.tolist() == [[3, 1], [11, 11]]
    assert both.dtype == torch.long


def _logits(pred, V=10):
    """logits [B, k + 1, V] whose argmax is pred [B, k + 1]"""
    p = torch.tensor(pred)
    lg = torch.zeros(p.shape + (V,))
    lg.scatter_(-1, p[..., None], 1.0)
    return lg


def test_accepted_lengths():
    d = _t([3, 4, 5])
    assert accepted_lengths(d, _logits([[3, 4, 5, 6]])).tolist() == [3]        # all
    assert accepted_lengths(d, _logits([[0, 4, 5, 6]])).tolist() == [0]        # none (later matches do not count)
    assert accepted_lengths(d, _logits([[3, 0, 5, 6]])).tolist() == [1]        # a mismatch in the middle
    assert accepted_lengths(d, _logits([[3, 4, 0, 6]])).tolist() == [2]


def test_accepted_lengths_batch_minimum():
    d = _t([3, 4, 5], [1, 1, 1])
    acc = accepted_lengths(d, _logits([[3, 4, 5, 0], [1, 2, 1, 1]]))
    assert acc.tolist() == [3, 1] and int(acc.min()) == 1
    assert accepted_lengths(_t([], []).view(2, 0), _logits([[1], [2]])).tolist() == [0, 0]
    with pytest.raises(ValueError):
        accepted_lengths(d, _logits([[3, 4, 5], [1, 1, 1]]))
