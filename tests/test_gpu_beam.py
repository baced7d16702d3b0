"""GPU tests of FastGearDecoder.generate_beam: beam search over a shared prefix, the tails following the beams through
gear_cache_reorder.  The reference is tests/beam_ref.py (the rule restated in plain Python) driving a second decoder whose reorder is
the torch gather of its pool buffers -- both run the same launches on the same bytes, so tokens and scores are compared exactly."""
import numpy as np
import pytest
import torch

import beam_ref as R
from test_gpu_verify import _tiny

pytestmark = pytest.mark.gpu

P = 150                   # 128 prompt tokens compressed into the prefix pool, 22 in every tail's window


@pytest.fixture(scope="module")
def model():
    return _tiny("gearslKIVI", 2, left=0.02)


@pytest.fixture(scope="module")
def ids():
    return torch.randint(0, 1000, (1, P), generator=torch.Generator().manual_seed(23)).cuda()


def _dec(model, S, cap=256):
    from gear_amd.fast_decode import FastGearDecoder
    return FastGearDecoder(model, cap, batch=S, seed=6, shared_prefix_tokens=128)


def _reference(model, ids, S, max_length, **kw):
    """beam_ref.search over a decoder of its own whose reorder is index_select over the full pool buffers."""
    dec = _dec(model, S)

    def reorder(idx):
        i = torch.tensor(idx, dtype=torch.long, device="cuda")
        for name, t in dec.pool.buf.items():
            t.copy_(t.index_select(2 if name in ("kPseg", "vPseg") else 1, i))

    step = lambda toks: dec.step(torch.tensor(toks, dtype=torch.long, device="cuda"))
    ref = R.search(dec.prefill_shared(ids), step, reorder, ids[0].tolist(), S, max_length, **kw)
    ref["n_comp"] = dec.layers[0]["cache"].n_comp
    return ref


def _beam(model, ids, S, max_length, **kw):
    dec = _dec(model, S)
    seen = []
    inner = dec.reorder
    dec.reorder = lambda idx: (seen.append(idx.tolist()), inner(idx))[1]
    seqs, scores = dec.generate_beam(ids, max_length, **kw)
    return dec, seqs, scores, seen


def _same(seqs, scores, ref):
    assert seqs.dtype == torch.long and scores.dtype == torch.float32
    assert seqs.tolist() == ref["sequences"]
    assert np.array_equal(scores.cpu().numpy(), ref["scores"]), (scores.tolist(), ref["scores"].tolist())


@pytest.mark.parametrize("S", [2, 4])
def test_generate_beam_equals_the_reference(model, ids, S):
    max_length = P + 50                                         # 22 + 49 rows per tail: one tail block boundary
    dec, seqs, scores, seen = _beam(model, ids, S, max_length, num_beams=S, num_return_sequences=S)
    ref = _reference(model, ids, S, max_length, n_return=S)
    assert seqs.shape == (S, max_length) and scores.shape == (S,)
    _same(seqs, scores, ref)
    assert torch.equal(seqs[:, :P], ids.expand(S, -1))
    # conditions of the test, not measurements: the beams really were permuted, and a tail boundary really was crossed
    assert seen == [t["beam_idx"] for t in ref["trace"][:-1]]
    assert any(idx != list(range(S)) for idx in seen)
    assert dec.layers[0]["cache"].n_comp == ref["n_comp"] == 64 and dec.layers[0]["prefix"].n_comp == 128
    assert len({tuple(r) for r in seqs.tolist()}) == S          # S distinct hypotheses
    assert all(a >= b for a, b in zip(scores.tolist(), scores.tolist()[1:]))
    # the default returns the best one
    _, one, sc, _ = _beam(model, ids, S, max_length)
    assert one.shape == (1, max_length) and torch.equal(one[0], seqs[0]) and torch.equal(sc, scores[:1])


def test_one_beam_is_greedy(model, ids):
    dec, seqs, scores, _ = _beam(model, ids, 1, P + 50, num_beams=1)
    greedy = _dec(model, 1).generate(ids, P + 50, shared_prefix=True)
    assert torch.equal(seqs, greedy)


@pytest.mark.parametrize("length_penalty", [1.0, 0.0])
def test_generate_beam_with_eos(model, ids, length_penalty):
    S, max_length, pad = 4, P + 40, -1
    _, plain, _, _ = _beam(model, ids, S, max_length, length_penalty=length_penalty)
    eos = int(plain[0, P + 4])                                  # what the best hypothesis emitted five steps after the prompt
    kw = dict(length_penalty=length_penalty)
    dec, seqs, scores, seen = _beam(model, ids, S, max_length, eos_token_id=eos, num_return_sequences=S, pad_token_id=pad, **kw)
    ref = _reference(model, ids, S, max_length, eos=eos, n_return=S, pad=pad, **kw)
    # until the first EOS event the search is the no-EOS search, whose best hypothesis takes `eos` at step 5 with a rank < S
    first = min(i for i, t in enumerate(ref["trace"]) if t["finished"])
    assert first <= 4
    _same(seqs, scores, ref)
    assert seen == [t["beam_idx"] for t in ref["trace"][:len(seen)]] and len(seen) in (len(ref["trace"]) - 1, len(ref["trace"]))
    sc = scores.tolist()
    assert all(a >= b for a, b in zip(sc, sc[1:]))
    ended = 0
    for row, s, raw, n in zip(seqs.tolist(), sc, ref["raw"], ref["lengths"]):
        assert row[:P] == ids[0].tolist() and all(t == pad for t in row[n:]) and all(t != pad for t in row[:n])
        if eos in row[P:]:                                      # finished by EOS: it ends there
            assert row.index(eos, P) == n - 1
            ended += 1
        else:
            assert n == ref["trace"][-1]["length"]
        assert s == float(np.float32(raw / n ** length_penalty))          # the length normalisation
        if length_penalty == 0.0:
            assert s == float(np.float32(raw))
    assert ended >= 1 or ref["trace"][-1]["length"] == max_length


def test_beam_scores_replay(model, ids):
    """The returned sequences fed to a fresh shared-prefix decoder, row b = sequence b, teacher-forced, no reorders: the summed
    log-probabilities of the chosen tokens are the returned scores -- what ties "the cache followed the beams" to the scores the
    user sees.  Expected bit for bit (same launches, same bytes per row; no tail boundary in this run)."""
    S, n = 4, 20
    dec, seqs, scores, seen = _beam(model, ids, S, P + n, length_penalty=0.0, num_return_sequences=S)
    assert any(idx != list(range(S)) for idx in seen) and dec.layers[0]["cache"].n_comp == 0
    fresh = _dec(model, S)
    logits = fresh.prefill_shared(ids)
    total = torch.zeros(S, dtype=torch.float32, device="cuda")
    worst = 0.0
    for i in range(n):
        tok = seqs[:, P + i]
        total = total + torch.log_softmax(logits.float(), -1).gather(1, tok[:, None])[:, 0]
        if i + 1 < n:
            logits = fresh.step(tok)
    worst = float((total - scores).abs().max())
    print(f"beam replay: worst |replayed - returned| score difference over {n} steps: {worst:.3e}")
    assert torch.equal(total, scores), worst


def test_generate_beam_refusals(model, ids):
    from gear_amd import _lib as L
    from gear_amd.fast_decode import FastGearDecoder
    with pytest.raises(ValueError):
        FastGearDecoder(model, 256, batch=2).generate_beam(ids, P + 10)          # no shared prefix
    dec = _dec(model, 4, cap=64)
    with pytest.raises(ValueError):
        dec.generate_beam(ids, P + 10, num_beams=2)
    with pytest.raises(ValueError):
        dec.generate_beam(ids.expand(2, -1), P + 10)
    with pytest.raises(ValueError):
        dec.generate_beam(ids[0], P + 10)
    with pytest.raises(ValueError):
        dec.generate_beam(ids, P + 10, num_return_sequences=5)
    with pytest.raises(ValueError):
        dec.generate_beam(ids, P)
    snap = [{k: t.clone() for k, t in p.buf.items()} for p in (dec.pool, dec.prefix_pool)]
    cap = dec.layers[0]["cache"].Tmax
    with pytest.raises(L.GearError):
        dec.generate_beam(ids, P + 1 + (cap + 64 - 22))                            # the tails would compress cap + 64 tokens
    assert dec.pos == 0 and not dec.shared_live and all(lw["cache"].seq_len == 0 for lw in dec.layers)
    for p, b in zip((dec.pool, dec.prefix_pool), snap):
        for k, t in p.buf.items():
            assert torch.equal(t, b[k]), k
    seqs, scores = dec.generate_beam(ids, P + 1 + (cap + 63 - 22))                 # the most the tails take
    assert seqs.shape == (1, P + cap + 42)
