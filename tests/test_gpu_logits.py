"""gear_logits_process / gear_eos_update (csrc/logits.hip) on the GPU against the numpy reference of tests/logits_ref.py -- every
output entry in the reference's admissible set, every untouched entry with the input's bits, nothing written behind a row -- and
the decoders' logits processors / EOS stopping end to end on a tiny 2-layer model."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import logits_ref as R
from gear_amd.logits import LogitsParams, TokenHistory, eos_update, process_logits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SENTINEL = 123.0
NINF = float("-inf")


def _logits(B, V, dtype, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, V)) * 4).astype(dtype)
    x[:, 1 % V] = -0.0
    x[:, 5 % V] = -np.inf                       # masked entries, also where a penalty / a bias lands
    x[:, 2 % V] = -abs(x[:, 2 % V]) - 1         # a negative entry for certain
    return x


def _hist(B, n, V, seed, alphabet=12):
    """Small alphabet (repeats, overlapping n-grams), tokens 0 and V - 1, and an end that repeats an earlier stretch."""
    rng = np.random.default_rng(seed)
    h = rng.integers(0, min(alphabet, V), size=(B, n))
    if n >= 8:
        h[:, -3:] = h[:, 2:5]
    if n >= 2:
        h[:, 0], h[:, 1] = 0, V - 1
    return h


def _strided(x, ld, offset, fill=SENTINEL):
    """x [B, V] in a device buffer with row pitch ld, starting `offset` elements into the allocation; returns (view, storage)."""
    B, V = x.shape
    store = torch.full((offset + B * ld + 8,), fill, dtype=torch.from_numpy(x[:1, :1]).dtype, device=DEV)
    view = store[offset:offset + B * ld].view(B, ld)[:, :V]
    view.copy_(torch.from_numpy(x))
    return view, store


def _run(x, hist, n, prompt_len, params, ld=None, offset=0, inplace=False, cur=None, cap=None):
    """-> (out [B, V] numpy, history buffer after the call); checks that nothing outside the rows' V columns was written."""
    B, V = x.shape
    ld = ld or V
    lg, lg_store = _strided(x, ld, offset)
    th = TokenHistory(B, cap or max(n, 1), DEV)
    if hist.shape[1]:
        th.load(torch.from_numpy(hist[:, :th.cap]))
    if inplace:
        out, out_store = lg, lg_store
    else:
        out, out_store = _strided(np.full_like(x, 77.0), ld, offset)
    before = out_store.clone()
    got = process_logits(lg, params, th, n, prompt_len, cur=None if cur is None else torch.as_tensor(cur, device=DEV), out=out)
    assert got is out
    torch.cuda.synchronize()
    mask = torch.ones_like(out_store, dtype=torch.bool)
    mask[offset:offset + B * ld].view(B, ld)[:, :V] = False
    assert torch.equal(out_store[mask], before[mask]), "written outside the rows"
    if not inplace:
        assert np.array_equal(R.bits(lg.cpu().numpy()), R.bits(x)), "the input changed"
    return out.cpu().numpy(), th.buf.cpu().numpy()


def _check(got, x, hist, n, prompt_len, params):
    for r in range(x.shape[0]):
        a, b, touched = R.process_row(x[r], hist[r], n, prompt_len, params.repetition_penalty, params.no_repeat_ngram_size,
                                      params.min_new_tokens, params.eos_ids, params.bias_items)
        msg = R.check_row(got[r], x[r], a, b, touched)
        assert msg is None, f"row {r}: {msg}"


EVERYTHING = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=40, eos_token_id=(3, 8),
                  logit_bias={2: 1.5, 7: -2.25, 0: 0.5}, bad_token_ids=(9,))


# ------------------------------------------------------------------------------------------------- 1. the kernel, per entry
@pytest.mark.parametrize("B,V,ld,offset,dtype", [
    (3, 1003, 1005, 3, np.float16),          # odd pitch, a sliced row start: no row on a 16-byte boundary
    (3, 1003, 1008, 0, np.float16),          # aligned rows with a V % 8 tail
    (3, 4096, 4096, 0, np.float16),
    (1, 262144, 262144, 0, np.float16),      # the largest row: 96 KiB of bitmaps
    (3, 1003, 1005, 1, np.float32),
    (2, 4096, 4096, 0, np.float32),
], ids=["v1003-odd", "v1003-tail", "v4096", "v262144", "f32-odd", "f32-v4096"])
def test_every_processor_at_once(B, V, ld, offset, dtype):
    p = LogitsParams(**dict(EVERYTHING, logit_bias={2: 1.5, 7: -2.25, 0: 0.5, V - 1: 1.0}))
    x, hist = _logits(B, V, dtype, 1), _hist(B, 64, V, 2)
    got, _ = _run(x, hist, 64, 30, p, ld=ld, offset=offset)
    _check(got, x, hist, 64, 30, p)
    got2, _ = _run(x, hist, 64, 30, p, ld=ld, offset=offset, inplace=True)      # out == logits: the same bits
    assert np.array_equal(R.bits(got2), R.bits(got))


@pytest.mark.parametrize("penalty", [1.3, 0.8])
def test_penalty_applies_exactly_once(penalty):
    """One token fills 500 of 512 history slots; tokens 0 and V - 1 are in it; negative, -0 and -inf entries are among the seen."""
    V = 1003
    p = LogitsParams(repetition_penalty=penalty)
    x = _logits(3, V, np.float16, 3)
    hist = np.full((3, 512), 17)
    hist[:, 500:] = [0, V - 1, 1, 2, 5, 6, 6, 40, 41, 42, 43, 44]
    hist[1] = np.roll(hist[1], 7)
    hist[2, :500] = 2                                  # the repeated token's logit is negative in this row
    got, _ = _run(x, hist, 512, 100, p)
    _check(got, x, hist, 512, 100, p)
    assert got[0, 17] == np.float16((np.float32(x[0, 17]) * np.float32(penalty)) if x[0, 17] < 0
                                    else (np.float32(x[0, 17]) / np.float32(penalty)))
    assert np.signbit(got[0, 1]) and got[0, 1] == 0 and got[0, 5] == NINF
    one = _run(x, hist, 1, 0, p)[0]                    # n = 1: only hist[0] counts
    _check(one, x, hist, 1, 0, p)


@pytest.mark.parametrize("g", [1, 2, 4])
def test_ngram_ban(g):
    V = 1003
    p = LogitsParams(no_repeat_ngram_size=g)
    x = _logits(3, V, np.float16, 4)
    for n in (g - 1, g, 64):
        hist = _hist(3, max(n, 1), V, 5 + n, alphabet=4)           # 4 symbols: many overlapping matches
        if n == 64:
            hist[0, :] = 3                                          # every window matches, all overlapping
            hist[1, -g:] = hist[1, :g]                              # the match that ends at the last token is the tail itself
        got, _ = _run(x, hist, n, 0, p)
        _check(got, x, hist, n, 0, p)
        banned = np.isneginf(got) & ~np.isneginf(x)
        assert banned.any() if n == 64 else (n >= g or not banned.any()), (g, n)


def test_bias_bans_and_min_new_tokens_boundaries():
    V = 1003
    x, hist = _logits(3, V, np.float16, 6), _hist(3, 50, V, 7)
    hist[:, 10:20] = 6                                              # a bias on a repeated token
    for m_off in (1, 0):                                            # n - prompt_len = m - 1 (EOS banned) and = m (free again)
        p = LogitsParams(repetition_penalty=1.3, min_new_tokens=11, eos_token_id=(4, 900, V - 1),
                         logit_bias={6: 3.0, 5: 1.0, 2: NINF, 33: -0.5}, bad_token_ids=(44,))
        n = 50
        prompt_len = n - 11 + m_off
        got, _ = _run(x, hist, n, prompt_len, p)
        _check(got, x, hist, n, prompt_len, p)
        assert (got[:, 900] == NINF).all() == bool(m_off)
        assert (got[:, 2] == NINF).all() and (got[:, 44] == NINF).all() and (got[:, 5] == NINF).all()
        assert got[0, 6] == np.float16((np.float32(x[0, 6]) + np.float32(3.0)) / np.float32(1.3)) or x[0, 6] + 3 < 0


def test_out_of_range_ids_are_skipped():
    V = 1003
    x, hist = _logits(2, V, np.float16, 8), _hist(2, 32, V, 9)
    hist[:, 3], hist[:, 4], hist[:, 5], hist[:, -1] = -1, V, 2 ** 31 - 1, -2 ** 31
    p = LogitsParams(repetition_penalty=1.3, no_repeat_ngram_size=1, min_new_tokens=5, eos_token_id=(V, 2 ** 31 - 1, 6),
                     logit_bias={V: 1.0, 2 ** 31 - 1: 2.0, 7: 1.0})
    got, _ = _run(x, hist, 32, 30, p)
    _check(got, x, hist, 32, 30, p)


def test_everything_off_is_the_identity():
    x, hist = _logits(3, 1003, np.float16, 10), _hist(3, 16, 1003, 11)
    for kw in (dict(), dict(ld=1005, offset=1), dict(inplace=True)):
        got, _ = _run(x, hist, 16, 4, LogitsParams(eos_token_id=3), **kw)
        assert np.array_equal(R.bits(got), R.bits(x))


def test_cur_appends_the_history():
    V = 1003
    p = LogitsParams(repetition_penalty=1.3, no_repeat_ngram_size=2)
    x = _logits(2, V, np.float16, 12)
    hist = _hist(2, 20, V, 13)
    cur = np.array([hist[0, 5], 777], dtype=np.int64)                # row 0 repeats a token (its bigram is banned), row 1 a new one
    want = hist.copy()
    want[:, 19] = cur
    stale = hist.copy()
    stale[:, 19] = 999                                               # what memory holds before the launch: must not be read
    lg = torch.from_numpy(x).to(DEV)
    th = TokenHistory(2, 32, DEV)
    th.load(torch.from_numpy(stale))
    got = process_logits(lg, p, th, 20, 4, cur=torch.from_numpy(cur).to(DEV)).cpu().numpy()
    _check(got, x, want, 20, 4, p)
    back = th.buf.cpu().numpy()
    assert np.array_equal(back[:, :20], want) and not back[:, 20:].any()
    # the next call, without cur, sees the appended token in memory; with a device-side length (pos_dev + n) too
    again = process_logits(lg, p, th, 20, 4).cpu().numpy()
    assert np.array_equal(R.bits(again), R.bits(got))
    dyn = process_logits(lg, p, th, 1, 4, pos_dev=torch.tensor([19, 0, 0, 0], dtype=torch.int32, device=DEV)).cpu().numpy()
    assert np.array_equal(R.bits(dyn), R.bits(got))
    assert got[1, 777] == np.float16(np.float32(x[1, 777]) * np.float32(1.3) if x[1, 777] < 0 else np.float32(x[1, 777]) / np.float32(1.3))


def test_eos_update():
    tok = torch.tensor([11, 7, 3, 9, 7], dtype=torch.int64, device=DEV)
    done = torch.tensor([0, 0, 1, 0, 5], dtype=torch.int32, device=DEV)
    n_done = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    eos_update(tok, done, (7, 9), 0, n_done)
    assert tok.tolist() == [11, 7, 0, 9, 0]          # finished rows are padded; a row that just emitted EOS keeps it
    assert [int(d != 0) for d in done.tolist()] == [0, 1, 1, 1, 1] and int(n_done) == 4
    tok2 = torch.tensor([[9], [5], [5], [5], [5]], dtype=torch.int64, device=DEV)
    eos_update(tok2, done, (7, 9), 2, n_done)
    assert tok2.view(-1).tolist() == [9, 2, 2, 2, 2] and int(n_done) == 5
    big = torch.arange(700, dtype=torch.int64, device=DEV)          # more rows than the workgroup has threads
    dn = torch.zeros(700, dtype=torch.int32, device=DEV)
    eos_update(big, dn, 699, 1, n_done)
    assert int(n_done) == 1 and dn[699] == 1 and dn[:699].sum() == 0 and torch.equal(big, torch.arange(700, device=DEV))


# ------------------------------------------------------------------------------------------------- 2. the decoders
def _tiny(method="gearslKIVI", n_kv=2, left=0.02, layers=2):
    from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
    cfg = LlamaConfigLite(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=layers,
                          num_attention_heads=4, num_key_value_heads=n_kv, k_bits=2, v_bits=2)
    cc = dict(compress_method=method, group_size=64, residual=64, quantize_bit=2, rank=4, rankv=4, loop=3, left=left)
    torch.manual_seed(0)
    return LlamaForCausalLM_GEARKIVI(cfg, cc).half().cuda().eval()


@pytest.fixture(scope="module")
def tiny():
    return _tiny()


def _ids(seed, B=2, T=100):
    return torch.randint(0, 1000, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()


def _dec(model, kind="gear", **kw):
    from gear_amd.fast_decode import FastGearDecoder
    return FastGearDecoder(model, 512, batch=2, seed=3, cache_kind=kind, **kw)


LP = LogitsParams(repetition_penalty=1.3, no_repeat_ngram_size=3, logit_bias={7: 2.0, 500: -1.0}, bad_token_ids=(11, 12))


def test_greedy_generate_follows_the_reference_loop(tiny):
    """Every token of generate(logits=LP) is the first-index argmax of the reference applied to the step() logits of a second
    decoder fed the same tokens.  Steps whose two best processed logits tie or lie within one fp16 ulp are skipped: at most 2 %."""
    # 100 -> 150 crosses the block boundary at 128.  The prompt seed is one where the reference loop alone meets no near-tie (the two
    # best processed logits stay >= 3 fp16 ulps apart over the 100 steps; other seeds of this tiny model give 0 - 2 near-ties)
    ids, L = _ids(27), 150
    toks = _dec(tiny).generate(ids, L, logits=LP)
    assert toks.shape == (2, L) and torch.equal(toks[:, :100], ids)
    t = toks.cpu().numpy()
    ref = _dec(tiny)
    lg = ref.prefill(ids)
    steps = skipped = 0
    for n in range(100, L):
        x = lg.cpu().numpy()
        for r in range(2):
            a, b, _ = R.process_row(x[r], t[r], n, 100, LP.repetition_penalty, LP.no_repeat_ngram_size, 0, (), LP.bias_items)
            top = np.sort(a.astype(np.float32))[-2:]
            steps += 1
            if top[1] - top[0] <= np.spacing(np.float16(top[1])) or int(a.argmax()) != int(b.argmax()):
                skipped += 1
                continue
            assert int(a.argmax()) == t[r, n], (r, n)
        if n + 1 < L:
            lg = ref.step(toks[:, n:n + 1])
    print(f"reference loop: {steps} steps, {skipped} skipped")
    assert skipped <= 0.02 * steps
    for r in range(2):                                               # and what the processors promise: no trigram twice, no banned token
        gen = t[r].tolist()
        grams = [tuple(gen[i:i + 3]) for i in range(len(gen) - 2)]
        new = grams[100 - 2:]
        assert all(grams.index(g) == 98 + i for i, g in enumerate(new)), "a generated trigram repeats an earlier one"
        assert not {11, 12} & set(gen[100:])


def test_graph_steps_equal_eager_and_leave_the_other_graphs_alone(tiny):
    """Every token of a graph step is, bit for bit, what the eager launches (process_logits + sample_tokens at that position) give
    on the graph's own raw logits and history.  Against a separate eager run the raw logits differ in their last bits, as they do
    without processors (tests/test_gpu_sampling.py), so a greedy run may leave the eager one only at a near-tie: two fp16 logits one
    ulp apart can swap when each moves by its own rounding, the processors' one rounding adds another -- 4 ulps bound that."""
    from gear_amd.sampling import SamplingParams, sample_tokens
    ids, L = _ids(22), 150
    S = SamplingParams(0.8, 50, 0.95, seed=7)
    for sampling in (None, S):
        lp = LogitsParams(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=4, eos_token_id=999)
        sp = sampling or SamplingParams(temperature=0.0)
        eager = _dec(tiny).generate(ids, L, logits=lp, sampling=sampling, stop_check_every=1000)
        d = _dec(tiny)
        recs, step = [], d._graph_step

        def spy(tok, smp, proc=None):
            out = step(tok, smp, proc)
            recs.append((d.pos, d.logits_proc_static.clone(), proc["hist"].buf.clone(), proc["done"].clone(), out.clone()))
            return out

        d._graph_step = spy
        graph = d.generate(ids, L, graph=True, logits=lp, sampling=sampling, stop_check_every=1000)
        assert graph.shape == eager.shape == (2, L) and len(recs) == L - 102
        assert d.graph_proc is not None and d.graph is None and d.graph_sampled is None
        for pos, raw, hist, done, tok in recs:
            assert torch.equal(hist[:, :pos], graph[:, :pos].int())                  # the capture appended the fed token itself
            src = process_logits(raw, lp, hist, pos, 100)
            want = sample_tokens(src, sp, pos=pos)[0].view(-1, 1)
            live = done.view(-1, 1) == 0
            assert torch.equal(tok[live], want[live]), pos
            assert torch.equal(graph[:, pos:pos + 1], tok)
        if sampling is None:
            for r in range(2):
                diff = (graph[r] != eager[r]).nonzero()
                if len(diff):
                    pos = int(diff[0])
                    raw, hist = next((x[1], x[2]) for x in recs if x[0] == pos)
                    top = process_logits(raw, lp, hist, pos, 100)[r].float().topk(2).values.cpu().numpy()
                    assert top[0] - top[1] <= 4 * np.spacing(np.float16(top[0])), (r, pos, top)
    plain = _dec(tiny).generate(ids, L, graph=True)
    assert plain.shape == (2, L) and (plain[:, 100:] != eager[:, 100:]).any()
    # return_logprobs reads each step's RAW logits (the processors write a buffer of their own): bit for bit the scoring launch on
    # the logits this very decoder returned, eager and graph alike.  (Two decoders' logits differ in their last bits from run to
    # run, so the check is made on each decoder's own logits, not across decoders.)
    from gear_amd.scoring import token_logprobs
    for graph_mode in (False, True):
        d = _dec(tiny)
        raws = []
        for name in ("prefill", "step"):
            def wrap(*a, _f=getattr(d, name), **kw):
                out = _f(*a, **kw)
                raws.append(out.clone())
                return out
            setattr(d, name, wrap)

        def wrap_g(*a, _f=d._graph_step, **kw):
            out = _f(*a, **kw)
            raws.append(d.logits_proc_static.clone())
            return out
        d._graph_step = wrap_g
        toks, lps = d.generate(ids, 120, graph=graph_mode, logits=LP, return_logprobs=True)
        assert toks.shape == (2, 120) and lps.shape == (2, 20) and len(raws) == 20
        want = token_logprobs(torch.stack(raws, 1), toks[:, 100:]).logprobs
        assert torch.equal(lps.view(torch.int32), want.view(torch.int32))
        assert not {11, 12} & set(toks[:, 100:].reshape(-1).tolist())


def test_no_bigram_repeats(tiny):
    pat = torch.randint(0, 1000, (2, 10), generator=torch.Generator().manual_seed(23))
    ids = pat.repeat(1, 9).cuda()                                    # a looping prompt: the plain run repeats bigrams
    toks = _dec(tiny).generate(ids, 140, logits=LogitsParams(no_repeat_ngram_size=2)).cpu().tolist()
    for row in toks:
        grams = [tuple(row[i:i + 2]) for i in range(len(row) - 1)]
        assert all(g not in grams[:89 + i] for i, g in enumerate(grams[89:])), "a generated bigram repeats an earlier one"


def test_eos_stopping(tiny):
    ids, L = _ids(24), 140
    plain = _dec(tiny).generate(ids, L)
    p = plain.cpu().numpy()
    # a token the plain run emits in row 0 only, as early as possible but not at once
    gen0, gen1 = p[0, 100:].tolist(), p[1, 100:].tolist()
    k = next(i for i in range(3, 40) if gen0[i] not in gen1 and gen0[i] not in gen0[:i])
    eos = gen0[k]
    for kw in (dict(), dict(graph=True)):
        out = _dec(tiny).generate(ids, L, eos_token_id=eos, pad_token_id=1, **kw).cpu().numpy()
        assert out.shape == (2, L)                                   # row 1 never stops
        assert np.array_equal(out[0, :100 + k + 1], p[0, :100 + k + 1]) and (out[0, 100 + k + 1:] == 1).all()
        assert np.array_equal(out[1], p[1])
    # the default pad is the EOS id; a tuple of ids; min_new_tokens holds the EOS back (the row then leaves the plain run's path)
    out = _dec(tiny).generate(ids, L, logits=LogitsParams(eos_token_id=(eos, 10 ** 6))).cpu().numpy()
    assert (out[0, 100 + k:] == eos).all() and np.array_equal(out[1], p[1])
    held = _dec(tiny).generate(ids, L, logits=LogitsParams(min_new_tokens=k + 5, eos_token_id=eos)).cpu().numpy()
    assert np.array_equal(held[0, :100 + k], p[0, :100 + k]) and eos not in held[0, 100:100 + k + 5].tolist()
    # every row stops: both rows' tokens as EOS ids -> the result ends behind the later EOS
    k1 = next(i for i in range(k + 1, 40) if gen1[i] not in gen1[:i] and gen1[i] not in gen0[:k + 1])
    for every in (1, 8):
        out = _dec(tiny).generate(ids, L, eos_token_id=(eos, gen1[k1]), pad_token_id=0, stop_check_every=every).cpu().numpy()
        assert out.shape == (2, 100 + k1 + 1) and out.shape[1] < L
        assert np.array_equal(out[1], p[1, :100 + k1 + 1]) and np.array_equal(out[0, :100 + k + 1], p[0, :100 + k + 1])
        assert (out[0, 100 + k + 1:] == 0).all()


@pytest.mark.parametrize("kind", ["gear", "fp16", "kivi"])
def test_every_cache_kind_runs_eager_steps(tiny, kind):
    model = tiny
    ids, L = _ids(25), 150
    a = _dec(model, kind).generate(ids, L, logits=LP, eos_token_id=998)
    b = _dec(model, kind).generate(ids, L, logits=LP, eos_token_id=998)
    plain = _dec(model, kind).generate(ids, L)
    assert a.shape[0] == 2 and a.shape[1] <= L and torch.equal(a, b) and torch.equal(a[:, :100], ids)
    assert not {11, 12} & set(a[:, 100:].reshape(-1).tolist())
    assert a.shape != plain.shape or (a != plain).any()


def test_shared_prefix_and_suffix_histories(tiny):
    """The history is loaded from the prompt columns of the shared-prefix paths: prompt | suffix | generated has no repeated bigram."""
    from gear_amd.fast_decode import FastGearDecoder
    ids = _ids(26, B=1, T=128)
    suf = _ids(27, B=2, T=6)
    dec = FastGearDecoder(tiny, 256, batch=2, seed=3, shared_prefix_tokens=128)
    out = dec.generate(ids, 170, shared_prefix=True, suffix_ids=suf, logits=LogitsParams(no_repeat_ngram_size=2)).cpu()
    assert out.shape == (2, 170) and torch.equal(out[:, :128], ids.cpu().expand(2, -1)) and torch.equal(out[:, 128:134], suf.cpu())
    for row in out.tolist():
        grams = [tuple(row[i:i + 2]) for i in range(len(row) - 1)]
        assert all(g not in grams[:133 + i] for i, g in enumerate(grams[133:]))


def test_out_of_scope_calls_are_refused(tiny):
    from gear_amd.fast_decode import FastGearDecoder
    ids = _ids(28)
    d = _dec(tiny)
    with pytest.raises(NotImplementedError, match="logits processors"):
        d.generate_speculative(ids, 120, logits=LP)
    d.prefill(ids)
    with pytest.raises(NotImplementedError, match="logits processors"):
        d.verify(ids[:, :2], logits=LP)
    with pytest.raises(NotImplementedError, match="logits processors"):
        d.verify_tree(ids[:, :2], torch.tensor([-1, 0]), logits=LP)
    sh = FastGearDecoder(tiny, 256, batch=2, seed=3, shared_prefix_tokens=128)
    with pytest.raises(NotImplementedError, match="logits processors"):
        sh.generate_beam(ids[:1], 120, logits=LP)
    with pytest.raises(NotImplementedError):
        _dec(tiny, "kivi").generate(ids, 120, graph=True, logits=LP)
    with pytest.raises(TypeError):
        _dec(tiny).generate(ids, 120, logits=dict(repetition_penalty=1.3))
    with pytest.raises(ValueError):
        _dec(tiny).generate(ids, 120, pad_token_id=0)
    with pytest.raises(ValueError):
        _dec(tiny).generate(ids, 120, eos_token_id=1, stop_check_every=0)


CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r})
from gear_amd.modeling_llamagear import LlamaConfigLite, LlamaForCausalLM_GEARKIVI
cfg = LlamaConfigLite(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, k_bits=2, v_bits=2)
cc = dict(compress_method="gearslKIVI", group_size=64, residual=64, quantize_bit=2, rank=4, rankv=4, loop=3, left=0.02)
torch.manual_seed(0)
model = LlamaForCausalLM_GEARKIVI(cfg, cc).half().cuda().eval()
ids = torch.randint(0, 1000, (2, 100), generator=torch.Generator().manual_seed(7)).cuda()
def gen(**kw):
    torch.manual_seed(0)
    return model.generate(ids, 130, **kw).cpu()
g = gen()
assert torch.equal(gen(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0), g)
a = gen(repetition_penalty=1.3, no_repeat_ngram_size=2)
assert a.shape == (2, 130) and torch.equal(a, gen(repetition_penalty=1.3, no_repeat_ngram_size=2)) and (a != g).any()
for row in a.tolist():
    grams = [tuple(row[i:i + 2]) for i in range(len(row) - 1)]
    assert all(x not in grams[:99 + i] for i, x in enumerate(grams[99:]))
eos = [int(g[0, 104]), int(g[1, 106])]
e = gen(eos_token_id=eos, pad_token_id=0)
first = [min(i for i in range(100, 130) if int(g[r, i]) in eos) for r in range(2)]
assert e.shape == (2, max(first) + 1), (e.shape, first)
for r in range(2):
    assert torch.equal(e[r, :first[r] + 1], g[r, :first[r] + 1]) and (e[r, first[r] + 1:] == 0).all()
s = gen(do_sample=True, temperature=0.8, seed=1, repetition_penalty=1.2, min_new_tokens=40, eos_token_id=int(g[0, 101]))
assert s.shape == (2, 130) and int(g[0, 101]) not in s[:, 100:].tolist()[0]
print("hook ok")
"""


def test_hook_model_generate_in_a_child_process():
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True,
                       timeout=330, cwd=ROOT)
    assert p.returncode == 0 and "hook ok" in p.stdout, p.stderr[-3000:]


def test_harness_flags():
    for extra in (["--model", "gearl", "--fast", "--graph", "--do_sample"], ["--model", "KIVI"]):
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "harness.py"), "--layers", "2", "--prompt_len", "200",
               "--max_length", "260", "--batch_size", "2", "--json", "--repetition_penalty", "1.1", "--no_repeat_ngram_size", "3",
               "--min_new_tokens", "4", "--stop_at_eos", "31999", *extra]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=330, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        res = json.loads(p.stdout.strip().splitlines()[-1])
        assert len(res) == 1 and 200 < res[0]["max_length"] <= 260 and res[0]["new_tokens_per_s"] > 0
