"""GPU tests of shared-prefix chunk extend: gear_attn_extend_shared (GearKVCache.attend_extend_shared) -- n query tokens of each of S
sequences over ONE stored prompt, the sequence's own tail, window and chunk -- probed at one-token resolution against float64, LSE
included (tests/attn_probe.py; bounds AP.ROW_BOUND / AP.LSE_BOUND) (A); one-token sensitivity of those probes (B); consistency with
attend_shared and with attend_extend on a plain cache (C); bit reproducibility (D); no state change and refusals (E);
FastGearDecoder.extend_shared / generate(suffix_ids=) / reset_shared (F)."""
import numpy as np
import pytest
import torch

import attn_probe as AP
from test_gpu_attn_probe import _cc
from test_gpu_shared import _pair, _randn_kv
from test_gpu_verify import _cos, _tiny

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for tag, (r, e) in sorted(WORST.items()):
        print(f"EXTEND_SHARED {tag}: row_err {r:.3e} (bound {AP.ROW_BOUND:g}) lse_err {e:.3e} (bound {AP.LSE_BOUND:g})")


def host(t):
    return t.detach().cpu().numpy()


def _chunk(S, Hkv, n, seed):
    g = torch.Generator().manual_seed(seed)
    return _randn_kv(S, Hkv, n, g)


def _joint(pre, tail, kn, vn):
    """(joint parts, (K, V) [S, Hkv, Tp + T + W + n, D]): the prefix's keys broadcast to the S sequences in front of each sequence's
    own compressed tokens, window and chunk rows.  The joint parts are the tail's with T advanced by Tp: AP.ref masks query row i at
    key positions > T + W + i, and reads nothing else of the parts when it is given the keys."""
    tp = AP.decompose(tail, kn=kn, vn=vn)
    Kp, Vp = AP.keys(AP.decompose(pre))
    Kt, Vt = AP.keys(tp)
    S = Kt.shape[0]
    bc = lambda x: np.broadcast_to(x, (S,) + x.shape[1:])
    jp = dict(tp)
    jp["T"] = tp["T"] + Kp.shape[2]
    return jp, (np.concatenate([bc(Kp), Kt], 2), np.concatenate([bc(Vp), Vt], 2))


def _sites(Tp, T, W, n):
    """Key positions and boundary pairs the probes must aim at: first / last prefix key, its piece edge 63 | 64, Tp - 1 | Tp, the
    tail | window | chunk boundaries."""
    base = Tp + T + W
    single = {0, 63, Tp - 1, Tp, base - 1, base} | ({64} if Tp > 64 else set()) | ({Tp + T - 1, Tp + T} if T else set())
    pairs = {(Tp - 1, Tp), (base - 1, base)} | ({(63, 64)} if Tp > 64 else set()) | ({(Tp + T - 1, Tp + T)} if T else set())
    return sorted(single), sorted(pairs)


def _rounds(jp, kv, Hq, Tp, rng, max_rounds=24):
    """Rounds of q [S, Hq, n, D] (one call each): Gaussian rows with, per (sequence, KV head), aimed probes at _sites (any row that
    sees the targets; every key competes), at chunk row i itself from row i (own@i) and at chunk row i + 1 from row i, which must
    not see it (next@i).  Returns ([(q, used rows)], labels placed for every (s, h))."""
    Kall = kv[0]
    S, Hkv, N = Kall.shape[:3]
    W, n = jp["W"], jp["n"]
    T = jp["T"] - Tp
    base, G = Tp + T + W, Hq // Hkv
    single, pairs = _sites(Tp, T, W, n)
    todo, placed = {}, {}
    for s in range(S):
        for h in range(Hkv):
            K = Kall[s, h]
            pr = []
            for i in sorted({0, n // 3, n - 1}):
                pr.append((AP.aim(K, [base + i], None, base + i + 1), f"own@{i}", i, i + 1))
            for i in sorted({0, n // 2, n - 2}):
                if 0 <= i < n - 1:
                    pr.append((AP.aim(K, [base + i + 1], None, base + i + 2), f"next@{i}", i, i + 1))
            for t in [[p] for p in single] + [list(p) for p in pairs]:
                pr.append((AP.aim(K, t), "at@" + "|".join(map(str, t)), max(0, max(t) - base), n))
            todo[s, h] = [p for p in pr if p[0] is not None]
            placed[s, h] = set()
            assert len(todo[s, h]) >= len(pr) - 2, (s, h, [p[1] for p in pr if p[0] is None])
    rounds = []
    while any(todo.values()) and len(rounds) < max_rounds:
        q = AP.f16(rng.standard_normal((S, Hq, n, AP.D)))
        used = np.zeros((S, Hq, n), bool)
        for (s, h), pr in todo.items():
            left = []
            for qv, lab, lo, hi in pr:
                free = [(x, i) for i in range(lo, hi) for x in range(h * G, h * G + G) if not used[s, x, i]]
                if free:
                    x, i = free[int(rng.integers(len(free)))]
                    q[s, x, i], used[s, x, i] = qv, True
                    placed[s, h].add(lab)
                else:
                    left.append((qv, lab, lo, hi))
            todo[s, h] = left
        rounds.append((q, used))
    assert not any(todo.values()), {k: [p[1] for p in v] for k, v in todo.items() if v}
    rounds.append((AP.f16(rng.standard_normal((S, Hq, n, AP.D))), np.zeros((S, Hq, n), bool)))      # one all-Gaussian call
    return rounds, placed


def _run(pre, tail, kn, vn, rounds):
    res = []
    for q, _ in rounds:
        o, l = tail.attend_extend_shared(torch.tensor(q, dtype=torch.float16, device="cuda"), kn, vn, pre, return_lse=True)
        res.append((host(o).astype(np.float64), host(l).astype(np.float64)))
    return res


def _check(tag, res, refs):
    r = e = 0.0
    for (out, lse), (ro, rl) in zip(res, refs):
        assert np.isfinite(out).all() and np.isfinite(lse).all(), tag
        r, e = max(r, AP.row_err(out, ro)), max(e, AP.lse_err(lse, rl))
    print(f"extend_shared probe {tag}: row_err {r:.3e} lse_err {e:.3e}")
    w = WORST.get(tag.split("|")[0], (0.0, 0.0))
    WORST[tag.split("|")[0]] = (max(w[0], r), max(w[1], e))
    assert r <= AP.ROW_BOUND and e <= AP.LSE_BOUND, (tag, r, e)


def _signal(res, refs):
    return max(AP.signal(out, lse, mo, ml) for (out, lse), (mo, ml) in zip(res, refs))


def _setup(method, bits, rank, R, Hq, Hkv, S, Tp, more, n, left=None, seed=0):
    cc = _cc(method, bits, 64, R, rank, left=(0.02 if method == "gearslKIVI" else 0.0) if left is None else left)
    pre, tail = _pair(cc, S, Hkv, Tp, more, seed=seed or Tp + more + S + n)
    assert (tail.n_comp, tail.n_win) == (more - more % R, more % R)
    kn, vn = _chunk(S, Hkv, n, seed=n + S)
    jp, kv = _joint(pre, tail, kn, vn)
    return pre, tail, kn, vn, jp, kv


# ------------------------------------------------------------------------------------------------ A. probes against float64
CASES = [  # method, bits, rank, residual, Hq, Hkv, S, Tp, tail tokens (T + W), n
    ("gearslKIVI", 2, 4, 64, 8, 2, 3, 1024, 64 + 17, 7),      # G 4: S n G = 84 rows -- two tiles, sequence edges inside, padding rows
    ("gearslKIVI", 2, 8, 64, 4, 4, 1, 1024, 64 + 30, 7),      # S = 1, MHA, rank 8
    ("gearslKIVI", 4, 4, 64, 8, 2, 3, 256, 192 + 5, 1),       # n = 1, 4 bits, three tail blocks
    ("gearlKIVI", 2, 4, 64, 8, 2, 2, 256, 0, 9),              # T = 0 and W = 0: prefix and chunk only; no outliers
    ("gearslKIVI", 2, 4, 64, 4, 2, 2, 256, 64 + 30, 100),     # W + n > 64: the chunk crosses an fp16 piece
    ("KIVI", 4, 4, 64, 8, 1, 2, 64, 17, 5),                   # Tp = 64: one piece, one split; G 8; T = 0
    ("gearlKIVI", 4, 8, 128, 4, 4, 2, 1024, 64, 6),           # residual 128: W = 64, T = 0; rank 8, 4 bits
    ("gearslKIVI", 2, 8, 64, 8, 1, 2, 4096, 64 + 1, 3),       # the long prefix; G 8, rank 8
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-b{c[1]}-r{c[2]}-R{c[3]}-{c[4]}x{c[5]}-S{c[6]}-Tp{c[7]}+{c[8]}-n{c[9]}" for c in CASES])
def test_attend_extend_shared_probes(case):
    method, bits, rank, R, Hq, Hkv, S, Tp, more, n = case
    pre, tail, kn, vn, jp, kv = _setup(method, bits, rank, R, Hq, Hkv, S, Tp, more, n)
    rounds, placed = _rounds(jp, kv, Hq, Tp, np.random.default_rng(S + n))
    assert all("own@0" in p and f"at@{Tp - 1}|{Tp}" in p and "at@0" in p for p in placed.values()), placed
    if n > 1:
        assert all("next@0" in p for p in placed.values()), placed
    refs = [AP.ref(q, jp, kv=kv) for q, _ in rounds]
    _check(f"attend_extend_shared[G{Hq // Hkv}]|{case}", _run(pre, tail, kn, vn, rounds), refs)


def test_attend_extend_shared_single_split():
    """Hkv ceil(S n G / 64) >= 1024 work items in the prefix pass and in the tail pass: both split plans give one workgroup all
    pieces of its tile (nsplit = 1).  Gaussian queries against float64, and two calls give the same bits."""
    pre, tail, kn, vn, jp, kv = _setup("gearslKIVI", 2, 4, 64, 8, 8, 8, 128, 64 + 3, 1024)
    q = AP.f16(np.random.default_rng(1).standard_normal((8, 8, 1024, AP.D)))
    res = _run(pre, tail, kn, vn, [(q, None)])
    _check("attend_extend_shared[nsplit=1]", res, [AP.ref(q, jp, kv=kv)])
    again = _run(pre, tail, kn, vn, [(q, None)])
    assert np.array_equal(res[0][0], again[0][0]) and np.array_equal(res[0][1], again[0][1])


@pytest.fixture(scope="module")
def main_case():
    Tp, Hq = 1024, 8
    pre, tail, kn, vn, jp, kv = _setup("gearslKIVI", 2, 4, 64, Hq, 2, 3, Tp, 64 + 30, 7, seed=21)      # G 4, 84 rows, T 64, W 30
    rounds, placed = _rounds(jp, kv, Hq, Tp, np.random.default_rng(5))
    refs = [AP.ref(q, jp, kv=kv) for q, _ in rounds]
    return pre, tail, kn, vn, jp, kv, rounds, placed, refs


# ------------------------------------------------------------------------------------------------ B. one-token sensitivity
def test_attend_extend_shared_probes_catch_one_token_faults(main_case):
    """A kernel that loses one prefix key, one tail key, one window row or a row's own chunk key, that shows row i chunk row i + 1,
    or that gives sequence s the tail or the chunk of sequence s + 1 would move the probe metric to at least 5 x a bound: the
    mutated float64 references lie that far from what the kernel computes."""
    pre, tail, kn, vn, jp, kv, rounds, placed, refs = main_case
    res = _run(pre, tail, kn, vn, rounds)
    assert _signal(res, refs) <= 1.0
    Tp, T, W, n = 1024, 64, 30, 7
    assert (jp["T"], jp["W"], jp["n"]) == (Tp + T, W, n)
    base = Tp + T + W
    sites = [0, 63, 64, Tp - 1, Tp, Tp + T - 1, Tp + T, base - 1]            # prefix keys, tail keys, window rows
    for p in sites:
        assert all(f"at@{p}" in pl for pl in placed.values()), p
        sig = _signal(res, [AP.ref(q, AP.mutate(jp, "M1-drop", p), kv=kv) for q, _ in rounds])
        assert sig >= 5.0, ("M1-drop", p, sig)
    for kind in ("M2-lose-own", "M2-gain-next"):                              # own chunk row i lost / chunk row i + 1 gained
        sig = _signal(res, [AP.ref(q, AP.mutate(jp, kind), kv=kv) for q, _ in rounds])
        assert sig >= 5.0, (kind, sig)
    K, V = kv
    for name, (a, e) in (("neighbour tail", (Tp, base)), ("neighbour chunk", (base, base + n))):
        swap = tuple(np.concatenate([x[:, :, :a], np.roll(x[:, :, a:e], -1, 0), x[:, :, e:]], 2) for x in (K, V))
        sig = _signal(res, [AP.ref(q, jp, kv=swap) for q, _ in rounds])
        assert sig >= 5.0, (name, sig)


# ------------------------------------------------------------------------------------------------ C. consistency
def test_extend_shared_of_one_token_agrees_with_attend_shared():
    """n = 1: attend_extend_shared(q, k, v) and attend_shared(q) after the row was appended to the window are each within the bounds
    of the same float64 reference."""
    pre, tail, kn, vn, jp, kv = _setup("gearslKIVI", 2, 4, 64, 8, 2, 3, 256, 64 + 20, 1)
    rng = np.random.default_rng(2)
    K = kv[0]
    q = AP.f16(rng.standard_normal((3, 8, 1, AP.D)))
    for s in range(3):
        for h, t in ((0, [0]), (1, [255, 256]), (2, [K.shape[2] - 1]), (4, [256 + 64 - 1, 256 + 64])):
            aimed = AP.aim(K[s, h // 4], t)
            if aimed is not None:
                q[s, h, 0] = aimed
    ref = [AP.ref(q, jp, kv=kv)]
    a = _run(pre, tail, kn, vn, [(q, None)])
    _check("n1-extend_shared", a, ref)
    tail.append(kn, vn)
    o, l = tail.attend_shared(torch.tensor(q, dtype=torch.float16, device="cuda"), pre, return_lse=True)
    b = [(host(o).astype(np.float64), host(l).astype(np.float64)[:, :, None])]
    _check("n1-attend_shared", b, ref)
    print(f"n = 1: extend_shared vs attend_shared row_err {AP.row_err(a[0][0], b[0][0]):.3e} lse_err {AP.lse_err(a[0][1], b[0][1]):.3e}")


@pytest.mark.parametrize("method,left", [("gearslKIVI", 0.02), ("gearlKIVI", 0.0)])
def test_extend_shared_composes_to_the_plain_cache(method, left):
    """S = 1: prefix + tail built from the K / V and the seed of a plain cache hold the plain cache's keys bit for bit;
    attend_extend_shared and attend_extend on the plain cache are each within the bounds of the same float64 reference."""
    from gear_amd.cache import GearKVCache
    cc = _cc(method, left=left)
    Hkv, Hq, Tp, w0, more, n = 2, 8, 256, 10, 150, 40
    g = torch.Generator().manual_seed(4)
    k, v = _randn_kv(1, Hkv, Tp + w0 + more, g)
    plain = GearKVCache(1, Hkv, Tp + w0 + more + 128, cc, "cuda", seed=6)
    plain.prefill(k[:, :, :Tp + w0], v[:, :, :Tp + w0])
    state = plain.gen.get_state()
    plain.extend(k[:, :, Tp + w0:], v[:, :, Tp + w0:])
    pre = GearKVCache(1, Hkv, Tp, cc, "cuda", seed=6)
    pre.prefill(k[:, :, :Tp], v[:, :, :Tp])
    tail = GearKVCache(1, Hkv, w0 + more + 128, cc, "cuda", seed=6)
    tail.gen.set_state(state)                                                 # the blocks draw what the plain cache's blocks drew
    tail.extend(k[:, :, Tp:], v[:, :, Tp:])
    kn, vn = _chunk(1, Hkv, n, seed=8)
    parts = AP.decompose(plain, kn=kn, vn=vn)
    jp, kv = _joint(pre, tail, kn, vn)
    Kj, Vj = AP.keys(parts)
    assert np.array_equal(Kj, kv[0]) and np.array_equal(Vj, kv[1])            # the joint keys ARE the plain cache's keys
    assert (jp["T"], jp["W"], jp["n"]) == (parts["T"], parts["W"], parts["n"])
    rounds, _ = _rounds(jp, kv, Hq, Tp, np.random.default_rng(3))
    refs = [AP.ref(q, parts, kv=kv) for q, _ in rounds]
    a = _run(pre, tail, kn, vn, rounds)
    _check(f"compose-extend_shared[{method}]", a, refs)
    b = []
    for q, _ in rounds:
        o, l = plain.attend_extend(torch.tensor(q, dtype=torch.float16, device="cuda"), kn, vn, return_lse=True)
        b.append((host(o).astype(np.float64), host(l).astype(np.float64)))
    _check(f"compose-attend_extend[{method}]", b, refs)


# ------------------------------------------------------------------------------------------------ D. bit reproducibility
def test_attend_extend_shared_is_bit_reproducible(main_case):
    """The same call on the same caches gives the same bits every time (a multi-split shape: few work items, the prefix pieces go
    over many splits; the single-split shape is in test_attend_extend_shared_single_split).  Bound: equality -- the kernels have no
    float atomics and the merge adds the splits in a fixed order."""
    pre, tail, kn, vn, jp, kv, rounds, _, _ = main_case
    first = _run(pre, tail, kn, vn, rounds[:3])
    for i in range(3):
        again = _run(pre, tail, kn, vn, rounds[:3])
        for (o, l), (o2, l2) in zip(first, again):
            assert np.array_equal(o, o2) and np.array_equal(l, l2), i


# ------------------------------------------------------------------------------------------------ E. no state change, refusals
def test_attend_extend_shared_changes_no_state():
    pre, tail = _pair(_cc(), 3, 2, 256, 100, seed=4)
    before = [{k: t.clone() for k, t in c.bufs.items()} for c in (pre, tail)]
    counters = [(c.n_comp, c.n_win, c.seg0, c.kk0) for c in (pre, tail)]
    g = torch.Generator().manual_seed(1)
    for n in (1, 5, 70):
        kn, vn = _randn_kv(3, 2, n, g)
        tail.attend_extend_shared(torch.randn(3, 8, n, 128, generator=g).half().cuda(), kn, vn, pre, return_lse=n != 5)
    torch.cuda.synchronize()
    assert [(c.n_comp, c.n_win, c.seg0, c.kk0) for c in (pre, tail)] == counters
    for c, b in zip((pre, tail), before):
        for k, t in c.bufs.items():
            assert torch.equal(t, b[k]), k


def test_attend_extend_shared_argument_checks():
    from gear_amd import _lib as L
    from gear_amd.cache import N_MAX_EXTEND, GearKVCache
    pre, tail = _pair(_cc(), 2, 2, 128, 10, seed=2)
    z = lambda *s: torch.zeros(*s, dtype=torch.float16, device="cuda")
    q, k, v = z(2, 8, 3, 128), z(2, 2, 3, 128), z(2, 2, 3, 128)
    assert tail.attend_extend_shared(q, k, v, pre).shape == (2, 8, 3, 128)
    with pytest.raises(ValueError):
        tail.attend_extend_shared(q, k, v, tail)                              # the prefix must have batch 1
    with pytest.raises(ValueError):
        tail.attend_extend_shared(q[:1], k, v, pre)                           # q rows != sequences
    with pytest.raises(ValueError):
        tail.attend_extend_shared(q, k[:, :, :2], v, pre)                     # K rows != q rows
    with pytest.raises(ValueError):
        tail.attend_extend_shared(q, k, v.float(), pre)                       # V not fp16
    with pytest.raises(ValueError):
        tail.attend_extend_shared(q.float(), k, v, pre)
    with pytest.raises(ValueError):
        tail.attend_extend_shared(q, k, v, GearKVCache(1, 2, 128, _cc(bits=4), "cuda"))     # another compress config
    with pytest.raises(ValueError):
        m = N_MAX_EXTEND + 1
        tail.attend_extend_shared(z(2, 8, m, 128), z(2, 2, m, 128), z(2, 2, m, 128), pre)
    with pytest.raises(L.GearError):
        tail.attend_extend_shared(q, k, v, GearKVCache(1, 2, 128, _cc(), "cuda"))          # an empty prefix: Tp = 0 is refused
    with pytest.raises(L.GearError):
        tail.attend_extend_shared(z(2, 3, 3, 128), k, v, pre)                 # Hq % Hkv


def _snap(dec):
    return ([{k: t.clone() for k, t in p.buf.items()} for p in (dec.pool, dec.prefix_pool)],
            [(lw["cache"].n_comp, lw["cache"].n_win, lw["prefix"].n_comp) for lw in dec.layers], dec.pos)


def _same(x, y):
    for bx, by in zip(x[0], y[0]):
        for k in bx:
            assert torch.equal(bx[k], by[k]), k
    assert x[1:] == y[1:]


def test_extend_shared_refusals_change_nothing():
    from gear_amd import _lib as L
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    dec = FastGearDecoder(model, 128, batch=2, seed=1, shared_prefix_tokens=128)
    tok = torch.randint(0, 1000, (2, 200)).cuda()
    with pytest.raises(ValueError):
        dec.extend_shared(tok[:, :4])                                         # no prefill_shared yet
    with pytest.raises(ValueError):
        dec.reset_shared()
    dec.prefill_shared(torch.randint(0, 1000, (1, 150)).cuda())               # 128 in the prefix, 22 in the windows
    before = _snap(dec)
    with pytest.raises(L.GearError):
        dec.extend_shared(tok)                                                # 22 + 200 would compress 192 tokens: the tails hold 128
    with pytest.raises(ValueError):
        dec.extend_shared(tok[:1, :4])                                        # one row for two sequences
    with pytest.raises(ValueError):
        dec.extend_shared(tok[0, :4])
    with pytest.raises(NotImplementedError, match="extend_shared"):
        dec.extend(tok[:, :4])                                                # extend() keeps refusing while a prefix is live
    torch.cuda.synchronize()
    _same(_snap(dec), before)
    assert dec.extend_shared(tok[:, :100]).shape == (2, 100, 1000) and dec.pos == 250          # and the decoder is still usable


# ------------------------------------------------------------------------------------------------ F. decoder
# The measure of the existing chunk-against-step comparisons (test_gpu_extend: extend() logits against a restatement and against
# step(); test_gpu_verify: verify() against extend()): the smallest cosine over all logits rows above 0.999.  test_gpu_verify's
# _threshold (twice the largest verify-against-step logit difference, 2e-3 .. 4e-3 on this model) does not carry over: verify() and
# step() share the fused GEMV projections, while the chunk path projects with the library GEMM and, past a block boundary, compresses
# K / V rows that differ in their last bits -- measured here, an argmax flipped at a top-2 margin above that threshold with the
# logits rows at cosine 0.99994.
COS = 0.999


@pytest.mark.parametrize("P,n", [(150, 50), (150, 130), (40, 30)], ids=["one-boundary", "two-boundaries", "prompt-below-residual"])
def test_decoder_extend_shared_matches_teacher_forced_steps(P, n):
    """extend_shared(ids) against n teacher-forced step() calls on a twin: same pos / n_comp / n_win, logits rows and the next step's
    logits within COS (the chunk path projects with the library GEMM, the step path with the fused GEMV: no
    bit equality even in layer 0).  P = 40: the prompt is
    shorter than `residual`, shared_live is False and the chunk runs over the tails alone."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    S = 3
    g = torch.Generator().manual_seed(P + n)
    prompt = torch.randint(0, 1000, (1, P), generator=g).cuda()
    ids = torch.randint(0, 1000, (S, n + 1), generator=g).cuda()
    a = FastGearDecoder(model, 256, batch=S, seed=3, shared_prefix_tokens=128)
    b = FastGearDecoder(model, 256, batch=S, seed=3, shared_prefix_tokens=128)
    a.prefill_shared(prompt)
    b.prefill_shared(prompt)
    assert a.shared_live == (P >= 64)
    steps = torch.stack([a.step(ids[:, i]) for i in range(n)], 1)
    le = b.extend_shared(ids[:, :n])
    assert le.shape == (S, n, 1000)
    ca, cb = a.layers[0]["cache"], b.layers[0]["cache"]
    assert (b.pos, cb.n_comp, cb.n_win) == (a.pos, ca.n_comp, ca.n_win) == (P + n, (P % 64 + n) // 64 * 64, (P + n) % 64)
    cos = _cos(le, steps)
    na, nb = a.step(ids[:, n]), b.step(ids[:, n])
    cos2 = _cos(na, nb)
    print(f"extend_shared vs steps P {P} n {n}: cos {cos:.6f} next-step cos {cos2:.6f}")
    assert cos > COS and cos2 > COS, (cos, cos2)


@pytest.mark.parametrize("P", [150, 40], ids=["shared-live", "prompt-below-residual"])
def test_decoder_extend_shared_rows_match_plain_batch1(P):
    """Row s of extend_shared with S different suffixes against a plain batch-1 decoder that prefills prompt | suffix_s: the last
    row's logits and the next step's, within COS.  n = 60 crosses a block boundary (150 + 60 > 192;
    40 + 60 > 64)."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    S, n = 3, 60
    g = torch.Generator().manual_seed(P)
    prompt = torch.randint(0, 1000, (1, P), generator=g).cuda()
    suf = torch.randint(0, 1000, (S, n), generator=g).cuda()
    dec = FastGearDecoder(model, 256, batch=S, seed=3, shared_prefix_tokens=128)
    dec.prefill_shared(prompt)
    le = dec.extend_shared(suf)
    tok = le[:, -1].argmax(-1, keepdim=True)
    ls = dec.step(tok)
    assert dec.layers[0]["cache"].seq_len + dec.layers[0]["prefix"].n_comp == P + n + 1
    for s in range(S):
        plain = FastGearDecoder(model, 512, seed=3)
        lp = plain.prefill(torch.cat([prompt, suf[s:s + 1]], 1))
        lq = plain.step(tok[s:s + 1])
        c1, c2 = _cos(le[s:s + 1, -1], lp), _cos(ls[s:s + 1], lq)
        print(f"extend_shared row {s} vs plain prefill P {P}: cos {c1:.6f} next-step cos {c2:.6f}")
        assert c1 > COS and c2 > COS, (s, c1, c2)


def test_generate_with_suffixes():
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.sampling import SamplingParams
    model = _tiny("gearslKIVI", 2, left=0.02)
    P, n, L, S = 150, 50, 230, 4
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, 1000, (1, P), generator=g).cuda()
    suf = torch.randint(0, 1000, (S, n), generator=g).cuda()
    suf[1] = suf[0]                                                           # rows 0 and 1: the same message
    out = FastGearDecoder(model, 256, batch=S, seed=8, shared_prefix_tokens=128).generate(prompt, L, shared_prefix=True, suffix_ids=suf)
    assert out.shape == (S, L) and torch.equal(out[:, :P], prompt.expand(S, -1)) and torch.equal(out[:, P:P + n], suf)
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2])
    sp = SamplingParams(1.0, 0, 1.0, 11)
    run = lambda: FastGearDecoder(model, 256, batch=S, seed=8, shared_prefix_tokens=128).generate(prompt, L, sampling=sp,
                                                                                                 shared_prefix=True, suffix_ids=suf)
    sam = run()
    assert sam.shape == (S, L) and torch.equal(sam[:, :P + n], out[:, :P + n])
    assert not torch.equal(sam[0], sam[1])                                    # one seed, the same message: draws are keyed by sequence
    assert torch.equal(sam, run())
    with pytest.raises(ValueError):
        FastGearDecoder(model, 256, batch=S, shared_prefix_tokens=128).generate(prompt, P + n, shared_prefix=True, suffix_ids=suf)
    with pytest.raises(ValueError):
        FastGearDecoder(model, 256, batch=S).generate(prompt, L, suffix_ids=suf)            # suffix_ids needs shared_prefix=True


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_reset_shared_serves_the_next_batch_bit_identically(sampled):
    """Batch A, reset_shared(), batch B on one decoder against batch B on a fresh decoder: tokens and final logits bit for bit, the
    prefix pool untouched.  A runs past two block boundaries of the tails and B past one, so B re-appends block 0 over A's (its
    codes, lists, tiles and counts are rebuilt) and leaves A's second block stale behind the live counters."""
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.sampling import SamplingParams
    model = _tiny("gearslKIVI", 2, left=0.02)
    P, S = 150, 3
    g = torch.Generator().manual_seed(9)
    prompt = torch.randint(0, 1000, (1, P), generator=g).cuda()
    sufA = torch.randint(0, 1000, (S, 90), generator=g).cuda()
    sufB = torch.randint(0, 1000, (S, 40), generator=g).cuda()
    sp = SamplingParams(1.0, 0, 1.0, 5) if sampled else None
    seen = {}

    def serve(dec, suf, L, key, **kw):
        step = dec.step

        def rec(x):
            seen[key] = step(x)
            return seen[key]
        dec.step = rec
        try:
            return dec.generate(prompt, L, sampling=sp, shared_prefix=True, suffix_ids=suf, **kw)
        finally:
            dec.step = step

    dec = FastGearDecoder(model, 256, batch=S, seed=8, shared_prefix_tokens=128)
    serve(dec, sufA, P + 90 + 60, "A")
    assert dec.layers[0]["cache"].n_comp == 128
    prefix = {k: t.clone() for k, t in dec.prefix_pool.buf.items()}
    with pytest.raises(ValueError):
        dec.generate(prompt.flip(1), P + 60, sampling=sp, shared_prefix=True, suffix_ids=sufB, reuse_prefix=True)       # another prompt
    outB = serve(dec, sufB, P + 40 + 30, "B", reuse_prefix=True)
    fresh = FastGearDecoder(model, 256, batch=S, seed=8, shared_prefix_tokens=128)
    wantB = serve(fresh, sufB, P + 40 + 30, "fresh")
    assert torch.equal(outB, wantB)
    assert torch.equal(seen["B"], seen["fresh"])
    assert (dec.pos, dec.layers[0]["cache"].n_comp, dec.layers[0]["cache"].n_win) == \
        (fresh.pos, fresh.layers[0]["cache"].n_comp, fresh.layers[0]["cache"].n_win)
    for k, t in dec.prefix_pool.buf.items():
        assert torch.equal(t, prefix[k]) and torch.equal(t, fresh.prefix_pool.buf[k]), k
    # reset_shared() on its own: the state right after prefill_shared()
    dec.reset_shared()
    again = FastGearDecoder(model, 256, batch=S, seed=8, shared_prefix_tokens=128)
    again.prefill_shared(prompt)
    c, f = dec.layers[1]["cache"], again.layers[1]["cache"]
    assert (dec.pos, c.n_comp, c.n_win, c.seg0, c.kk0) == (again.pos, f.n_comp, f.n_win, f.seg0, f.kk0) == (P, 0, 22, 0, 0)
    assert torch.equal(c.kwin[:, :, :22], f.kwin[:, :, :22]) and torch.equal(c.vwin[:, :, :22], f.vwin[:, :, :22])
    assert torch.equal(dec.pool.gen.get_state(), again.pool.gen.get_state()) and torch.equal(c.gen.get_state(), f.gen.get_state())
