"""GPU tests of tree speculative verification: gear_attn_verify_tree (GearKVCache.attend_verify_tree) against the unchanged chain
kernel -- the chain mask repeats it, every row of a tree equals the chain of its root path --, aimed one-row probes of the mask
(tests/attn_probe.py), mask isolation, the mask sanitisation, no state change; FastGearDecoder.verify_tree / accept_path on both
cache kinds; generate_speculative(tree_width=2) against plain greedy decoding; and the refusals."""
import numpy as np
import pytest
import torch

import attn_probe as AP
from conftest import rel_fro
from test_gpu_attn_probe import _cc
from test_gpu_verify import _chunk, _compare, _cos, _filled, _greedy, _same_state, _state, _threshold, _tiny, host

pytestmark = pytest.mark.gpu

NS = (1, 2, 5, 16)


def chain(n):
    return [-1] + list(range(n - 1))


def star(n):
    return [-1] + [0] * (n - 1)


def binary(n):
    return [-1] + [(i - 1) // 2 for i in range(1, n)]


def two_chains(n):
    return ([-1, 0, 0] + list(range(1, n - 2)))[:n]


def _layout(par, dev="cuda"):
    from gear_amd.speculative import tree_layout
    anc, depth = tree_layout(torch.tensor(par))
    return anc.view(torch.int32)[0].to(dev), depth[0].tolist()


def _path(par, i):
    p = []
    while i >= 0:
        p.append(i)
        i = par[i]
    return p[::-1]


# method, bits, group, residual, rank, left, Hq, Hkv, prompt, committed: 128 compressed tokens (none in the last), W = committed
CASES = [
    ("KIVI", 2, 64, 64, 4, 0.0, 2, 2, 128, 0),
    ("KIVI", 2, 64, 64, 4, 0.0, 8, 2, 128, 63),
    ("gearlKIVI", 2, 64, 64, 4, 0.0, 8, 2, 128, 5),
    ("gearslKIVI", 2, 64, 64, 4, 0.02, 2, 2, 128, 5),
    ("gearslKIVI", 2, 64, 64, 4, 0.02, 8, 2, 128, 63),
    ("gearslKIVI", 2, 64, 64, 4, 0.02, 8, 2, 128, 0),
    ("gearlKIVI", 4, 32, 128, 8, 0.0, 8, 2, 128, 5),           # 4 bits
    ("gearlKIVI", 2, 64, 64, 4, 0.0, 2, 2, 30, 0),             # T = 0: the window only
]
IDS = [f"{c[0]}-b{c[1]}-{c[6]}x{c[7]}-{c[8]}+{c[9]}" for c in CASES]


def _case(case, seed=11):
    method, bits, group, R, rank, left, Hq, Hkv, T0, more = case
    c = _filled(_cc(method, bits, group, R, rank, left=left), 2, Hkv, T0, more, seed=seed)
    assert (c.n_comp, c.n_win) == ((128, more) if T0 == 128 else (0, T0))
    return c, Hq


def _inputs(c, Hq, n, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(c.B, Hq, n, 128, generator=g).half().cuda()
    kn, vn = _chunk(c, n, seed + 1)
    return q, kn, vn


def _noise(fn, repeats=4):
    """Identical calls: (first result, largest |difference| to it of out, of lse).  The vector kernels add the outlier terms with
    LDS float atomics, so a cache with outliers may differ in the last bits from run to run -- in some runs only: a sample of
    identical calls that agree does not show that the next one will."""
    a, la = fn()
    noise = lnoise = 0.0
    for _ in range(repeats):
        b, lb = fn()
        noise, lnoise = max(noise, float((a.float() - b.float()).abs().max())), max(lnoise, float((la - lb).abs().max()))
    return a, la, noise, lnoise


def _same(tag, a, la, b, lb, noise, lnoise, exact):
    """exact (no outliers: the sums are order-fixed, identical calls give identical bits): equal in every element.  With outliers:
    within test_verify_is_causal's max(4 x noise, 5e-4), also where the sampled noise happened to be zero."""
    assert (noise == 0.0 and lnoise == 0.0) or not exact, (tag, noise, lnoise)
    assert a.shape == b.shape and la.shape == lb.shape and a.dtype == b.dtype and la.dtype == lb.dtype
    assert bool(torch.isfinite(b).all()) and bool(torch.isfinite(lb).all()), tag
    do, dl = float((a.float() - b.float()).abs().max()), float((la - lb).abs().max())
    print(f"{tag}: out diff {do:.3g} (noise {noise:.3g}), lse diff {dl:.3g} (noise {lnoise:.3g})")
    if exact:
        assert do == 0.0 and dl == 0.0, (tag, do, dl)
    else:
        assert do <= max(4 * noise, 5e-4) and dl <= max(4 * lnoise, 5e-4), (tag, do, dl)


# ------------------------------------------------------------------------------------------------ 1: the chain mask
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chain_mask_equals_verify(case):
    c, Hq = _case(case)
    for n in NS:
        q, kn, vn = _inputs(c, Hq, n, n)
        a, la, noise, lnoise = _noise(lambda: c.attend_verify(q, kn, vn, return_lse=True))
        anc, _ = _layout(chain(n))
        b, lb = c.attend_verify_tree(q, kn, vn, anc, return_lse=True)
        _same(f"chain n={n}", a, la, b, lb, noise, lnoise, case[5] == 0.0)
        b2 = c.attend_verify_tree(q, kn, vn, anc.view(torch.uint32).expand(2, n))          # uint32 [B, n], no lse
        _same(f"chain n={n} [B, n]", a, la, b2, la, noise, lnoise, case[5] == 0.0)


# ------------------------------------------------------------------------------------------------ 2: rows against their path
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_row_equals_the_chain_of_its_root_path(case):
    c, Hq = _case(case, seed=12)
    worst = worst_l = 0.0
    for topo in (star, binary, two_chains):
        for n in (2, 5, 16):
            par = topo(n)
            anc, depth = _layout(par)
            q, kn, vn = _inputs(c, Hq, n, 3 * n)
            out, lse = c.attend_verify_tree(q, kn, vn, anc, return_lse=True)
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
            for i in range(n):
                p = _path(par, i)
                assert len(p) == depth[i] + 1
                ro, rl = c.attend_verify(q[:, :, p].contiguous(), kn[:, :, p].contiguous(), vn[:, :, p].contiguous(), return_lse=True)
                e = rel_fro(host(out[:, :, i]), host(ro[:, :, -1]))
                el = float((lse[:, :, i] - rl[:, :, -1]).abs().max())
                worst, worst_l = max(worst, e), max(worst_l, el)
                assert e < 2e-3 and el < 1e-2, (topo.__name__, n, i, e, el)
    print(f"rows vs root-path chains: rel_fro {worst:.3g}, lse {worst_l:.3g}")


# ------------------------------------------------------------------------------------------------ 3: aimed probes
@pytest.mark.parametrize("topo,n,case", [(binary, 7, CASES[3]), (binary, 7, CASES[2]), (two_chains, 16, CASES[4])],
                         ids=["binary7-W5-mha", "binary7-W5-gqa", "two-chains16-W63"])
def test_aimed_probes_read_ancestors_only(topo, n, case):
    """Round r aims row i (i >= r) at chunk row r: an ancestor-or-self must be read (the reference without it lies past 5 x the
    bounds), any other row must not (the row stays within the bounds of its root path's float64 reference, where the chain kernel
    -- which does read it -- lies past 5 x).  Every pair (i, j <= i) is probed, so a mask that is off by one row fails."""
    c, Hq = _case(case, seed=13)
    B, Hkv = c.B, c.H
    G = Hq // Hkv
    par = topo(n)
    anc, depth = _layout(par)
    kn, vn = _chunk(c, n, 7)
    full = AP.decompose(c, kn=kn, vn=vn)
    Kall, _ = AP.keys(full)
    base = full["T"] + full["W"]
    rng = np.random.default_rng(5)
    paths = [_path(par, i) for i in range(n)]
    row_parts = []
    for p in paths:
        m = dict(full)
        m.update(kn=full["kn"][:, :, p], vn=full["vn"][:, :, p], n=len(p))
        row_parts.append(m)
    seen = {"anc": set(), "non": set()}
    worst = 0.0
    for r in range(n):
        q = AP.f16(rng.standard_normal((B, Hq, n, 128)))
        probed = []                                     # (b, hq, i)
        for b in range(B):
            for h in range(Hkv):
                qv = AP.aim(Kall[b, h], [base + r])
                if qv is None:
                    continue
                for i in range(r, n):
                    hq = h * G + (i + r) % G
                    q[b, hq, i] = qv
                    probed.append((b, hq, i))
        qt = torch.tensor(q, dtype=torch.float16, device="cuda")
        out, lse = c.attend_verify_tree(qt, kn, vn, anc, return_lse=True)
        cout, clse = c.attend_verify(qt, kn, vn, return_lse=True)
        out, lse, cout, clse = (host(t).astype(np.float64) for t in (out, lse, cout, clse))
        assert np.isfinite(out).all() and np.isfinite(lse).all()
        refs = [AP.ref(q[:, :, i:i + 1], row_parts[i], rows=[depth[i]]) for i in range(n)]
        for i in range(n):                              # every row, probed or not, against its path
            ro, rl = refs[i]
            s = AP.signal(out[:, :, i:i + 1], lse[:, :, i:i + 1], ro, rl)
            worst = max(worst, s)
            assert s <= 1.0, ("row", r, i, s)
        for b, hq, i in probed:
            sl = (slice(b, b + 1), slice(hq, hq + 1))
            ro, rl = refs[i]
            if r in paths[i]:
                mo, ml = AP.ref(q[:, :, i:i + 1], AP.mutate(row_parts[i], "M1-drop", base + paths[i].index(r)), rows=[depth[i]])
                s = AP.signal(out[sl][:, :, i:i + 1], lse[sl][:, :, i:i + 1], mo[sl], ml[sl])
                assert s > 5.0, ("ancestor not read", r, i, s)
                seen["anc"].add((i, r))
            else:
                s = AP.signal(cout[sl][:, :, i:i + 1], clse[sl][:, :, i:i + 1], ro[sl], rl[sl])
                assert s > 5.0, ("the probe does not tell the chain kernel apart", r, i, s)
                seen["non"].add((i, r))
    pairs = {(i, j) for i in range(n) for j in range(i + 1)}
    want_anc = {(i, j) for i, j in pairs if j in paths[i]}
    assert seen["anc"] == want_anc and seen["non"] == pairs - want_anc, (want_anc - seen["anc"], pairs - want_anc - seen["non"])
    print(f"aimed probes: {len(want_anc)} ancestor pairs, {len(pairs - want_anc)} other pairs, worst signal {worst:.3g} of 1")


# ------------------------------------------------------------------------------------------------ 4: mask isolation
@pytest.mark.parametrize("method,left", [("gearlKIVI", 0.0), ("gearslKIVI", 0.02)], ids=["no-outliers", "outliers"])
def test_mask_isolation(method, left):
    """Perturbing chunk row j moves row i iff j is i or an ancestor of i (test_verify_is_causal's bounds)."""
    c = _filled(_cc(method, left=left), 2, 2, 128, 5, seed=3)
    n = 16
    par = two_chains(n)
    anc, _ = _layout(par)
    q, kn, vn = _inputs(c, 8, n, 5)
    a = c.attend_verify_tree(q, kn, vn, anc)
    noise = float((c.attend_verify_tree(q, kn, vn, anc).float() - a.float()).abs().max())
    if left == 0.0:
        assert noise == 0.0
    for j in (0, 1, 2, 6, 9, 15):
        kn2, vn2 = kn.clone(), vn.clone()
        kn2[:, :, j] += 1.0
        vn2[:, :, j] -= 1.0
        b = c.attend_verify_tree(q, kn2, vn2, anc)
        for i in range(n):
            d = float((a[:, :, i].float() - b[:, :, i].float()).abs().max())
            if j in _path(par, i):
                assert d > max(16 * noise, 2e-3), (j, i, d, noise)
            elif left == 0.0:
                assert torch.equal(a[:, :, i], b[:, :, i]), (j, i)
            else:
                assert d <= max(4 * noise, 5e-4), (j, i, d, noise)


# ------------------------------------------------------------------------------------------------ 5: sanitisation
@pytest.mark.parametrize("case", [CASES[2], CASES[4], CASES[7]], ids=["no-outliers", "outliers", "T0"])
def test_mask_sanitisation(case):
    """Bits above i and a clear bit i change nothing: the kernel uses (anc | 1 << i) & ((2 << i) - 1).  All-zero masks: every row
    sees the cache, the window and itself."""
    c, Hq = _case(case, seed=14)
    g = torch.Generator().manual_seed(8)
    for n in (1, 5, 16):
        q, kn, vn = _inputs(c, Hq, n, 20 + n)
        raw = torch.randint(0, 1 << 32, (2, n), generator=g)
        raw[0, 0] = 0xFFFFFFFF
        row = torch.arange(n)
        clean = (raw | (1 << row)) & ((2 << row) - 1)

        def dev(m):                                     # the 32 bits as int32 (n = 5) or uint32
            m = torch.where(m >= 1 << 31, m - (1 << 32), m).to(torch.int32)
            return (m if n == 5 else m.view(torch.uint32)).cuda()
        a, la, noise, lnoise = _noise(lambda: c.attend_verify_tree(q, kn, vn, dev(clean), return_lse=True))
        b, lb = c.attend_verify_tree(q, kn, vn, dev(raw), return_lse=True)
        assert bool(torch.isfinite(b).all()) and bool(torch.isfinite(lb).all())
        _same(f"sanitised n={n}", a, la, b, lb, noise, lnoise, case[5] == 0.0)
        b, lb = c.attend_verify_tree(q, kn, vn, dev(clean & ~(1 << row)), return_lse=True)      # bit i clear
        _same(f"own bit n={n}", a, la, b, lb, noise, lnoise, case[5] == 0.0)
        z, lz = c.attend_verify_tree(q, kn, vn, torch.zeros(n, dtype=torch.int32, device="cuda"), return_lse=True)
        assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(lz).all())
        s, ls = c.attend_verify_tree(q, kn, vn, (1 << row).to(torch.int32).cuda(), return_lse=True)
        _same(f"zero n={n}", s, ls, z, lz, noise, lnoise, case[5] == 0.0)
        for i in range(n):
            ro, rl = c.attend_verify(q[:, :, i:i + 1].contiguous(), kn[:, :, i:i + 1].contiguous(), vn[:, :, i:i + 1].contiguous(),
                                     return_lse=True)
            assert rel_fro(host(z[:, :, i]), host(ro[:, :, 0])) < 2e-3 and float((lz[:, :, i] - rl[:, :, 0]).abs().max()) < 1e-2


# ------------------------------------------------------------------------------------------------ 6: no state change
def test_verify_tree_changes_no_state():
    c = _filled(_cc(), 2, 2, 200, 100, seed=4)
    before = {k: t.clone() for k, t in c.bufs.items()}
    counters = (c.n_comp, c.n_win, c.seg0, c.kk0)
    for n in (1, 4, 16):
        q, kn, vn = _inputs(c, 8, n, n)
        c.attend_verify_tree(q, kn, vn, _layout(binary(n))[0], return_lse=True)
    torch.cuda.synchronize()
    assert (c.n_comp, c.n_win, c.seg0, c.kk0) == counters
    for k, t in c.bufs.items():
        assert torch.equal(t, before[k]), k
    with pytest.raises(ValueError):
        c.attend_verify_tree(q, kn, vn, torch.zeros(3, dtype=torch.int32, device="cuda"))          # [3] for n = 16
    with pytest.raises(ValueError):
        c.attend_verify_tree(q, kn, vn, torch.zeros(16, dtype=torch.int64, device="cuda"))


def test_fp16_baseline_matches_the_kernel():
    """Fp16KVCache.attend_verify_tree (torch SDPA) against the kernel over a window-only cache with the same rows."""
    from gear_amd.cache import Fp16KVCache
    c = _filled(_cc("gearlKIVI", left=0.0), 2, 2, 30, 0, seed=6)
    f = Fp16KVCache(2, 2, 64, "cuda")
    f.prefill(c.kwin[:, :, :30].clone(), c.vwin[:, :, :30].clone())
    for n, topo in ((5, binary), (16, two_chains)):
        anc, _ = _layout(topo(n))
        q, kn, vn = _inputs(c, 8, n, n)
        a, la = c.attend_verify_tree(q, kn, vn, anc, return_lse=True)
        b, lb = f.attend_verify_tree(q, kn, vn, anc, return_lse=True)
        assert rel_fro(host(a), host(b)) < 2e-3 and float((la - lb).abs().max()) < 1e-2
        garbage = anc | (-1 << 16)                      # bits no row may use
        assert torch.equal(f.attend_verify_tree(q, kn, vn, garbage), b)


# ------------------------------------------------------------------------------------------------ 7: decoder
@pytest.mark.parametrize("kind,method,left", [("gear", "gearlKIVI", 0.0), ("gear", "gearslKIVI", 0.02), ("fp16", "gearslKIVI", 0.02)],
                         ids=["gear-no-outliers", "gear-outliers", "fp16"])
def test_decoder_chain_tree_equals_verify_and_accept(kind, method, left):
    """verify_tree with chain parents = verify(); accept_path(arange(m)) leaves the state of verify() + accept(m), bit for bit.
    P = 190: the rows cross the block boundary at 192 for m = n."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny(method, 2, left=left)
    P, n, B = 190, 6, 2
    ids = torch.randint(0, 1000, (B, P + n)).cuda()
    par = torch.tensor(chain(n))
    for m in (0, 1, n):
        a = FastGearDecoder(model, 512, batch=B, seed=4, cache_kind=kind)
        b = FastGearDecoder(model, 512, batch=B, seed=4, cache_kind=kind)
        a.prefill(ids[:, :P])
        b.prefill(ids[:, :P])
        before = _state(a)
        lv = b.verify(ids[:, P:])
        noise = float((b.verify(ids[:, P:]).float() - lv.float()).abs().max())
        lt = a.verify_tree(ids[:, P:], par if m else par.expand(B, n).cuda())
        torch.cuda.synchronize()
        _same_state(_state(a), before)
        d = float((lt.float() - lv.float()).abs().max())
        print(f"{kind} m={m}: |verify_tree - verify| logits {d:.3g}, verify run-to-run {noise:.3g}")
        exact = left == 0.0 or kind == "fp16"         # (no outlier sums in the pass: identical calls give identical bits)
        if exact:
            assert noise == 0.0 and torch.equal(lt, lv)
        else:
            assert d <= max(4 * noise, 5e-4)
        assert a.accept_path(torch.arange(m)) == m
        assert b.accept(m) == m
        torch.cuda.synchronize()
        if exact:
            _same_state(_state(a), _state(b))
        else:                                   # (each pass commits its own rows; the counters agree)
            assert _state(a)[1:] == _state(b)[1:]
        assert a.pos == P + m
        c0 = a.layers[0]["cache"]
        if kind == "gear":
            assert (c0.n_comp, c0.n_win) == ((192, P + m - 192) if P + m >= 192 else (128, P + m - 128))


@pytest.mark.parametrize("kind", ["gear", "fp16"])
def test_decoder_accept_path_commits_exactly_the_rows(kind):
    """accept_path(idx) = extend_all of the pending rows idx, bit for bit, on a branching tree (the second branch), across the
    block boundary at 192."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    P, n = 190, 7
    ids = torch.randint(0, 1000, (1, P + n)).cuda()
    a = FastGearDecoder(model, 512, seed=4, cache_kind=kind)
    b = FastGearDecoder(model, 512, seed=4, cache_kind=kind)
    a.prefill(ids[:, :P])
    b.prefill(ids[:, :P])
    a.verify_tree(ids[:, P:], torch.tensor(two_chains(n)))
    idx = [0, 2, 4, 6]
    ks = [k[:, :, idx].clone() for k in a._pending_tree["ks"]]
    vs = [v[:, :, idx].clone() for v in a._pending_tree["vs"]]
    assert a.accept_path(torch.tensor(idx)) == 4
    if kind == "gear":
        b.pool.extend_all(ks, vs)
    else:
        for lw, k, v in zip(b.layers, ks, vs):
            lw["cache"].extend(k, v)
    b.pos += 4
    torch.cuda.synchronize()
    _same_state(_state(a), _state(b))


@pytest.mark.parametrize("kind", ["gear", "fp16"])
def test_decoder_branch_then_step_matches_token_steps(kind):
    """A branching tree: the logits of the second branch's nodes, and of a step() after accept_path of that branch, agree with a
    decoder stepped token by token along the same path (test_decoder_verify_matches_extend_and_changes_nothing's measure)."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    P, B, n = 150, 2, 7
    ids = torch.randint(0, 1000, (B, P + n + 1)).cuda()
    par = two_chains(n)
    idx = [0, 2, 4, 6]
    a = FastGearDecoder(model, 512, batch=B, seed=3, cache_kind=kind)
    b = FastGearDecoder(model, 512, batch=B, seed=3, cache_kind=kind)
    a.prefill(ids[:, :P])
    b.prefill(ids[:, :P])
    before = _state(a)
    lt = a.verify_tree(ids[:, P:P + n], torch.tensor(par))
    torch.cuda.synchronize()
    _same_state(_state(a), before)
    assert lt.shape == (B, n, 1000)
    steps = torch.stack([b.step(ids[:, P + i:P + i + 1]) for i in idx], 1)
    assert a.accept_path(torch.tensor(idx).expand(B, -1)) == 4
    la, lb = a.step(ids[:, P + n:]), b.step(ids[:, P + n:])
    rel = float((lt[:, idx].float() - steps.float()).abs().max() / steps.float().abs().max())
    print(f"{kind}: cos(tree rows, steps) {_cos(lt[:, idx], steps):.6f}, rel max {rel:.3g}; cos(step after) {_cos(la, lb):.6f}")
    assert _cos(lt[:, idx], steps) > 0.999
    assert _cos(la, lb) > 0.999
    assert a.pos == b.pos == P + 5
    assert _state(a)[1:] == _state(b)[1:]


def test_verify_tree_refusals(monkeypatch):
    from gear_amd import _lib as L
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.sampling import SamplingParams
    model = _tiny("gearslKIVI", 2, left=0.02)
    dec = FastGearDecoder(model, 192, seed=1)
    tok = lambda n: torch.randint(0, 1000, (1, n)).cuda()
    par = torch.tensor(binary(7))
    with pytest.raises(ValueError):
        dec.verify_tree(tok(7), par)                               # no prefill yet
    with pytest.raises(ValueError):
        dec.accept_path(torch.tensor([0]))                         # nothing pending
    with pytest.raises(NotImplementedError):
        dec.generate_speculative(tok(100), 120, tree_width=2, sampling=SamplingParams(temperature=0.8, seed=1))
    assert dec.pos == 0
    dec.prefill(tok(240))                                          # 192 compressed (the capacity) + 48 in the window
    assert dec._room() == 15
    snap = _state(dec)
    with pytest.raises(L.GearError):
        dec.verify_tree(tok(16), torch.tensor(chain(16)))          # the deepest path has 16 rows: one block too many
    dec.verify_tree(tok(16), torch.tensor(two_chains(16)))         # ... 9 rows: fits
    with pytest.raises(ValueError):
        dec.verify_tree(tok(7), torch.tensor(binary(6)))           # n nodes, n - 1 parents
    with pytest.raises(ValueError):
        dec.verify_tree(tok(3), torch.tensor([-1, 1, 0]))          # out of order
    with pytest.raises(ValueError):
        dec.verify_tree(tok(17), torch.tensor(chain(17)))
    dec.verify(tok(3))
    with pytest.raises(ValueError):
        dec.accept_path(torch.tensor([0, 1]))                      # a verify() is pending: accept() only
    assert dec.accept(0) == 0
    dec.verify_tree(tok(7), par)
    with pytest.raises(ValueError):
        dec.accept(1)                                              # a verify_tree() is pending: accept_path() only
    for bad in ([1], [0, 3], [0, 1, 2], [0, 2, 7], [0, -1], [0] * 8, [[0, 1], [0, 2]]):
        with pytest.raises(ValueError):
            dec.accept_path(torch.tensor(bad))
    with pytest.raises(ValueError):
        dec.accept_path(torch.tensor([0, 1], dtype=torch.int32))
    torch.cuda.synchronize()
    _same_state(_state(dec), snap)
    assert dec.accept_path(torch.tensor([0, 2, 5])) == 3           # the pending pass survived the refusals
    with pytest.raises(ValueError):
        dec.accept_path(torch.tensor([0]))                         # ... and is consumed now
    snap = _state(dec)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(NotImplementedError):
        dec.verify_tree(tok(7), par)
    monkeypatch.undo()
    dec.tp_world = 2                                               # (a sharded decoder's attribute: the check comes first)
    with pytest.raises(NotImplementedError):
        dec.verify_tree(tok(7), par)
    dec.tp_world = 1
    with pytest.raises(ValueError):
        dec.generate_speculative(tok(100), 120, tree_width=2, draft=lambda t, k: t[:, :k])
    with pytest.raises(ValueError):
        dec.generate_speculative(tok(100), 120, tree_width=0)
    _same_state(_state(dec), snap)
    # a live shared prefix refuses trees as it refuses verify()
    sh = FastGearDecoder(model, 256, batch=2, seed=1, shared_prefix_tokens=128)
    sh.prefill_shared(tok(150))
    snap = _state(sh)
    for call in (lambda: sh.verify_tree(torch.randint(0, 1000, (2, 7)).cuda(), par), lambda: sh.accept_path(torch.tensor([0])),
                 lambda: sh.generate_speculative(tok(150), 160, tree_width=2)):
        with pytest.raises(NotImplementedError):
            call()
    _same_state(_state(sh), snap)


# ------------------------------------------------------------------------------------------------ 8: generation
def _repetitive(rows, seed=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1000, (rows, 12), generator=g).repeat(1, 12).cuda()      # 144 tokens per row, a 12-token pattern each


def test_generate_tree_matches_greedy():
    """test_generate_speculative_matches_greedy's rule (_compare: equal up to the first token whose top-2 margin is under the
    measured threshold, at least 24 tokens compared): first for the chain at the same draft size, then for tree_width = 2."""
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    ids = _repetitive(3)
    P, gen = ids.shape[1], 64
    thr = _threshold(model, ids)
    plain, margins = _greedy(model, ids, P + gen)
    for width in (1, 2):
        dec = FastGearDecoder(model, 1024, batch=3, seed=8)
        out, st = dec.generate_speculative(ids, P + gen, draft="ngram", n_draft=7, return_stats=True, tree_width=width)
        assert out.shape == (3, P + gen) and st["tokens"] == gen
        assert set(st) == {"passes", "tokens", "tokens_per_pass", "drafted", "accepted", "acceptance_rate"}
        total = _compare(out, plain, margins, P, thr, 24)
        print(f"tree_width {width}: {total} tokens compared (thr {thr:.3g}), {st}")


def _planted(model, P=150, tries=12, seed=21, older=True):
    """A prompt [1, P] whose last token + the model's first generated token (the trailing bigram of the first pass) occur twice
    before: the older occurrence continues as plain greedy decoding does (teacher forcing: the continuation is read off a greedy
    run of the prompt itself, re-planted until the run agrees with what was planted), the more recent one otherwise."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 500, (1, P), generator=g).cuda()
    right, other = (20, 80) if older else (80, 20)
    last = int(ids[0, -1])
    planted = None
    for _ in range(tries):
        plain, margins = _greedy(model, ids, P + 10)
        f, g1, g2, g3 = (int(t) for t in plain[0, P:P + 4])
        if planted == (f, g1, g2, g3):
            return ids, plain, margins
        planted = (f, g1, g2, g3)
        ids[0, right:right + 5] = torch.tensor([last, f, g1, g2, g3])             # (older: the first occurrence) what greedy does
        ids[0, other:other + 5] = torch.tensor([last, f, 500 + g1 % 400, 901, 902])          # the other one: something else
    raise AssertionError("no self-consistent planted prompt found")


def test_tree_accepts_the_older_continuation():
    """The behavioural reason for trees: the model follows the second-most-recent continuation of the trailing bigram.  The
    chain drafter proposes the most recent one and its first pass accepts nothing; the tree holds both and accepts more."""
    from gear_amd.fast_decode import FastGearDecoder
    from gear_amd.speculative import ngram_draft, ngram_tree_draft
    model = _tiny("gearslKIVI", 2, left=0.02)
    ids, plain, margins = _planted(model)
    P = ids.shape[1]
    thr = _threshold(model, ids)
    assert float(margins[0, :3].min()) > thr, (margins[0, :4], thr)                 # the planted tokens are no near-ties
    seen = plain[:, :P + 1]
    assert ngram_draft(seen, 7)[0, 0] != plain[0, P + 1]                          # the chain draft starts on the wrong branch
    d, par = ngram_tree_draft(seen, 8, 2)
    assert int(plain[0, P + 1]) in d[0, (par[0, 1:] == 0)].tolist()               # the tree has the right one under the root
    first = {}
    for width in (1, 2):
        dec = FastGearDecoder(model, 1024, seed=8)
        commits = []
        for name in ("accept", "accept_path"):
            def spy(x, _f=getattr(dec, name)):
                commits.append(x if isinstance(x, int) else x.shape[-1])
                return _f(x)
            setattr(dec, name, spy)
        out = dec.generate_speculative(ids, P + 10, draft="ngram", n_draft=7, tree_width=width)
        assert torch.equal(out[:, :P + 3], plain[:, :P + 3]), width
        first[width] = commits[0] - 1                                            # a pass commits its accepted drafts + 1
    print(f"first pass: accepted {first}")
    assert first[1] == 0 and first[2] > first[1]


def test_generate_tree_batch_commits_the_minimum(monkeypatch):
    """Batch 2: row 0 follows the older continuation (the tree's second branch), row 1 the most recent one (its first branch).
    Every pass commits the batch's minimum path length, each row its own path, and both rows stay greedy."""
    from gear_amd import speculative as S
    from gear_amd.fast_decode import FastGearDecoder
    model = _tiny("gearslKIVI", 2, left=0.02)
    ids = torch.cat([_planted(model)[0], _planted(model, seed=22, older=False)[0]], 0)
    P, gen = ids.shape[1], 24
    thr = _threshold(model, ids)
    plain, margins = _greedy(model, ids, P + gen)
    lengths, commits = [], []
    real = S.tree_accept

    def accept_spy(*a):
        r = real(*a)
        lengths.append(r[1].tolist())
        return r
    monkeypatch.setattr(S, "tree_accept", accept_spy)
    dec = FastGearDecoder(model, 1024, batch=2, seed=8)
    path_real = dec.accept_path

    def path_spy(idx):
        commits.append(idx.clone().cpu())
        return path_real(idx)
    dec.accept_path = path_spy
    out, st = dec.generate_speculative(ids, P + gen, draft="ngram", n_draft=7, return_stats=True, tree_width=2)
    print(f"batch 2: {st}, path lengths {lengths}, first commit {commits[0].tolist()}")
    _compare(out, plain, margins, P, thr, 16)
    assert len(lengths) == len(commits) == st["passes"]
    assert all(c.shape == (2, min(l)) for c, l in zip(commits, lengths))
    assert st["accepted"] == sum(min(l) - 1 for l in lengths)
    assert commits[0].shape[1] >= 2 and not torch.equal(commits[0][0], commits[0][1]), "the rows took no different paths"
