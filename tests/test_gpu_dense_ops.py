"""The dense decode-step kernels (csrc/gemv_f16.hip, csrc/decode_ops.hip) element by element against the float64 reference of
tests/dense_ref.py: every output element must be one of the fp16 values the reference derives as admissible (one value for most
elements, two near a rounding boundary) -- no scalar tolerance anywhere.  tests/test_dense_ref_cpu.py shows on the CPU that a correct
implementation passes these very cases and that the faults the sets are for are caught.

Every reachable gemv_tok_kernel<NB, SK, NORM, EPI> and the case that launches it (checked against pick_sk's rules, read from the
code: sk = 4 for N <= 8192 and K >= 8192, else 2, capped at 2 by the SwiGLU and RoPE entry points -- SK = 1 is never launched; NB is
the batch, and every case runs B = 1 .. 4 unless noted):"""
import numpy as np
import pytest
import torch

import dense_ref as R

gpu = pytest.mark.gpu
PLAIN, SWIGLU, ROPE = 0, 1, 2

# (SK, NORM, EPI) -> the case; each stands for the four NB = 1 .. 4 instantiations
INSTANTIATIONS = {
    (2, 0, PLAIN): "test_gemv_plain_and_residual, K < 8192",
    (4, 0, PLAIN): "test_gemv_plain_and_residual, K = 8192 and 8264",
    (2, 1, PLAIN): "test_gemv_norm, no delta, no norm_w, swiglu 0, K < 8192",
    (2, 2, PLAIN): "test_gemv_norm, delta with and without norm_w, swiglu 0, K < 8192",
    (2, 3, PLAIN): "test_gemv_norm, norm_w only, swiglu 0, K < 8192",
    (4, 1, PLAIN): "test_gemv_norm, no delta, no norm_w, K = 8264",
    (4, 2, PLAIN): "test_gemv_norm, delta with and without norm_w, K = 8264",
    (4, 3, PLAIN): "test_gemv_norm, norm_w only, K = 8264",
    (2, 1, SWIGLU): "test_gemv_norm, no delta, no norm_w, swiglu 1 and 2",
    (2, 2, SWIGLU): "test_gemv_norm, delta with and without norm_w, swiglu 1 and 2",
    (2, 3, SWIGLU): "test_gemv_norm, norm_w only, swiglu 1 and 2",
    (2, 1, ROPE): "test_gemv_qkv_rope_and_rope_append, no delta, no norm_w",
    (2, 2, ROPE): "test_gemv_qkv_rope_and_rope_append, delta (with and without norm_w)",
    (2, 3, ROPE): "test_gemv_qkv_rope_and_rope_append, norm_w only",
}


def test_instantiation_table_matches_the_launch_rules():
    """The table above against what the cases reach under pick_sk's rules as dense_ref.pick_sk mirrors them from gemv_f16.hip."""
    reached = set()
    for K, N in R.GEMV_SHAPES:
        reached |= {(B, R.pick_sk(K, N, 4), 0, PLAIN) for B in (1, 2, 3, 4)}
    for K, N, modes in R.NORM_SHAPES:
        for _, norm in R.norm_variants():
            for sw in modes:
                reached |= {(B, R.pick_sk(K, N, 2 if sw else 4), norm, SWIGLU if sw else PLAIN) for B in (1, 2, 3, 4)}
    for rc in R.rope_cases():
        Hq, Hkv = rc["heads"]
        norm = dict(R.norm_variants())[(rc["has_d"], rc["has_w"])]
        reached.add((rc["B"], R.pick_sk(rc["K"], (Hq + 2 * Hkv) * 128, 2), norm, ROPE))
    want = {(B,) + k for k in INSTANTIATIONS for B in (1, 2, 3, 4)}
    assert len(want) == 56
    # the RoPE cases spread B = 1 .. 4 over each norm variant's five cases instead of crossing them
    assert reached >= {w for w in want if w[3] != ROPE} and reached <= want
    assert {(w[1], w[2]) for w in reached if w[3] == ROPE} == {(2, 1), (2, 2), (2, 3)}
    assert {w[0] for w in reached if w[3] == ROPE} == {1, 2, 3, 4}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def host(t):
    return t.cpu().numpy()


def sentinel(*shape):
    """An fp16 tensor filled with a NaN payload no kernel produces: a write of anything, zeros included, shows."""
    return torch.full(shape, R.SENTINEL, dtype=torch.int16).view(torch.float16).cuda()


def untouched(t):
    return bool((t.view(torch.int16) == R.SENTINEL).all())


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.fixture(scope="module")
def lib():
    from gear_amd import _lib as L
    return L, L.load()


@gpu
@pytest.mark.parametrize("K,N", R.GEMV_SHAPES)
def test_gemv_plain_and_residual(lib, K, N):
    L, g = lib
    for B in (1, 2, 3, 4):
        c = R.gemv_case(K, N, B)
        x, W, res = dev(c["x"]), dev(c["W"]), dev(c["res"])
        what = "K=%d N=%d B=%d" % (K, N, B)
        y = sentinel(B, N)
        L.check(g.gear_gemv_f16(L.ptr(x), L.ptr(W), B, K, N, L.ptr(y), L.stream_ptr()), "gemv")
        R.assert_admissible(host(y), R.gemv_f16(c["x"], c["W"]), "gear_gemv_f16 " + what)
        y2 = sentinel(B, N)
        L.check(g.gear_gemv_f16_add(L.ptr(x), L.ptr(W), B, K, N, L.ptr(res), L.ptr(y2), L.stream_ptr()), "add")
        R.assert_admissible(host(y2), R.gemv_f16(c["x"], c["W"], c["res"]), "gear_gemv_f16_add " + what)
        r1 = res.clone()                                   # res_in aliasing y, as the decoders call it
        L.check(g.gear_gemv_f16_add(L.ptr(x), L.ptr(W), B, K, N, L.ptr(r1), L.ptr(r1), L.stream_ptr()), "add in place")
        assert same_bits(r1, y2), "in-place residual add differs " + what
        assert same_bits(x, dev(c["x"])) and same_bits(res, dev(c["res"]))


@gpu
@pytest.mark.parametrize("K,N,modes", R.NORM_SHAPES)
def test_gemv_norm(lib, K, N, modes):
    L, g = lib
    for k_, n_, m_, B, has_d, has_w, c in R.norm_cases():
        if (k_, n_) != (K, N):
            continue
        x, d, nw = dev(c["x"]), dev(c["delta"]), dev(c["norm_w"])
        ys = {}
        for sw in modes:
            Wn = R.swiglu_weight(c["W"], sw)
            W = dev(Wn)
            what = "K=%d N=%d B=%d delta=%s norm_w=%s swiglu=%d" % (K, N, B, has_d, has_w, sw)
            y, ro = sentinel(B, N // 2 if sw else N), sentinel(B, K)
            L.check(g.gear_gemv_f16_norm(L.ptr(x), L.ptr(d), L.ptr(nw), R.EPS, L.ptr(W), B, K, N, sw, L.ptr(ro), L.ptr(y),
                                         L.stream_ptr()), "norm")
            res_out, sets = R.gemv_f16_norm(c["x"], c["delta"], c["norm_w"], R.EPS, Wn, sw)
            R.assert_admissible(host(y), sets, "gear_gemv_f16_norm " + what)
            if has_d:
                R.assert_bits(host(ro), res_out, "res_out " + what)
            else:
                assert untouched(ro), "res_out written without a delta " + what
            assert same_bits(x, dev(c["x"])) and (d is None or same_bits(d, dev(c["delta"]))), "inputs changed " + what
            ys[sw] = y
        if 1 in ys:
            assert same_bits(ys[1], ys[2]), "blocked and interleaved SwiGLU differ"


def _windows(B, Hq, Hkv, wcap):
    return sentinel(B, Hq, 128), sentinel(B, Hkv, wcap, 128), sentinel(B, Hkv, wcap, 128)


def _check_windows(kw, vw, slot, wcap, what):
    if slot > 0:
        assert untouched(kw[:, :, :slot]) and untouched(vw[:, :, :slot]), "slots before the addressed one written: " + what
    if slot + 1 < wcap:
        assert untouched(kw[:, :, slot + 1:]) and untouched(vw[:, :, slot + 1:]), "slots after the addressed one written: " + what


@gpu
@pytest.mark.parametrize("rc", list(R.rope_cases()), ids=lambda rc: "d%d-w%d-pos%d" % (rc["has_d"], rc["has_w"], rc["pos"]))
def test_gemv_qkv_rope_and_rope_append(lib, rc):
    L, g = lib
    c, (Hq, Hkv), B, K = R.rope_case_inputs(rc), rc["heads"], rc["B"], rc["K"]
    pos, theta, (slot, wcap) = rc["pos"], rc["theta"], rc["slot"]
    x, d, nw, W = dev(c["x"]), dev(c["delta"]), dev(c["norm_w"]), dev(c["W"])
    res_out, qs, ks, vs = R.gemv_qkv_rope(c["x"], c["delta"], c["norm_w"], R.EPS, c["W"], Hq, Hkv, pos, theta)
    state = torch.tensor([pos, slot, 0, slot + 1], dtype=torch.int32).cuda()
    outs = []
    for dyn in (None, state):
        q, kw, vw = _windows(B, Hq, Hkv, wcap)
        ro = sentinel(B, K)
        L.check(g.gear_gemv_qkv_rope(L.ptr(x), L.ptr(d), L.ptr(nw), R.EPS, L.ptr(W), B, K, Hq, Hkv, 128,
                                     0 if dyn is not None else pos, 0 if dyn is not None else slot, wcap, theta, L.ptr(dyn),
                                     L.ptr(ro), L.ptr(q), L.ptr(kw), L.ptr(vw), L.stream_ptr()), "qkv_rope")
        what = "gear_gemv_qkv_rope %r dyn=%s" % (rc, dyn is not None)
        R.assert_admissible(host(q), qs, what + " q")
        R.assert_admissible(host(kw[:, :, slot]), ks, what + " k")
        R.assert_admissible(host(vw[:, :, slot]), vs, what + " v")
        _check_windows(kw, vw, slot, wcap, what)
        if rc["has_d"]:
            R.assert_bits(host(ro), res_out, what + " res_out")
        else:
            assert untouched(ro)
        outs.append((q, kw, vw))
    assert all(same_bits(a, b) for a, b in zip(*outs)), "device-state variant differs from the host-argument variant"
    assert state.tolist() == [pos, slot, 0, slot + 1]
    # gear_rope_append / _dyn on a plain fp16 row
    qkv_n = R.rope_qkv(rc)
    qkv = dev(qkv_n)
    qs, ks, vcopy = R.rope_append(qkv_n, Hq, Hkv, pos, theta)
    outs = []
    for dyn in (None, state):
        q, kw, vw = _windows(B, Hq, Hkv, wcap)
        if dyn is None:
            L.check(g.gear_rope_append(L.ptr(qkv), B, Hq, Hkv, 128, pos, theta, L.ptr(q), L.ptr(kw), L.ptr(vw), slot, wcap,
                                       L.stream_ptr()), "rope_append")
        else:
            L.check(g.gear_rope_append_dyn(L.ptr(qkv), B, Hq, Hkv, 128, L.ptr(dyn), theta, L.ptr(q), L.ptr(kw), L.ptr(vw), wcap,
                                           L.stream_ptr()), "rope_append_dyn")
        what = "gear_rope_append %r dyn=%s" % (rc, dyn is not None)
        R.assert_admissible(host(q), qs, what + " q")
        R.assert_admissible(host(kw[:, :, slot]), ks, what + " k")
        R.assert_bits(host(vw[:, :, slot]), vcopy, what + " v")
        _check_windows(kw, vw, slot, wcap, what)
        outs.append((q, kw, vw))
    assert all(same_bits(a, b) for a, b in zip(*outs)), "gear_rope_append_dyn differs from gear_rope_append"
    assert same_bits(qkv, dev(qkv_n))


@gpu
def test_rope_append_every_fp16_bit_pattern(lib):
    """All 65536 fp16 bit patterns as x1 at pos 777: NaN in, NaN out; +-inf, +-0 and the subnormals against the reference."""
    L, g = lib
    qkv_n, Hq, Hkv = R.all_patterns_qkv()
    qkv = dev(qkv_n)
    q, kw, vw = _windows(4, Hq, Hkv, 1)
    L.check(g.gear_rope_append(L.ptr(qkv), 4, Hq, Hkv, 128, 777, 1e4, L.ptr(q), L.ptr(kw), L.ptr(vw), 0, 1, L.stream_ptr()), "rope")
    qs, ks, vcopy = R.rope_append(qkv_n, Hq, Hkv, 777, 1e4)
    R.assert_admissible(host(q), qs, "q")
    R.assert_admissible(host(kw[:, :, 0]), ks, "k")
    R.assert_bits(host(vw[:, :, 0]), vcopy, "v")
    x1 = qkv_n.reshape(4, Hq + 2 * Hkv, 128)[:, :Hq + Hkv, :64]
    out = np.concatenate([host(q), host(kw[:, :, 0])], 1)
    assert np.isnan(x1).sum() == 2 * 1023
    assert np.isnan(out[:, :, :64][np.isnan(x1)]).all() and np.isnan(out[:, :, 64:][np.isnan(x1)]).all()
    assert not np.isnan(out[:, :, :64][~np.isnan(x1)]).any()


@gpu
@pytest.mark.parametrize("H", [8, 2056, 8192])
def test_add_rmsnorm(lib, H):
    L, g = lib
    for h_, rows, xn, dn, wn in R.rmsnorm_cases():
        if h_ != H:
            continue
        w = dev(wn)
        for delta in (dn, None):
            res_ref, sets = R.add_rmsnorm(xn, delta, wn, R.EPS)
            for mode in ("own", "null", "alias"):
                x, d, y = dev(xn), dev(delta), sentinel(rows, H)
                ro = {"own": sentinel(rows, H), "null": None, "alias": x}[mode]
                L.check(g.gear_add_rmsnorm(L.ptr(x), L.ptr(d), L.ptr(w), rows, H, R.EPS, L.ptr(ro), L.ptr(y), L.stream_ptr()), "n")
                what = "gear_add_rmsnorm H=%d rows=%d delta=%s res_out=%s" % (H, rows, delta is not None, mode)
                R.assert_admissible(host(y), sets, what)
                if ro is not None:
                    R.assert_bits(host(ro), res_ref, what + " res_out")
                else:
                    assert same_bits(x, dev(xn))
                assert d is None or same_bits(d, dev(dn))


@gpu
@pytest.mark.parametrize("H", [8200, 12])
def test_add_rmsnorm_refuses_unsupported_widths(lib, H):
    L, g = lib
    x, w, y, ro = dev(R.f16(np.ones((2, H)))), dev(R.f16(np.ones(H))), sentinel(2, H), sentinel(2, H)
    with pytest.raises(L.GearError):
        L.check(g.gear_add_rmsnorm(L.ptr(x), None, L.ptr(w), 2, H, R.EPS, L.ptr(ro), L.ptr(y), L.stream_ptr()), "refused")
    torch.cuda.synchronize()
    assert untouched(y) and untouched(ro)


@gpu
def test_silu_mul(lib, capsys):
    """Every gate bit pattern against four ups, and a tail that is no multiple of the block; the share of elements where the kernel
    equals torch CPU eager bit for bit is printed (pytest -s)."""
    L, g = lib
    for gu_n in (R.all_gate_patterns(), R.silu_tail_case()):
        B, I = gu_n.shape[0], gu_n.shape[1] // 2
        gu, out = dev(gu_n), sentinel(B, I + 1)           # one spare element per call: nothing past B * I is written
        flat = out.view(-1)[:B * I].view(B, I)
        L.check(g.gear_silu_mul(L.ptr(gu), B, I, L.ptr(out), L.stream_ptr()), "silu")
        R.assert_admissible(host(flat), R.silu_mul(gu_n), "gear_silu_mul B=%d I=%d" % (B, I))
        assert untouched(out.view(-1)[B * I:])
        t = torch.from_numpy(gu_n.copy())
        ref = (torch.nn.functional.silu(t[:, :I]) * t[:, I:]).numpy()
        got = host(flat)
        same = (got.view(np.uint16) == ref.view(np.uint16)) | (np.isnan(got) & np.isnan(ref))
        with capsys.disabled():
            print("gear_silu_mul [%d, %d]: %.4f %% of the elements equal torch CPU eager bit for bit" % (B, I, 100.0 * same.mean()))


@gpu
def test_decode_state_advance(lib):
    L, g = lib
    st = torch.tensor([5, 63, 4096, 7], dtype=torch.int32).cuda()
    for _ in range(3):
        L.check(g.gear_decode_state_advance(L.ptr(st), L.stream_ptr()), "advance")
    assert st.tolist() == [8, 66, 4096, 10]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(g.gear_decode_state_advance(L.ptr(st), L.stream_ptr()), "advance (captured)")
    assert st.tolist() == [8, 66, 4096, 10]               # capturing runs nothing
    graph.replay()
    graph.replay()
    assert st.tolist() == [10, 68, 4096, 12]


@gpu
def test_gemv_subnormal_activations(lib, capsys):
    """Activations that are all fp16 subnormals against weights of +-2^14 (dense_ref.subnormal_case): per element exactly two
    outcomes are accepted -- the exact result, or 0 (subnormal operands flushed by the dot-product instruction) -- and it must be
    the same one for every element of every instantiation tried (plain and folded-norm GEMV, SK 2 and 4, B 1 .. 4).  Which one the
    GPU gives is recorded in DESIGN.md section 6."""
    L, g = lib
    seen = set()
    for K, N in ((520, 5), (8264, 5)):
        for B in (1, 2, 3, 4):
            xn, Wn = R.subnormal_case(K + B, B, K, N)
            x, W = dev(xn), dev(Wn)
            full = R.gemv_f16(xn, Wn)
            assert (np.abs(full.ref) > 2.0 ** -10).all()
            _, full_n = R.gemv_f16_norm(xn, None, None, R.EPS, Wn, 0)
            for norm, sets in ((False, full), (True, full_n)):
                y = sentinel(B, N)
                if norm:
                    L.check(g.gear_gemv_f16_norm(L.ptr(x), None, None, R.EPS, L.ptr(W), B, K, N, 0, None, L.ptr(y), L.stream_ptr()), "n")
                else:
                    L.check(g.gear_gemv_f16(L.ptr(x), L.ptr(W), B, K, N, L.ptr(y), L.stream_ptr()), "p")
                got = host(y)
                kept, flushed = sets.contains(got), got == 0
                assert (kept | flushed).all(), "neither the full result nor the flushed one: K=%d B=%d norm=%s\n%s" % (
                    K, B, norm, "\n".join(R.mismatches(got, sets)[1]))
                assert kept.all() or flushed.all(), "subnormal operands honoured for some elements only: K=%d B=%d norm=%s" % (K, B, norm)
                seen.add("kept" if kept.all() else "flushed")
    assert len(seen) == 1, "the instantiations disagree: %s" % seen
    with capsys.disabled():
        print("fp16 subnormal operands of the GEMV dot product: %s" % seen.pop())
