"""The admissible sets of tests/dense_ref.py are (a) wide enough for a correct implementation and (b) narrow enough to catch the
bugs they are for -- shown on the CPU, before any GPU run.

(a) Admissibility: a numpy float32 emulation of every kernel (the kernels' chunking over lanes, waves and SK, their reduction order,
np.float32 arithmetic, numpy's own exp / cos / sin in float32) lands inside the set of every element of every case that
tests/test_gpu_dense_ops.py runs.  torch CPU eager on fp16 tensors and LlamaRMSNorm / LlamaRotaryEmbedding / apply_rotary_pos_emb of
gear_amd/modeling_llamagear.py, which the kernels claim to follow, land inside the same sets (the fused norm applies its row scale
after the dot product, so torch is compared at the level of the unfused gear_add_rmsnorm).

Measured here per case family (share of elements with more than one admissible value / largest set; pytest -s prints them):
  plain and residual GEMV 2.67 % / 2      norm GEMV 0.96 % / 2        (asserted: at most 15 % and 2)
  SwiGLU 1.66 % / 3      gear_silu_mul 0.03 % / 2      gear_add_rmsnorm 0.34 % / 2
  fused qkv RoPE 12.42 % / 13985      gear_rope_append 15.53 % / 13057 -- the large sets are pos = 32767 alone, where the derived
  uncertainty of the angle (about 1e-2 rad) spans that many fp16 values of a cos or sin near 0; up to pos = 4095 a set holds a few.

(b) Sensitivity (the pattern of tests/test_attn_probe_sensitivity.py): each fault of the issue's list, injected into the emulation,
is reported (the test_fault_* functions)."""
import math

import numpy as np
import pytest

import dense_ref as R

F32 = np.float32


# ------------------------------------------------------------------------------------------------ float32 emulation of the kernels
def _lane_sum(prod, sk):
    """prod float32 [..., K] (K % 8 == 0) -> [...]: chunk c to lane c % 64 of K part (c / 64) % SK, fdot2 pairs in order (two
    roundings each), xor-shuffle butterfly 32 .. 1, then the SK partial sums added in order."""
    K = prod.shape[-1]
    per = 64 * sk
    it = math.ceil((K // 8) / per)
    pad = np.zeros(prod.shape[:-1] + (it * per * 8 - K,), F32)
    p = np.concatenate([prod, pad], -1).reshape(prod.shape[:-1] + (it, sk, 64, 4, 2))
    acc = np.zeros(prod.shape[:-1] + (sk, 64), F32)
    for i in range(it):
        for j in range(4):
            acc = (p[..., i, :, :, j, 0] + p[..., i, :, :, j, 1]) + acc
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ m]
    t = np.zeros(prod.shape[:-1], F32)
    for k in range(sk):
        t = t + acc[..., k, 0]
    return t


def _f32(a):
    return np.asarray(a, np.float16).astype(F32)


def emu_values(x, delta, norm_w, eps, W, sk, norm):
    """val() of gemv_tok_kernel: fp16 [B, N] (and v = fp16(x + delta))."""
    v = x if delta is None else (_f32(x) + _f32(delta)).astype(np.float16)
    act = v if norm_w is None else (_f32(v) * _f32(norm_w)).astype(np.float16)
    t = _lane_sum(_f32(act)[:, None, :] * _f32(W)[None], sk)
    if norm:
        u = _lane_sum(_f32(v) * _f32(v), sk)[:, None]
        arg = u / F32(x.shape[1]) + F32(eps)
        with np.errstate(divide="ignore"):
            t = t * (1.0 / np.sqrt(arg.astype(np.float64))).astype(F32)
    return t.astype(np.float16), v


def emu_silu_mul(g, u):
    g, u = _f32(g), _f32(u)
    with np.errstate(over="ignore", invalid="ignore"):
        sg = (g / (F32(1) + np.exp(-g))).astype(np.float16)
        return (_f32(sg) * u).astype(np.float16)


def emu_rope(x1, x2, pos, theta, partner_bug=False, sin_sign_bug=False):
    """fp16 [..., 64] halves -> fp16 [..., 128]."""
    p = np.arange(64)
    inv_freq = np.exp2(-(2 * p).astype(F32) / F32(128) * F32(np.log2(F32(theta))))
    ang = F32(pos) * inv_freq
    c, s = _f32(np.cos(ang).astype(np.float16)), _f32(np.sin(ang).astype(np.float16))
    a, b = _f32(x1), _f32(x2)
    if partner_bug:                       # rotation partner p + 1 in place of p + 64
        b = np.roll(a, -1, -1)
    h = lambda t: _f32(t.astype(np.float16))
    lo = (h(a * c) + h(-b * s)).astype(np.float16)
    hi = (h(b * c) + h(a * (-s if sin_sign_bug else s))).astype(np.float16)
    return np.concatenate([lo, hi], -1)


def emu_gemv(x, W, res_in=None):
    y, _ = emu_values(x, None, None, 0.0, W, R.pick_sk(x.shape[1], W.shape[0], 4), False)
    return y if res_in is None else (_f32(y) + _f32(res_in)).astype(np.float16)


def emu_gemv_norm(x, delta, norm_w, eps, W, swiglu):
    val, v = emu_values(x, delta, norm_w, eps, W, R.pick_sk(x.shape[1], W.shape[0], 2 if swiglu else 4), True)
    if swiglu == 1:
        return emu_silu_mul(val[:, 0::2], val[:, 1::2]), v
    if swiglu == 2:
        return emu_silu_mul(val[:, :val.shape[1] // 2], val[:, val.shape[1] // 2:]), v
    return val, v


def emu_qkv_rope(x, delta, norm_w, eps, W, Hq, Hkv, pos, theta, **bugs):
    val, v = emu_values(x, delta, norm_w, eps, W, 2, True)
    h = val.reshape(x.shape[0], Hq + 2 * Hkv, 128)
    rot = emu_rope(h[:, :Hq + Hkv, :64], h[:, :Hq + Hkv, 64:], pos, theta, **bugs)
    return rot[:, :Hq], rot[:, Hq:], h[:, Hq + Hkv:], v


def emu_add_rmsnorm(res_in, delta, weight, eps):
    """One block of 256 threads per row; thread t keeps vectors t + 256 p; fmaf chain (one rounding per step)."""
    v = res_in if delta is None else (_f32(res_in) + _f32(delta)).astype(np.float16)
    rows, H = v.shape
    vp = np.zeros((rows, 4 * 256 * 8), np.float64)
    vp[:, :H] = v.astype(np.float64)
    vp = vp.reshape(rows, 4, 256, 8)
    ss = np.zeros((rows, 256), F32)
    for p in range(4):
        for j in range(8):
            ss = (vp[:, p, :, j] ** 2 + ss.astype(np.float64)).astype(F32)
    ss = ss.reshape(rows, 4, 64)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        ss = ss + ss[..., lanes ^ m]
    red = ss[..., 0]
    tot = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    inv = (1.0 / np.sqrt((tot / F32(H) + F32(eps)).astype(np.float64))).astype(F32)[:, None]
    n = (_f32(v) * inv).astype(np.float16)
    return v, (_f32(weight) * _f32(n)).astype(np.float16)


# ---------------------------------------------------------------------------------------------------------------- admissibility
class Stats:
    def __init__(self):
        self.n = self.multi = self.largest = 0

    def add(self, sets):
        sz = sets.size()
        self.n += sz.size
        self.multi += int((sz > 1).sum())
        self.largest = max(self.largest, int(sz.max()))

    def __str__(self):
        return "%.2f %% / %d" % (100.0 * self.multi / max(self.n, 1), self.largest)


def test_gemv_emulation_is_admissible_and_sets_are_tight():
    st = Stats()
    for K, N in R.GEMV_SHAPES:
        for B in (1, 2, 3, 4):
            c = R.gemv_case(K, N, B)
            res = c["res"]
            for r in (None, res):
                sets = R.gemv_f16(c["x"], c["W"], r)
                R.assert_admissible(emu_gemv(c["x"], c["W"], r), sets, "gemv K=%d N=%d B=%d res=%s" % (K, N, B, r is not None))
                st.add(sets)
            # the inputs are what the case promises: one near-cancelling output, every other one far from cancelling
            ratio = c["ratio"].copy()
            assert R.RHO / 1.5 < ratio[0, N - 1] < R.RHO * 1.5, ratio[0, N - 1]
            ratio[0, N - 1] = 1.0
            assert ratio.min() > 0.2, (K, N, B, ratio.min())
    print("plain / residual GEMV:", st)
    assert st.multi <= 0.15 * st.n and st.largest <= 2, str(st)


def test_norm_gemv_emulation_is_admissible_and_sets_are_tight():
    st, sw = Stats(), Stats()
    for K, N, modes, B, has_d, has_w, c in R.norm_cases():
        for swiglu in modes:
            W = R.swiglu_weight(c["W"], swiglu)
            res_out, sets = R.gemv_f16_norm(c["x"], c["delta"], c["norm_w"], R.EPS, W, swiglu)
            y, v = emu_gemv_norm(c["x"], c["delta"], c["norm_w"], R.EPS, W, swiglu)
            what = "norm gemv K=%d N=%d B=%d delta=%s w=%s swiglu=%d" % (K, N, B, has_d, has_w, swiglu)
            R.assert_admissible(y, sets, what)
            R.assert_bits(v, res_out, what + " res_out")
            (sw if swiglu else st).add(sets)
        ratio = c["ratio"].copy()
        assert R.RHO / 1.5 < ratio[0, N - 1] < R.RHO * 1.5, ratio[0, N - 1]
        ratio[0, N - 1] = 1.0
        if c["special"]:
            ratio[1, N - 1] = 1.0
        assert ratio.min() > 0.2, (K, N, B, ratio.min())
    print("norm GEMV:", st, " SwiGLU:", sw)
    assert st.multi <= 0.15 * st.n and st.largest <= 2, str(st)


def test_rope_emulation_is_admissible():
    fused, plain = Stats(), Stats()
    for rc in R.rope_cases():
        c, (Hq, Hkv) = R.rope_case_inputs(rc), rc["heads"]
        res_out, qs, ks, vs = R.gemv_qkv_rope(c["x"], c["delta"], c["norm_w"], R.EPS, c["W"], Hq, Hkv, rc["pos"], rc["theta"])
        q, k, v, vv = emu_qkv_rope(c["x"], c["delta"], c["norm_w"], R.EPS, c["W"], Hq, Hkv, rc["pos"], rc["theta"])
        for got, sets, name in ((q, qs, "q"), (k, ks, "k"), (v, vs, "v")):
            R.assert_admissible(got, sets, "qkv_rope %s %r" % (name, rc))
            fused.add(sets)
        R.assert_bits(vv, res_out, "res_out")
        qkv = R.rope_qkv(rc)
        qs, ks, vcopy = R.rope_append(qkv, Hq, Hkv, rc["pos"], rc["theta"])
        h = qkv.reshape(rc["B"], Hq + 2 * Hkv, 128)
        rot = emu_rope(h[:, :Hq + Hkv, :64], h[:, :Hq + Hkv, 64:], rc["pos"], rc["theta"])
        R.assert_admissible(rot[:, :Hq], qs, "rope_append q %r" % rc)
        R.assert_admissible(rot[:, Hq:], ks, "rope_append k %r" % rc)
        plain.add(qs)
        plain.add(ks)
    print("fused qkv RoPE:", fused, " rope_append:", plain)


def test_silu_mul_emulation_and_torch_are_admissible():
    import torch
    st = Stats()
    rng = np.random.default_rng(5)
    for gu in (R.all_gate_patterns(), R.silu_tail_case()):
        sets = R.silu_mul(gu)
        I = gu.shape[1] // 2
        R.assert_admissible(emu_silu_mul(gu[:, :I], gu[:, I:]), sets, "silu_mul emulation")
        t = torch.from_numpy(gu.copy())
        ref = (torch.nn.functional.silu(t[:, :I]) * t[:, I:]).numpy()
        R.assert_admissible(ref, sets, "silu_mul torch CPU eager")
        st.add(sets)
    print("silu_mul:", st)
    assert st.largest <= 4


def test_add_rmsnorm_emulation_and_torch_are_admissible():
    import torch
    from gear_amd.modeling_llamagear import LlamaRMSNorm
    st = Stats()
    for H, rows, x, d, w in R.rmsnorm_cases():
        for delta in (d, None):
            res_out, sets = R.add_rmsnorm(x, delta, w, R.EPS)
            v, y = emu_add_rmsnorm(x, delta, w, R.EPS)
            R.assert_bits(v, res_out, "res_out")
            R.assert_admissible(y, sets, "add_rmsnorm emulation H=%d rows=%d" % (H, rows))
            norm = LlamaRMSNorm(H, R.EPS).half()
            norm.weight.data = torch.from_numpy(w.copy())
            tv = torch.from_numpy(x.copy()) + torch.from_numpy(delta.copy()) if delta is not None else torch.from_numpy(x.copy())
            R.assert_bits(tv.numpy(), res_out, "res_out against torch")
            with torch.no_grad():
                R.assert_admissible(norm(tv).numpy(), sets, "LlamaRMSNorm H=%d rows=%d" % (H, rows))
            st.add(sets)
    print("add_rmsnorm:", st)


def test_rope_append_reference_holds_the_model_code():
    """LlamaRotaryEmbedding + apply_rotary_pos_emb on the CPU land in the reference's sets (every pos and theta of the GPU cases)."""
    import torch
    from gear_amd.modeling_llamagear import LlamaRotaryEmbedding, apply_rotary_pos_emb
    rng = np.random.default_rng(9)
    B, Hq, Hkv = 2, 4, 2
    for theta in (1e4, 5e5):
        rot = LlamaRotaryEmbedding(128, 65536, theta)
        for pos in (0, 1, 777, 4095, 32767):
            qkv = R.f16(rng.standard_normal((B, (Hq + 2 * Hkv) * 128)))
            qs, ks, _ = R.rope_append(qkv, Hq, Hkv, pos, theta)
            t = torch.from_numpy(qkv.copy()).view(B, Hq + 2 * Hkv, 128)
            q, k = t[:, :Hq].unsqueeze(2), t[:, Hq:Hq + Hkv].unsqueeze(2)                # [B, H, 1, D]
            cos, sin = rot(q, torch.tensor([[pos]]))
            qr, kr = apply_rotary_pos_emb(q, k, cos, sin)
            R.assert_admissible(qr[:, :, 0].numpy(), qs, "q pos=%d theta=%g" % (pos, theta))
            R.assert_admissible(kr[:, :, 0].numpy(), ks, "k pos=%d theta=%g" % (pos, theta))


def test_rope_all_bit_patterns_emulation():
    qkv, Hq, Hkv = R.all_patterns_qkv()
    qs, ks, _ = R.rope_append(qkv, Hq, Hkv, 777, 1e4)
    h = qkv.reshape(4, Hq + 2 * Hkv, 128)
    rot = emu_rope(h[:, :Hq + Hkv, :64], h[:, :Hq + Hkv, 64:], 777, 1e4)
    R.assert_admissible(rot[:, :Hq], qs, "q")
    R.assert_admissible(rot[:, Hq:], ks, "k")
    x1 = h[:, :Hq + Hkv, :64]
    assert np.isnan(rot[:, :, :64][np.isnan(x1)]).all() and np.isnan(rot[:, :, 64:][np.isnan(x1)]).all()


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def _flagged(got, sets):
    return R.mismatches(got, sets)[0]


def _norm_case(B=4, K=520, N=12, has_d=True, has_w=True):
    c = R.make_case(77, B, K, N, has_d, has_w, True)
    return c, R.gemv_f16_norm(c["x"], c["delta"], c["norm_w"], R.EPS, c["W"], 0)[1]


@pytest.mark.parametrize("K,N", R.GEMV_SHAPES)
def test_fault_skipped_chunk_and_neighbour_row(K, N):
    c = R.make_case(1000 + K + 3, 3, K, N)
    sets = R.gemv_f16(c["x"], c["W"])
    assert _flagged(emu_gemv(c["x"], c["W"]), sets) == 0
    W = c["W"].copy()
    W[N - 1, K - 8:] = 0                                     # the last (ragged) chunk of one row skipped
    assert _flagged(emu_gemv(c["x"], W), sets) >= 1
    if N > 1:
        W = c["W"].copy()
        W[N - 1] = W[N - 2]                                  # the last block's clamped row computed from its neighbour's weights
        got = emu_gemv(c["x"], W)
        assert _flagged(got, sets) >= 1 and not sets.contains(got)[:, N - 1].any()
    if c["x"].shape[0] > 1:
        x = c["x"].copy()
        x[1] = x[0]                                          # one batch row reading another's x
        assert not sets.contains(emu_gemv(x, c["W"]))[1].any()


def test_fault_one_ulp():
    c = R.make_case(1000 + 520 + 3, 3, 520, 5)
    sets = R.gemv_f16(c["x"], c["W"])
    got = emu_gemv(c["x"], c["W"])
    idx = tuple(np.argwhere(sets.size() == 1)[0])
    for step in (1, -1):
        bad = got.copy()
        bad[idx] = (bad[idx].view(np.uint16) + np.uint16(step % 65536)).view(np.float16)
        n, lines = R.mismatches(bad, sets)
        assert n == 1 and str(idx) in lines[0]


def test_fault_norm_weight_and_eps():
    c, sets = _norm_case()
    got, _ = emu_gemv_norm(c["x"], c["delta"], c["norm_w"], R.EPS, c["W"], 0)
    assert _flagged(got, sets) == 0
    got, _ = emu_gemv_norm(c["x"], c["delta"], None, R.EPS, c["W"], 0)           # the norm weight not applied
    assert _flagged(got, sets) > got.size // 2
    got, _ = emu_gemv_norm(c["x"], c["delta"], c["norm_w"], 0.0, c["W"], 0)      # eps dropped: row 1 has mean square << eps
    ok = sets.contains(got)
    assert not ok[1].any()
    v, y = emu_add_rmsnorm(c["x"], c["delta"], c["norm_w"], 0.0)
    assert not R.add_rmsnorm(c["x"], c["delta"], c["norm_w"], R.EPS)[1].contains(y)[1].any()


def test_fault_swapped_gate_up_pair():
    c = R.make_case(78, 2, 520, 12, False, True, True)
    for swiglu in (1, 2):
        W = R.swiglu_weight(c["W"], swiglu)
        _, sets = R.gemv_f16_norm(c["x"], None, c["norm_w"], R.EPS, W, swiglu)
        assert _flagged(emu_gemv_norm(c["x"], None, c["norm_w"], R.EPS, W, swiglu)[0], sets) == 0
        Wb = c["W"].copy()
        Wb[[2, 3]] = Wb[[3, 2]]                              # pair 1: gate and up swapped
        got, _ = emu_gemv_norm(c["x"], None, c["norm_w"], R.EPS, R.swiglu_weight(Wb, swiglu), swiglu)
        ok = sets.contains(got)
        assert not ok[:, 1].all() and ok[:, [0, 2, 3, 4, 5]].all()       # (silu(g) u ~ silu(u) g where both are large)


@pytest.mark.parametrize("bug", ["partner_bug", "sin_sign_bug"])
def test_fault_rotation(bug):
    for rc in R.rope_cases():
        if rc["pos"] == 0:
            continue                                         # sin == 0: no rotation to get wrong
        c, (Hq, Hkv) = R.rope_case_inputs(rc), rc["heads"]
        _, qs, ks, _ = R.gemv_qkv_rope(c["x"], c["delta"], c["norm_w"], R.EPS, c["W"], Hq, Hkv, rc["pos"], rc["theta"])
        q, k, _, _ = emu_qkv_rope(c["x"], c["delta"], c["norm_w"], R.EPS, c["W"], Hq, Hkv, rc["pos"], rc["theta"], **{bug: True})
        nq, nk = _flagged(q, qs), _flagged(k, ks)
        assert nq >= 1 and nk >= 1, (bug, rc, nq, nk)
