"""CPU checks of RoPE scaling (gear_amd/rope.py and the gear_*_freq entry points): rope_parameters against the formulas restated
in float64, its refusals, ScaledRotaryEmbedding against float64 cos / sin and against the stock module, and the four table
entry points -- declared, bound, exported, ABI version unchanged, a null table and attn_factor = 0 refused before any launch
(the device pointers below are never dereferenced)."""
import ctypes
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gear_amd import _lib
from gear_amd.modeling_llamagear import LlamaAttention_GEAR, LlamaConfigLite, LlamaRotaryEmbedding
from gear_amd.rope import ScaledRotaryEmbedding, rope_parameters

REL = 1e-6        # fp32 evaluation of a handful of operations against float64
SMALL = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=64)
LLAMA31 = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192)
YARN = dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=64)


def _cfg(scaling, theta=10000.0, **kw):
    return SimpleNamespace(rope_theta=theta, rope_scaling=scaling, max_position_embeddings=4096, **kw)


def _inv64(theta, D=128):
    return 1.0 / np.float64(theta) ** (np.arange(0, D, 2, dtype=np.float64) / D)


def _llama3_64(rs, theta, D=128):
    inv = _inv64(theta, D)
    f, lo, hi, orig = (float(rs[k]) for k in ("factor", "low_freq_factor", "high_freq_factor", "original_max_position_embeddings"))
    wl = 2 * np.pi / inv
    s = (orig / wl - lo) / (hi - lo)
    out = (1 - s) * inv / f + s * inv
    low_band, high_band = wl > orig / lo, wl < orig / hi
    out = np.where(low_band, inv / f, out)
    out = np.where(high_band, inv, out)
    return out, low_band, high_band


def _yarn_64(rs, theta, D=128, max_pos=4096):
    inv = _inv64(theta, D)
    f = float(rs["factor"])
    orig = float(rs.get("original_max_position_embeddings", max_pos))

    def cd(n):
        return D * math.log(orig / (2 * math.pi * n)) / (2 * math.log(theta))

    low, high = max(math.floor(cd(rs.get("beta_fast", 32))), 0), min(math.ceil(cd(rs.get("beta_slow", 1))), D - 1)
    if low == high:
        high += 0.001
    ramp = np.clip((np.arange(D // 2, dtype=np.float64) - low) / (high - low), 0, 1)
    return (inv / f) * ramp + inv * (1 - ramp), rs.get("attention_factor", 0.1 * math.log(f) + 1)


def _close(got, want):
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    err = np.abs(got.numpy().astype(np.float64) - want) / np.abs(want)
    assert err.max() <= REL, err.max()


# ------------------------------------------------------------------------------------------------------- rope_parameters
@pytest.mark.parametrize("scaling", [None, {"rope_type": "default"}, {"type": "default"}])
def test_no_scaling_gives_none(scaling):
    assert rope_parameters(_cfg(scaling)) == (None, 1.0)
    assert rope_parameters(LlamaConfigLite(rope_scaling=scaling)) == (None, 1.0)


@pytest.mark.parametrize("key", ["rope_type", "type"])
def test_linear(key):
    inv, af = rope_parameters(_cfg({key: "linear", "factor": 4.0}))
    _close(inv, _inv64(10000.0) / 4.0)
    assert af == 1.0


@pytest.mark.parametrize("rs,theta", [(LLAMA31, 500000.0), (SMALL, 10000.0)])
def test_llama3(rs, theta):
    inv, af = rope_parameters(_cfg(rs, theta))
    want, low_band, high_band = _llama3_64(rs, theta)
    _close(inv, want)
    assert af == 1.0
    if rs is SMALL:     # the config of the GPU tests: every band occurs among the 64 pairs
        assert low_band.any() and high_band.any() and (~low_band & ~high_band).any()
        assert not np.allclose(want, _inv64(theta), rtol=1e-3)


def test_yarn():
    inv, af = rope_parameters(_cfg(YARN))
    want, waf = _yarn_64(YARN, 10000.0)
    _close(inv, want)
    assert abs(af - waf) <= 1e-12 and af == pytest.approx(0.1 * math.log(4.0) + 1)
    # an explicit attention_factor wins; original_max_position_embeddings defaults to max_position_embeddings
    inv2, af2 = rope_parameters(_cfg(dict(rope_type="yarn", factor=4.0, attention_factor=1.25, beta_fast=16, beta_slow=2)))
    want2, _ = _yarn_64(dict(factor=4.0, beta_fast=16, beta_slow=2), 10000.0, max_pos=4096)
    _close(inv2, want2)
    assert af2 == 1.25


def test_head_dim_argument():
    inv, _ = rope_parameters(_cfg({"rope_type": "linear", "factor": 2.0}), head_dim=64)
    _close(inv, _inv64(10000.0, 64) / 2.0)


@pytest.mark.parametrize("scaling,word", [
    ({"rope_type": "dynamic", "factor": 2.0}, "dynamic"),
    ({"type": "dynamic", "factor": 2.0}, "dynamic"),
    ({"rope_type": "longrope", "short_factor": [1.0] * 64, "long_factor": [1.0] * 64}, "longrope"),
    ({"rope_type": "su", "factor": 2.0}, "su"),
    ({"rope_type": "linear"}, "linear"),
    ({"rope_type": "linear", "factor": 0.0}, "linear"),
    ({"rope_type": "linear", "factor": -2.0}, "linear"),
    ({"rope_type": "linear", "factor": float("nan")}, "linear"),
    ({"rope_type": "linear", "factor": "4"}, "linear"),
    (dict(LLAMA31, factor=0), "llama3"),
    ({k: v for k, v in LLAMA31.items() if k != "original_max_position_embeddings"}, "llama3"),
    ({k: v for k, v in LLAMA31.items() if k != "low_freq_factor"}, "llama3"),
    (dict(LLAMA31, high_freq_factor=-4.0), "llama3"),
    (dict(LLAMA31, high_freq_factor=1.0), "llama3"),
    (dict(LLAMA31, original_max_position_embeddings=0), "llama3"),
    ({"rope_type": "yarn"}, "yarn"),
    (dict(YARN, factor=-1.0), "yarn"),
    (dict(YARN, beta_fast=0), "yarn"),
    (dict(YARN, attention_factor=0.0), "yarn"),
    (dict(YARN, mscale=1.0), "yarn"),
    (dict(YARN, mscale_all_dim=0.5), "yarn"),
])
def test_refusals_name_the_type(scaling, word):
    with pytest.raises(ValueError, match=word):
        rope_parameters(_cfg(scaling))


def test_refuses_bad_theta_and_non_dict():
    with pytest.raises(ValueError, match="linear"):
        rope_parameters(_cfg({"rope_type": "linear", "factor": 2.0}, theta=0.0))
    with pytest.raises(ValueError):
        rope_parameters(_cfg("linear"))


# ------------------------------------------------------------------------------------------------- ScaledRotaryEmbedding
@pytest.mark.parametrize("scaling", [SMALL, YARN])
def test_scaled_rotary_against_float64(scaling):
    inv, af = rope_parameters(_cfg(scaling))
    rot = ScaledRotaryEmbedding(128, inv, af)
    pos = torch.tensor([[0, 1, 63, 64, 65, 1000, 16383]])
    cos, sin = rot(torch.zeros(1, dtype=torch.float16), pos)
    assert cos.dtype == sin.dtype == torch.float16 and tuple(cos.shape) == (1, 7, 128)
    # the angle is the module's own fp32 product; cos / sin / the factor in float64, rounded once to fp16.  The module rounds
    # three times (fp32 cos, fp32 product, fp16): half an fp16 ulp plus two fp32 roundings
    ang = (pos[0, :, None].float() * inv[None, :]).numpy().astype(np.float64)
    ang = np.concatenate([ang, ang], -1)
    for got, fn in ((cos, np.cos), (sin, np.sin)):
        want = fn(ang) * af
        err = np.abs(got[0].numpy().astype(np.float64) - want)
        bound = 2.0 ** -11 * np.maximum(np.abs(want), 2.0 ** -14) * (1 + 2.0 ** -10) + 2.0 ** -22
        assert (err <= bound).all(), float((err - bound).max())


def test_scaled_rotary_equals_the_stock_module_on_the_unscaled_table():
    stock = LlamaRotaryEmbedding(128, 4096, 10000.0)
    rot = ScaledRotaryEmbedding(128, stock.inv_freq, 1.0)
    pos = torch.arange(0, 5000, 7)[None, :]
    x = torch.zeros(1, dtype=torch.float16)
    for a, b in zip(stock(x, pos), rot(x, pos)):
        assert torch.equal(a, b)


def test_scaled_rotary_keeps_fp32_under_half():
    inv, af = rope_parameters(_cfg(SMALL))
    rot = ScaledRotaryEmbedding(128, inv, af).half()
    assert rot.inv_freq.dtype == torch.float32 and torch.equal(rot.inv_freq, inv)
    assert rot.table("cpu").dtype == torch.float32
    with pytest.raises(ValueError):
        ScaledRotaryEmbedding(128, inv[:32], 1.0)


def test_attention_modules_pick_the_rotary_class():
    cc = dict(compress_method="gearlKIVI", group_size=64, residual=64, quantize_bit=2, rank=2, rankv=2, loop=3)
    small = dict(vocab_size=64, hidden_size=256, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                 num_key_value_heads=2)
    for scaling in (None, {"rope_type": "default"}):
        at = LlamaAttention_GEAR(0, LlamaConfigLite(rope_scaling=scaling, **small), cc)
        assert type(at.rotary_emb) is LlamaRotaryEmbedding
    at = LlamaAttention_GEAR(0, LlamaConfigLite(rope_scaling=SMALL, **small), cc)
    assert type(at.rotary_emb) is ScaledRotaryEmbedding and at.rotary_emb.attention_factor == 1.0
    assert torch.equal(at.rotary_emb.inv_freq, rope_parameters(_cfg(SMALL))[0])
    at = LlamaAttention_GEAR(0, LlamaConfigLite(rope_scaling=YARN, **small), cc)
    assert at.rotary_emb.attention_factor == pytest.approx(0.1 * math.log(4.0) + 1)
    with pytest.raises(ValueError, match="dynamic"):
        LlamaAttention_GEAR(0, LlamaConfigLite(rope_scaling={"rope_type": "dynamic", "factor": 2.0}, **small), cc)


# ------------------------------------------------------------------------------------------------------------ the C ABI
_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
FAKE = 4096
WANT = {
    "gear_rope_append_freq": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _i, _i, _vp]),
    "gear_rope_append_dyn_freq": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _f, _vp, _vp, _vp, _i, _vp]),
    "gear_gemv_qkv_rope_freq": (_i, [_vp, _vp, _vp, _f, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gear_kivi_rope_append_freq": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _f, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i,
                                        _vp]),
}


def _calls(table, af, D=128, B=1, src=FAKE, bits=2):
    lib = _lib.load()
    return {
        "gear_rope_append_freq": lambda: lib.gear_rope_append_freq(src, B, 4, 2, D, 5, table, af, FAKE, FAKE, FAKE, 3, 64, None),
        "gear_rope_append_dyn_freq": lambda: lib.gear_rope_append_dyn_freq(src, B, 4, 2, D, FAKE, table, af, FAKE, FAKE, FAKE, 64, None),
        "gear_gemv_qkv_rope_freq": lambda: lib.gear_gemv_qkv_rope_freq(src, None, None, 1e-5, FAKE, B, 256, 4, 2, D, 5, 3, 64, table, af,
                                                                      None, None, FAKE, FAKE, FAKE, None),
        "gear_kivi_rope_append_freq": lambda: lib.gear_kivi_rope_append_freq(src, B, 4, 2, D, 70, table, af, FAKE, FAKE, 3, FAKE, 70, 64,
                                                                            5, FAKE, FAKE, FAKE, 256, 64, bits, None),
    }


def test_freq_entries_are_declared_bound_and_exported():
    with open(os.path.join(os.path.dirname(_lib._HERE), "include", "gear_hip.h")) as f:
        text = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, sig in WANT.items():
        assert _lib.SIGNATURES[name] == sig, name
        assert hasattr(raw, name), name
        assert f"int {name}(const void* " in text, name
    for decl in ("int D, int pos, const float* inv_freq, float attn_factor,", "const void* dyn_state, const float* inv_freq,",
                 "int wcap, const float* inv_freq, float attn_factor,"):
        assert decl in text, decl
    assert _lib.load().gear_abi_version() == _lib.ABI_VERSION == 5


def test_freq_entries_refuse_bad_tables_without_gpu():
    err = _lib.load().gear_last_error
    for name, call in _calls(None, 1.0).items():
        assert call() < 0 and name.encode() in err() and b"null inv_freq table" in err(), name
    for af in (0.0, -1.0, float("inf"), float("nan")):
        for name, call in _calls(FAKE, af).items():
            assert call() < 0 and name.encode() in err() and b"attn_factor" in err(), (name, af)


def test_freq_entries_keep_their_parents_checks_without_gpu():
    err = _lib.load().gear_last_error
    for name, call in _calls(FAKE, 1.0, D=64).items():
        assert call() < 0 and name.encode() in err() and b"head_dim must be 128" in err(), name
    for name, call in _calls(FAKE, 1.0, src=None).items():
        assert call() < 0 and name.encode() in err() and b"null pointer" in err(), name
    c = _calls(FAKE, 1.0, B=0)
    assert c["gear_rope_append_freq"]() < 0 and b"bad arguments" in err()
    assert c["gear_gemv_qkv_rope_freq"]() < 0 and b"batch must be in [1,4]" in err()
    assert c["gear_kivi_rope_append_freq"]() < 0 and b"bad shape" in err()
    assert _calls(FAKE, 1.0, bits=3)["gear_kivi_rope_append_freq"]() < 0 and b"bits must be 2 or 4" in err()
    lib = _lib.load()
    assert lib.gear_rope_append_freq(FAKE, 1, 4, 2, 128, 5, FAKE, 1.0, FAKE, FAKE, FAKE, 64, 64, None) < 0 and b"bad arguments" in err()
    assert lib.gear_gemv_qkv_rope_freq(FAKE, None, None, 1e-5, FAKE, 1, 256, 4, 2, 128, -1, 3, 64, FAKE, 1.0, None, None, FAKE, FAKE,
                                       FAKE, None) < 0 and b"bad pos / slot" in err()
