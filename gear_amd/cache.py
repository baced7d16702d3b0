"""Pre-allocated, kernel-native GEAR KV cache for one attention layer (the build's own
design: the reference rebuilds every payload tensor with torch.cat on each block boundary,
cuda_supported_gear/modeling_llamagear.py:273-286, :365-378, and re-lays the whole packed K out on every token,
quant/matmul.py:205, :215-216).

State machine = the attention hook's (modeling_llamagear.py:177-484): an fp16 window of the most recent < `residual`
tokens; when it fills, the block is compressed IN PLACE behind the already compressed tokens: quantized backbone, per-block
rank-r factors and -- when the config carries a sparsity (`left`, the simulated path's name,
GenerationBench/.../Simulated/compress_config.py) -- the sparse outliers of the block, which is what the reference's
streaming hook applies to every new block (Simulated/modeling_llama_new.py:979-1019 -> compress_function.py:261-333).
Layout = what gear_attn_decode_cache streams: K channel-major with a fixed row pitch (a block append is 128 short row
segments, never a re-layout), V token-major, token-side factors per token, channel-side factors per segment (segment 0 =
the prompt, then one per block), K outlier lists per (channel, side) that grow by `kk_blk` entries per block (later blocks
hold later tokens, so the lists stay sorted), V outlier lists per token row.

The compress calls write straight into these tensors (gear_compress_key_fused / gear_compress_value_fused with a token
offset and row pitches): no intermediate payload, no strided copies.

Outlier counts.  V rows (a token across the heads) and the K rows of the prompt segment use the reference's formula
(compress_function.py:264-267, :299-303: int(H*D*s/2) per side, capped at half the row).  For the K rows of a 64-token
decode block that formula asks for more outliers than the row has elements (defect B7: it depends on H*D, not on the
row length; torch.topk then takes overlapping sets and the block ends up stored losslessly); the cache uses the NOMINAL
count max(1, round(64*s/2)) per side there (`block_outlier_count="reference"` in the config selects the reference's count, capped at
half the row).

Differences from the hook, on purpose: K and V are compressed in lockstep (the hook compresses V only when T > residual,
:416, which strands V in fp16 when the prompt is exactly `residual` long), and the block factors start from a
channel-side random basis (the simulated path's orientation, compress_function.py:83) so that the Gram-matrix kernel
applies; both are rank-r power-iteration approximations of the same error matrix.
"""
from __future__ import annotations

import ctypes as C_
import math

import torch

from . import _lib as L
from . import compress as C


def _sparsity(cc) -> float:
    return float(cc.get("left", cc.get("sparsity", 0.0)) or 0.0)


def _cache_dims(batch, n_kv_heads, max_tokens, cc, head_dim=128, heads_total=None, v_exact=False):
    bits, group, R = cc["quantize_bit"], cc["group_size"], cc["residual"]
    m = cc["compress_method"]
    lowrank = ("gearl" in m) or ("gearsl" in m)
    rk = int(cc["rank"]) if lowrank else 0
    rv = int(cc["rankv"]) if lowrank else 0
    if R not in (64, 128):
        raise L.GearError(f"GearKVCache: residual must be 64 or 128 (got {R}): the decode attention kernel holds at most 128 "
                          "window tokens (gear_attn_decode: 0 <= W <= 128) and blocks are whole 64-token tiles")
    assert R % group == 0 and group in (32, 64) and bits in (2, 4), "GearKVCache: group 32 / 64, 2 or 4 bits"
    fpi = 32 // bits
    Tmax = (max_tokens + R - 1) // R * R
    assert Tmax <= 16384, "GearKVCache: at most 16384 tokens"
    nseg = 1 + Tmax // R
    B, H, D, T = batch, n_kv_heads, head_dim, Tmax
    s = _sparsity(cc)
    kv = int(int(B * H * T * D * s) / B / T / 2) if s > 0 else 0          # per side per token row (compress_function.py:300-303)
    # the same formula for the prompt's channel rows -- on the FULL head count when this cache is one head shard of several
    # (a K row lives inside one head, so its outlier count must not depend on how the heads are spread over GPUs; a V row
    # spans the heads, so a shard selects k / world inside its own heads: see parallel.py)
    Ht = heads_total or H
    if v_exact and Ht != H:
        # exact cross-shard V selection (parallel.exact_v_selection): the row's outliers are chosen over ALL heads, a shard keeps
        # the ones that fall into its heads -- anything between 0 and the full count, so its lists hold the full count per side
        kv = int(int(B * Ht * T * D * s) / B / T / 2) if s > 0 else 0
        if kv > H * D:
            raise L.GearError(f"GearKVCache: {kv} V outliers per side and row exceed the shard's row length {H * D} (sparsity > 1 / "
                              "world): not a configuration the exact cross-shard selection supports; use v_selection='per_shard'")
    kk0_max = int(int(B * Ht * T * D * s) / B / T / 2) if s > 0 else 0
    # K outliers per side and channel row of a decode block: "nominal" = the sparsity applied to the row's own length; "reference" =
    # the reference's formula (B7: it depends on H*D, not on the row length), capped at half the row -- what gears_channelQ does to a
    # 64-token block with the streaming hook's config (compress_function.py:264-267): at s = 0.02 on 7B that stores the block losslessly
    if cc.get("block_outlier_count", "nominal") == "reference":
        kk_blk = min(int(int(B * Ht * R * D * s) / B / R / 2), R // 2) if s > 0 else 0
    else:
        kk_blk = max(1, round(R * s / 2)) if s > 0 else 0                 # nominal count for a 64-token block (B7)
    kcap = kk0_max + (Tmax // R) * kk_blk
    shapes = dict(kcode=((B, H, D, T // fpi), torch.int32), kscale=((B, H, D, T // group), torch.float16),
                  kmn=((B, H, D, T // group), torch.float16), vcode=((B, H, T, D // fpi), torch.int32),
                  vscale=((B, H, T, D // group), torch.float16), vmn=((B, H, T, D // group), torch.float16),
                  kwin=((B, H, R, D), torch.float16), vwin=((B, H, R, D), torch.float16))
    if lowrank:
        shapes.update(kPseg=((nseg, B, H, D, rk), torch.float16), kQtok=((B, H, T, rk), torch.float16),
                      vPseg=((nseg, B, H, D, rv), torch.float16), vQtok=((B, H, T, rv), torch.float16))
    nbk = Tmax // 128 + 2                 # pitch of the K chunk index: bounds 0, 128, ... over the prompt segment
    if kk_blk > 0:
        shapes.update(koidx=((B, H, D, 2, kcap), torch.int16), koval=((B, H, D, 2, kcap), torch.float16))
        if kk0_max <= 255:
            shapes.update(kochunk=((B, H, D, 2, nbk), torch.uint8))
    if kv > 0:
        shapes.update(voidx=((B, T, 2 * kv), torch.int16), voval=((B, T, 2 * kv), torch.float16))
        if kv <= 255:
            shapes.update(vochunk=((B, T, 2, H + 1), torch.uint8))
    # sparse tiles (gear_cache_tiles_build): the outlier corrections of a 128-token K chunk / 64-token V block as a flat list,
    # sized for the expected count plus slack; a chunk that overflows falls back to the lists (count -1)
    nck, nblk = Tmax // 128 + 1, 2 * (Tmax // 128 + 1)
    ktile_cap = vtile_cap = 0
    if kk_blk > 0:
        per_chunk = D * 2 * max(2 * kk_blk, math.ceil(128 * kk0_max / max(Tmax, 1)))
        ktile_cap = (int(per_chunk * 1.25) + 64 + 255) // 256 * 256
        ktile_cap = max(ktile_cap, 512)
        shapes.update(ktile=((B, H, nck, ktile_cap), torch.int32), kcnt=((B, H, nck), torch.int32))
    if kv > 0:
        per_blk = 64 * 2 * kv / H
        vtile_cap = max(256, (int(per_blk * 1.25) + 32 + 255) // 256 * 256)
        shapes.update(vtile=((B, H, nblk, vtile_cap), torch.int32), vcnt=((B, H, nblk), torch.int32))
    return shapes, dict(bits=bits, group=group, R=R, lowrank=lowrank, rk=rk, rv=rv, fpi=fpi, Tmax=Tmax, nseg=nseg,
                        kv=kv, kk0_max=kk0_max, kk_blk=kk_blk, kcap=kcap, nbk=nbk, nck=nck, nblk=nblk, ktile_cap=ktile_cap,
                        vtile_cap=vtile_cap)


def _view(bufs, d, NB, H, D, kk0, seg0, kwin=True):
    """The gear_cache_view of a set of cache tensors (NB = leading batch dimension: layers * batch for pooled storage)."""
    v = L.CacheView()
    p = L.ptr
    for f, n in (("kcode", "kcode"), ("kscale", "kscale"), ("kmn", "kmn"), ("kP", "kPseg"), ("kQ", "kQtok"), ("koidx", "koidx"),
                 ("koval", "koval"), ("vcode", "vcode"), ("vscale", "vscale"), ("vmn", "vmn"), ("vP", "vPseg"), ("vQ", "vQtok"),
                 ("voidx", "voidx"), ("voval", "voval"), ("vochunk", "vochunk"), ("ktile", "ktile"), ("kcnt", "kcnt"),
                 ("vtile", "vtile"), ("vcnt", "vcnt")):
        setattr(v, f, p(bufs.get(n)))
    v.kochunk = p(bufs.get("kochunk")) if kk0 else None
    if kwin:
        v.kwin, v.vwin = p(bufs["kwin"]), p(bufs["vwin"])
    v.B, v.Hkv, v.D, v.tcap = NB, H, D, d["Tmax"]
    v.ldk, v.lsk, v.group, v.bits, v.mode = d["Tmax"] // d["fpi"], d["Tmax"] // d["group"], d["group"], d["bits"], 0
    v.rk, v.rv = d["rk"], d["rv"]
    v.kk_cap, v.kk0, v.kkb, v.kv = (d["kcap"] if d["kk_blk"] else 0), kk0, d["kk_blk"], d["kv"]
    v.seg0, v.seglen, v.wcap = seg0, (d["R"] if (d["lowrank"] or d["kk_blk"]) else 0), d["R"]
    v.nbk_pitch, v.ktile_cap, v.nck, v.vtile_cap, v.nblk = d["nbk"], d["ktile_cap"], d["nck"], d["vtile_cap"], d["nblk"]
    return v


USE_BLOCK_KERNEL = True      # tests switch it off to compare the single-launch block compressor with the chain
# With V outliers every K tile's wave first selects 64 / (2 H) token rows (one after the other): at 2 - 3 KV heads per rank that
# serial part outweighs the saved launches (measured in round 3 at 80 layers x 1 head: 367 us against the chain's 222).  ONE KV head
# per rank (70B on 8 GPUs) needs no hand-off at all -- the row is the tile's own -- and takes the block kernel (round 4).
BLOCK_KERNEL_MIN_HEADS = 4
_BLOCK_WS = {}


def _block_sync_ws(lib, NB, H, dev):
    """Hand-off buffer of gear_compress_block (row flags, masks, means): zeroed once, then owned by the kernel."""
    key = (str(dev), NB, H)
    ws = _BLOCK_WS.get(key)
    if ws is None:
        ws = _BLOCK_WS[key] = torch.zeros((lib.gear_compress_block_workspace(NB, H),), dtype=torch.uint8, device=dev)
    return ws


def block_kernel_status(dev="cuda") -> int:
    """OR of the status words of every block-compress hand-off buffer on `dev` (non-zero: a V tile gave up waiting)."""
    st = 0
    want = torch.device(dev)
    if want.type == "cuda" and want.index is None:
        want = torch.device("cuda", torch.cuda.current_device())
    for ws in _BLOCK_WS.values():
        if ws.device == want:
            off = (-ws.data_ptr()) % 256
            st |= int(ws[off:off + 4].view(torch.int32).item())
    return st


def _draw_p0(shape_local, gen, dev, tp):
    """Random start bases [NB, H_local, D, r].  Head-sharded: every rank draws the bases of ALL heads from the same stream and keeps
    its own (so that a head's factors do not depend on how the heads are spread over GPUs)."""
    NB, H, D, r = shape_local
    if tp is None or tp["world"] == 1:
        return torch.rand(shape_local, device=dev, generator=gen)
    full = torch.rand((NB, H * tp["world"], D, r), device=dev, generator=gen)
    return full[:, tp["rank"] * H:(tp["rank"] + 1) * H].contiguous()


def _compress_value_exact(bufs, d, lead, B, H, D, v_src, T, t_off, seg, loop, P0v, tp, kk0, seg0):
    """V payload of a head shard with the outliers selected over the WHOLE token row (all ranks' heads), bit-identical to the matching
    head slice of the unsharded payload (tests/test_gpu_parallel.py).  Round 5: in HIP -- gear_vsel_candidates, ONE all-gather of
    4 (2 kv + 2) bytes per row and rank, gear_vsel_thresholds, then gear_compress_value_sharded (the row compressor with the selection
    given + the usual low-rank step) writing straight behind token t_off of the cache: 3 launches + the chain's low-rank kernels where
    round 4 ran ~25 torch launches (parallel.exact_v_selection: two topk, where, gather ...; kept as the tests' cross-check with
    tp["exact"] == "torch")."""
    from .parallel import exact_v_selection, exact_v_thresholds
    lib = L.load()
    p = L.ptr
    NB = lead * B
    Tmax, g, bits, kv = d["Tmax"], d["group"], d["bits"], d["kv"]
    st = L.stream_ptr(v_src)
    if tp.get("exact", True) == "torch":
        from .quant.new_pack import triton_quantize_and_pack_along_last_dim_witherror
        v4 = v_src.reshape(NB, H, -1, D)[:, :, :T]
        filled, mask, oidx, oval = exact_v_selection(v4, kv, tp["rank"], tp["world"], tp.get("group"))
        code, scale, mn, err = triton_quantize_and_pack_along_last_dim_witherror(filled, g, bits)
        bufs["vcode"].view(NB, H, Tmax, -1)[:, :, t_off:t_off + T] = code
        bufs["vscale"].view(NB, H, Tmax, -1)[:, :, t_off:t_off + T] = scale
        bufs["vmn"].view(NB, H, Tmax, -1)[:, :, t_off:t_off + T] = mn
        bufs["voidx"].view(NB, Tmax, 2 * kv)[:, t_off:t_off + T] = oidx
        bufs["voval"].view(NB, Tmax, 2 * kv)[:, t_off:t_off + T] = oval
        if d["lowrank"]:
            err = err.view(NB, H, T, D).masked_fill_(mask, 0)
            P, Q = C.lowrank(err, d["rv"], loop, P0v)
            bufs["vPseg"].view(lead, d["nseg"], B, H, D, d["rv"])[:, seg] = P.view(lead, B, H, D, d["rv"])
            bufs["vQtok"].view(NB, H, Tmax, d["rv"])[:, :, t_off:t_off + T] = Q
    else:
        v4 = v_src.reshape(NB, H, -1, D)
        if v4.shape[2] != T:
            v4 = v4[:, :, :T].contiguous()
        thr, fill = exact_v_thresholds(v4, kv, tp["rank"], tp["world"], tp.get("group"), mode=0)
        seg_v = B * H * D * d["rv"]
        vP = bufs["vPseg"].view(-1)[seg * seg_v:] if d["lowrank"] else None
        wsb = lib.gear_compress_value_fused_workspace(NB, H, T, d["rv"])
        ws = C._workspace(wsb, v_src.device)
        rc = lib.gear_compress_value_sharded(
            p(v4), NB, H, T, g, bits, 0, kv, p(bufs["vcode"]), p(bufs["vscale"]), p(bufs["vmn"]), Tmax, t_off, d["rv"], loop, p(P0v),
            p(vP), B * H, d["nseg"] * seg_v, p(bufs.get("vQtok")), Tmax, t_off, p(bufs["voidx"]), p(bufs["voval"]),
            tp["rank"] * H * D, p(thr), p(fill), p(ws), ws.numel(), st)
        L.check(rc, "gear_compress_value_sharded")
    if "vochunk" in bufs:     # (the sentinel index 0xFFFF of an unused list slot lies beyond every head bound: the terminal entry is the count)
        rc = lib.gear_outlier_chunk_index_ex(p(bufs["voidx"]), NB, 2 * T, 2 * Tmax, 2 * t_off, kv, kv, 128, H + 1,
                                             p(bufs["vochunk"]), H + 1, st)
        L.check(rc, "gear_outlier_chunk_index_ex(V)")


def _compress_into(bufs, d, lead, B, H, D, k_src, v_src, T, t_off, seg, kk, o_off, loop, gen, kk0=0, seg0=0, tp=None):
    """Compress K / V [lead*B, H, T, 128] (lead = layers riding in the batch dimension of pooled storage) and write the
    payload behind token t_off of the cache tensors in `bufs` (same leading dimension), factors into segment `seg`, K outlier
    lists at position o_off.  fp16-stepwise arithmetic (the fused path's mode)."""
    lib = L.load()
    p = L.ptr
    NB = lead * B
    dev = k_src.device
    Tmax, g, fpi, bits = d["Tmax"], d["group"], d["fpi"], d["bits"]
    P0k = P0v = None
    if d["lowrank"]:
        P0k = _draw_p0((NB, H, D, d["rk"]), gen, dev, tp)
        P0v = _draw_p0((NB, H, D, d["rv"]), gen, dev, tp)
    v_exact = tp is not None and tp["world"] > 1 and tp.get("exact", True) and d["kv"] > 0
    if (USE_BLOCK_KERNEL and not v_exact and T == d["R"] == 64 and k_src is bufs.get("kwin") and v_src is bufs.get("vwin") and H <= 64
            and kk <= 16 and (d["kv"] <= 255 or "vochunk" not in bufs) and (H >= BLOCK_KERNEL_MIN_HEADS or H == 1 or not d["kv"])):
        # the decode-time block boundary: ONE launch over all (layer, head, K | V) tiles (csrc/block_fused.hip) instead of the
        # chain below (select, fused quantize + Gram, solve, Q pass; row compressor, Gram + solve, Q pass; chunk index; 2 tile
        # builders).  Same payload bits; the factors come from the token-side iteration (same subspace).
        view = _view(bufs, d, NB, H, D, kk0, seg0, kwin=True)
        if not kk:
            view.koidx = view.koval = None
        seg_k, seg_v = B * H * D * d["rk"], B * H * D * d["rv"]
        kP = bufs["kPseg"].view(-1)[seg * seg_k:] if d["lowrank"] else None
        vP = bufs["vPseg"].view(-1)[seg * seg_v:] if d["lowrank"] else None
        ws = _block_sync_ws(lib, NB, H, dev)
        rc = lib.gear_compress_block(C_.byref(view), t_off, o_off, loop, p(P0k), p(P0v), p(kP), p(vP), B * H, d["nseg"] * seg_k,
                                     d["nseg"] * seg_v, p(ws), ws.numel(), L.stream_ptr(k_src))
        L.check(rc, "gear_compress_block")
        return
    # per-segment channel factors [lead, nseg, B, H, D, r]: head (l, b, h) of segment seg
    def pseg(name, r):
        if not d["lowrank"]:
            return None, 0
        t = bufs[name]
        seg_elems = B * H * D * r
        return t.view(-1)[seg * seg_elems:], d["nseg"] * seg_elems
    kP, kP_stride = pseg("kPseg", d["rk"])
    vP, vP_stride = pseg("vPseg", d["rv"])
    wsb = max(lib.gear_compress_key_fused_workspace(NB * H, T, kk, d["rk"]),
              lib.gear_compress_value_fused_workspace(NB, H, T, d["rv"]))
    ws = C._workspace(wsb, dev)
    st = L.stream_ptr(k_src)
    rc = lib.gear_compress_key_fused(
        p(k_src), NB * H, T, g, bits, 0, kk, p(bufs["kcode"]), p(bufs["kscale"]), p(bufs["kmn"]), Tmax // fpi, Tmax // g,
        t_off, d["rk"], loop, p(P0k), p(kP), B * H, kP_stride, p(bufs.get("kQtok")), Tmax, t_off,
        p(bufs.get("koidx")) if kk else None, p(bufs.get("koval")) if kk else None, d["kcap"], o_off, 0, p(ws), ws.numel(), st)
    L.check(rc, "gear_compress_key_fused")
    if v_exact:
        _compress_value_exact(bufs, d, lead, B, H, D, v_src, T, t_off, seg, loop, P0v, tp, kk0, seg0)
    else:
        rc = lib.gear_compress_value_fused(
            p(v_src), NB, H, T, g, bits, 0, d["kv"], p(bufs["vcode"]), p(bufs["vscale"]), p(bufs["vmn"]), Tmax, t_off, d["rv"],
            loop, p(P0v), p(vP), B * H, vP_stride, p(bufs.get("vQtok")), Tmax, t_off, p(bufs.get("voidx")), p(bufs.get("voval")),
            p(ws), ws.numel(), st)
        L.check(rc, "gear_compress_value_fused")
    # chunk indices of the sparse lists (what lets a 128-token attention chunk find its outliers without a search):
    # V: one row of H + 1 head bounds per new (token row, side); K: the prompt segment's entries, once, at prefill
    if d["kv"] and "vochunk" in bufs and not v_exact:
        rc = lib.gear_outlier_chunk_index_ex(p(bufs["voidx"]), NB, 2 * T, 2 * Tmax, 2 * t_off, d["kv"], d["kv"], 128, H + 1,
                                             p(bufs["vochunk"]), H + 1, st)
        L.check(rc, "gear_outlier_chunk_index_ex(V)")
    if kk and seg == 0 and t_off == 0 and "kochunk" in bufs:
        rc = lib.gear_outlier_chunk_index_ex(p(bufs["koidx"]), 1, NB * H * D * 2, 0, 0, kk, d["kcap"], 128, (T + 127) // 128 + 1,
                                             p(bufs["kochunk"]), d["nbk"], st)
        L.check(rc, "gear_outlier_chunk_index_ex(K)")
    if "ktile" in bufs or "vtile" in bufs:      # sparse tiles of the chunks / blocks the new tokens lie in
        view = _view(bufs, d, NB, H, D, kk0, seg0, kwin=False)
        rc = lib.gear_cache_tiles_build(C_.byref(view), t_off + T, t_off // 128, (t_off + T + 127) // 128, t_off // 64,
                                        (t_off + T) // 64, st)
        L.check(rc, "gear_cache_tiles_build")


N_MAX_EXTEND = 2048      # query tokens per gear_attn_extend_cache call
N_MAX_VERIFY = 16        # query tokens per gear_attn_verify_cache call


def _rope_table(rope, like):
    """rope = (inv_freq, attn_factor) of a scaled model (gear_amd/rope.py): the table must be 64 fp32 values on the tensors' device."""
    inv_freq, attn_factor = rope
    if inv_freq.dtype != torch.float32 or inv_freq.numel() != 64 or inv_freq.device != like.device or not inv_freq.is_contiguous():
        raise L.GearError(f"rope table: 64 contiguous float32 values on {like.device} expected, got {list(inv_freq.shape)} "
                          f"{inv_freq.dtype} on {inv_freq.device}")
    return inv_freq, float(attn_factor)


def _rope_append(qkv, B, Hq, Hkv, D, pos, theta, rope, q, kwin, vwin, slot, W):
    """gear_rope_append, or its table flavour when `rope` is given."""
    if rope is None:
        rc = L.load().gear_rope_append(L.ptr(qkv), B, Hq, Hkv, D, pos, theta, L.ptr(q), L.ptr(kwin), L.ptr(vwin), slot, W,
                                       L.stream_ptr(qkv))
        L.check(rc, "gear_rope_append")
        return
    inv_freq, attn_factor = _rope_table(rope, qkv)
    rc = L.load().gear_rope_append_freq(L.ptr(qkv), B, Hq, Hkv, D, pos, L.ptr(inv_freq), attn_factor, L.ptr(q), L.ptr(kwin),
                                        L.ptr(vwin), slot, W, L.stream_ptr(qkv))
    L.check(rc, "gear_rope_append_freq")


def _check_rows(k, v, B, H, D, n):
    want = (B, H, n, D)
    if tuple(k.shape) != want or tuple(v.shape) != want or k.dtype != torch.float16 or v.dtype != torch.float16:
        raise ValueError(f"extend: K / V must be fp16 {list(want)}, got {list(k.shape)} {k.dtype} / {list(v.shape)} {v.dtype}")


def _check_room(c, n):
    """Refuse (before anything changes) n tokens that would take the compressed part past its capacity."""
    if n < 1:
        raise ValueError(f"extend: n = {n}, at least one token")
    fill = c.n_win + n
    n_comp = c.n_comp + (fill // c.R) * c.R
    if n_comp > c.Tmax:
        raise L.GearError(f"extend: {n} tokens after {c.seq_len} would compress {n_comp} tokens, the cache holds {c.Tmax}: "
                          "capacity exceeded")


def _tree_mask(anc, B, n, dev):
    """anc of an attend_verify_tree call -> contiguous 32-bit device tensor [B, n] ([n]: the same tree for every sequence)."""
    if not isinstance(anc, torch.Tensor) or anc.dtype not in (torch.int32, torch.uint32) or anc.device != dev:
        raise ValueError(f"attend_verify_tree: anc must be an int32 / uint32 tensor on {dev}")
    if anc.dtype == torch.uint32:
        anc = anc.view(torch.int32)           # (the same bits; torch has few uint32 operators)
    if anc.dim() == 1 or (anc.dim() == 2 and anc.shape[0] == 1 and B > 1):
        anc = anc.reshape(1, -1).expand(B, -1)
    if tuple(anc.shape) != (B, n):
        raise ValueError(f"attend_verify_tree: anc must be [{B}, {n}] or [{n}], got {list(anc.shape)}")
    return anc.contiguous()


def _reorder_index(src_idx, B, dev):
    """src_idx of a reorder call -> int32 device tensor [B].  A host list or CPU tensor is checked here (every entry in [0, B));
    a device tensor is not read on the host -- gear_cache_reorder treats an entry outside [0, B) as identity."""
    if isinstance(src_idx, torch.Tensor) and src_idx.is_cuda:
        if src_idx.dtype not in (torch.int32, torch.int64) or tuple(src_idx.shape) != (B,):
            raise ValueError(f"reorder: src_idx must be an int32 / int64 tensor [{B}], got {list(src_idx.shape)} {src_idx.dtype}")
        return src_idx.to(torch.int32).contiguous()
    if isinstance(src_idx, torch.Tensor):
        if src_idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"reorder: src_idx must be an int32 / int64 tensor, got {src_idx.dtype}")
        src_idx = src_idx.tolist()
    idx = [int(i) for i in src_idx] if isinstance(src_idx, (list, tuple)) else None
    if idx is None or len(idx) != B:
        raise ValueError(f"reorder: src_idx must hold {B} sequence indices, got {src_idx!r}")
    if any(i < 0 or i >= B for i in idx):
        raise ValueError(f"reorder: src_idx {idx} has entries outside [0, {B})")
    return torch.tensor(idx, dtype=torch.int32, device=dev)


def _state_view(obj, bufs, d, NB, H, D, kk0, seg0):
    """The window-carrying view of `bufs` at (kk0, seg0), kept on `obj`: what gear_cache_reorder and the snapshot entry points walk
    (the live ranges and the snapshot blob's layout depend on both counters)."""
    key = (kk0, seg0)
    if obj._rview_key != key:
        obj._rview, obj._rview_key = _view(bufs, d, NB, H, D, kk0, seg0, kwin=True), key
    return obj._rview


def _reorder(obj, bufs, d, n_layers, B, H, D, c0, src_idx):
    """gear_cache_reorder over `bufs` ([n_layers * B, ...] storage) at the counters of cache c0; the view and the workspace are kept
    on `obj`."""
    lib = L.load()
    dev = bufs["kwin"].device
    idx = _reorder_index(src_idx, B, dev)
    view = _state_view(obj, bufs, d, n_layers * B, H, D, c0.kk0, c0.seg0)
    wsb = lib.gear_cache_reorder_workspace(C_.byref(view), n_layers, B, c0.n_comp, c0.n_win)
    if wsb and (obj._rws is None or obj._rws.numel() < wsb):
        obj._rws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    rc = lib.gear_cache_reorder(C_.byref(view), n_layers, B, c0.n_comp, c0.n_win, L.ptr(idx), L.ptr(obj._rws) if wsb else None,
                                obj._rws.numel() if wsb else 0, L.stream_ptr(bufs["kwin"]))
    L.check(rc, "gear_cache_reorder")


class GearKVCachePool:
    """The buffers of ALL layers' caches as one tensor per field with a leading layer dimension.  Every layer's
    GearKVCache takes its (contiguous) slice, so nothing changes for the kernels; what the pool buys is the block boundary:
    all layers fill their fp16 windows on the same token, and with pooled storage the 32 per-layer compress sequences become
    ONE gear_compress_key_fused + ONE gear_compress_value_fused over [layers * batch, H, residual, 128] that write the block
    of every layer in place (compress_all): 7 launches per block boundary."""

    def __init__(self, n_layers: int, batch: int, n_kv_heads: int, max_tokens: int, compress_config: dict, device,
                 head_dim: int = 128, seed: int = 0, heads_total: int = None, tp: dict = None):
        """tp = dict(rank, world, group[, exact=True]): this pool holds one head shard of `world`; with exact (default) the V outliers
        of a token row are selected over all ranks' heads (one small all-gather per compress call, parallel.exact_v_selection)
        instead of k / world inside the shard."""
        self.tp = tp
        v_exact = tp is not None and tp["world"] > 1 and tp.get("exact", True)
        shapes, self.dims = _cache_dims(batch, n_kv_heads, max_tokens, compress_config, head_dim, heads_total, v_exact)
        if batch * n_kv_heads > 65535:
            raise L.GearError(f"GearKVCachePool: batch * kv heads = {batch * n_kv_heads} exceeds 65535 (one layer's heads ride on a "
                              "grid dimension of the prefill kernels)")
        self.L, self.B, self.H, self.D = n_layers, batch, n_kv_heads, head_dim
        self.loop = int(compress_config.get("loop", 3))
        self.buf = {}
        for n, (shp, dt) in shapes.items():
            if n in ("kPseg", "vPseg"):
                self.buf[n] = torch.zeros((n_layers,) + shp, dtype=dt, device=device)     # [L, nseg, B, H, D, r]
            else:
                self.buf[n] = torch.zeros((n_layers,) + shp, dtype=dt, device=device)
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(seed)
        self.caches = []
        self._rws = None
        self._rview = self._rview_key = None

    def reorder(self, src_idx):
        """Beam-search gather along the batch axis, in place, of every layer at once (gear_cache_reorder, two launches): afterwards
        sequence b holds in every layer what sequence src_idx[b] held -- compressed tokens, factors, outlier lists, tiles, window.
        src_idx: int32 / int64 device tensor [batch] (read on the device, no synchronisation), a CPU tensor or a list (checked
        here); repeats and cycles are allowed, sequences with src_idx[b] == b are not touched.  No counter changes."""
        c0 = self.caches[0]
        assert all(c.n_comp == c0.n_comp and c.n_win == c0.n_win and c.kk0 == c0.kk0 and c.seg0 == c0.seg0 for c in self.caches)
        _reorder(self, self.buf, self.dims, self.L, self.B, self.H, self.D, c0, src_idx)

    def snapshot(self, seq=None):
        """The live state of every layer as one packed blob (snapshot.CacheSnapshot; gear_cache_snapshot, one launch over the live
        bytes): all sequences with the counters and the generator states of the pool and of every layer's cache (seq=None), or
        sequence `seq` alone (no generator states: they belong to the whole batch)."""
        from . import snapshot as S
        return S.take(self, self.buf, self.dims, self.L, self.B, self.H, self.D, self.caches, self.gen, seq)

    def restore(self, snap, seq=None):
        """Put a snapshot back (gear_cache_restore, one launch).  A whole-batch snapshot of this batch size with seq=None restores
        everything -- buffers, every cache's counters, the generator states: what follows is bit-identical to what followed the
        snapshot.  A one-sequence snapshot with seq=None is broadcast to every sequence and sets the counters (one stored history
        forked `batch` ways); with seq=b it writes slot b alone and its counters must equal the current ones (the sequences of a
        pool advance in lockstep; ValueError otherwise).  In both one-sequence modes the generators are left alone: they draw the
        start bases of all batch rows at once, so later blocks of a fork follow the destination's generator.  A whole snapshot of
        a batch-1 standalone cache (which carries no pool generator state) counts as a one-sequence snapshot here.
        Refused before anything changes: a geometry that differs from this pool's (ValueError naming the entry), more tokens
        than the capacity (GearError).  Nothing is cleared past the live ranges: every block, list and tile is rewritten from
        the counters on and nothing reads past them (the argument DESIGN.md "Shared-prefix extend" gives for reset_shared())."""
        from . import snapshot as S
        S.put(self, self.buf, self.dims, self.L, self.B, self.H, self.D, self.caches, self.gen, snap, seq)

    def compress_all(self):
        """Every layer's window holds `residual` tokens: compress all of them in one go, in place behind the compressed
        tokens (the layers ride in the batch dimension)."""
        d, b, c0 = self.dims, self.buf, self.caches[0]
        R = d["R"]
        assert all(c.n_win == R and c.n_comp == c0.n_comp and c.kk0 == c0.kk0 for c in self.caches)
        t0, seg = c0.n_comp, c0._segment_of(c0.n_comp)
        assert t0 + R <= d["Tmax"], "cache capacity exceeded"
        o_off = c0.kk0 + ((t0 - c0.seg0) // R) * d["kk_blk"]
        # the chain's kernels put (layer, batch, head) on grid.y (<= 65535): when the single-launch block kernel does not apply
        # (see _compress_into) and the pool is larger than that, the layers go in groups
        per = max(1, 65535 // (self.B * self.H))
        groups = [(0, self.L)] if self.L <= per else [(l0, min(self.L, l0 + per)) for l0 in range(0, self.L, per)]
        for l0, l1 in groups:
            sub = b if (l0, l1) == (0, self.L) else {n: t[l0:l1] for n, t in b.items()}
            _compress_into(sub, d, l1 - l0, self.B, self.H, self.D, sub["kwin"], sub["vwin"], R, t0, seg, d["kk_blk"], o_off,
                           self.loop, self.gen, c0.kk0, c0.seg0, self.tp)
        for c in self.caches:
            c.n_comp += R
            c.n_win = 0

    def extend_all(self, k_list, v_list) -> int:
        """Commit n new tokens to every layer: k_list / v_list hold one fp16 [B, H, n, 128] (post-RoPE) per layer.  The windows
        fill up to `residual` and compress_all() runs at each boundary, exactly as n token steps would run it (same window
        contents, same generator order), so the result is bit-identical to that.  Refused before anything changes when the
        cache cannot take the tokens.  Returns the number of block boundaries crossed."""
        c0, R = self.caches[0], self.dims["R"]
        if len(k_list) != self.L or len(v_list) != self.L:
            raise ValueError(f"extend_all: {len(k_list)} / {len(v_list)} K / V tensors for {self.L} layers")
        n = k_list[0].shape[2]
        for k, v in zip(k_list, v_list):
            _check_rows(k, v, self.B, self.H, self.D, n)
        _check_room(c0, n)
        done = nb = 0
        while done < n:
            m = min(R - c0.n_win, n - done)
            w = c0.n_win
            for c, k, v in zip(self.caches, k_list, v_list):
                c.kwin[:, :, w:w + m] = k[:, :, done:done + m]
                c.vwin[:, :, w:w + m] = v[:, :, done:done + m]
                c.n_win += m
            done += m
            if c0.n_win == R:
                self.compress_all()
                nb += 1
        return nb


class GearKVCache:
    def __init__(self, batch: int, n_kv_heads: int, max_tokens: int, compress_config: dict, device, head_dim: int = 128,
                 seed: int = 0, state: torch.Tensor = None, pool: GearKVCachePool = None, layer: int = 0,
                 heads_total: int = None, tp: dict = None):
        assert head_dim == 128
        cc = compress_config
        self.tp = tp
        v_exact = tp is not None and tp["world"] > 1 and tp.get("exact", True)
        shapes, d = _cache_dims(batch, n_kv_heads, max_tokens, cc, head_dim, heads_total, v_exact)
        self.dims = d
        self.B, self.H, self.D = batch, n_kv_heads, head_dim
        self.bits, self.group, self.R = d["bits"], d["group"], d["R"]
        self.lowrank, self.rk, self.rv = d["lowrank"], d["rk"], d["rv"]
        self.loop = int(cc.get("loop", 3))
        self.fpi, self.Tmax = d["fpi"], d["Tmax"]
        self.kv, self.kk_blk, self.kcap = d["kv"], d["kk_blk"], d["kcap"]
        self.bufs = {}
        for name in ("kcode", "kscale", "kmn", "vcode", "vscale", "vmn", "kPseg", "kQtok", "vPseg", "vQtok", "kwin", "vwin",
                     "koidx", "koval", "voidx", "voval", "kochunk", "vochunk", "ktile", "kcnt", "vtile", "vcnt"):
            if name not in shapes:
                t = None
            elif pool is not None:          # this layer's slice of the pooled storage (contiguous, same layout)
                t = pool.buf[name][layer]
            else:
                shp, dt = shapes[name]
                t = torch.zeros(shp, dtype=dt, device=device)
            setattr(self, name, t)
            if t is not None:
                self.bufs[name] = t
        if pool is not None:
            pool.caches.append(self)
        self.n_comp = 0      # compressed tokens
        self.n_win = 0       # tokens in the fp16 window
        self.seg0 = 0        # tokens of segment 0 (the compressed part of the prompt)
        self.kk0 = 0         # K outliers per side and channel row of segment 0
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(seed)
        self._ws = None
        self._xws = None
        self._xsws = None
        self._vws = None
        self._sws = None
        self._rws = None
        self._rview = self._rview_key = None
        self.use_tiles = True     # tests switch these off to compare the list paths
        self.use_chunk_index = True
        self._views = {}
        # optional device-side {pos, slot, T, W} shared by all layers (the _dyn methods read it: hipGraph replay)
        self.state = state

    # ------------------------------------------------------------------------------------------------ state
    @property
    def seq_len(self) -> int:
        return self.n_comp + self.n_win

    def _segment_of(self, t0: int) -> int:
        return 0 if t0 < self.seg0 else 1 + (t0 - self.seg0) // self.R

    def _store(self, k_src, v_src, T, seg, kk, o_off):
        assert self.n_comp + T <= self.Tmax, "cache capacity exceeded"
        _compress_into(self.bufs, self.dims, 1, self.B, self.H, self.D, k_src, v_src, T, self.n_comp, seg, kk, o_off, self.loop,
                       self.gen, self.kk0, self.seg0, self.tp)
        self.n_comp += T

    def prefill(self, k: torch.Tensor, v: torch.Tensor):
        """k, v fp16 [B,Hkv,T,128] (post-RoPE): the first T - T % residual tokens are compressed as segment 0, the tail
        stays in the fp16 window (modeling_llamagear.py:390-434)."""
        assert self.seq_len == 0
        T = k.shape[2]
        nq = T - T % self.R
        if nq:
            self.seg0 = nq
            self.kk0 = min(self.dims["kk0_max"], nq // 2) if self.kk_blk else 0
            self._store(k[:, :, :nq].contiguous(), v[:, :, :nq].contiguous(), nq, 0, self.kk0, 0)
        self.n_win = T - nq
        if self.n_win:
            self.kwin[:, :, :self.n_win] = k[:, :, nq:]
            self.vwin[:, :, :self.n_win] = v[:, :, nq:]

    def append_rope(self, qkv: torch.Tensor, n_q_heads: int, pos: int, theta: float, rope=None) -> torch.Tensor:
        """qkv fp16 [B, (Hq + 2 Hkv) * 128] of the new token -> RoPE, k / v into the window; returns q [B,Hq,1,128].
        rope = (inv_freq fp32 device tensor [64], attn_factor): the frequencies of a scaled model (gear_amd/rope.py) instead of theta."""
        q = torch.empty((self.B, n_q_heads, 1, self.D), dtype=torch.float16, device=qkv.device)
        _rope_append(qkv, self.B, n_q_heads, self.H, self.D, pos, theta, rope, q, self.kwin, self.vwin, self.n_win, self.R)
        self.n_win += 1
        return q

    def append(self, k_new: torch.Tensor, v_new: torch.Tensor):
        """k_new, v_new fp16 [B,Hkv,1,128] (already rotated) into the window."""
        self.kwin[:, :, self.n_win] = k_new[:, :, 0]
        self.vwin[:, :, self.n_win] = v_new[:, :, 0]
        self.n_win += 1

    def _attend(self, q, T, W, dyn, return_lse=False):
        B, Hq = q.shape[0], q.shape[1]
        lib = L.load()
        out = torch.empty((B, Hq, 1, self.D), dtype=torch.float16, device=q.device)
        lse = torch.empty((B, Hq), dtype=torch.float32, device=q.device) if return_lse else None
        wsb = lib.gear_attn_decode_workspace(B, Hq, self.Tmax, self.bits)
        if self._ws is None or self._ws.numel() < wsb:
            self._ws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)
        key = (self.kk0, self.seg0, bool(W or dyn is not None), self.use_tiles, self.use_chunk_index)
        view = self._views.get(key)
        if view is None:      # the view is a function of the prompt split only: built once per cache, not per token
            view = _view(self.bufs, self.dims, B, self.H, self.D, self.kk0, self.seg0, kwin=key[2])
            if not self.use_tiles:
                view.ktile = view.vtile = None
            if not self.use_chunk_index:
                view.kochunk = view.vochunk = None
            self._views[key] = view
        rc = lib.gear_attn_decode_cache(C_.byref(view), L.ptr(q), Hq, T, W, L.ptr(dyn), 1.0 / math.sqrt(self.D), L.ptr(out),
                                        L.ptr(lse), L.ptr(self._ws), self._ws.numel(), L.stream_ptr(q))
        L.check(rc, "gear_attn_decode_cache")
        return (out, lse) if return_lse else out

    def attend(self, q: torch.Tensor, return_lse: bool = False):
        """q fp16 [B,Hq,1,128] -> softmax(q Khat^T / sqrt(128)) Vhat over compressed + window tokens, fp16 [B,Hq,1,128]; with
        return_lse also the fp32 [B,Hq] log-sum-exp of the scaled scores (the merge then runs in its own launch: attn_fold
        does not apply)."""
        return self._attend(q, self.n_comp, self.n_win, None, return_lse)

    # ---- device-state variants: no host-side counters change here (a captured graph replays these launches) ----------
    def append_rope_dyn(self, qkv: torch.Tensor, n_q_heads: int, theta: float, rope=None) -> torch.Tensor:
        q = torch.empty((self.B, n_q_heads, 1, self.D), dtype=torch.float16, device=qkv.device)
        if rope is None:
            rc = L.load().gear_rope_append_dyn(L.ptr(qkv), self.B, n_q_heads, self.H, self.D, L.ptr(self.state), theta, L.ptr(q),
                                               L.ptr(self.kwin), L.ptr(self.vwin), self.R, L.stream_ptr(qkv))
            L.check(rc, "gear_rope_append_dyn")
        else:
            inv_freq, attn_factor = _rope_table(rope, qkv)
            rc = L.load().gear_rope_append_dyn_freq(L.ptr(qkv), self.B, n_q_heads, self.H, self.D, L.ptr(self.state), L.ptr(inv_freq),
                                                    attn_factor, L.ptr(q), L.ptr(self.kwin), L.ptr(self.vwin), self.R,
                                                    L.stream_ptr(qkv))
            L.check(rc, "gear_rope_append_dyn_freq")
        return q

    def attend_dyn(self, q: torch.Tensor) -> torch.Tensor:
        return self._attend(q, self.Tmax, self.R, self.state)

    def maybe_compress(self):
        """Compress the window when it holds `residual` tokens (modeling_llamagear.py:265, :335)."""
        if self.n_win == self.R:
            seg = self._segment_of(self.n_comp)
            o_off = self.kk0 + ((self.n_comp - self.seg0) // self.R) * self.kk_blk
            self._store(self.kwin, self.vwin, self.R, seg, self.kk_blk, o_off)
            self.n_win = 0

    def attend_extend(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, return_lse: bool = False):
        """Chunk attention: q fp16 [B,Hq,n,128] at positions seq_len .. seq_len + n - 1, k_new / v_new fp16 [B,Hkv,n,128] (post-RoPE)
        -> fp16 [B,Hq,n,128] (with return_lse also the fp32 [B,Hq,n] log-sum-exp of the scaled scores).  Query i attends over the
        compressed tokens, the window and chunk rows 0 .. i (one fp32 softmax, gear_attn_extend_cache).  Changes no state; extend()
        commits the rows.  At most N_MAX_EXTEND tokens per call."""
        B, Hq, n = q.shape[0], q.shape[1], q.shape[2]
        _check_rows(k_new, v_new, self.B, self.H, self.D, n)
        if tuple(q.shape) != (self.B, Hq, n, self.D) or q.dtype != torch.float16:
            raise ValueError(f"attend_extend: q must be fp16 [{self.B}, Hq, {n}, {self.D}], got {list(q.shape)} {q.dtype}")
        lib = L.load()
        q, k_new, v_new = q.contiguous(), k_new.contiguous(), v_new.contiguous()
        out = torch.empty_like(q)
        lse = torch.empty((B, Hq, n), dtype=torch.float32, device=q.device) if return_lse else None
        wsb = lib.gear_attn_extend_workspace(B, Hq, n, self.n_comp, self.n_win)
        if self._xws is None or self._xws.numel() < wsb:
            self._xws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)
        key = (self.kk0, self.seg0, True, True, True)
        view = self._views.get(key)
        if view is None:
            view = self._views[key] = _view(self.bufs, self.dims, B, self.H, self.D, self.kk0, self.seg0, kwin=True)
        rc = lib.gear_attn_extend_cache(C_.byref(view), L.ptr(q), Hq, n, self.n_comp, self.n_win, L.ptr(k_new), L.ptr(v_new),
                                        1.0 / math.sqrt(self.D), L.ptr(out), L.ptr(lse), L.ptr(self._xws), self._xws.numel(),
                                        L.stream_ptr(q))
        L.check(rc, "gear_attn_extend_cache")
        return (out, lse) if return_lse else out

    def attend_verify(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, return_lse: bool = False):
        """attend_extend for the draft sizes of speculative decoding (n <= N_MAX_VERIFY): the same result through the decode
        kernels (gear_attn_verify_cache; the attention options apply as for attend(), except attn_fold).  Changes no state."""
        B, Hq, n = q.shape[0], q.shape[1], q.shape[2]
        if n > N_MAX_VERIFY:
            raise ValueError(f"attend_verify: n = {n} query tokens, at most N_MAX_VERIFY = {N_MAX_VERIFY}: use attend_extend")
        _check_rows(k_new, v_new, self.B, self.H, self.D, n)
        if tuple(q.shape) != (self.B, Hq, n, self.D) or q.dtype != torch.float16:
            raise ValueError(f"attend_verify: q must be fp16 [{self.B}, Hq, {n}, {self.D}], got {list(q.shape)} {q.dtype}")
        lib = L.load()
        q, k_new, v_new = q.contiguous(), k_new.contiguous(), v_new.contiguous()
        out = torch.empty_like(q)
        lse = torch.empty((B, Hq, n), dtype=torch.float32, device=q.device) if return_lse else None
        wsb = lib.gear_attn_verify_workspace(B, Hq, n, self.n_comp, self.n_win)
        if self._vws is None or self._vws.numel() < wsb:
            self._vws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)
        key = (self.kk0, self.seg0, True, self.use_tiles, self.use_chunk_index)
        view = self._views.get(key)
        if view is None:
            view = _view(self.bufs, self.dims, B, self.H, self.D, self.kk0, self.seg0, kwin=True)
            if not self.use_tiles:
                view.ktile = view.vtile = None
            if not self.use_chunk_index:
                view.kochunk = view.vochunk = None
            self._views[key] = view
        rc = lib.gear_attn_verify_cache(C_.byref(view), L.ptr(q), Hq, n, self.n_comp, self.n_win, L.ptr(k_new), L.ptr(v_new),
                                        1.0 / math.sqrt(self.D), L.ptr(out), L.ptr(lse), L.ptr(self._vws), self._vws.numel(),
                                        L.stream_ptr(q))
        L.check(rc, "gear_attn_verify_cache")
        return (out, lse) if return_lse else out

    def attend_verify_tree(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, anc: torch.Tensor,
                           return_lse: bool = False):
        """attend_verify over a draft tree (gear_attn_verify_tree): row i attends over the cache and those chunk rows j whose bit j
        is set in anc[b, i] -- anc int32 / uint32 device tensor [B, n] (speculative.tree_layout), an [n] tensor serves every
        sequence.  The kernel forces bit i and drops the bits above it.  Workspace and view are attend_verify's.  Changes no state."""
        B, Hq, n = q.shape[0], q.shape[1], q.shape[2]
        if n > N_MAX_VERIFY:
            raise ValueError(f"attend_verify_tree: n = {n} query tokens, at most N_MAX_VERIFY = {N_MAX_VERIFY}")
        _check_rows(k_new, v_new, self.B, self.H, self.D, n)
        if tuple(q.shape) != (self.B, Hq, n, self.D) or q.dtype != torch.float16:
            raise ValueError(f"attend_verify_tree: q must be fp16 [{self.B}, Hq, {n}, {self.D}], got {list(q.shape)} {q.dtype}")
        anc = _tree_mask(anc, self.B, n, q.device)
        lib = L.load()
        q, k_new, v_new = q.contiguous(), k_new.contiguous(), v_new.contiguous()
        out = torch.empty_like(q)
        lse = torch.empty((B, Hq, n), dtype=torch.float32, device=q.device) if return_lse else None
        wsb = lib.gear_attn_verify_tree_workspace(B, Hq, n, self.n_comp, self.n_win)
        if self._vws is None or self._vws.numel() < wsb:
            self._vws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)
        key = (self.kk0, self.seg0, True, self.use_tiles, self.use_chunk_index)
        view = self._views.get(key)
        if view is None:
            view = _view(self.bufs, self.dims, B, self.H, self.D, self.kk0, self.seg0, kwin=True)
            if not self.use_tiles:
                view.ktile = view.vtile = None
            if not self.use_chunk_index:
                view.kochunk = view.vochunk = None
            self._views[key] = view
        rc = lib.gear_attn_verify_tree(C_.byref(view), L.ptr(q), Hq, n, self.n_comp, self.n_win, L.ptr(k_new), L.ptr(v_new),
                                       L.ptr(anc), 1.0 / math.sqrt(self.D), L.ptr(out), L.ptr(lse), L.ptr(self._vws),
                                       self._vws.numel(), L.stream_ptr(q))
        L.check(rc, "gear_attn_verify_tree")
        return (out, lse) if return_lse else out

    def attend_shared(self, q: torch.Tensor, prefix: "GearKVCache", return_lse: bool = False):
        """Shared-prefix decode attention: this cache (batch S) holds what each of S sequences appended after ONE common prompt,
        `prefix` (a GearKVCache with batch 1, an empty window and the same compress config) holds that prompt's compressed tokens.
        q fp16 [S,Hq,1,128] -> fp16 [S,Hq,1,128]: row (s, hq) is one fp32 softmax over the prefix's tokens, then sequence s's
        compressed tokens, then its window (gear_attn_decode_shared; with return_lse also the fp32 [S,Hq] log-sum-exp).  Changes
        no state of either cache.  use_tiles / use_chunk_index of this cache apply to both views."""
        if not isinstance(prefix, GearKVCache) or prefix.B != 1 or prefix.n_win != 0:
            raise ValueError("attend_shared: prefix must be a GearKVCache with batch 1 and an empty window")
        if (prefix.H, prefix.D, prefix.bits, prefix.group, prefix.R, prefix.rk, prefix.rv, prefix.kv, prefix.kk_blk) != \
                (self.H, self.D, self.bits, self.group, self.R, self.rk, self.rv, self.kv, self.kk_blk):
            raise ValueError("attend_shared: prefix and tail caches were built with different compress configs / head counts")
        S, Hq = q.shape[0], q.shape[1]
        if tuple(q.shape) != (self.B, Hq, 1, self.D) or q.dtype != torch.float16:
            raise ValueError(f"attend_shared: q must be fp16 [{self.B}, Hq, 1, {self.D}], got {list(q.shape)} {q.dtype}")
        lib = L.load()
        q = q.contiguous()
        L.require_gpu(q)
        out = torch.empty((S, Hq, 1, self.D), dtype=torch.float16, device=q.device)
        lse = torch.empty((S, Hq), dtype=torch.float32, device=q.device) if return_lse else None
        wsb = lib.gear_attn_decode_shared_workspace(S, Hq, prefix.Tmax, self.Tmax, self.bits)
        if self._sws is None or self._sws.numel() < wsb:
            self._sws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)
        views = []
        for c, win in ((prefix, False), (self, True)):
            key = (c.kk0, c.seg0, win, self.use_tiles, self.use_chunk_index)
            view = c._views.get(key)
            if view is None:
                view = _view(c.bufs, c.dims, c.B, c.H, c.D, c.kk0, c.seg0, kwin=win)
                if not self.use_tiles:
                    view.ktile = view.vtile = None
                if not self.use_chunk_index:
                    view.kochunk = view.vochunk = None
                c._views[key] = view
            views.append(view)
        rc = lib.gear_attn_decode_shared(C_.byref(views[0]), prefix.n_comp, C_.byref(views[1]), self.n_comp, self.n_win, L.ptr(q),
                                         Hq, 1.0 / math.sqrt(self.D), L.ptr(out), L.ptr(lse), L.ptr(self._sws), self._sws.numel(),
                                         L.stream_ptr(q))
        L.check(rc, "gear_attn_decode_shared")
        return (out, lse) if return_lse else out

    def attend_extend_shared(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, prefix: "GearKVCache",
                             return_lse: bool = False):
        """Shared-prefix chunk attention: attend_extend for the S sequences of this (tail) cache behind ONE stored prompt, `prefix`
        (as for attend_shared: batch 1, an empty window, the same compress config).  q fp16 [S,Hq,n,128], k_new / v_new fp16
        [S,Hkv,n,128] (post-RoPE) -> fp16 [S,Hq,n,128] (with return_lse also the fp32 [S,Hq,n] log-sum-exp): row (s, hq, i) is one
        fp32 softmax over the prefix's tokens, sequence s's compressed tokens, its window and its chunk rows 0 .. i
        (gear_attn_extend_shared).  Changes no state of either cache.  At most N_MAX_EXTEND tokens per call."""
        if not isinstance(prefix, GearKVCache) or prefix.B != 1 or prefix.n_win != 0:
            raise ValueError("attend_extend_shared: prefix must be a GearKVCache with batch 1 and an empty window")
        if (prefix.H, prefix.D, prefix.bits, prefix.group, prefix.R, prefix.rk, prefix.rv, prefix.kv, prefix.kk_blk) != \
                (self.H, self.D, self.bits, self.group, self.R, self.rk, self.rv, self.kv, self.kk_blk):
            raise ValueError("attend_extend_shared: prefix and tail caches were built with different compress configs / head counts")
        if q.dim() != 4:
            raise ValueError(f"attend_extend_shared: q must be fp16 [{self.B}, Hq, n, {self.D}], got {list(q.shape)} {q.dtype}")
        S, Hq, n = q.shape[0], q.shape[1], q.shape[2]
        _check_rows(k_new, v_new, self.B, self.H, self.D, n)
        if tuple(q.shape) != (self.B, Hq, n, self.D) or q.dtype != torch.float16:
            raise ValueError(f"attend_extend_shared: q must be fp16 [{self.B}, Hq, {n}, {self.D}], got {list(q.shape)} {q.dtype}")
        if n > N_MAX_EXTEND:
            raise ValueError(f"attend_extend_shared: n = {n} query tokens, at most N_MAX_EXTEND = {N_MAX_EXTEND}")
        lib = L.load()
        q, k_new, v_new = q.contiguous(), k_new.contiguous(), v_new.contiguous()
        L.require_gpu(q, k_new, v_new)
        out = torch.empty_like(q)
        lse = torch.empty((S, Hq, n), dtype=torch.float32, device=q.device) if return_lse else None
        wsb = lib.gear_attn_extend_shared_workspace(S, Hq, n, max(prefix.n_comp, 64), self.n_comp, self.n_win)
        if self._xsws is None or self._xsws.numel() < wsb:
            self._xsws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)
        views = []
        for c, win in ((prefix, False), (self, True)):
            key = (c.kk0, c.seg0, win, True, True)
            view = c._views.get(key)
            if view is None:
                view = c._views[key] = _view(c.bufs, c.dims, c.B, c.H, c.D, c.kk0, c.seg0, kwin=win)
            views.append(view)
        rc = lib.gear_attn_extend_shared(C_.byref(views[0]), prefix.n_comp, C_.byref(views[1]), self.n_comp, self.n_win, L.ptr(q), Hq,
                                         n, L.ptr(k_new), L.ptr(v_new), 1.0 / math.sqrt(self.D), L.ptr(out), L.ptr(lse),
                                         L.ptr(self._xsws), self._xsws.numel(), L.stream_ptr(q))
        L.check(rc, "gear_attn_extend_shared")
        return (out, lse) if return_lse else out

    def reorder(self, src_idx):
        """GearKVCachePool.reorder for one cache (standalone, or one layer of a pool): sequence b takes over the state of sequence
        src_idx[b], in place; n_comp / n_win / seg0 / kk0 do not change."""
        _reorder(self, self.bufs, self.dims, 1, self.B, self.H, self.D, self, src_idx)

    def snapshot(self, seq=None):
        """GearKVCachePool.snapshot for one cache (standalone, or one layer of a pool): the live state as one packed blob, all
        sequences with the counters and this cache's generator state (seq=None) or one sequence."""
        from . import snapshot as S
        return S.take(self, self.bufs, self.dims, 1, self.B, self.H, self.D, [self], None, seq)

    def restore(self, snap, seq=None):
        """GearKVCachePool.restore for one cache: whole batch (counters and generator state included), a one-sequence snapshot
        broadcast to every sequence (seq=None) or into slot `seq` at equal counters; the same refusals, the same reliance on
        nothing reading past the live counters."""
        from . import snapshot as S
        S.put(self, self.bufs, self.dims, 1, self.B, self.H, self.D, [self], None, snap, seq)

    def extend(self, k_new: torch.Tensor, v_new: torch.Tensor):
        """Commit n tokens (fp16 [B,Hkv,n,128], post-RoPE): through the window, compressing each time it holds `residual` tokens --
        bit-identical to n x (append + maybe_compress).  Refused before anything changes when the cache cannot take them."""
        n = k_new.shape[2]
        _check_rows(k_new, v_new, self.B, self.H, self.D, n)
        _check_room(self, n)
        done = 0
        while done < n:
            m = min(self.R - self.n_win, n - done)
            self.kwin[:, :, self.n_win:self.n_win + m] = k_new[:, :, done:done + m]
            self.vwin[:, :, self.n_win:self.n_win + m] = v_new[:, :, done:done + m]
            self.n_win += m
            done += m
            self.maybe_compress()


class Fp16KVCache:
    """The UNCOMPRESSED baseline behind the same decoder (the model "None" the reference's harness times beside gearl / KIVI,
    cuda_supported_gear/test.py:41-62): every token's K / V stays fp16 in a pre-allocated [B, Hkv, capacity, 128] pair, the
    attention is gear_attn_decode_f16 (the same split / merge kernels as the compressed path).  It has GearKVCache's window
    interface -- the "window" is the whole cache --, so FastGearDecoder's fused q/k/v projection appends to it unchanged."""

    MAX_TOKENS = 8320      # gear_attn_decode_f16: 65 chunks of 128 tokens in one merge (csrc/attention.hip RS_MAX)

    def __init__(self, batch: int, n_kv_heads: int, max_tokens: int, device, head_dim: int = 128):
        if max_tokens > self.MAX_TOKENS:
            raise L.GearError(f"Fp16KVCache: capacity {max_tokens} > {self.MAX_TOKENS} tokens, the longest context "
                              "gear_attn_decode_f16 merges in one launch (the baseline would fail at its first attend())")
        self.B, self.H, self.D = batch, n_kv_heads, head_dim
        self.R = max_tokens
        self.kwin = torch.zeros((batch, n_kv_heads, max_tokens, head_dim), dtype=torch.float16, device=device)
        self.vwin = torch.zeros_like(self.kwin)
        self.n_win = 0
        self.n_comp = 0
        self.state = None

    @property
    def seq_len(self) -> int:
        return self.n_win

    def prefill(self, k: torch.Tensor, v: torch.Tensor):
        assert self.n_win == 0 and k.shape[2] <= self.R
        T = k.shape[2]
        self.kwin[:, :, :T] = k
        self.vwin[:, :, :T] = v
        self.n_win = T

    def append_rope(self, qkv: torch.Tensor, n_q_heads: int, pos: int, theta: float, rope=None) -> torch.Tensor:
        if self.n_win >= self.R:
            raise L.GearError(f"Fp16KVCache: capacity {self.R} reached")
        q = torch.empty((self.B, n_q_heads, 1, self.D), dtype=torch.float16, device=qkv.device)
        _rope_append(qkv, self.B, n_q_heads, self.H, self.D, pos, theta, rope, q, self.kwin, self.vwin, self.n_win, self.R)
        self.n_win += 1
        return q

    def attend(self, q: torch.Tensor) -> torch.Tensor:
        from .attention import decode_attention_f16
        return decode_attention_f16(q, self.kwin, self.vwin, T=self.n_win)

    def attend_extend(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor) -> torch.Tensor:
        """Chunk attention of the uncompressed baseline: query i over the cached rows and chunk rows 0 .. i (torch SDPA with the
        causal offset; not a product path).  Changes no state."""
        n, Hq = q.shape[2], q.shape[1]
        _check_rows(k_new, v_new, self.B, self.H, self.D, n)
        k = torch.cat([self.kwin[:, :, :self.n_win], k_new], 2)
        v = torch.cat([self.vwin[:, :, :self.n_win], v_new], 2)
        if Hq != self.H:
            k, v = k.repeat_interleave(Hq // self.H, 1), v.repeat_interleave(Hq // self.H, 1)
        mask = torch.ones((n, self.n_win + n), dtype=torch.bool, device=q.device).tril(self.n_win)
        return torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask)

    def attend_verify(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, return_lse: bool = False):
        """The speculative-verify interface of GearKVCache on the baseline: attend_extend (torch SDPA), with return_lse also the
        fp32 [B, Hq, n] log-sum-exp of the scaled scores.  Changes no state."""
        n, Hq = q.shape[2], q.shape[1]
        if n > N_MAX_VERIFY:
            raise ValueError(f"attend_verify: n = {n} query tokens, at most N_MAX_VERIFY = {N_MAX_VERIFY}: use attend_extend")
        out = self.attend_extend(q, k_new, v_new)
        if not return_lse:
            return out
        k = torch.cat([self.kwin[:, :, :self.n_win], k_new], 2).float()
        if Hq != self.H:
            k = k.repeat_interleave(Hq // self.H, 1)
        s = torch.einsum("bhid,bhtd->bhit", q.float(), k) / math.sqrt(self.D)
        mask = torch.ones((n, self.n_win + n), dtype=torch.bool, device=q.device).tril(self.n_win)
        return out, torch.logsumexp(s.masked_fill(~mask, float("-inf")), -1)

    def attend_verify_tree(self, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, anc: torch.Tensor,
                           return_lse: bool = False):
        """GearKVCache.attend_verify_tree on the baseline: torch SDPA with a boolean mask built from anc (bit i forced, the bits
        above i dropped, as the kernel does); not a product path.  Changes no state."""
        n, Hq = q.shape[2], q.shape[1]
        if n > N_MAX_VERIFY:
            raise ValueError(f"attend_verify_tree: n = {n} query tokens, at most N_MAX_VERIFY = {N_MAX_VERIFY}")
        _check_rows(k_new, v_new, self.B, self.H, self.D, n)
        row = torch.arange(n, device=q.device)
        m = (_tree_mask(anc, self.B, n, q.device).long() & 0xFFFFFFFF | (1 << row)) & ((2 << row) - 1)          # [B, n]
        mask = torch.cat([torch.ones((self.B, n, self.n_win), dtype=torch.bool, device=q.device),
                          (m[:, :, None] >> row) & 1 != 0], 2)[:, None]                                          # [B, 1, n, W + n]
        k = torch.cat([self.kwin[:, :, :self.n_win], k_new], 2)
        v = torch.cat([self.vwin[:, :, :self.n_win], v_new], 2)
        if Hq != self.H:
            k, v = k.repeat_interleave(Hq // self.H, 1), v.repeat_interleave(Hq // self.H, 1)
        out = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask)
        if not return_lse:
            return out
        s = torch.einsum("bhid,bhtd->bhit", q.float(), k.float()) / math.sqrt(self.D)
        return out, torch.logsumexp(s.masked_fill(~mask, float("-inf")), -1)

    def extend(self, k_new: torch.Tensor, v_new: torch.Tensor):
        n = k_new.shape[2]
        _check_rows(k_new, v_new, self.B, self.H, self.D, n)
        if self.n_win + n > self.R:
            raise L.GearError(f"Fp16KVCache: {n} tokens after {self.n_win} exceed the capacity {self.R}")
        self.kwin[:, :, self.n_win:self.n_win + n] = k_new
        self.vwin[:, :, self.n_win:self.n_win + n] = v_new
        self.n_win += n



class KiviKVCache:
    """The KIVI baseline's cache for one attention layer on the fused decode path (csrc/kivi.hip): the state machine of the KIVI
    attention hook (modeling_llama_kivi.py; cuda_supported_gear/modeling_llama_kivi.py:149-162, :200-248), pre-allocated.

    K: an fp16 window `kwin` [B, Hkv, R, 128] that is quantized per channel as ONE block when it holds R = `residual` tokens
       (maybe_compress(), eagerly between steps); the prompt is split at T - T % R.
    V: a sliding fp16 window kept as a RING `vring` [B, Hkv, R + 1, 128] -- token t lives in row t % (R + 1).  The hook quantizes
       the oldest of R + 1 rows right after the step's attention; here that row stays where it is until the NEXT token's append
       overwrites it, and the append launch quantizes it first (gear_kivi_rope_append: no launch of its own).  Every attend()
       therefore sees what the hook's attention sees: R + 1 fp16 rows and `n_vpacked` = L - (R + 1) packed rows.  The prompt keeps
       its last R rows in fp16.
    The packed fields have GearKVCache's layouts (kcode [B,Hkv,128,Tmax/fpi], kscale / kmn [B,Hkv,128,Tmax/group]; vcode
    [B,Hkv,Tmax,128/fpi], vscale / vmn [B,Hkv,Tmax,128/group]): the decode partial kernels read them unchanged.

    State (host counters): seq_len = L; n_kpacked (a multiple of R) and n_kwin = L - n_kpacked; n_vpacked rows written to vcode,
    n_vwin = L - n_vpacked fp16 rows in the ring (at most R + 1), the oldest of them in row ring_start.  v_pending is 1 while the
    ring holds R + 1 rows: the hook's tuple then already counts the oldest as packed (hook_counters())."""

    def __init__(self, batch: int, n_kv_heads: int, max_tokens: int, bits: int, group: int, residual: int, device,
                 head_dim: int = 128):
        if head_dim != 128 or bits not in (2, 4) or group != 64 or residual not in (64, 128):
            raise L.GearError(f"KiviKVCache: head_dim 128, bits 2 / 4, group 64 and residual 64 / 128 are built (got head_dim "
                              f"{head_dim}, bits {bits}, group {group}, residual {residual})")
        R = residual
        self.B, self.H, self.D = batch, n_kv_heads, head_dim
        self.bits, self.group, self.R = bits, group, R
        self.fpi = 32 // bits
        self.Tmax = (max_tokens + R - 1) // R * R
        if self.Tmax > 16384 or max_tokens < 1:
            raise L.GearError(f"KiviKVCache: capacity {max_tokens} tokens, must lie in [1, 16384]")
        B, H, D, T, fpi = batch, n_kv_heads, head_dim, self.Tmax, self.fpi
        z = lambda shp, dt: torch.zeros(shp, dtype=dt, device=device)
        self.kcode, self.kscale, self.kmn = z((B, H, D, T // fpi), torch.int32), z((B, H, D, T // group), torch.float16), \
            z((B, H, D, T // group), torch.float16)
        self.vcode, self.vscale, self.vmn = z((B, H, T, D // fpi), torch.int32), z((B, H, T, D // group), torch.float16), \
            z((B, H, T, D // group), torch.float16)
        self.kwin = z((B, H, R, D), torch.float16)
        self.vring = z((B, H, R + 1, D), torch.float16)
        self.n_tok = 0           # L
        self.n_kpacked = 0       # Tk
        self.n_vpacked = 0       # Nv
        self._ws = None
        v = L.CacheView()
        for f in ("kcode", "kscale", "kmn", "vcode", "vscale", "vmn", "kwin"):
            setattr(v, f, L.ptr(getattr(self, f)))
        v.vwin = L.ptr(self.vring)
        v.B, v.Hkv, v.D, v.tcap = B, H, D, T
        v.ldk, v.lsk, v.group, v.bits, v.mode, v.wcap = T // fpi, T // group, group, bits, 0, R
        self._view = v

    # ------------------------------------------------------------------------------------------------ state
    @property
    def seq_len(self) -> int:
        return self.n_tok

    @property
    def n_kwin(self) -> int:
        return self.n_tok - self.n_kpacked

    @property
    def n_vwin(self) -> int:
        return self.n_tok - self.n_vpacked

    @property
    def ring_start(self) -> int:
        """Ring row of the oldest fp16 V token (token n_vpacked)."""
        return self.n_vpacked % (self.R + 1)

    @property
    def v_pending(self) -> int:
        return 1 if self.n_vwin == self.R + 1 else 0

    def hook_counters(self):
        """(packed K tokens, fp16 K rows, packed V rows, fp16 V rows) as the hook's 9-slot tuple shows them after the same
        tokens: the oldest of R + 1 ring rows counts as packed (the next append writes its codes)."""
        return self.n_kpacked, self.n_kwin, self.n_vpacked + self.v_pending, self.n_vwin - self.v_pending

    def ring_tokens(self) -> torch.Tensor:
        """The fp16 V rows in token order: [B, Hkv, n_vwin, 128] (tokens n_vpacked .. L - 1)."""
        idx = torch.arange(self.n_vpacked, self.n_tok, device=self.vring.device) % (self.R + 1)
        return self.vring.index_select(2, idx)

    def _quantize_k(self, k_rows: torch.Tensor, t0: int):
        """k_rows fp16 [B, Hkv, n, 128] (n a multiple of R) -> codes, scales and minima of tokens [t0, t0 + n), per channel along
        the tokens: the quantizer call of the hook (modeling_llama_kivi.py: K^T packed along its last dimension)."""
        from .quant.new_pack import triton_quantize_and_pack_along_last_dim
        n = k_rows.shape[2]
        code, scale, mn = triton_quantize_and_pack_along_last_dim(k_rows.transpose(2, 3).contiguous(), self.group, self.bits)
        self.kcode[:, :, :, t0 // self.fpi:(t0 + n) // self.fpi] = code
        self.kscale[:, :, :, t0 // self.group:(t0 + n) // self.group] = scale
        self.kmn[:, :, :, t0 // self.group:(t0 + n) // self.group] = mn

    def prefill(self, k: torch.Tensor, v: torch.Tensor):
        """k, v fp16 [B, Hkv, T, 128] (post-RoPE).  K: the first T - T % R tokens are packed, the rest go to the window.  V:
        T <= R: every row stays fp16; otherwise the first T - R rows are packed per token and the last R go to the ring."""
        from .quant.new_pack import triton_quantize_and_pack_along_last_dim
        assert self.n_tok == 0
        T, R = k.shape[2], self.R
        if tuple(k.shape) != (self.B, self.H, T, self.D) or tuple(v.shape) != tuple(k.shape) or k.dtype != torch.float16 \
                or v.dtype != torch.float16:
            raise ValueError(f"KiviKVCache.prefill: K / V must be fp16 [{self.B}, {self.H}, T, {self.D}], got {list(k.shape)} "
                             f"{k.dtype} / {list(v.shape)} {v.dtype}")
        if T < 1 or T > self.Tmax:
            raise L.GearError(f"KiviKVCache.prefill: {T} tokens, the cache holds {self.Tmax}")
        nq = T - T % R
        if nq:
            self._quantize_k(k[:, :, :nq], 0)
        if nq < T:
            self.kwin[:, :, :T - nq] = k[:, :, nq:]
        nv = max(0, T - R)
        if nv:
            code, scale, mn = triton_quantize_and_pack_along_last_dim(v[:, :, :nv].contiguous(), self.group, self.bits)
            self.vcode[:, :, :nv], self.vscale[:, :, :nv], self.vmn[:, :, :nv] = code, scale, mn
        idx = torch.arange(nv, T, device=v.device) % (R + 1)
        self.vring.index_copy_(2, idx, v[:, :, nv:])
        self.n_tok, self.n_kpacked, self.n_vpacked = T, nq, nv

    def _evict_row(self) -> int:
        """The vcode row the next append must write before it overwrites its ring row (-1: that row is free or already packed)."""
        if self.n_kwin >= self.R:
            raise L.GearError(f"KiviKVCache: the K window is full ({self.n_kwin} of {self.R} rows): call maybe_compress() after "
                              "every step")
        if self.n_kwin == self.R - 1 and self.n_kpacked + self.R > self.Tmax:
            raise L.GearError(f"KiviKVCache: capacity reached ({self.n_tok} tokens; {self.Tmax} packed K tokens at most)")
        row = self.n_tok - (self.R + 1)
        return row if row >= self.n_vpacked else -1

    def _appended(self, row):
        if row >= 0:
            self.n_vpacked = row + 1
        self.n_tok += 1

    def append_rope(self, qkv: torch.Tensor, n_q_heads: int, pos: int, theta: float, rope=None) -> torch.Tensor:
        """qkv fp16 [B, (Hq + 2 Hkv) * 128] of the new token -> RoPE, k into the K window, v into the ring (its evicted row
        quantized in the same launch); returns q [B, Hq, 1, 128].  rope = (inv_freq device tensor [64], attn_factor): a scaled
        model's frequencies instead of theta."""
        L.require_gpu(qkv)
        row = self._evict_row()
        q = torch.empty((self.B, n_q_heads, 1, self.D), dtype=torch.float16, device=qkv.device)
        tail = (L.ptr(q), L.ptr(self.kwin), self.n_kwin, L.ptr(self.vring), self.n_tok, self.R, row, L.ptr(self.vcode),
                L.ptr(self.vscale), L.ptr(self.vmn), self.Tmax, self.group, self.bits, L.stream_ptr(qkv))
        if rope is None:
            rc = L.load().gear_kivi_rope_append(L.ptr(qkv), self.B, n_q_heads, self.H, self.D, pos, theta, *tail)
            L.check(rc, "gear_kivi_rope_append")
        else:
            inv_freq, attn_factor = _rope_table(rope, qkv)
            rc = L.load().gear_kivi_rope_append_freq(L.ptr(qkv), self.B, n_q_heads, self.H, self.D, pos, L.ptr(inv_freq), attn_factor,
                                                     *tail)
            L.check(rc, "gear_kivi_rope_append_freq")
        self._appended(row)
        return q

    def append(self, k_new: torch.Tensor, v_new: torch.Tensor):
        """k_new, v_new fp16 [B, Hkv, 1, 128] (already rotated): gear_kivi_append, the same launch without the rotation."""
        want = (self.B, self.H, 1, self.D)
        if tuple(k_new.shape) != want or tuple(v_new.shape) != want or k_new.dtype != torch.float16 or v_new.dtype != torch.float16:
            raise ValueError(f"KiviKVCache.append: K / V must be fp16 {list(want)}, got {list(k_new.shape)} / {list(v_new.shape)}")
        k_new, v_new = k_new.contiguous(), v_new.contiguous()
        L.require_gpu(k_new, v_new)
        row = self._evict_row()
        rc = L.load().gear_kivi_append(L.ptr(k_new), L.ptr(v_new), self.B, self.H, self.D, L.ptr(self.kwin), self.n_kwin,
                                       L.ptr(self.vring), self.n_tok, self.R, row, L.ptr(self.vcode), L.ptr(self.vscale),
                                       L.ptr(self.vmn), self.Tmax, self.group, self.bits, L.stream_ptr(k_new))
        L.check(rc, "gear_kivi_append")
        self._appended(row)

    def attend(self, q: torch.Tensor, return_lse: bool = False):
        """q fp16 [B, Hq, 1, 128] -> one fp32 softmax over all seq_len tokens (gear_attn_decode_kivi: packed K + K window, packed V
        + ring), fp16 [B, Hq, 1, 128]; with return_lse also the fp32 [B, Hq] log-sum-exp of the scaled scores.  Two launches;
        changes no state."""
        B, Hq = q.shape[0], q.shape[1]
        if tuple(q.shape) != (self.B, Hq, 1, self.D) or q.dtype != torch.float16:
            raise ValueError(f"KiviKVCache.attend: q must be fp16 [{self.B}, Hq, 1, {self.D}], got {list(q.shape)} {q.dtype}")
        q = q.contiguous()
        L.require_gpu(q)
        lib = L.load()
        out = torch.empty((B, Hq, 1, self.D), dtype=torch.float16, device=q.device)
        lse = torch.empty((B, Hq), dtype=torch.float32, device=q.device) if return_lse else None
        wsb = lib.gear_attn_decode_kivi_workspace(B, Hq, self.Tmax, self.bits)
        if self._ws is None or self._ws.numel() < wsb:
            self._ws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)
        rc = lib.gear_attn_decode_kivi(C_.byref(self._view), L.ptr(q), Hq, self.n_tok, self.n_kpacked, self.n_vpacked,
                                       1.0 / math.sqrt(self.D), L.ptr(out), L.ptr(lse), L.ptr(self._ws), self._ws.numel(),
                                       L.stream_ptr(q))
        L.check(rc, "gear_attn_decode_kivi")
        return (out, lse) if return_lse else out

    def maybe_compress(self):
        """Quantize the K window as one block when it holds `residual` tokens (modeling_llama_kivi.py:95-103)."""
        if self.n_kwin == self.R:
            self._quantize_k(self.kwin, self.n_kpacked)
            self.n_kpacked += self.R
