// cache_fields.h -- the ONE description of the per-sequence state of a streaming cache: which tensors of a gear_cache_view hold it,
// where a sequence's share of each lies and how much of it is live at T compressed and W window tokens.  Shared by reorder.hip
// (gear_cache_reorder: gather along the batch axis) and snapshot.hip (gear_cache_snapshot / gear_cache_restore: a packed image).
//
// The state of a sequence is spread over up to 22 tensors of the cache view with different batch-axis positions, row pitches and
// live ranges.  The host side describes each field with one descriptor -- base, two outer levels (layer; factor segment for
// kP / vP, whose batch axis lies behind the segment axis), batch stride, rows, row pitch, live bytes per row -- and ONE grid walks
// (field, outer index, sequence, piece of 16 KiB).  The packed side of a field (reorder's workspace, a snapshot's blob) holds per
// (outer index, sequence) one slab of `rows` rows, each its live bytes rounded up to 16.
#pragma once
#include "common.h"

namespace {

constexpr int RO_MAX_FIELDS = 24;
constexpr int RO_THREADS = 256;
constexpr int RO_UNROLL = 4;                                  // 16-byte units per thread and block: 4 loads in flight, 16 KiB per block
constexpr int RO_UNITS = RO_THREADS * RO_UNROLL;

struct RoField {
    char* base;
    long long s_o1, s_o2, s_b, pitch;      // byte strides: outer level 1 (layer), outer level 2 (segment), batch, row
    long long ws_off, ws_slab;             // packed side: offset of the field, bytes per (outer, sequence) slab = rows * lbp
    long long units;                       // 16-byte units per slab = rows * (lbp / 16)
    long long blk0;                        // first block of the field in the grid
    int n_o2, rows, lb, lbp;               // segments per layer; rows per slab; live bytes per row; lb rounded up to 16
    int pieces;                            // blocks per slab
    int wa, wt;                            // access width of whole units (a power of two <= 16 that divides base and every stride), of a row's tail
};

struct RoPlan {
    RoField f[RO_MAX_FIELDS];
    int n_fields, batch, too_big;          // batch: the sequences that have a slab on the packed side
    long long n_blocks;
    size_t ws_bytes;
};

__device__ __forceinline__ void ro_copy_narrow(const char* __restrict__ s, char* __restrict__ d, int n, int w) {
    if (w >= 8) {
        for (int i = 0; i < n; i += 8) *(uint2*)(d + i) = *(const uint2*)(s + i);
    } else if (w == 4) {
        for (int i = 0; i < n; i += 4) *(uint32_t*)(d + i) = *(const uint32_t*)(s + i);
    } else if (w == 2) {
        for (int i = 0; i < n; i += 2) *(uint16_t*)(d + i) = *(const uint16_t*)(s + i);
    } else {
        for (int i = 0; i < n; ++i) d[i] = s[i];
    }
}

inline int ro_pow2_div(unsigned long long x, int cap) {          // the largest power of two <= cap that divides x (x == 0: cap)
    int w = cap;
    while (w > 1 && (x & (unsigned long long)(w - 1))) w >>= 1;
    return w;
}

// One field: n_o1 x n_o2 outer slabs of p.batch sequences; per sequence `rows` rows of `lb` live bytes at pitch `pitch`.
void ro_add(RoPlan& p, const void* base, int n_o1, long long s_o1, int n_o2, long long s_o2, long long s_b, long long rows,
            long long pitch, long long lb) {
    if (!base || lb <= 0 || rows <= 0 || n_o2 <= 0 || p.n_fields >= RO_MAX_FIELDS) return;
    // rows that are live to the end, or whose pitch is within one 128-byte line anyway: one contiguous run per sequence
    if (lb == pitch || pitch <= 128) {
        lb = rows * pitch;
        pitch = lb;
        rows = 1;
    }
    if (rows * ((lb + 15) / 16) >= (1LL << 31) || lb >= (1LL << 31) - 16) {      // (a sequence's share of a field beyond 32 GiB)
        p.too_big = 1;
        return;
    }
    RoField& f = p.f[p.n_fields++];
    f.base = (char*)base;
    f.s_o1 = s_o1; f.s_o2 = s_o2; f.s_b = s_b; f.pitch = pitch;
    f.n_o2 = n_o2; f.rows = (int)rows; f.lb = (int)lb; f.lbp = (int)((lb + 15) / 16 * 16);
    f.ws_slab = rows * f.lbp;
    f.units = rows * (f.lbp / 16);
    f.pieces = (int)((f.units + RO_UNITS - 1) / RO_UNITS);
    unsigned long long al = (unsigned long long)(uintptr_t)base | (unsigned long long)s_b;
    if (rows > 1) al |= (unsigned long long)pitch;
    if (n_o1 > 1) al |= (unsigned long long)s_o1;
    if (n_o2 > 1) al |= (unsigned long long)s_o2;
    f.wa = ro_pow2_div(al, 16);
    f.wt = ro_pow2_div((unsigned long long)lb, f.wa);
    f.ws_off = (long long)p.ws_bytes;
    f.blk0 = p.n_blocks;
    const long long slabs = (long long)n_o1 * n_o2 * p.batch;
    p.ws_bytes += (size_t)slabs * (size_t)f.ws_slab;
    p.n_blocks += slabs * f.pieces;
}

// The fields of view v (B = n_layers * batch) with their live ranges at T compressed and W window tokens; n_seq of the batch's
// sequences get a slab on the packed side (reorder: all of them).
void ro_plan(const gear_cache_view* v, int n_layers, int batch, int n_seq, int T, int W, RoPlan& p) {
    p.n_fields = 0; p.batch = n_seq; p.too_big = 0; p.n_blocks = 0; p.ws_bytes = 0;
    const long long H = v->Hkv, D = v->D, tcap = v->tcap;
    const long long fpi = 32 / v->bits, esz = v->mode == GEAR_MODE_FP32 ? 4 : 2;
    const int L = n_layers;
    // every field but kP / vP is [L, B, ...]: layer stride = batch * per-sequence bytes
    auto plain = [&](const void* base, long long per_seq, long long rows, long long pitch, long long lb) {
        ro_add(p, base, L, per_seq * batch, 1, 0, per_seq, rows, pitch, lb);
    };
    if (T > 0) {
        plain(v->kcode, H * D * v->ldk * 4, H * D, (long long)v->ldk * 4, T / fpi * 4);
        plain(v->kscale, H * D * v->lsk * esz, H * D, v->lsk * esz, T / v->group * esz);
        plain(v->kmn, H * D * v->lsk * esz, H * D, v->lsk * esz, T / v->group * esz);
        const long long cw = D / fpi * 4, sw = D / v->group * esz;
        plain(v->vcode, H * tcap * cw, H, tcap * cw, T * cw);
        plain(v->vscale, H * tcap * sw, H, tcap * sw, T * sw);
        plain(v->vmn, H * tcap * sw, H, tcap * sw, T * sw);
        const int nblocks = v->seglen > 0 && T >= v->seg0 ? (T - v->seg0) / v->seglen : 0;
        if (v->rk > 0 || v->rv > 0) {
            // channel-side factors [L, nseg, B, H, D, r]: the segments written so far (0 = the prompt, then one per block)
            const int nseg = v->seglen > 0 ? 1 + v->tcap / v->seglen : 1;
            const int live = min(nseg, 1 + nblocks);
            if (v->rk > 0) {
                const long long hb = H * D * v->rk * 2;
                ro_add(p, v->kP, L, hb * batch * nseg, live, hb * batch, hb, 1, hb, hb);
                plain(v->kQ, H * tcap * v->rk * 2, H, tcap * v->rk * 2, (long long)T * v->rk * 2);
            }
            if (v->rv > 0) {
                const long long hb = H * D * v->rv * 2;
                ro_add(p, v->vP, L, hb * batch * nseg, live, hb * batch, hb, 1, hb, hb);
                plain(v->vQ, H * tcap * v->rv * 2, H, tcap * v->rv * 2, (long long)T * v->rv * 2);
            }
        }
        if (v->kk_cap > 0) {
            const long long kl = min((long long)v->kk_cap, (long long)v->kk0 + (long long)nblocks * v->kkb);
            plain(v->koidx, H * D * 2 * v->kk_cap * 2, H * D * 2, (long long)v->kk_cap * 2, kl * 2);
            plain(v->koval, H * D * 2 * v->kk_cap * 2, H * D * 2, (long long)v->kk_cap * 2, kl * 2);
            const long long kc = H * D * 2 * v->nbk_pitch;
            plain(v->kochunk, kc, 1, kc, kc);
        }
        if (v->kv > 0) {
            const long long rw = 2LL * v->kv * 2;
            plain(v->voidx, tcap * rw, 1, tcap * rw, T * rw);
            plain(v->voval, tcap * rw, 1, tcap * rw, T * rw);
            const long long cb = 2 * (H + 1);
            plain(v->vochunk, tcap * cb, 1, tcap * cb, T * cb);
        }
        if (v->ktile && v->kcnt && v->nck > 0) {                // tiles of the 128-token chunks that hold tokens
            const long long tw = (long long)v->ktile_cap * 4, nc = min((long long)v->nck, ((long long)T + 127) / 128);
            plain(v->ktile, H * v->nck * tw, H, v->nck * tw, nc * tw);
            plain(v->kcnt, H * v->nck * 4, 1, H * v->nck * 4, H * v->nck * 4);
        }
        if (v->vtile && v->vcnt && v->nblk > 0) {               // tiles of the 64-token blocks
            const long long tw = (long long)v->vtile_cap * 4, nb = min((long long)v->nblk, (long long)T / 64);
            plain(v->vtile, H * v->nblk * tw, H, v->nblk * tw, nb * tw);
            plain(v->vcnt, H * v->nblk * 4, 1, H * v->nblk * 4, H * v->nblk * 4);
        }
    }
    if (W > 0) {
        const long long wr = D * 2;
        plain(v->kwin, H * v->wcap * wr, H, v->wcap * wr, W * wr);
        plain(v->vwin, H * v->wcap * wr, H, v->wcap * wr, W * wr);
    }
}

bool ro_shape_ok(const gear_cache_view* v, int n_layers, int batch, int T, int W) {
    return v && n_layers >= 1 && batch >= 1 && (long long)n_layers * batch == v->B && T >= 0 && T % 64 == 0 && T <= v->tcap && W >= 0 &&
           W <= v->wcap && v->Hkv > 0 && v->D > 0 && (v->bits == 2 || v->bits == 4 || v->bits == 8) && v->group > 0;
}

}  // namespace
