// reorder.hip -- gear_cache_reorder: gather the live per-sequence state of a streaming cache along its batch axis, in place
// (beam search: after every token hypothesis b continues from the history of hypothesis src_idx[b]).
//
// The state of a sequence is spread over up to 22 tensors of the cache view with different batch-axis positions, row pitches and
// live ranges.  The host side of the call describes each field to the kernel with one descriptor -- base, two outer levels (layer;
// factor segment for kP / vP, whose batch axis lies behind the segment axis), batch stride, rows, row pitch, live bytes per row --
// and ONE grid walks (field, outer index, destination sequence, piece of 16 KiB).  A destination may be another row's source, so
// the call runs the grid twice: sources of all moved rows -> workspace, then workspace -> destinations.  Rows with
// src_idx[b] == b (or an index outside [0, batch)) are not touched in either phase.  src_idx is read on the device.
#include "common.h"

namespace {

constexpr int RO_MAX_FIELDS = 24;
constexpr int RO_THREADS = 256;
constexpr int RO_UNROLL = 4;                                  // 16-byte units per thread and block: 4 loads in flight, 16 KiB per block
constexpr int RO_UNITS = RO_THREADS * RO_UNROLL;

struct RoField {
    char* base;
    long long s_o1, s_o2, s_b, pitch;      // byte strides: outer level 1 (layer), outer level 2 (segment), batch, row
    long long ws_off, ws_slab;             // workspace: offset of the field, bytes per (outer, sequence) slab = rows * lbp
    long long units;                       // 16-byte units per slab = rows * (lbp / 16)
    long long blk0;                        // first block of the field in the grid
    int n_o2, rows, lb, lbp;               // segments per layer; rows per slab; live bytes per row; lb rounded up to 16
    int pieces;                            // blocks per slab
    int wa, wt;                            // access width of whole units (a power of two <= 16 that divides base and every stride), of a row's tail
};

struct RoPlan {
    RoField f[RO_MAX_FIELDS];
    int n_fields, batch, too_big;
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

// phase 0: field rows of sequence src_idx[b] -> workspace slab b; phase 1: workspace slab b -> field rows of sequence b
__global__ __launch_bounds__(RO_THREADS) void ro_kernel(const RoPlan p, const int32_t* __restrict__ src_idx, char* __restrict__ ws,
                                                        const int phase) {
    const long long blk = blockIdx.x;
    int fi = 0;
    while (fi + 1 < p.n_fields && blk >= p.f[fi + 1].blk0) ++fi;
    const RoField& f = p.f[fi];
    long long r = blk - f.blk0;
    const int piece = (int)(r % f.pieces);
    r /= f.pieces;
    const int b = (int)(r % p.batch);
    r /= p.batch;                                               // outer index = o1 * n_o2 + o2
    const int src = src_idx[b];
    if (src == b || src < 0 || src >= p.batch) return;
    const long long o1 = r / f.n_o2, o2 = r % f.n_o2;
    char* fld = f.base + o1 * f.s_o1 + o2 * f.s_o2 + (long long)(phase == 0 ? src : b) * f.s_b;
    char* slab = ws + f.ws_off + (r * p.batch + b) * f.ws_slab;
    const uint32_t cpr = (uint32_t)f.lbp >> 4, units = (uint32_t)f.units;
    const bool one_row = f.rows == 1;
    const uint32_t u0 = (uint32_t)piece * RO_UNITS + threadIdx.x;

    if (f.wa == 16 && f.lb == f.lbp) {                          // every unit a whole 16-byte vector on both sides
        uint4 v[RO_UNROLL];
        char* dst[RO_UNROLL];
#pragma unroll
        for (int j = 0; j < RO_UNROLL; ++j) {                   // all loads of the block first: 4 x 16 bytes in flight per lane
            const uint32_t u = u0 + j * RO_THREADS;
            const uint32_t row = one_row ? 0u : u / cpr;
            const uint32_t c = u - row * cpr;
            char* a = fld + (long long)row * f.pitch + ((long long)c << 4);
            char* w = slab + ((long long)u << 4);
            dst[j] = phase == 0 ? w : a;
            v[j] = make_uint4(0, 0, 0, 0);
            if (u < units) v[j] = *(const uint4*)(phase == 0 ? a : w);
        }
#pragma unroll
        for (int j = 0; j < RO_UNROLL; ++j)
            if (u0 + j * RO_THREADS < units) *(uint4*)dst[j] = v[j];
        return;
    }
    for (int j = 0; j < RO_UNROLL; ++j) {
        const uint32_t u = u0 + j * RO_THREADS;
        if (u >= units) break;
        const uint32_t row = one_row ? 0u : u / cpr;
        const uint32_t c = u - row * cpr;
        char* a = fld + (long long)row * f.pitch + ((long long)c << 4);
        char* w = slab + ((long long)u << 4);
        const int n = (int)min((long long)16, (long long)f.lb - ((long long)c << 4));                 // the last unit of a row may be short
        const int wd = n == 16 ? f.wa : f.wt;
        if (n == 16 && wd == 16) {
            if (phase == 0) *(uint4*)w = *(const uint4*)a; else *(uint4*)a = *(const uint4*)w;
        } else if (phase == 0) {
            ro_copy_narrow(a, w, n, wd);
        } else {
            ro_copy_narrow(w, a, n, wd);
        }
    }
}

inline int ro_pow2_div(unsigned long long x, int cap) {          // the largest power of two <= cap that divides x (x == 0: cap)
    int w = cap;
    while (w > 1 && (x & (unsigned long long)(w - 1))) w >>= 1;
    return w;
}

// One field: n_o1 x n_o2 outer slabs of `batch` sequences; per sequence `rows` rows of `lb` live bytes at pitch `pitch`.
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

// The fields of view v (B = n_layers * batch) with their live ranges at T compressed and W window tokens.
void ro_plan(const gear_cache_view* v, int n_layers, int batch, int T, int W, RoPlan& p) {
    p.n_fields = 0; p.batch = batch; p.too_big = 0; p.n_blocks = 0; p.ws_bytes = 0;
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

extern "C" size_t gear_cache_reorder_workspace(const gear_cache_view* v, int n_layers, int batch, int T, int W) {
    if (!ro_shape_ok(v, n_layers, batch, T, W)) return 0;
    RoPlan p;
    ro_plan(v, n_layers, batch, T, W, p);
    return p.ws_bytes;
}

extern "C" int gear_cache_reorder(const gear_cache_view* v, int n_layers, int batch, int T, int W, const int32_t* src_idx,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    GEAR_CHECK_ARG(v, "gear_cache_reorder: null cache view");
    GEAR_CHECK_ARG(src_idx, "gear_cache_reorder: null index pointer (src_idx: device int32 [batch])");
    GEAR_CHECK_ARG(n_layers >= 1 && batch >= 1, "gear_cache_reorder: n_layers = %d, batch = %d: both at least 1", n_layers, batch);
    GEAR_CHECK_ARG((long long)n_layers * batch == v->B, "gear_cache_reorder: the view has B = %d, n_layers * batch = %d * %d", v->B,
                   n_layers, batch);
    GEAR_CHECK_ARG(T >= 0 && T % 64 == 0 && T <= v->tcap, "gear_cache_reorder: T = %d compressed tokens, must be a multiple of 64 in "
                   "[0, tcap = %d]", T, v->tcap);
    GEAR_CHECK_ARG(W >= 0 && W <= v->wcap, "gear_cache_reorder: W = %d window tokens, the window holds wcap = %d", W, v->wcap);
    GEAR_CHECK_ARG(ro_shape_ok(v, n_layers, batch, T, W), "gear_cache_reorder: view with Hkv %d, D %d, bits %d, group %d", v->Hkv, v->D,
                   v->bits, v->group);
    GEAR_CHECK_ARG(W == 0 || (v->kwin && v->vwin), "gear_cache_reorder: W > 0 needs the window tensors");
    RoPlan p;
    ro_plan(v, n_layers, batch, T, W, p);
    GEAR_CHECK_ARG(p.ws_bytes == 0 || (workspace && workspace_bytes >= p.ws_bytes), "gear_cache_reorder: workspace of %zu bytes, needs "
                   "%zu (gear_cache_reorder_workspace)", workspace ? workspace_bytes : (size_t)0, p.ws_bytes);
    GEAR_CHECK_ARG(!p.too_big, "gear_cache_reorder: a field's per-sequence share exceeds 2^31 bytes / units");
    GEAR_CHECK_ARG(p.n_blocks < (1LL << 31), "gear_cache_reorder: %lld blocks exceed the grid", p.n_blocks);
    if (p.n_blocks == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    for (int phase = 0; phase < 2; ++phase) {
        ro_kernel<<<dim3((unsigned)p.n_blocks), dim3(RO_THREADS), 0, st>>>(p, src_idx, (char*)workspace, phase);
        GEAR_CHECK_LAUNCH("gear_cache_reorder");
    }
    return 0;
}
