// reorder.hip -- gear_cache_reorder: gather the live per-sequence state of a streaming cache along its batch axis, in place
// (beam search: after every token hypothesis b continues from the history of hypothesis src_idx[b]).
//
// The state of a sequence is spread over up to 22 tensors of the cache view with different batch-axis positions, row pitches and
// live ranges.  The host side of the call describes each field to the kernel with one descriptor -- base, two outer levels (layer;
// factor segment for kP / vP, whose batch axis lies behind the segment axis), batch stride, rows, row pitch, live bytes per row --
// and ONE grid walks (field, outer index, destination sequence, piece of 16 KiB).  A destination may be another row's source, so
// the call runs the grid twice: sources of all moved rows -> workspace, then workspace -> destinations.  Rows with
// src_idx[b] == b (or an index outside [0, batch)) are not touched in either phase.  src_idx is read on the device.
#include "cache_fields.h"

namespace {

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

}  // namespace

extern "C" size_t gear_cache_reorder_workspace(const gear_cache_view* v, int n_layers, int batch, int T, int W) {
    if (!ro_shape_ok(v, n_layers, batch, T, W)) return 0;
    RoPlan p;
    ro_plan(v, n_layers, batch, batch, T, W, p);
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
    ro_plan(v, n_layers, batch, batch, T, W, p);
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
