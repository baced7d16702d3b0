// snapshot.hip -- gear_cache_snapshot / gear_cache_restore: the live per-sequence state of a streaming cache as ONE packed,
// contiguous blob, and back (prompt store: switching the stored prompt is a copy of the live compressed bytes, not a prefill).
//
// The blob is the packed side of the field plan of cache_fields.h for sequences seq0 .. seq0 + n_seq - 1: fields in the planner's
// order, within a field (outer index, sequence, row), each row its live bytes rounded up to 16; no header (the caller keeps T, W,
// seg0, kk0).  ONE grid walks (field, outer index, sequence, piece of 16 KiB) and copies field -> blob (snapshot) or blob -> field
// (restore); nothing aliases and no index is read from device memory, so each call is one launch.  A restore from a blob of one
// sequence into n_seq > 1 destinations puts the destinations on grid.y: every block reads the one slab and writes its own sequence.
#include "cache_fields.h"

namespace {

// restore == 0: field rows of sequence seq0 + b (+ blockIdx.y) -> blob slab b; restore == 1: blob slab b -> those field rows
__global__ __launch_bounds__(RO_THREADS) void snap_kernel(const RoPlan p, char* __restrict__ blob, const int seq0, const int restore) {
    const long long blk = blockIdx.x;
    int fi = 0;
    while (fi + 1 < p.n_fields && blk >= p.f[fi + 1].blk0) ++fi;
    const RoField& f = p.f[fi];
    long long r = blk - f.blk0;
    const int piece = (int)(r % f.pieces);
    r /= f.pieces;
    const int b = (int)(r % p.batch);
    r /= p.batch;                                               // outer index = o1 * n_o2 + o2
    const long long o1 = r / f.n_o2, o2 = r % f.n_o2;
    char* fld = f.base + o1 * f.s_o1 + o2 * f.s_o2 + (long long)(seq0 + b + (int)blockIdx.y) * f.s_b;
    char* slab = blob + f.ws_off + (r * p.batch + b) * f.ws_slab;
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
            dst[j] = restore ? a : w;
            v[j] = make_uint4(0, 0, 0, 0);
            if (u < units) v[j] = *(const uint4*)(restore ? w : a);
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
        char* w = slab + ((long long)u << 4);                    // (the blob side is 16-byte aligned whatever the field is)
        const int n = (int)min((long long)16, (long long)f.lb - ((long long)c << 4));                 // the last unit of a row may be short
        const int wd = n == 16 ? f.wa : f.wt;
        if (n == 16 && wd == 16) {
            if (restore) *(uint4*)a = *(const uint4*)w; else *(uint4*)w = *(const uint4*)a;
        } else if (restore) {
            ro_copy_narrow(w, a, n, wd);                         // exactly the n live bytes: nothing past a row's live range is written
        } else {
            if (n < 16) *(uint4*)w = make_uint4(0, 0, 0, 0);     // the padding of a ragged row end is defined (zero) in the blob
            ro_copy_narrow(a, w, n, wd);
        }
    }
}

// The checks both calls share, in the order of the header; on success the plan of `plan_seqs` packed sequences (fan: grid.y).
int snap_check(const char* fn, const gear_cache_view* v, int n_layers, int batch, int T, int W, int seq0, int n_seq, const void* blob,
               size_t blob_bytes, int plan_seqs, int fan, RoPlan& p) {
    GEAR_CHECK_ARG(v, "%s: null cache view", fn);
    GEAR_CHECK_ARG(blob, "%s: null blob pointer", fn);
    GEAR_CHECK_ARG(n_layers >= 1 && batch >= 1, "%s: n_layers = %d, batch = %d: both at least 1", fn, n_layers, batch);
    GEAR_CHECK_ARG((long long)n_layers * batch == v->B, "%s: the view has B = %d, n_layers * batch = %d * %d", fn, v->B, n_layers,
                   batch);
    GEAR_CHECK_ARG(T >= 0 && T % 64 == 0 && T <= v->tcap, "%s: T = %d compressed tokens, must be a multiple of 64 in [0, tcap = %d]",
                   fn, T, v->tcap);
    GEAR_CHECK_ARG(W >= 0 && W <= v->wcap, "%s: W = %d window tokens, the window holds wcap = %d", fn, W, v->wcap);
    GEAR_CHECK_ARG(ro_shape_ok(v, n_layers, batch, T, W), "%s: view with Hkv %d, D %d, bits %d, group %d", fn, v->Hkv, v->D, v->bits,
                   v->group);
    GEAR_CHECK_ARG(W == 0 || (v->kwin && v->vwin), "%s: W > 0 needs the window tensors", fn);
    GEAR_CHECK_ARG(seq0 >= 0 && n_seq >= 1 && (long long)seq0 + n_seq <= batch, "%s: sequences seq0 = %d, n_seq = %d lie outside "
                   "[0, batch = %d)", fn, seq0, n_seq, batch);
    GEAR_CHECK_ARG(((uintptr_t)blob & 15) == 0, "%s: the blob pointer must be 16-byte aligned", fn);
    ro_plan(v, n_layers, batch, plan_seqs, T, W, p);
    GEAR_CHECK_ARG(!p.too_big, "%s: a field's per-sequence share exceeds 2^31 bytes / units", fn);
    GEAR_CHECK_ARG(blob_bytes >= p.ws_bytes, "%s: blob of %zu bytes, needs %zu (gear_cache_snapshot_bytes)", fn, blob_bytes,
                   p.ws_bytes);
    GEAR_CHECK_ARG(p.n_blocks < (1LL << 31) && fan <= 65535, "%s: %lld blocks x %d destinations exceed the grid", fn, p.n_blocks,
                   fan);
    return 0;
}

}  // namespace

extern "C" size_t gear_cache_snapshot_bytes(const gear_cache_view* v, int n_layers, int batch, int T, int W, int n_seq) {
    if (!ro_shape_ok(v, n_layers, batch, T, W) || n_seq < 1 || n_seq > batch) return 0;
    RoPlan p;
    ro_plan(v, n_layers, batch, n_seq, T, W, p);
    return p.too_big ? 0 : p.ws_bytes;
}

extern "C" int gear_cache_snapshot(const gear_cache_view* v, int n_layers, int batch, int T, int W, int seq0, int n_seq, void* blob,
                                   size_t blob_bytes, void* stream) {
    RoPlan p;
    if (int rc = snap_check("gear_cache_snapshot", v, n_layers, batch, T, W, seq0, n_seq, blob, blob_bytes, n_seq, 1, p)) return rc;
    if (p.n_blocks == 0) return 0;
    snap_kernel<<<dim3((unsigned)p.n_blocks), dim3(RO_THREADS), 0, (hipStream_t)stream>>>(p, (char*)blob, seq0, 0);
    GEAR_CHECK_LAUNCH("gear_cache_snapshot");
    return 0;
}

extern "C" int gear_cache_restore(const gear_cache_view* v, int n_layers, int batch, int T, int W, int seq0, int n_seq,
                                  const void* blob, size_t blob_bytes, int blob_seqs, void* stream) {
    GEAR_CHECK_ARG(blob_seqs == n_seq || blob_seqs == 1, "gear_cache_restore: blob_seqs = %d: the blob holds either the n_seq = %d "
                   "destination sequences or one sequence for all of them", blob_seqs, n_seq);
    RoPlan p;
    const int fan = blob_seqs == n_seq ? 1 : n_seq;                          // broadcast: the destinations ride on grid.y
    if (int rc = snap_check("gear_cache_restore", v, n_layers, batch, T, W, seq0, n_seq, blob, blob_bytes, blob_seqs, fan, p)) return rc;
    if (p.n_blocks == 0) return 0;
    snap_kernel<<<dim3((unsigned)p.n_blocks, (unsigned)fan), dim3(RO_THREADS), 0, (hipStream_t)stream>>>(p, (char*)blob, seq0, 1);
    GEAR_CHECK_LAUNCH("gear_cache_restore");
    return 0;
}
