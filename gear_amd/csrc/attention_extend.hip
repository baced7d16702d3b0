// attention_extend.hip -- chunk attention: n new query tokens at once over the compressed GEAR cache (gfx950, head_dim 128).
//
// Query i of the chunk (position pos + i) attends, with one fp32 softmax, over the T compressed tokens (reconstructed as
// gear_attn_decode_cache reconstructs them: dequant, stored outlier values in place of the dequantized ones, + Q P^T of the token's
// factor segment), the W fp16 window tokens and the chunk's own fp16 K / V rows 0 .. i (causal).  It replaces n single-token
// decode steps, each of which reads and dequantizes the whole compressed prefix again.
//
// Rows of the contraction: M = n * G rows (query token i, grouped query head gh), row m = i * G + gh, in tiles of 64.
// Keys: 64-token pieces -- the T / 64 compressed ones first, then the fp16 part (window rows, then chunk rows) in pieces of 64.
// Grid (split x M-tile, B * Hkv): a workgroup owns a run of pieces for one M-tile of one KV head, so the compressed bytes of a
// piece are read and dequantized ONCE per 64 query rows (per 64 / G query tokens) instead of once per query token.  Per piece:
//   1. the piece becomes two fp16 LDS tiles, K [token][channel] and V^T [channel][token]: dequant + low-rank term of the piece's
//      factor segment in fp32, then the outliers (from the sorted lists: the block entries sit at fixed list positions, the prompt
//      segment's are found by binary search) overwrite their elements with value + low-rank term;
//   2. S = Q K^T on v_mfma_f32_32x32x16_f16 (4 waves, one 32 x 32 block each), causal mask, scale;
//   3. online softmax per row (fp32 running max / sum), P in fp16;
//   4. O = alpha O + P V on v_mfma_f32_32x32x16_f16 (each wave two 32 x 32 blocks of the 64 x 128 output, in registers).
// A second launch merges the splits' partial (o, m, l) per output row and normalises.
#include <math.h>

#include "common.h"

namespace {

constexpr int XD = 128;           // head_dim
constexpr int X_NMAX = 2048;      // query tokens per call
constexpr int XQP = 136;          // row pitch (halfs) of the Q and K tiles: 272 B rows, 16-byte aligned
constexpr int XVP = 72;           // row pitch (halfs) of the V^T and P tiles: 144 B rows
constexpr int XSP = 65;           // row pitch (floats) of the score tile
constexpr int XFP = 17;           // row pitch (floats) of the staged low-rank factors (r <= 16)
constexpr int X_TARGET_WG = 1024; // workgroups the split plan aims at (256 CUs, two resident workgroups each, two waves of them)

typedef _Float16 xh8 __attribute__((ext_vector_type(8)));
typedef float xf16 __attribute__((ext_vector_type(16)));

struct ExtArgs {
    gear_cache_view c;
    const uint16_t* q;        // [B, Hq, n, 128]
    const uint16_t* knew;     // [B, Hkv, n, 128]
    const uint16_t* vnew;
    int Hq, G, n, T, W;
    float qscale;
    int nmt, nsplit, pps, npc, np;
    int64_t kP_seg, vP_seg;   // elements between two factor segments
    float* part_o;            // [slots, 64, 128]
    float* part_ml;           // [slots, 64, 2]
    uint16_t* out;            // [B, Hq, n, 128]
    float* lse;               // [B, Hq, n] or null
};

struct ExtPlan {
    int nmt, nsplit, pps, npc, np;
};

void ext_plan(int64_t BH, int G, int n, int T, int W, ExtPlan& p) {
    p.nmt = (n * G + 63) / 64;
    p.npc = T / 64;
    p.np = p.npc + (W + n + 63) / 64;
    const int64_t nwork = BH * p.nmt;
    const int64_t want = std::min<int64_t>(p.np, std::max<int64_t>(1, (X_TARGET_WG + nwork - 1) / nwork));
    p.pps = (int)((p.np + want - 1) / want);
    p.nsplit = (p.np + p.pps - 1) / p.pps;
}

// upper bound of the partial-result slots for any Hkv dividing Hq: slots = nwork * nsplit < X_TARGET_WG + nwork and <= nwork * np,
// nwork = B Hkv ceil(n G / 64) <= B Hq n / 64 + B Hq
int64_t ext_slots_bound(int B, int Hq, int n, int T, int W) {
    const int64_t nw = ((int64_t)B * Hq * n + 63) / 64 + (int64_t)B * Hq;
    const int64_t np = T / 64 + (W + n + 63) / 64;
    return std::min<int64_t>(X_TARGET_WG + nw, nw * np);
}

__device__ __forceinline__ int x_lower_bound(const uint16_t* a, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int)a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the low-rank term of element (token row of qs, channel row of ps) from the staged factors
__device__ __forceinline__ float x_lr(const float* qrow, const float* prow, int r) {
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < 16; c++)
        if (c < r) s = fmaf(qrow[c], prow[c], s);
    return s;
}

// compressed piece [t0, t0 + 64) -> kt [token][channel], vt [channel][token] (fp16), outliers applied
template <int BITS>
__device__ __forceinline__ void x_fill_comp(const ExtArgs& a, int64_t bh, int b, int hkv, int t0, uint16_t* kt, uint16_t* vt,
                                            float* stage, float* stage2) {
    constexpr int CPW = 32 / BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    constexpr int WPP = 64 / CPW;     // K words per channel and piece
    constexpr int NWV = XD / CPW;     // V words per token row
    const gear_cache_view& c = a.c;
    const int tid = threadIdx.x;
    const int rk = c.kP ? c.rk : 0, rv = c.vP ? c.rv : 0;
    const int seg = (c.seglen == 0 || t0 < c.seg0) ? 0 : 1 + (t0 - c.seg0) / c.seglen;   // a 64-token piece never straddles one
    float* kPs = stage;               // [128][XFP]
    float* vPs = stage + XD * XFP;    // [128][XFP]
    float* kQs = stage2;              // [64][XFP]
    float* vQs = stage2 + 64 * XFP;   // [64][XFP]
    const uint16_t* kP = (const uint16_t*)c.kP;
    const uint16_t* vP = (const uint16_t*)c.vP;
    const uint16_t* kQ = (const uint16_t*)c.kQ;
    const uint16_t* vQ = (const uint16_t*)c.vQ;
    for (int i = tid; i < XD * rk; i += 256)
        kPs[(i / rk) * XFP + i % rk] = h2f_bits(kP[seg * a.kP_seg + bh * XD * rk + i]);
    for (int i = tid; i < XD * rv; i += 256)
        vPs[(i / rv) * XFP + i % rv] = h2f_bits(vP[seg * a.vP_seg + bh * XD * rv + i]);
    for (int i = tid; i < 64 * rk; i += 256)
        kQs[(i / rk) * XFP + i % rk] = h2f_bits(kQ[(bh * c.tcap + t0) * rk + i]);
    for (int i = tid; i < 64 * rv; i += 256)
        vQs[(i / rv) * XFP + i % rv] = h2f_bits(vQ[(bh * c.tcap + t0) * rv + i]);
    __syncthreads();
    const uint32_t* kcode = (const uint32_t*)c.kcode;
    const uint16_t* kscale = (const uint16_t*)c.kscale;
    const uint16_t* kmn = (const uint16_t*)c.kmn;
    for (int it = tid; it < XD * WPP; it += 256) {
        const int w = it % WPP, d = it / WPP;
        const int64_t rowk = bh * XD + d;
        const uint32_t word = kcode[rowk * c.ldk + t0 / CPW + w];
        const int g = (t0 + w * CPW) / c.group;
        const float sc = h2f_bits(kscale[rowk * c.lsk + g]), mn = h2f_bits(kmn[rowk * c.lsk + g]);
        float pk[16];
#pragma unroll
        for (int q = 0; q < 16; q++) pk[q] = q < rk ? kPs[d * XFP + q] : 0.0f;
#pragma unroll
        for (int j = 0; j < CPW; j++) {
            const int t = w * CPW + j;
            const float v = fmaf(sc, (float)((word >> (BITS * j)) & MASK), mn) + x_lr(kQs + t * XFP, pk, rk);
            kt[t * XQP + d] = f2h_bits(v);
        }
    }
    const uint32_t* vcode = (const uint32_t*)c.vcode;
    const uint16_t* vscale = (const uint16_t*)c.vscale;
    const uint16_t* vmn = (const uint16_t*)c.vmn;
    const int ngv = XD / c.group;
    for (int it = tid; it < 64 * NWV; it += 256) {
        const int w = it % NWV, t = it / NWV;
        const int64_t row = bh * c.tcap + t0 + t;
        const uint32_t word = vcode[row * NWV + w];
        const int d0 = w * CPW, gv = d0 / c.group;
        const float sc = h2f_bits(vscale[row * ngv + gv]), mn = h2f_bits(vmn[row * ngv + gv]);
        float qv[16];
#pragma unroll
        for (int q = 0; q < 16; q++) qv[q] = q < rv ? vQs[t * XFP + q] : 0.0f;
#pragma unroll
        for (int j = 0; j < CPW; j++) {
            const int d = d0 + j;
            const float v = fmaf(sc, (float)((word >> (BITS * j)) & MASK), mn) + x_lr(qv, vPs + d * XFP, rv);
            vt[d * XVP + t] = f2h_bits(v);
        }
    }
    const bool kout = c.koidx && c.koval && (c.kk0 > 0 || c.kkb > 0);
    const bool vout = c.voidx && c.voval && c.kv > 0;
    if (!kout && !vout) return;
    __syncthreads();
    // outliers: the stored value replaces the dequantized one, the low-rank term is added on top
    if (kout) {        // one (channel, side) list per thread
        const int d = tid >> 1, side = tid & 1;
        const int64_t lo = ((bh * XD + d) * 2 + side) * (int64_t)c.kk_cap;
        const uint16_t* oi = (const uint16_t*)c.koidx + lo;
        const uint16_t* ov = (const uint16_t*)c.koval + lo;
        auto put = [&](int t, uint16_t val) {
            const int tl = t - t0;
            float pk[16];
#pragma unroll
            for (int q = 0; q < 16; q++) pk[q] = q < rk ? kPs[d * XFP + q] : 0.0f;
            kt[tl * XQP + d] = f2h_bits(h2f_bits(val) + x_lr(kQs + tl * XFP, pk, rk));
        };
        if (t0 < c.seg0 && c.kk0 > 0) {
            for (int i = x_lower_bound(oi, c.kk0, t0); i < c.kk0; i++) {
                const int t = oi[i];
                if (t >= t0 + 64) break;
                put(t, ov[i]);
            }
        } else if (t0 >= c.seg0 && c.kkb > 0 && c.seglen > 0) {      // block j of the cache wrote list positions kk0 + j kkb ..
            const int base = c.kk0 + (t0 - c.seg0) / c.seglen * c.kkb;
            const int end = min(base + c.kkb, c.kk_cap);
            for (int i = base; i < end; i++) {
                const int t = oi[i];
                if (t >= t0 && t < t0 + 64) put(t, ov[i]);
            }
        }
    }
    if (vout && tid < 128) {   // one (token row, side) list per thread; a row's list spans the heads, columns hkv * 128 + d
        const int t = tid >> 1, side = tid & 1;
        const int64_t lo = (((int64_t)b * c.tcap + t0 + t) * 2 + side) * c.kv;
        const uint16_t* oi = (const uint16_t*)c.voidx + lo;
        const uint16_t* ov = (const uint16_t*)c.voval + lo;
        const int c_lo = hkv * XD;
        for (int i = x_lower_bound(oi, c.kv, c_lo); i < c.kv; i++) {
            const int col = oi[i];
            if (col >= c_lo + XD) break;
            const int d = col - c_lo;
            vt[d * XVP + t] = f2h_bits(h2f_bits(ov[i]) + x_lr(vQs + t * XFP, vPs + d * XFP, rv));
        }
    }
}

// fp16 piece: positions T + j0 .. T + j0 + 63 = window rows, then chunk rows, then zeros (masked)
__device__ __forceinline__ void x_fill_f16(const ExtArgs& a, int64_t bh, int j0, uint16_t* kt, uint16_t* vt) {
    const int tid = threadIdx.x;
    for (int it = tid; it < 64 * 16; it += 256) {
        const int r = it >> 4, c8 = it & 15, idx = j0 + r;
        uint4 kv4 = make_uint4(0, 0, 0, 0), vv4 = make_uint4(0, 0, 0, 0);
        if (idx < a.W) {
            const int64_t o = (bh * a.c.wcap + idx) * XD + c8 * 8;
            kv4 = *(const uint4*)((const uint16_t*)a.c.kwin + o);
            vv4 = *(const uint4*)((const uint16_t*)a.c.vwin + o);
        } else if (idx - a.W < a.n) {
            const int64_t o = (bh * a.n + idx - a.W) * XD + c8 * 8;
            kv4 = *(const uint4*)(a.knew + o);
            vv4 = *(const uint4*)(a.vnew + o);
        }
        *(uint4*)(kt + r * XQP + c8 * 8) = kv4;
        const uint32_t e[4] = {vv4.x, vv4.y, vv4.z, vv4.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            vt[(c8 * 8 + 2 * j) * XVP + r] = (uint16_t)(e[j] & 0xFFFFu);
            vt[(c8 * 8 + 2 * j + 1) * XVP + r] = (uint16_t)(e[j] >> 16);
        }
    }
}

template <int BITS>
__global__ __launch_bounds__(256) void attn_extend_partial(ExtArgs a) {
    __shared__ __align__(16) uint16_t qs[64 * XQP];
    __shared__ __align__(16) uint16_t kt[64 * XQP];
    __shared__ __align__(16) uint16_t vt[XD * XVP];
    __shared__ __align__(16) uint16_t ps[64 * XVP];       // P (fp16); during a piece's fill: the staged token-side factors
    __shared__ __align__(16) float un[2 * XD * XFP];      // staged channel-side factors, then the score tile [64][XSP]
    __shared__ float sm[64], sl[64], sal[64];
    static_assert(64 * XSP <= 2 * XD * XFP, "score tile fits the staging area");
    static_assert(2 * 64 * XFP * 4 <= 64 * XVP * 2, "token-side factors fit the P tile");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const int64_t bh = blockIdx.y;
    const int b = (int)(bh / a.c.Hkv), hkv = (int)(bh % a.c.Hkv);
    const int mt = blockIdx.x % a.nmt, split = blockIdx.x / a.nmt;
    const int m0 = mt * 64, rows = a.n * a.G;
    float* S = un;

    for (int it = tid; it < 64 * 16; it += 256) {
        const int r = it >> 4, c8 = it & 15, m = m0 + r;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (m < rows) {
            const int i = m / a.G, hq = hkv * a.G + m % a.G;
            v = *(const uint4*)(a.q + (((int64_t)b * a.Hq + hq) * a.n + i) * XD + c8 * 8);
        }
        *(uint4*)(qs + r * XQP + c8 * 8) = v;
    }
    if (tid < 64) { sm[tid] = -INFINITY; sl[tid] = 0.0f; }

    const int i_max = min(a.n - 1, (min(m0 + 63, rows - 1)) / a.G);
    const int kend = a.T + a.W + i_max + 1;                  // keys [0, kend) can be visible to this tile
    const int p_last = a.npc + (kend - a.T - 1) / 64;        // (kend > T always: every query sees itself)
    const int p0 = split * a.pps, p1 = min(min(a.np, p0 + a.pps), p_last + 1);
    xf16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; r++) { o0[r] = 0.0f; o1[r] = 0.0f; }

    for (int pc = p0; pc < p1; pc++) {
        __syncthreads();                                     // the previous piece's tiles are no longer read
        const bool comp = pc < a.npc;
        if (comp) x_fill_comp<BITS>(a, bh, b, hkv, pc * 64, kt, vt, un, (float*)ps);
        else x_fill_f16(a, bh, (pc - a.npc) * 64, kt, vt);
        __syncthreads();
        {   // S = Q K^T: wave -> rows 32 (wave >> 1), keys 32 (wave & 1)
            const int rb = wave >> 1, cb = wave & 1;
            xf16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < 8; ks++) {
                const xh8 A = *(const xh8*)(qs + (rb * 32 + l31) * XQP + ks * 16 + 8 * h);
                const xh8 B = *(const xh8*)(kt + (cb * 32 + l31) * XQP + ks * 16 + 8 * h);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B, acc, 0, 0, 0);
            }
            const int key = cb * 32 + l31;
            const int kpos = comp ? pc * 64 + key : a.T + (pc - a.npc) * 64 + key;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int i = min((m0 + row) / a.G, a.n - 1);
                const bool ok = kpos <= a.T + a.W + i;
                S[row * XSP + key] = ok ? acc[r] * a.qscale : -INFINITY;
            }
        }
        __syncthreads();
        {   // online softmax: 4 lanes per row, 16 keys each
            const int row = tid >> 2, sub = tid & 3;
            const float* sr = S + row * XSP + sub * 16;
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < 16; j++) mx = fmaxf(mx, sr[j]);
            mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
            const float mold = sm[row], mnew = fmaxf(mold, mx);
            float alpha = 1.0f, sum = 0.0f;
            uint32_t pk[8];
            if (mnew == -INFINITY) {
#pragma unroll
                for (int j = 0; j < 8; j++) pk[j] = 0u;
            } else {
                alpha = __expf(mold - mnew);
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const float e0 = __expf(sr[2 * j] - mnew), e1 = __expf(sr[2 * j + 1] - mnew);
                    sum += e0 + e1;
                    pk[j] = f2h2_bits(e0, e1);
                }
            }
            uint4* dst = (uint4*)(ps + row * XVP + sub * 16);
            dst[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            dst[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
            sum += __shfl_xor(sum, 1, 64);
            sum += __shfl_xor(sum, 2, 64);
            if (sub == 0) {
                sm[row] = mnew;
                sl[row] = sl[row] * alpha + sum;
                sal[row] = alpha;
            }
        }
        __syncthreads();
        {   // O = alpha O + P V: wave -> rows 32 (wave >> 1), channels 64 (wave & 1) as two 32-column blocks
            const int rb = wave >> 1, cd = (wave & 1) * 2;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float al = sal[rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
                o0[r] *= al;
                o1[r] *= al;
            }
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                const xh8 A = *(const xh8*)(ps + (rb * 32 + l31) * XVP + ks * 16 + 8 * h);
                const xh8 B0 = *(const xh8*)(vt + (cd * 32 + l31) * XVP + ks * 16 + 8 * h);
                const xh8 B1 = *(const xh8*)(vt + ((cd + 1) * 32 + l31) * XVP + ks * 16 + 8 * h);
                o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B0, o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B1, o1, 0, 0, 0);
            }
        }
    }
    __syncthreads();
    const int64_t slot = (bh * a.nmt + mt) * a.nsplit + split;
    {
        const int rb = wave >> 1, cd = (wave & 1) * 2;
        float* po = a.part_o + slot * 64 * XD;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            po[row * XD + cd * 32 + l31] = o0[r];
            po[row * XD + (cd + 1) * 32 + l31] = o1[r];
        }
    }
    if (tid < 64) {
        a.part_ml[(slot * 64 + tid) * 2] = sm[tid];
        a.part_ml[(slot * 64 + tid) * 2 + 1] = sl[tid];
    }
}

// one output row (b, hq, i) per workgroup, one channel per thread: merge the splits' partials
__global__ __launch_bounds__(128) void attn_extend_merge(ExtArgs a) {
    const int64_t x = blockIdx.x;
    const int i = (int)(x % a.n);
    const int64_t bhq = x / a.n;
    const int b = (int)(bhq / a.Hq), hq = (int)(bhq % a.Hq);
    const int hkv = hq / a.G, m = i * a.G + hq % a.G;
    const int64_t bh = (int64_t)b * a.c.Hkv + hkv;
    const int64_t base = (bh * a.nmt + m / 64) * a.nsplit;
    const int r = m % 64, d = threadIdx.x;
    float M = -INFINITY;
    for (int s = 0; s < a.nsplit; s++) M = fmaxf(M, a.part_ml[((base + s) * 64 + r) * 2]);
    float L = 0.0f, acc = 0.0f;
    for (int s = 0; s < a.nsplit; s++) {
        const float ms = a.part_ml[((base + s) * 64 + r) * 2];
        if (ms == -INFINITY) continue;
        const float e = __expf(ms - M);
        L = fmaf(e, a.part_ml[((base + s) * 64 + r) * 2 + 1], L);
        acc = fmaf(e, a.part_o[((base + s) * 64 + r) * XD + d], acc);
    }
    a.out[x * XD + d] = f2h_bits(acc / L);
    if (a.lse && d == 0) a.lse[x] = M + logf(L);
}

}  // namespace

extern "C" size_t gear_attn_extend_workspace(int B, int Hq, int n, int T, int W) {
    if (B <= 0 || Hq <= 0 || n <= 0 || T < 0 || W < 0) return 0;
    return (size_t)ext_slots_bound(B, Hq, n, T, W) * 64 * (XD + 2) * sizeof(float) + 256;
}

extern "C" int gear_attn_extend_cache(const gear_cache_view* c, const void* q, int Hq, int n, int T, int W, const void* k_new,
                                      const void* v_new, float qscale, void* out, void* lse, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    GEAR_CHECK_ARG(c, "gear_attn_extend_cache: null cache view");
    GEAR_CHECK_ARG(n >= 1 && n <= X_NMAX, "gear_attn_extend_cache: n = %d query tokens, must be in [1, %d]", n, X_NMAX);
    GEAR_CHECK_ARG(c->D == XD, "gear_attn_extend_cache: head_dim %d, must be 128", c->D);
    GEAR_CHECK_ARG(c->B > 0 && c->Hkv > 0 && (int64_t)c->B * c->Hkv <= 65535, "gear_attn_extend_cache: B %d x Hkv %d", c->B, c->Hkv);
    GEAR_CHECK_ARG(Hq > 0 && Hq % c->Hkv == 0, "gear_attn_extend_cache: Hq %d not a multiple of Hkv %d", Hq, c->Hkv);
    GEAR_CHECK_ARG(W >= 0 && W <= c->wcap, "gear_attn_extend_cache: W = %d window tokens, the window holds wcap = %d", W, c->wcap);
    GEAR_CHECK_ARG(T >= 0 && T <= c->tcap && T % 64 == 0,
                   "gear_attn_extend_cache: T = %d compressed tokens, must be a multiple of 64 in [0, tcap = %d]", T, c->tcap);
    GEAR_CHECK_ARG((int64_t)T + W + n <= 65535, "gear_attn_extend_cache: T + W + n = %lld positions", (long long)T + W + n);
    GEAR_CHECK_ARG(q && k_new && v_new && out, "gear_attn_extend_cache: null q / k_new / v_new / out");
    GEAR_CHECK_ARG(W == 0 || (c->kwin && c->vwin), "gear_attn_extend_cache: W > 0 needs the window tensors");
    if (T > 0) {
        GEAR_CHECK_ARG(c->bits == 2 || c->bits == 4, "gear_attn_extend_cache: bits %d, must be 2 or 4", c->bits);
        GEAR_CHECK_ARG(c->group == 32 || c->group == 64, "gear_attn_extend_cache: group %d, must be 32 or 64", c->group);
        GEAR_CHECK_ARG(c->mode == GEAR_MODE_FP16_STEPWISE, "gear_attn_extend_cache: mode %d, the cache stores fp16 scales (mode 0)",
                       c->mode);
        GEAR_CHECK_ARG(c->kcode && c->kscale && c->kmn && c->vcode && c->vscale && c->vmn,
                       "gear_attn_extend_cache: T > 0 needs the quantized payload");
        GEAR_CHECK_ARG(c->ldk * (32 / c->bits) >= c->tcap && c->lsk * c->group >= c->tcap,
                       "gear_attn_extend_cache: K row pitches ldk %d / lsk %d below the capacity %d", c->ldk, c->lsk, c->tcap);
        GEAR_CHECK_ARG(c->rk >= 0 && c->rk <= 16 && c->rv >= 0 && c->rv <= 16, "gear_attn_extend_cache: rank %d / %d, at most 16",
                       c->rk, c->rv);
        GEAR_CHECK_ARG((!c->kP || !c->rk || c->kQ) && (!c->vP || !c->rv || c->vQ), "gear_attn_extend_cache: factor P without Q");
        GEAR_CHECK_ARG(!(c->koidx && (c->kk0 > 0 || c->kkb > 0)) || (c->koval && c->kk_cap >= c->kk0 && c->kk_cap > 0),
                       "gear_attn_extend_cache: K outlier lists (kk0 %d, kkb %d, kk_cap %d)", c->kk0, c->kkb, c->kk_cap);
        GEAR_CHECK_ARG(c->kkb == 0 || c->seglen % 64 == 0, "gear_attn_extend_cache: segment length %d, must be a multiple of 64",
                       c->seglen);
        GEAR_CHECK_ARG(c->seg0 % 64 == 0, "gear_attn_extend_cache: seg0 %d, must be a multiple of 64", c->seg0);
    }
    ExtPlan p;
    ext_plan((int64_t)c->B * c->Hkv, Hq / c->Hkv, n, T, W, p);
    const int64_t slots = (int64_t)c->B * c->Hkv * p.nmt * p.nsplit;
    const size_t need = (size_t)slots * 64 * (XD + 2) * sizeof(float) + 256;
    GEAR_CHECK_ARG(workspace && workspace_bytes >= need, "gear_attn_extend_cache: workspace of %zu bytes, needs %zu "
                   "(gear_attn_extend_workspace)", workspace_bytes, need);
    ExtArgs a;
    a.c = *c;
    if (T == 0) { a.c.kP = a.c.vP = nullptr; }
    a.q = (const uint16_t*)q;
    a.knew = (const uint16_t*)k_new;
    a.vnew = (const uint16_t*)v_new;
    a.Hq = Hq; a.G = Hq / c->Hkv; a.n = n; a.T = T; a.W = W;
    a.qscale = qscale;
    a.nmt = p.nmt; a.nsplit = p.nsplit; a.pps = p.pps; a.npc = p.npc; a.np = p.np;
    a.kP_seg = (int64_t)c->B * c->Hkv * XD * c->rk;
    a.vP_seg = (int64_t)c->B * c->Hkv * XD * c->rv;
    uintptr_t base = ((uintptr_t)workspace + 255) & ~(uintptr_t)255;
    a.part_o = (float*)base;
    a.part_ml = a.part_o + slots * 64 * XD;
    a.out = (uint16_t*)out;
    a.lse = (float*)lse;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(p.nsplit * p.nmt), (unsigned)(c->B * c->Hkv));
    if (c->bits == 4) hipLaunchKernelGGL((attn_extend_partial<4>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_extend_partial<2>), grid, dim3(256), 0, st, a);
    GEAR_CHECK_LAUNCH("attn_extend_partial");
    hipLaunchKernelGGL(attn_extend_merge, dim3((unsigned)((int64_t)c->B * Hq * n)), dim3(XD), 0, st, a);
    GEAR_CHECK_LAUNCH("attn_extend_merge");
    return 0;
}
