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
//
// Shared-prefix extend (gear_attn_extend_shared): S sequences behind ONE stored prompt.  The prefix pass is the same kernel with
// PFX = true over the prefix view (B == 1): the batch is folded into the row axis -- M = S n G rows per KV head, row
// m = (s n + i) G + gh, q addressed in place --, the keys are the Tp / 64 compressed pieces, nothing is masked.  A 64-row tile may
// hold rows of several sequences: a prefix piece is read and dequantized once per 64 query rows of ANY sequences.  The tail pass is
// the PFX = false kernel over the batch-S tail view (compressed tail pieces, window, chunk; tail-local causality), and
// attn_extend_shared_merge joins both slot sets per output row (prefix splits first, then tail splits: a fixed order).
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
    int S;                    // prefix pass only: sequences folded into the row axis
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

// the prefix pass of gear_attn_extend_shared: Hkv grid rows, S n G query rows each, the Tp / 64 compressed pieces only
void ext_plan_prefix(int Hkv, int64_t rows, int Tp, ExtPlan& p) {
    p.nmt = (int)((rows + 63) / 64);
    p.npc = p.np = Tp / 64;
    const int64_t nwork = (int64_t)Hkv * p.nmt;
    const int64_t want = std::min<int64_t>(p.np, std::max<int64_t>(1, (X_TARGET_WG + nwork - 1) / nwork));
    p.pps = (int)((p.np + want - 1) / want);
    p.nsplit = (p.np + p.pps - 1) / p.pps;
}

// its slots for any Hkv dividing Hq: nwork = Hkv ceil(S n G / 64) <= S Hq n / 64 + Hq
int64_t ext_prefix_slots_bound(int S, int Hq, int n, int Tp) {
    const int64_t nw = ((int64_t)S * Hq * n + 63) / 64 + Hq;
    return std::min<int64_t>(X_TARGET_WG + nw, nw * (Tp / 64));
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

// PFX = false: one sequence per grid row (blockIdx.y = b * Hkv + hkv), rows m = i G + gh, causal over window + chunk.
// PFX = true: the prefix pass of the shared call (blockIdx.y = hkv of the B == 1 view), rows m = (s n + i) G + gh of all S
// sequences, compressed pieces only, no mask; padding rows (m >= S n G) carry q = 0 and are never merged.
template <int BITS, bool PFX = false>
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
    const int m0 = mt * 64, rows = PFX ? a.S * a.n * a.G : a.n * a.G;
    float* S = un;

    for (int it = tid; it < 64 * 16; it += 256) {
        const int r = it >> 4, c8 = it & 15, m = m0 + r;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (m < rows) {
            if constexpr (PFX) {
                const int si = m / a.G, hq = hkv * a.G + m % a.G;            // si = s n + i
                v = *(const uint4*)(a.q + (((int64_t)(si / a.n) * a.Hq + hq) * a.n + si % a.n) * XD + c8 * 8);
            } else {
                const int i = m / a.G, hq = hkv * a.G + m % a.G;
                v = *(const uint4*)(a.q + (((int64_t)b * a.Hq + hq) * a.n + i) * XD + c8 * 8);
            }
        }
        *(uint4*)(qs + r * XQP + c8 * 8) = v;
    }
    if (tid < 64) { sm[tid] = -INFINITY; sl[tid] = 0.0f; }

    const int p0 = split * a.pps;
    int p1;
    if constexpr (PFX) {
        p1 = min(a.np, p0 + a.pps);                          // np == npc: every prefix piece is visible to every row
    } else {
        const int i_max = min(a.n - 1, (min(m0 + 63, rows - 1)) / a.G);
        const int kend = a.T + a.W + i_max + 1;              // keys [0, kend) can be visible to this tile
        const int p_last = a.npc + (kend - a.T - 1) / 64;    // (kend > T always: every query sees itself)
        p1 = min(min(a.np, p0 + a.pps), p_last + 1);
    }
    xf16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; r++) { o0[r] = 0.0f; o1[r] = 0.0f; }

    for (int pc = p0; pc < p1; pc++) {
        __syncthreads();                                     // the previous piece's tiles are no longer read
        const bool comp = PFX || pc < a.npc;
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
                if constexpr (PFX) {
                    S[row * XSP + key] = acc[r] * a.qscale;
                } else {
                    const int i = min((m0 + row) / a.G, a.n - 1);
                    const bool ok = kpos <= a.T + a.W + i;
                    S[row * XSP + key] = ok ? acc[r] * a.qscale : -INFINITY;
                }
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

struct ExtSharedMerge {
    const float* po_p;        // prefix pass: [slots, 64, 128], [slots, 64, 2]
    const float* pml_p;
    const float* po_t;        // tail pass
    const float* pml_t;
    int nmt_p, nsplit_p, nmt_t, nsplit_t;
    int Hq, Hkv, G, n;
    uint16_t* out;            // [S, Hq, n, 128]
    float* lse;               // [S, Hq, n] or null
};

// one output row (s, hq, i) per workgroup, one channel per thread: the prefix splits, then the tail splits (attn_extend_merge's
// arithmetic; a split that saw no key has m = -inf and is skipped; the tail pass always holds the row's own chunk key, so L > 0)
__global__ __launch_bounds__(128) void attn_extend_shared_merge(ExtSharedMerge a) {
    const int64_t x = blockIdx.x;
    const int i = (int)(x % a.n);
    const int64_t shq = x / a.n;
    const int s = (int)(shq / a.Hq), hq = (int)(shq % a.Hq);
    const int hkv = hq / a.G, gh = hq % a.G;
    const int64_t mp = ((int64_t)s * a.n + i) * a.G + gh;
    const int mt = i * a.G + gh;
    const int64_t base_p = ((int64_t)hkv * a.nmt_p + mp / 64) * a.nsplit_p;
    const int64_t base_t = (((int64_t)s * a.Hkv + hkv) * a.nmt_t + mt / 64) * a.nsplit_t;
    const int rp = (int)(mp % 64), rt = mt % 64, d = threadIdx.x;
    float M = -INFINITY;
    for (int k = 0; k < a.nsplit_p; k++) M = fmaxf(M, a.pml_p[((base_p + k) * 64 + rp) * 2]);
    for (int k = 0; k < a.nsplit_t; k++) M = fmaxf(M, a.pml_t[((base_t + k) * 64 + rt) * 2]);
    float L = 0.0f, acc = 0.0f;
    for (int k = 0; k < a.nsplit_p; k++) {
        const float ms = a.pml_p[((base_p + k) * 64 + rp) * 2];
        if (ms == -INFINITY) continue;
        const float e = __expf(ms - M);
        L = fmaf(e, a.pml_p[((base_p + k) * 64 + rp) * 2 + 1], L);
        acc = fmaf(e, a.po_p[((base_p + k) * 64 + rp) * XD + d], acc);
    }
    for (int k = 0; k < a.nsplit_t; k++) {
        const float ms = a.pml_t[((base_t + k) * 64 + rt) * 2];
        if (ms == -INFINITY) continue;
        const float e = __expf(ms - M);
        L = fmaf(e, a.pml_t[((base_t + k) * 64 + rt) * 2 + 1], L);
        acc = fmaf(e, a.po_t[((base_t + k) * 64 + rt) * XD + d], acc);
    }
    a.out[x * XD + d] = f2h_bits(acc / L);
    if (a.lse && d == 0) a.lse[x] = M + logf(L);
}

// the checks a view's compressed payload must pass before a kernel reads it (fn: the entry point's name in the message)
int ext_check_payload(const gear_cache_view* c, const char* fn) {
    GEAR_CHECK_ARG(c->bits == 2 || c->bits == 4, "%s: bits %d, must be 2 or 4", fn, c->bits);
    GEAR_CHECK_ARG(c->group == 32 || c->group == 64, "%s: group %d, must be 32 or 64", fn, c->group);
    GEAR_CHECK_ARG(c->mode == GEAR_MODE_FP16_STEPWISE, "%s: mode %d, the cache stores fp16 scales (mode 0)", fn, c->mode);
    GEAR_CHECK_ARG(c->kcode && c->kscale && c->kmn && c->vcode && c->vscale && c->vmn, "%s: T > 0 needs the quantized payload", fn);
    GEAR_CHECK_ARG(c->ldk * (32 / c->bits) >= c->tcap && c->lsk * c->group >= c->tcap,
                   "%s: K row pitches ldk %d / lsk %d below the capacity %d", fn, c->ldk, c->lsk, c->tcap);
    GEAR_CHECK_ARG(c->rk >= 0 && c->rk <= 16 && c->rv >= 0 && c->rv <= 16, "%s: rank %d / %d, at most 16", fn, c->rk, c->rv);
    GEAR_CHECK_ARG((!c->kP || !c->rk || c->kQ) && (!c->vP || !c->rv || c->vQ), "%s: factor P without Q", fn);
    GEAR_CHECK_ARG(!(c->koidx && (c->kk0 > 0 || c->kkb > 0)) || (c->koval && c->kk_cap >= c->kk0 && c->kk_cap > 0),
                   "%s: K outlier lists (kk0 %d, kkb %d, kk_cap %d)", fn, c->kk0, c->kkb, c->kk_cap);
    GEAR_CHECK_ARG(c->kkb == 0 || c->seglen % 64 == 0, "%s: segment length %d, must be a multiple of 64", fn, c->seglen);
    GEAR_CHECK_ARG(c->seg0 % 64 == 0, "%s: seg0 %d, must be a multiple of 64", fn, c->seg0);
    return 0;
}

// the launch arguments of one partial pass over view c (slots at part_o / part_ml follow from the plan)
void ext_fill_args(ExtArgs& a, const gear_cache_view* c, bool comp, const void* q, const void* k_new, const void* v_new, int Hq, int n,
                   int T, int W, float qscale, const ExtPlan& p, float* part_o, int64_t slots) {
    a.c = *c;
    if (!comp) { a.c.kP = a.c.vP = nullptr; }
    a.q = (const uint16_t*)q;
    a.knew = (const uint16_t*)k_new;
    a.vnew = (const uint16_t*)v_new;
    a.Hq = Hq; a.G = Hq / c->Hkv; a.n = n; a.T = T; a.W = W;
    a.qscale = qscale;
    a.nmt = p.nmt; a.nsplit = p.nsplit; a.pps = p.pps; a.npc = p.npc; a.np = p.np;
    a.S = c->B;
    a.kP_seg = (int64_t)c->B * c->Hkv * XD * c->rk;
    a.vP_seg = (int64_t)c->B * c->Hkv * XD * c->rv;
    a.part_o = part_o;
    a.part_ml = part_o + slots * 64 * XD;
    a.out = nullptr;
    a.lse = nullptr;
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
    if (T > 0 && ext_check_payload(c, "gear_attn_extend_cache")) return -1;
    ExtPlan p;
    ext_plan((int64_t)c->B * c->Hkv, Hq / c->Hkv, n, T, W, p);
    const int64_t slots = (int64_t)c->B * c->Hkv * p.nmt * p.nsplit;
    const size_t need = (size_t)slots * 64 * (XD + 2) * sizeof(float) + 256;
    GEAR_CHECK_ARG(workspace && workspace_bytes >= need, "gear_attn_extend_cache: workspace of %zu bytes, needs %zu "
                   "(gear_attn_extend_workspace)", workspace_bytes, need);
    ExtArgs a;
    const uintptr_t base = ((uintptr_t)workspace + 255) & ~(uintptr_t)255;
    ext_fill_args(a, c, T > 0, q, k_new, v_new, Hq, n, T, W, qscale, p, (float*)base, slots);
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

extern "C" size_t gear_attn_extend_shared_workspace(int S, int Hq, int n, int Tp, int T, int W) {
    if (S <= 0 || Hq <= 0 || n <= 0 || Tp < 64 || T < 0 || W < 0) return 0;
    return (size_t)(ext_prefix_slots_bound(S, Hq, n, Tp) + ext_slots_bound(S, Hq, n, T, W)) * 64 * (XD + 2) * sizeof(float) + 256;
}

extern "C" int gear_attn_extend_shared(const gear_cache_view* prefix, int Tp, const gear_cache_view* tail, int T, int W, const void* q,
                                       int Hq, int n, const void* k_new, const void* v_new, float qscale, void* out, void* lse,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "gear_attn_extend_shared";
    GEAR_CHECK_ARG(prefix && tail, "gear_attn_extend_shared: null cache view");
    GEAR_CHECK_ARG(prefix->B == 1, "gear_attn_extend_shared: the prefix view must have B == 1 (got %d)", prefix->B);
    GEAR_CHECK_ARG(prefix->Hkv == tail->Hkv && prefix->D == tail->D && prefix->bits == tail->bits && prefix->group == tail->group &&
                       prefix->mode == tail->mode && prefix->rk == tail->rk && prefix->rv == tail->rv,
                   "gear_attn_extend_shared: prefix and tail views disagree (Hkv %d / %d, D %d / %d, bits %d / %d, group %d / %d, mode "
                   "%d / %d, ranks %d,%d / %d,%d)", prefix->Hkv, tail->Hkv, prefix->D, tail->D, prefix->bits, tail->bits, prefix->group,
                   tail->group, prefix->mode, tail->mode, prefix->rk, prefix->rv, tail->rk, tail->rv);
    GEAR_CHECK_ARG(prefix->D == XD, "gear_attn_extend_shared: head_dim %d, must be 128", prefix->D);
    const int S = tail->B, Hkv = tail->Hkv;
    GEAR_CHECK_ARG(S > 0 && Hkv > 0 && (int64_t)S * Hkv <= 65535, "gear_attn_extend_shared: S %d x Hkv %d (at most 65535)", S, Hkv);
    GEAR_CHECK_ARG(n >= 1 && n <= X_NMAX, "gear_attn_extend_shared: n = %d query tokens, must be in [1, %d]", n, X_NMAX);
    GEAR_CHECK_ARG(Tp > 0 && Tp % 64 == 0 && Tp <= prefix->tcap,
                   "gear_attn_extend_shared: Tp = %d prefix tokens, must be a positive multiple of 64 within tcap = %d", Tp, prefix->tcap);
    GEAR_CHECK_ARG(T >= 0 && T % 64 == 0 && T <= tail->tcap,
                   "gear_attn_extend_shared: T = %d compressed tail tokens, must be a multiple of 64 in [0, tcap = %d]", T, tail->tcap);
    GEAR_CHECK_ARG(W >= 0 && W <= tail->wcap, "gear_attn_extend_shared: W = %d window tokens, the window holds wcap = %d", W,
                   tail->wcap);
    GEAR_CHECK_ARG((int64_t)Tp + T + W + n <= 65535, "gear_attn_extend_shared: Tp + T + W + n = %lld positions (at most 65535)",
                   (long long)Tp + T + W + n);
    GEAR_CHECK_ARG(Hq > 0 && Hq % Hkv == 0, "gear_attn_extend_shared: Hq %d not a multiple of Hkv %d", Hq, Hkv);
    GEAR_CHECK_ARG((int64_t)S * Hq * n <= 0x7FFFFF00, "gear_attn_extend_shared: S %d x Hq %d x n %d query rows (at most 2^31 - 256)", S,
                   Hq, n);
    GEAR_CHECK_ARG(q && k_new && v_new && out, "gear_attn_extend_shared: null q / k_new / v_new / out");
    GEAR_CHECK_ARG(W == 0 || (tail->kwin && tail->vwin), "gear_attn_extend_shared: W > 0 needs the window tensors");
    if (ext_check_payload(prefix, fn)) return -1;
    if (T > 0 && ext_check_payload(tail, fn)) return -1;
    const int G = Hq / Hkv;
    ExtPlan pp, pt;
    ext_plan_prefix(Hkv, (int64_t)S * n * G, Tp, pp);
    ext_plan((int64_t)S * Hkv, G, n, T, W, pt);
    const int64_t slots_p = (int64_t)Hkv * pp.nmt * pp.nsplit, slots_t = (int64_t)S * Hkv * pt.nmt * pt.nsplit;
    GEAR_CHECK_ARG((int64_t)pp.nsplit * pp.nmt <= 0x7FFFFFFF, "gear_attn_extend_shared: %lld prefix workgroups per KV head",
                   (long long)pp.nsplit * pp.nmt);
    const size_t need = (size_t)(slots_p + slots_t) * 64 * (XD + 2) * sizeof(float) + 256;
    GEAR_CHECK_ARG(workspace && workspace_bytes >= need, "gear_attn_extend_shared: workspace of %zu bytes, needs %zu "
                   "(gear_attn_extend_shared_workspace)", workspace_bytes, need);
    float* ws_p = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* ws_t = ws_p + slots_p * 64 * (XD + 2);
    ExtArgs ap, at;
    ext_fill_args(ap, prefix, true, q, k_new, v_new, Hq, n, Tp, 0, qscale, pp, ws_p, slots_p);
    ap.S = S;
    ext_fill_args(at, tail, T > 0, q, k_new, v_new, Hq, n, T, W, qscale, pt, ws_t, slots_t);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid_p((unsigned)(pp.nsplit * pp.nmt), (unsigned)Hkv), grid_t((unsigned)(pt.nsplit * pt.nmt), (unsigned)(S * Hkv));
    if (tail->bits == 4) hipLaunchKernelGGL((attn_extend_partial<4, true>), grid_p, dim3(256), 0, st, ap);
    else hipLaunchKernelGGL((attn_extend_partial<2, true>), grid_p, dim3(256), 0, st, ap);
    GEAR_CHECK_LAUNCH("attn_extend_partial (prefix)");
    if (tail->bits == 4) hipLaunchKernelGGL((attn_extend_partial<4, false>), grid_t, dim3(256), 0, st, at);
    else hipLaunchKernelGGL((attn_extend_partial<2, false>), grid_t, dim3(256), 0, st, at);
    GEAR_CHECK_LAUNCH("attn_extend_partial (tail)");
    ExtSharedMerge m;
    m.po_p = ap.part_o; m.pml_p = ap.part_ml; m.po_t = at.part_o; m.pml_t = at.part_ml;
    m.nmt_p = pp.nmt; m.nsplit_p = pp.nsplit; m.nmt_t = pt.nmt; m.nsplit_t = pt.nsplit;
    m.Hq = Hq; m.Hkv = Hkv; m.G = G; m.n = n;
    m.out = (uint16_t*)out;
    m.lse = (float*)lse;
    hipLaunchKernelGGL(attn_extend_shared_merge, dim3((unsigned)((int64_t)S * Hq * n)), dim3(XD), 0, st, m);
    GEAR_CHECK_LAUNCH("attn_extend_shared_merge");
    return 0;
}
