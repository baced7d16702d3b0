// kivi.hip -- the KIVI cache on the fused decode path (gfx950): the state machine of cuda_supported_gear/modeling_llama_kivi.py
// (:149-162 K block window, :200-213 sliding V window) on a pre-allocated cache whose packed fields have GearKVCache's layouts.
//   gear_kivi_rope_append / gear_kivi_append : the new token's K row into the K window, its V row into the V ring -- and, in the
//       same launch and before the overwrite, the ring row it evicts quantized per token into the packed V part
//   gear_attn_decode_kivi : single-token attention over packed K [0, Tk) + fp16 K window [Tk, L) and packed V [0, Nv) + fp16 V
//       ring [Nv, L): the whole 64-token chunks below Nv through the decode partial dispatch (attention.hip), then one seam kernel
//       per output row that scores the <= 63 + R + 1 remaining tokens itself -- K from codes or the window, V from codes or the
//       ring, chosen per token -- and merges them with the partial slots in one fp32 softmax.  Two launches whatever L is.
#include <math.h>

#include "attn_partials.h"
#include "common.h"

namespace {

constexpr int KD = 128;          // head_dim
constexpr int KS_MAX = 66;       // partial slots per row (attention.hip RS_MAX)
constexpr int SEAM_MAX = 192;    // seam tokens: 63 + R + 1, R <= 128
constexpr int KP = KD + 8;       // LDS pitch (fp16 elements) of a dequantized K row: 272 bytes, 16-byte aligned

// ------------------------------------------------------------------------------------------------------------- append
// One thread per (b, head, pair index p): elements p and p + 64 of the head's row, as rope_append_kernel; the 64 threads of a head
// are one wave, so the two 64-channel groups of an evicted V row are reduced with wave shuffles and its code words are put
// together with an OR butterfly over the CPW lanes of a word.
struct KiviAppend {
    const uint16_t *qsrc, *ksrc, *vsrc;      // row (b, h) of a source at b * bstride + h * 128
    int64_t bstride;
    int B, Hq, Hkv, rope, pos;
    float log2_theta;
    const float* inv_tab;                    // table flavour (rope_scaling): 64 inverse frequencies in place of log2_theta
    float attn_factor;
    uint16_t *q_out, *kwin, *vring;
    int kslot, R, vslot;
    int evict_row;                           // row of vcode / vscale / vmn the ring row at vslot goes to (-1: nothing to evict)
    uint32_t* vcode;
    uint16_t *vscale, *vmn;
    int tcap;
};

template <int BITS, bool TAB>
__global__ __launch_bounds__(256) void kivi_append_kernel(KiviAppend a) {
    constexpr int CPW = 32 / BITS, LEVELS = (1 << BITS) - 1;
    const int HT = a.Hq + 2 * a.Hkv;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.B * HT * 64) return;                   // (whole waves: the bound is a multiple of 64)
    const int p = (int)(i % 64);
    const int h = (int)((i / 64) % HT);
    const int b = (int)(i / (64 * HT));
    if (h >= a.Hq + a.Hkv) {                                   // V head (wave-uniform)
        const int hv = h - a.Hq - a.Hkv;
        const int64_t bh = (int64_t)b * a.Hkv + hv;
        uint16_t* dst = a.vring + (bh * (a.R + 1) + a.vslot) * KD;
        if (a.evict_row >= 0) {
            // the row this token overwrites: quantized per token, groups of 64 channels, gear_quant_pack_lastdim's fp16-stepwise
            // arithmetic (make_qparams<0> / quant_one<0>); lane p holds channel p of group 0 and channel p of group 1
            const float x0 = h2f_bits(dst[p]), x1 = h2f_bits(dst[p + 64]);
            float lo0 = x0, hi0 = x0, lo1 = x1, hi1 = x1;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                lo0 = fminf(lo0, __shfl_xor(lo0, m, 64));
                hi0 = fmaxf(hi0, __shfl_xor(hi0, m, 64));
                lo1 = fminf(lo1, __shfl_xor(lo1, m, 64));
                hi1 = fmaxf(hi1, __shfl_xor(hi1, m, 64));
            }
            const QuantParams<0> q0 = make_qparams<0>(lo0, hi0, LEVELS), q1 = make_qparams<0>(lo1, hi1, LEVELS);
            uint32_t w0 = (uint32_t)quant_one<0>(x0, q0) << (BITS * (p % CPW));
            uint32_t w1 = (uint32_t)quant_one<0>(x1, q1) << (BITS * (p % CPW));
#pragma unroll
            for (int m = 1; m < CPW; m <<= 1) {
                w0 |= (uint32_t)__shfl_xor((int)w0, m, 64);
                w1 |= (uint32_t)__shfl_xor((int)w1, m, 64);
            }
            const int64_t row = bh * a.tcap + a.evict_row;
            if (p % CPW == 0) {
                a.vcode[row * (KD / CPW) + p / CPW] = w0;
                a.vcode[row * (KD / CPW) + (p + 64) / CPW] = w1;
            }
            if (p == 0) {
                a.vscale[row * 2] = f2h_bits(q0.scale);
                a.vmn[row * 2] = f2h_bits(q0.mn);
                a.vscale[row * 2 + 1] = f2h_bits(q1.scale);
                a.vmn[row * 2 + 1] = f2h_bits(q1.mn);
            }
        }
        const uint16_t* src = a.vsrc + (int64_t)b * a.bstride + (int64_t)hv * KD;
        dst[p] = src[p];
        dst[p + 64] = src[p + 64];
        return;
    }
    const bool is_q = h < a.Hq;
    const uint16_t* src = is_q ? a.qsrc + (int64_t)b * a.bstride + (int64_t)h * KD
                               : a.ksrc + (int64_t)b * a.bstride + (int64_t)(h - a.Hq) * KD;
    uint16_t* dst = is_q ? a.q_out + ((int64_t)b * a.Hq + h) * KD
                         : a.kwin + (((int64_t)b * a.Hkv + (h - a.Hq)) * a.R + a.kslot) * KD;
    if (!a.rope) {
        dst[p] = src[p];
        dst[p + 64] = src[p + 64];
        return;
    }
    // rope_append_kernel's arithmetic (decode_ops.hip): cos / sin in fp32 cast to fp16, every elementwise op rounded to fp16
    float c, sn;
    rope_cos_sin<TAB>(p, a.pos, a.log2_theta, a.inv_tab, a.attn_factor, c, sn);
    const float x1 = h2f_bits(src[p]), x2 = h2f_bits(src[p + 64]);
    dst[p] = f2h_bits(hround(hround(x1 * c) + hround(-x2 * sn)));
    dst[p + 64] = f2h_bits(hround(hround(x2 * c) + hround(x1 * sn)));
}

int kivi_append_launch(const char* fn, KiviAppend& a, int D, int n, int group, int bits, void* stream) {
    GEAR_CHECK_ARG(D == KD, "%s: head_dim must be 128 (got %d)", fn, D);
    GEAR_CHECK_ARG(bits == 2 || bits == 4, "%s: bits must be 2 or 4 (got %d)", fn, bits);
    GEAR_CHECK_ARG(group == 64, "%s: group must be 64 (got %d)", fn, group);
    GEAR_CHECK_ARG(a.R == 64 || a.R == 128, "%s: residual length R must be 64 or 128 (got %d)", fn, a.R);
    GEAR_CHECK_ARG(a.B > 0 && a.Hq >= 0 && a.Hkv > 0 && a.pos >= 0, "%s: bad shape B %d, Hq %d, Hkv %d, pos %d", fn, a.B, a.Hq, a.Hkv, a.pos);
    GEAR_CHECK_ARG((int64_t)a.B * (a.Hq + 2 * a.Hkv) * 64 < 0x7FFFFFFFLL, "%s: too many rows", fn);
    GEAR_CHECK_ARG(a.ksrc && a.vsrc && a.kwin && a.vring && (a.Hq == 0 || (a.qsrc && a.q_out)), "%s: null pointer", fn);
    GEAR_CHECK_ARG(a.kslot >= 0 && a.kslot < a.R, "%s: K window slot %d outside [0, R = %d)", fn, a.kslot, a.R);
    GEAR_CHECK_ARG(n >= 0, "%s: token index n = %d", fn, n);
    GEAR_CHECK_ARG(a.evict_row == -1 || (a.evict_row == n - (a.R + 1) && a.evict_row >= 0),
                   "%s: evict_row = %d, must be -1 or n - (R + 1) = %d (the token the ring slot of token n holds)", fn, a.evict_row,
                   n - (a.R + 1));
    GEAR_CHECK_ARG(a.evict_row < 0 || (a.vcode && a.vscale && a.vmn && a.evict_row < a.tcap),
                   "%s: evicting row %d needs vcode / vscale / vmn with tcap > row (tcap = %d)", fn, a.evict_row, a.tcap);
    a.vslot = n % (a.R + 1);
    const int64_t nthr = (int64_t)a.B * (a.Hq + 2 * a.Hkv) * 64;
    const dim3 grid((unsigned)((nthr + 255) / 256));
    if (a.inv_tab) {
        if (bits == 2) hipLaunchKernelGGL((kivi_append_kernel<2, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((kivi_append_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
    } else {
        if (bits == 2) hipLaunchKernelGGL((kivi_append_kernel<2, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((kivi_append_kernel<4, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    }
    GEAR_CHECK_LAUNCH(fn);
    return 0;
}

// --------------------------------------------------------------------------------------------------------------- seam
struct KiviSeam {
    const uint16_t* q;               // [B Hq, 128]
    const float* po;                 // partial slots of the chunks below T0 (ns == 0: none)
    const float* ml;
    int ns;
    const uint32_t* kcode;           // [B Hkv, 128, ldk]
    const uint16_t *kscale, *kmn;    // [B Hkv, 128, lsk]
    int ldk, lsk;
    const uint32_t* vcode;           // [B Hkv, tcap, 128 / CPW]
    const uint16_t *vscale, *vmn;    // [B Hkv, tcap, 2]
    int tcap;
    const uint16_t* kwin;            // [B Hkv, R, 128]: token t >= Tk in row t - Tk
    const uint16_t* vring;           // [B Hkv, R + 1, 128]: token t >= Nv in row t % (R + 1)
    int R, Hq, Hkv;
    int L, Tk, Nv, T0;               // the seam is [T0, L), T0 = Nv rounded down to 64
    float qscale;
    uint16_t* out;                   // [B Hq, 128]
    float* lse;                      // [B Hq] or null
};

// One output row x = (b, hq) per workgroup.  Phase 0: the packed K tokens of the seam ([T0, Tk): up to 3 whole 64-token groups)
// dequantized into LDS as fp16 rows, thread = (group, channel).  Phase 1: scores of the nk = L - T0 seam keys, 8 threads per key and
// 16 channels each, the row from LDS or from the K window.  Phase 2: one fp32 softmax over the partial slots' (m, l) and the seam
// scores (wave 0; a slot with m = -inf gets the coefficient 0).  Phase 3: the weighted sum, two groups of 128 channel threads, a
// seam token's V row from the codes (t < Nv) or from the ring.  attn_shared_merge_kernel's arithmetic and order: nothing in it
// depends on the order in which waves run.
template <int BITS>
__global__ __launch_bounds__(256) void kivi_seam_kernel(KiviSeam v) {
    constexpr int CPW = 32 / BITS;
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    __shared__ __attribute__((aligned(16))) uint16_t kd[SEAM_MAX * KP];
    __shared__ float qs[KD];
    __shared__ float sc[SEAM_MAX];
    __shared__ float sml[2][KS_MAX];
    __shared__ float coef[KS_MAX + SEAM_MAX];
    __shared__ float og[2][KD];
    __shared__ float stat[2];
    const int tid = threadIdx.x;
    const int64_t x = blockIdx.x;
    const int b = (int)(x / v.Hq), hq = (int)(x % v.Hq);
    const int hkv = hq / (v.Hq / v.Hkv);
    const int64_t bhk = (int64_t)b * v.Hkv + hkv;
    const int ns = v.ns, nk = v.L - v.T0;
    const int npk = max(0, v.Tk - v.T0);                   // packed K tokens of the seam: a multiple of 64, <= nk <= 192
    if (tid < KD) qs[tid] = h2f_bits(v.q[x * KD + tid]) * v.qscale;
    if (tid < ns) {
        sml[0][tid] = v.ml[(x * ns + tid) * 2];
        sml[1][tid] = v.ml[(x * ns + tid) * 2 + 1];
    }
    {
        const int d = tid & (KD - 1);
        for (int g = tid >> 7; g * 64 < npk; g += 2) {
            const int t0 = v.T0 + g * 64;
            const int64_t ch = bhk * KD + d;
            const uint32_t* row = v.kcode + ch * v.ldk + t0 / CPW;
            const float s = h2f_bits(v.kscale[ch * v.lsk + t0 / 64]), m = h2f_bits(v.kmn[ch * v.lsk + t0 / 64]);
            uint32_t w[64 / CPW];
#pragma unroll
            for (int i = 0; i < 64 / CPW; i++) w[i] = row[i];
#pragma unroll
            for (int i = 0; i < 64 / CPW; i++)
#pragma unroll
                for (int j = 0; j < CPW; j++)
                    kd[(g * 64 + i * CPW + j) * KP + d] = f2h_bits(fmaf((float)((w[i] >> (BITS * j)) & MASK), s, m));
        }
    }
    __syncthreads();
    const int kj = tid >> 3, part = tid & 7;
    for (int k0 = 0; k0 < nk; k0 += 32) {                  // (block-uniform)
        const int k = k0 + kj;
        float acc = 0.0f;
        if (k < nk) {
            const int t = v.T0 + k;
            const uint4* kr4 = t < v.Tk ? (const uint4*)(kd + k * KP + part * 16)
                                        : (const uint4*)(v.kwin + (bhk * v.R + (t - v.Tk)) * (int64_t)KD + part * 16);
            float f[8];
            unpack8(kr4[0], f);
#pragma unroll
            for (int c = 0; c < 8; c++) acc = fmaf(qs[part * 16 + c], f[c], acc);
            unpack8(kr4[1], f);
#pragma unroll
            for (int c = 0; c < 8; c++) acc = fmaf(qs[part * 16 + 8 + c], f[c], acc);
        }
        acc += __shfl_xor(acc, 4, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 1, 64);
        if (k < nk && part == 0) sc[k] = acc;
    }
    __syncthreads();
    if (tid < 64) {   // statistics over <= 66 slots and <= 192 keys, strided over the 64 lanes of wave 0
        float M = -INFINITY;
        for (int s = tid; s < ns; s += 64) M = fmaxf(M, sml[0][s]);
        for (int k = tid; k < nk; k += 64) M = fmaxf(M, sc[k]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
        float Ls = 0.0f;
        for (int s = tid; s < ns; s += 64) {
            const float c = sml[0][s] == -INFINITY ? 0.0f : __expf(sml[0][s] - M);
            coef[s] = c;
            Ls = fmaf(c, sml[1][s], Ls);
        }
        for (int k = tid; k < nk; k += 64) {
            const float c = __expf(sc[k] - M);
            coef[KS_MAX + k] = c;
            Ls += c;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) Ls += __shfl_xor(Ls, o, 64);
        if (tid == 0) { stat[0] = M; stat[1] = Ls; }
    }
    __syncthreads();
    const int grp = tid >> 7, d = tid & (KD - 1);
    float o = 0.0f;
    for (int s = grp; s < ns; s += 2) o = fmaf(coef[s], v.po[(x * ns + s) * KD + d], o);
    for (int k = grp; k < nk; k += 2) {
        const int t = v.T0 + k;
        float val;
        if (t < v.Nv) {
            const int64_t row = bhk * v.tcap + t;
            const uint32_t w = v.vcode[row * (KD / CPW) + d / CPW];
            val = fmaf((float)((w >> (BITS * (d % CPW))) & MASK), h2f_bits(v.vscale[row * 2 + (d >> 6)]),
                       h2f_bits(v.vmn[row * 2 + (d >> 6)]));
        } else {
            val = h2f_bits(v.vring[(bhk * (v.R + 1) + t % (v.R + 1)) * (int64_t)KD + d]);
        }
        o = fmaf(coef[KS_MAX + k], val, o);
    }
    og[grp][d] = o;
    __syncthreads();
    if (tid < KD) {
        v.out[x * KD + tid] = f2h_bits((og[0][tid] + og[1][tid]) / stat[1]);
        if (v.lse && tid == 0) v.lse[x] = stat[0] + logf(stat[1]);
    }
}

}  // namespace

static int kivi_rope_append(const char* fn, const void* qkv, int B, int Hq, int Hkv, int D, int pos, float theta,
                            const float* inv_freq, float attn_factor, void* q_out, void* kwin, int kslot, void* vring, int n, int R,
                            int evict_row, void* vcode, void* vscale, void* vmn, int tcap, int group, int bits, void* stream) {
    KiviAppend a;
    const uint16_t* s = (const uint16_t*)qkv;
    a.qsrc = s;
    a.ksrc = s ? s + (int64_t)Hq * KD : nullptr;
    a.vsrc = s ? s + (int64_t)(Hq + Hkv) * KD : nullptr;
    a.bstride = (int64_t)(Hq + 2 * Hkv) * KD;
    a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.rope = 1; a.pos = pos;
    a.log2_theta = inv_freq ? 0.0f : log2f(theta);
    a.inv_tab = inv_freq; a.attn_factor = attn_factor;
    a.q_out = (uint16_t*)q_out; a.kwin = (uint16_t*)kwin; a.vring = (uint16_t*)vring;
    a.kslot = kslot; a.R = R; a.evict_row = evict_row;
    a.vcode = (uint32_t*)vcode; a.vscale = (uint16_t*)vscale; a.vmn = (uint16_t*)vmn; a.tcap = tcap;
    return kivi_append_launch(fn, a, D, n, group, bits, stream);
}

extern "C" int gear_kivi_rope_append(const void* qkv, int B, int Hq, int Hkv, int D, int pos, float theta, void* q_out, void* kwin,
                                     int kslot, void* vring, int n, int R, int evict_row, void* vcode, void* vscale, void* vmn,
                                     int tcap, int group, int bits, void* stream) {
    GEAR_CHECK_ARG(Hq > 0 && theta > 0.0f, "gear_kivi_rope_append: Hq %d, theta %g", Hq, (double)theta);
    return kivi_rope_append("gear_kivi_rope_append", qkv, B, Hq, Hkv, D, pos, theta, nullptr, 1.0f, q_out, kwin, kslot, vring, n, R,
                            evict_row, vcode, vscale, vmn, tcap, group, bits, stream);
}

extern "C" int gear_kivi_rope_append_freq(const void* qkv, int B, int Hq, int Hkv, int D, int pos, const float* inv_freq,
                                          float attn_factor, void* q_out, void* kwin, int kslot, void* vring, int n, int R,
                                          int evict_row, void* vcode, void* vscale, void* vmn, int tcap, int group, int bits,
                                          void* stream) {
    GEAR_CHECK_ARG(Hq > 0, "gear_kivi_rope_append_freq: Hq %d", Hq);
    GEAR_CHECK_ROPE_TABLE("gear_kivi_rope_append_freq", inv_freq, attn_factor);
    return kivi_rope_append("gear_kivi_rope_append_freq", qkv, B, Hq, Hkv, D, pos, 0.0f, inv_freq, attn_factor, q_out, kwin, kslot,
                            vring, n, R, evict_row, vcode, vscale, vmn, tcap, group, bits, stream);
}

extern "C" int gear_kivi_append(const void* k_new, const void* v_new, int B, int Hkv, int D, void* kwin, int kslot, void* vring,
                                int n, int R, int evict_row, void* vcode, void* vscale, void* vmn, int tcap, int group, int bits,
                                void* stream) {
    KiviAppend a;
    a.qsrc = nullptr; a.ksrc = (const uint16_t*)k_new; a.vsrc = (const uint16_t*)v_new;
    a.bstride = (int64_t)Hkv * KD;
    a.B = B; a.Hq = 0; a.Hkv = Hkv; a.rope = 0; a.pos = 0;
    a.log2_theta = 0.0f;
    a.inv_tab = nullptr; a.attn_factor = 1.0f;
    a.q_out = nullptr; a.kwin = (uint16_t*)kwin; a.vring = (uint16_t*)vring;
    a.kslot = kslot; a.R = R; a.evict_row = evict_row;
    a.vcode = (uint32_t*)vcode; a.vscale = (uint16_t*)vscale; a.vmn = (uint16_t*)vmn; a.tcap = tcap;
    return kivi_append_launch("gear_kivi_append", a, D, n, group, bits, stream);
}

extern "C" size_t gear_attn_decode_kivi_workspace(int B, int Hq, int T, int bits) {
    if (B <= 0 || Hq <= 0 || T < 0 || (bits != 2 && bits != 4)) return 0;
    return gear_attn_decode_workspace(B, Hq, T, bits);      // the partial slots of the chunks below the seam
}

extern "C" int gear_attn_decode_kivi(const gear_cache_view* c, const void* q, int Hq, int L, int Tk, int Nv, float qscale, void* out,
                                     void* lse, void* workspace, size_t workspace_bytes, void* stream) {
    GEAR_CHECK_ARG(c, "gear_attn_decode_kivi: null cache view");
    const int R = c->wcap, B = c->B, Hkv = c->Hkv;
    GEAR_CHECK_ARG(c->D == KD, "gear_attn_decode_kivi: head_dim must be 128 (got %d)", c->D);
    GEAR_CHECK_ARG(c->bits == 2 || c->bits == 4, "gear_attn_decode_kivi: bits must be 2 or 4 (got %d)", c->bits);
    GEAR_CHECK_ARG(c->group == 64, "gear_attn_decode_kivi: group must be 64 (got %d)", c->group);
    GEAR_CHECK_ARG(R == 64 || R == 128, "gear_attn_decode_kivi: residual length R (the view's wcap) must be 64 or 128 (got %d)", R);
    GEAR_CHECK_ARG(c->mode == 0, "gear_attn_decode_kivi: fp16 scales only (mode 0, got %d)", c->mode);
    GEAR_CHECK_ARG(c->rk == 0 && c->rv == 0 && c->kv == 0 && c->kk_cap == 0 && c->kk0 == 0 && c->kkb == 0,
                   "gear_attn_decode_kivi: a KIVI cache has no low-rank factors and no outliers (rk %d, rv %d, kv %d, kk_cap %d)",
                   c->rk, c->rv, c->kv, c->kk_cap);
    GEAR_CHECK_ARG(B > 0 && Hkv > 0 && Hq > 0 && Hq % Hkv == 0, "gear_attn_decode_kivi: bad head counts B %d, Hq %d, Hkv %d", B, Hq, Hkv);
    GEAR_CHECK_ARG((int64_t)B * Hq <= 65535, "gear_attn_decode_kivi: B %d x Hq %d query rows (at most 65535)", B, Hq);
    const int cpw = 32 / c->bits;
    GEAR_CHECK_ARG(c->tcap > 0 && c->tcap % 64 == 0 && (int64_t)c->ldk * cpw >= c->tcap && (int64_t)c->lsk * 64 >= c->tcap,
                   "gear_attn_decode_kivi: tcap %d must be a positive multiple of 64 covered by the K pitches (ldk %d, lsk %d)", c->tcap,
                   c->ldk, c->lsk);
    GEAR_CHECK_ARG(L > 0, "gear_attn_decode_kivi: L = %d tokens", L);
    GEAR_CHECK_ARG(Nv >= 0 && Nv <= L && Nv <= c->tcap, "gear_attn_decode_kivi: Nv = %d packed V rows, must lie in [0, min(L = %d, "
                   "tcap = %d)]", Nv, L, c->tcap);
    GEAR_CHECK_ARG(L - Nv <= R + 1, "gear_attn_decode_kivi: L - Nv = %d fp16 V rows, the ring holds R + 1 = %d", L - Nv, R + 1);
    GEAR_CHECK_ARG(Tk >= 0 && Tk % R == 0, "gear_attn_decode_kivi: Tk = %d packed K tokens, Tk %% R != 0 (R = %d)", Tk, R);
    GEAR_CHECK_ARG(Tk <= L && L - Tk <= R && Tk <= c->tcap, "gear_attn_decode_kivi: Tk = %d packed K tokens of L = %d: the K window "
                   "holds at most R = %d, the cache tcap = %d", Tk, L, R, c->tcap);
    const int T0 = Nv & ~63;
    GEAR_CHECK_ARG(T0 <= Tk, "gear_attn_decode_kivi: the packed V chunks [0, %d) need packed K (Tk = %d)", T0, Tk);
    GEAR_CHECK_ARG(q && out, "gear_attn_decode_kivi: null q / out");
    GEAR_CHECK_ARG(Tk == 0 || (c->kcode && c->kscale && c->kmn), "gear_attn_decode_kivi: packed K missing");
    GEAR_CHECK_ARG(Nv == 0 || (c->vcode && c->vscale && c->vmn), "gear_attn_decode_kivi: packed V missing");
    GEAR_CHECK_ARG((L == Tk || c->kwin) && (L == Nv || c->vwin), "gear_attn_decode_kivi: K window / V ring missing");
    const size_t need = gear_attn_decode_kivi_workspace(B, Hq, T0, c->bits);
    GEAR_CHECK_ARG(workspace && workspace_bytes >= need, "gear_attn_decode_kivi: workspace of %zu bytes, needs %zu "
                   "(gear_attn_decode_kivi_workspace)", workspace_bytes, need);
    gear_attn_partials pt;
    pt.part_o = pt.part_ml = nullptr;
    pt.pslots = 0;
    if (T0 > 0) {
        const int rc = gear_attn_partials_dense(c, q, Hq, T0, qscale, workspace, workspace_bytes, stream, &pt);
        if (rc != 0) return rc;
        GEAR_CHECK_ARG(pt.pslots <= KS_MAX, "gear_attn_decode_kivi: %d partial slots (at most %d)", pt.pslots, KS_MAX);
    }
    KiviSeam v;
    v.q = (const uint16_t*)q;
    v.po = pt.part_o; v.ml = pt.part_ml; v.ns = pt.pslots;
    v.kcode = (const uint32_t*)c->kcode; v.kscale = (const uint16_t*)c->kscale; v.kmn = (const uint16_t*)c->kmn;
    v.ldk = c->ldk; v.lsk = c->lsk;
    v.vcode = (const uint32_t*)c->vcode; v.vscale = (const uint16_t*)c->vscale; v.vmn = (const uint16_t*)c->vmn;
    v.tcap = c->tcap;
    v.kwin = (const uint16_t*)c->kwin; v.vring = (const uint16_t*)c->vwin;
    v.R = R; v.Hq = Hq; v.Hkv = Hkv;
    v.L = L; v.Tk = Tk; v.Nv = Nv; v.T0 = T0;
    v.qscale = qscale;
    v.out = (uint16_t*)out;
    v.lse = (float*)lse;
    const dim3 grid((unsigned)((int64_t)B * Hq));
    if (c->bits == 2) hipLaunchKernelGGL(kivi_seam_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, v);
    else hipLaunchKernelGGL(kivi_seam_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, v);
    GEAR_CHECK_LAUNCH("gear_attn_decode_kivi(seam)");
    return 0;
}
