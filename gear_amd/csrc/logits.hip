// logits.hip -- the logits processors of the decoders in ONE launch (gfx950): logit bias / token bans, repetition penalty, n-gram ban
// and the minimum-length EOS ban, in HF's processor order (gear_logits_process), and the per-sequence EOS bookkeeping
// (gear_eos_update).  Semantics: include/gear_hip.h.
//
// gear_logits_process: one 1024-thread workgroup per row, three bitmaps of V bits in LDS (seen / banned / biased):
//   1. one lane stores the token just fed at hist[n - 1] (plain vector store), the bitmaps are cleared, barrier;
//   2. the history marks `seen` (atomicOr: a token that fills the history 500 times sets one bit), every n-gram start whose g - 1
//      tokens equal the history's last g - 1 marks the token behind it in `banned`, as do the EOS ids below the minimum length; the
//      bias table marks `biased`; barrier;
//   3. the row streams through once, 16 bytes per access when input and output rows start on a 16-byte boundary (narrower
//      accesses otherwise: same columns, same bits).  A vector without a marked bit is copied as it is (skipped when out == logits);
//      a marked entry becomes fp32, takes the penalty (x < 0 ? x p : x / p, IEEE division) and / or -inf and is rounded once;
//   4. the entries with a bias belong to the bias pass alone (the stream never reads or writes them): one thread per pair computes
//      fp32(logit) + bias, then the penalty / ban its bits ask for, one rounding.
// No entry is written by two threads and none is read after another thread wrote it, so out == logits needs no ordering between
// the passes; every value is a function of the row, its history and the parameters alone: the same bits from run to run.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int LG_NT = 1024;
constexpr int LG_V_MAX = 262144;
constexpr int LG_EOS_MAX = 8;

struct LgBias {
    int32_t tok;
    float bias;
};

struct LgArgs {
    const void* x;
    void* y;
    int V;
    int64_t ld, ldo;
    int32_t* hist;
    int hist_cap;
    const int* pos_dev;
    int pos0;
    const int64_t* cur;
    int prompt_len;
    float p;
    int g, min_new, n_eos;
    int eos[LG_EOS_MAX];
    int n_bias;
    const LgBias* bias;
};

__device__ __forceinline__ float lg_ld(uint16_t v) { return h2f_bits(v); }
__device__ __forceinline__ float lg_ld(float v) { return v; }
template <typename T>
__device__ __forceinline__ T lg_st(float v);
template <>
__device__ __forceinline__ uint16_t lg_st<uint16_t>(float v) { return f2h_bits(v); }
template <>
__device__ __forceinline__ float lg_st<float>(float v) { return v; }

// 16 bytes of a row: on a 16-byte boundary, or only element-aligned (the compiler picks the widest accesses that alignment allows)
template <typename T>
struct alignas(16) LgVecA {
    T e[16 / sizeof(T)];
};
template <typename T>
struct __attribute__((packed, aligned(sizeof(T)))) LgVecU {
    T e[16 / sizeof(T)];
};

// penalty, then ban, of one entry whose fp32 value (bias included) is v; one rounding
template <typename T>
__device__ __forceinline__ T lg_apply(float v, bool seen, bool ban, float p) {
    if (seen) v = v < 0.0f ? v * p : div_rn(v, p);
    if (ban) v = -INFINITY;
    return lg_st<T>(v);
}

template <typename T, typename VEC>
__device__ __forceinline__ void lg_stream(const T* x, T* y, int V, bool inplace, const uint32_t* seen,
                                          const uint32_t* ban, const uint32_t* biased, float p, int tid) {
    constexpr int E = 16 / sizeof(T);
    constexpr uint32_t M = (1u << E) - 1u;
    const int nvec = V / E;
    for (int v = tid; v < nvec; v += LG_NT) {
        const int base = v * E, w = base >> 5, sh = base & 31;          // E divides 32: a vector's bits lie in one word
        const uint32_t s = (seen[w] >> sh) & M, bn = (ban[w] >> sh) & M, bi = (biased[w] >> sh) & M;
        const uint32_t touched = s | bn;
        if (!(touched | bi)) {
            if (!inplace) ((VEC*)y)[v] = ((const VEC*)x)[v];
            continue;
        }
        VEC in = ((const VEC*)x)[v];
        if (!bi) {
#pragma unroll
            for (int e = 0; e < E; ++e)
                if ((touched >> e) & 1u) in.e[e] = lg_apply<T>(lg_ld(in.e[e]), (s >> e) & 1u, (bn >> e) & 1u, p);
            ((VEC*)y)[v] = in;
        } else {                                                          // entries with a bias are the bias pass's alone
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if ((bi >> e) & 1u) continue;
                if ((touched >> e) & 1u) y[base + e] = lg_apply<T>(lg_ld(in.e[e]), (s >> e) & 1u, (bn >> e) & 1u, p);
                else if (!inplace) y[base + e] = in.e[e];
            }
        }
    }
    for (int i = nvec * E + tid; i < V; i += LG_NT) {                     // the V % E columns behind the last whole vector
        const uint32_t bit = 1u << (i & 31);
        const bool s = seen[i >> 5] & bit, bn = ban[i >> 5] & bit;
        if (biased[i >> 5] & bit) continue;
        if (s || bn) y[i] = lg_apply<T>(lg_ld(x[i]), s, bn, p);
        else if (!inplace) y[i] = x[i];
    }
}

template <typename T>
__global__ __launch_bounds__(LG_NT) void logits_process_kernel(LgArgs a) {
    extern __shared__ uint32_t lg_bits[];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int V = a.V, W = (V + 31) >> 5;
    uint32_t *seen = lg_bits, *ban = lg_bits + W, *biased = lg_bits + 2 * W;
    const T* x = (const T*)a.x + row * a.ld;
    T* y = (T*)a.y + row * a.ldo;
    int32_t* h = a.hist + row * (int64_t)a.hist_cap;
    int64_t n64 = (int64_t)a.pos0 + (a.pos_dev ? (int64_t)a.pos_dev[0] : 0);
    n64 = n64 < 0 ? 0 : (n64 > (int64_t)a.hist_cap ? (int64_t)a.hist_cap : n64);
    const int n = (int)n64;

    // ---- 1. the token just fed becomes entry n - 1 (this launch reads that entry from `cur`, later launches from memory)
    const bool have_cur = a.cur != nullptr && n >= 1;
    int32_t curtok = -1;
    if (have_cur) {
        const int64_t c = a.cur[row];
        curtok = (c < (int64_t)INT_MIN || c > (int64_t)INT_MAX) ? -1 : (int32_t)c;
        if (tid == 0) h[n - 1] = curtok;
    }
    for (int i = tid; i < 3 * W; i += LG_NT) lg_bits[i] = 0u;
    __syncthreads();
    auto H = [&](int i) -> int32_t { return (have_cur && i == n - 1) ? curtok : h[i]; };
    auto mark = [&](uint32_t* bits, int32_t t) {
        if (t >= 0 && t < V) atomicOr(&bits[t >> 5], 1u << (t & 31));
    };

    // ---- 2. the bitmaps
    if (a.p != 1.0f)
        for (int i = tid; i < n; i += LG_NT) mark(seen, H(i));
    const int g = a.g;
    if (g > 0 && n >= g) {
        const int tail = n - g + 1;                                       // the last g - 1 tokens start here
        for (int i = tid; i <= n - g; i += LG_NT) {
            bool same = true;
            for (int k = 0; k < g - 1 && same; ++k) same = H(i + k) == H(tail + k);
            if (same) mark(ban, H(i + g - 1));
        }
    }
    if ((int64_t)n - (int64_t)a.prompt_len < (int64_t)a.min_new && tid == 0) {
#pragma unroll
        for (int k = 0; k < LG_EOS_MAX; ++k)
            if (k < a.n_eos) mark(ban, a.eos[k]);
    }
    for (int i = tid; i < a.n_bias; i += LG_NT) mark(biased, a.bias[i].tok);
    __syncthreads();

    // ---- 3. the row, once
    const bool inplace = (const void*)x == (const void*)y;
    const bool aligned = ((((uintptr_t)x) | ((uintptr_t)y)) & 15u) == 0;      // (uniform over the workgroup)
    if (aligned)
        lg_stream<T, LgVecA<T>>(x, y, V, inplace, seen, ban, biased, a.p, tid);
    else
        lg_stream<T, LgVecU<T>>(x, y, V, inplace, seen, ban, biased, a.p, tid);

    // ---- 4. the entries with a bias
    for (int i = tid; i < a.n_bias; i += LG_NT) {
        const LgBias b = a.bias[i];
        if (b.tok < 0 || b.tok >= V) continue;
        const uint32_t bit = 1u << (b.tok & 31);
        y[b.tok] = lg_apply<T>(lg_ld(x[b.tok]) + b.bias, seen[b.tok >> 5] & bit, ban[b.tok >> 5] & bit, a.p);
    }
}

constexpr int EOS_NT = 256;

struct EosArgs {
    int64_t* tok;
    int32_t* done;
    int B, n_eos;
    int eos[LG_EOS_MAX];
    int64_t pad;
    int32_t* n_done;
};

__global__ __launch_bounds__(EOS_NT) void eos_update_kernel(EosArgs a) {
    __shared__ int red[EOS_NT / GEAR_WAVE];
    const int tid = threadIdx.x, lane = tid % GEAR_WAVE, wave = tid / GEAR_WAVE;
    int cnt = 0;
    for (int b = tid; b < a.B; b += EOS_NT) {
        int d = a.done[b] != 0;
        if (d) {
            a.tok[b] = a.pad;
        } else {
            const int64_t t = a.tok[b];
            bool hit = false;
#pragma unroll
            for (int k = 0; k < LG_EOS_MAX; ++k) hit = hit || (k < a.n_eos && t == (int64_t)a.eos[k]);
            if (hit) {
                a.done[b] = 1;                                            // (the EOS token itself stays)
                d = 1;
            }
        }
        cnt += d;
    }
#pragma unroll
    for (int o = GEAR_WAVE / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < EOS_NT / GEAR_WAVE; ++w) s += red[w];         // wave order
        a.n_done[0] = s;
    }
}

}  // namespace

extern "C" int gear_logits_process(const void* logits, void* out, int logits_fp32, int B, int V, int64_t ld, int64_t ld_out,
                                   int32_t* hist, int hist_cap, const int* pos_dev, int pos0, const int64_t* cur, int prompt_len,
                                   const gear_logits_params* p, void* stream) {
    GEAR_CHECK_ARG(p, "gear_logits_process: null params");
    GEAR_CHECK_ARG(logits && out && hist, "gear_logits_process: null logits / out / hist pointer");
    GEAR_CHECK_ARG(V >= 1 && V <= LG_V_MAX, "gear_logits_process: V = %d outside [1, %d]", V, LG_V_MAX);
    GEAR_CHECK_ARG(B >= 0, "gear_logits_process: B = %d < 0", B);
    GEAR_CHECK_ARG(ld >= V && ld_out >= V, "gear_logits_process: row pitch ld = %lld / ld_out = %lld < V = %d", (long long)ld,
                   (long long)ld_out, V);
    GEAR_CHECK_ARG(p->repetition_penalty > 0.0f && isfinite(p->repetition_penalty),
                   "gear_logits_process: repetition_penalty = %g must be finite and > 0", (double)p->repetition_penalty);
    GEAR_CHECK_ARG(p->no_repeat_ngram >= 0, "gear_logits_process: no_repeat_ngram = %d < 0", p->no_repeat_ngram);
    GEAR_CHECK_ARG(p->min_new_tokens >= 0, "gear_logits_process: min_new_tokens = %d < 0", p->min_new_tokens);
    GEAR_CHECK_ARG(p->n_eos >= 0 && p->n_eos <= LG_EOS_MAX, "gear_logits_process: n_eos = %d outside [0, %d]", p->n_eos, LG_EOS_MAX);
    GEAR_CHECK_ARG(p->n_bias >= 0, "gear_logits_process: n_bias = %d < 0", p->n_bias);
    GEAR_CHECK_ARG(p->n_bias == 0 || p->bias, "gear_logits_process: n_bias = %d with a null bias table", p->n_bias);
    GEAR_CHECK_ARG(pos0 >= 0, "gear_logits_process: pos0 = %d < 0", pos0);
    GEAR_CHECK_ARG(hist_cap > 0, "gear_logits_process: hist_cap = %d <= 0", hist_cap);
    if (B == 0) return 0;
    LgArgs a;
    a.x = logits;
    a.y = out;
    a.V = V;
    a.ld = ld;
    a.ldo = ld_out;
    a.hist = hist;
    a.hist_cap = hist_cap;
    a.pos_dev = pos_dev;
    a.pos0 = pos0;
    a.cur = cur;
    a.prompt_len = prompt_len;
    a.p = p->repetition_penalty;
    a.g = p->no_repeat_ngram;
    a.min_new = p->min_new_tokens;
    a.n_eos = p->n_eos;
    for (int k = 0; k < LG_EOS_MAX; ++k) a.eos[k] = k < p->n_eos ? p->eos[k] : -1;
    a.n_bias = p->n_bias;
    a.bias = (const LgBias*)p->bias;
    const hipStream_t st = (hipStream_t)stream;
    const size_t shmem = (size_t)3 * ((V + 31) / 32) * sizeof(uint32_t);          // <= 96 KiB
    static bool attr_set = false;      // (idempotent; set once for the largest size)
    if (!attr_set) {
        const int most = 3 * (LG_V_MAX / 32) * (int)sizeof(uint32_t);
        (void)hipFuncSetAttribute((const void*)logits_process_kernel<uint16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
        (void)hipFuncSetAttribute((const void*)logits_process_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
        attr_set = true;
    }
    if (logits_fp32)
        hipLaunchKernelGGL(logits_process_kernel<float>, dim3((unsigned)B), dim3(LG_NT), shmem, st, a);
    else
        hipLaunchKernelGGL(logits_process_kernel<uint16_t>, dim3((unsigned)B), dim3(LG_NT), shmem, st, a);
    GEAR_CHECK_LAUNCH("gear_logits_process");
    return 0;
}

extern "C" int gear_eos_update(int64_t* tok, int32_t* done, int B, const int* eos, int n_eos, int64_t pad, int32_t* n_done,
                               void* stream) {
    GEAR_CHECK_ARG(tok && done && n_done, "gear_eos_update: null tok / done / n_done pointer");
    GEAR_CHECK_ARG(B >= 0, "gear_eos_update: B = %d < 0", B);
    GEAR_CHECK_ARG(n_eos >= 0 && n_eos <= LG_EOS_MAX, "gear_eos_update: n_eos = %d outside [0, %d]", n_eos, LG_EOS_MAX);
    GEAR_CHECK_ARG(n_eos == 0 || eos, "gear_eos_update: n_eos = %d with null ids", n_eos);
    if (B == 0) return 0;
    EosArgs a;
    a.tok = tok;
    a.done = done;
    a.B = B;
    a.n_eos = n_eos;
    for (int k = 0; k < LG_EOS_MAX; ++k) a.eos[k] = k < n_eos ? eos[k] : -1;
    a.pad = pad;
    a.n_done = n_done;
    hipLaunchKernelGGL(eos_update_kernel, dim3(1), dim3(EOS_NT), 0, (hipStream_t)stream, a);
    GEAR_CHECK_LAUNCH("gear_eos_update");
    return 0;
}
