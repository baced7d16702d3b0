// logprob.hip -- scoring in ONE launch (gfx950): the log-prob of a target token per logits row, the row's log-sum-exp, the target's
// rank, the KL divergence against a second set of logits for the same tokens, argmax agreement and the top-k log-probs
// (gear_token_logprobs; semantics: include/gear_hip.h).
//
// One workgroup per row, 256 threads up to 8192 columns and 1024 beyond (a function of V alone).  The row is streamed once, 8 columns
// per load (two loads in flight per thread and matrix): 16-byte loads when the row starts on a 16-byte boundary, narrower ones
// otherwise (an odd pitch) -- same columns, same order, same bits.  Thread t takes vectors t, t + NT, ... so its column indices only
// grow, which is what makes "first seen wins" the lowest-index tie rule.  Per thread a running maximum m and s = sum exp(x - m) (rescaled when a
// vector raises m: one extra exp per vector at most), the count of entries above the target's logit, the best (value, index); with
// ref_logits the same pair for the other row plus t = sum exp(r - m_r) (r - x) -- KL = t / s_r - lse_r + lse_x needs no second pass.
// The partial results merge over the wave by an xor butterfly (the merge is commutative: every lane ends with the same bits), over the
// waves in wave order by thread 0.  No atomics, no workspace.  The final log / subtractions are fp64 on one thread.
// k_top > 1: pass j finds the best entry that comes after pass j - 1's winner in (value descending, index ascending) order -- k_top - 1
// re-reads of a row the workgroup has just pulled through the caches.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int LP_KMAX = 8;
constexpr int LP_V_SMALL = 8192;       // up to here 256 threads per row, beyond 1024
constexpr float LP_LOG2E = 1.4426950408889634f;

struct LpArgs {
    const uint16_t* x;
    const uint16_t* r;
    const int64_t* ids;
    int V, k_top;
    int64_t ld;
    float *lp, *lse, *kl, *top_lp;
    int32_t *rank, *agree, *top_idx;
};

// exp(d) for d <= 0 (-inf -> 0): one v_mul + one v_exp_f32
__device__ __forceinline__ float lp_exp(float d) { return __builtin_amdgcn_exp2f(d * LP_LOG2E); }

// running softmax statistics of one matrix: m = maximum so far (-inf: nothing finite yet), s = sum exp(x - m), t = sum exp(x - m) w
// (w = x - other matrix: the KL numerator; 0 for the scored matrix itself), best = (largest value, its lowest index)
struct LpStat {
    float m, s, t, bv;
    int bi;
};
__device__ __forceinline__ LpStat lp_stat_init() { return LpStat{-INFINITY, 0.0f, 0.0f, -INFINITY, INT_MAX}; }

__device__ __forceinline__ bool lp_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// commutative merge of two partial results (accurate expf: a handful of calls per row)
__device__ __forceinline__ LpStat lp_merge(const LpStat& a, const LpStat& b) {
    LpStat o;
    o.m = fmaxf(a.m, b.m);
    const float ea = a.m == -INFINITY ? 0.0f : expf(a.m - o.m), eb = b.m == -INFINITY ? 0.0f : expf(b.m - o.m);
    o.s = a.s * ea + b.s * eb;
    const float ta = a.t == INFINITY ? a.t : a.t * ea, tb = b.t == INFINITY ? b.t : b.t * eb;
    o.t = ta + tb;
    const bool pa = lp_better(a.bv, a.bi, b.bv, b.bi);
    o.bv = pa ? a.bv : b.bv;
    o.bi = pa ? a.bi : b.bi;
    return o;
}
__device__ __forceinline__ LpStat lp_wave_merge(LpStat v) {
#pragma unroll
    for (int o = GEAR_WAVE / 2; o > 0; o >>= 1) {
        LpStat n;
        n.m = __shfl_xor(v.m, o);
        n.s = __shfl_xor(v.s, o);
        n.t = __shfl_xor(v.t, o);
        n.bv = __shfl_xor(v.bv, o);
        n.bi = __shfl_xor(v.bi, o);
        v = lp_merge(v, n);
    }
    return v;
}

// N consecutive columns i0 .. i0 + N - 1 of one matrix into its statistics; w[e] = the KL weight of column e (KLW)
template <int N, bool KLW>
__device__ __forceinline__ void lp_accum(LpStat& st, const float* f, const float* other, int i0) {
    float cm = f[0];
#pragma unroll
    for (int e = 1; e < N; ++e) cm = fmaxf(cm, f[e]);
    if (cm > st.m) {                                   // (m = -inf: s = t = 0 stay 0)
        const float sc = lp_exp(st.m - cm);
        st.s *= sc;
        if (KLW) st.t = st.t == INFINITY ? st.t : st.t * sc;
        st.m = cm;
    }
    if (cm > st.bv || st.bi == INT_MAX) {              // columns only grow within a thread: the first seen is the lowest index
        int p = 0;
#pragma unroll
        for (int e = N - 1; e >= 0; --e) p = f[e] == cm ? e : p;
        st.bv = cm;
        st.bi = i0 + p;
    }
    const float base = st.m == -INFINITY ? 0.0f : st.m;
    float cs = 0.0f, ct = 0.0f;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const float ex = lp_exp(f[e] - base);
        cs += ex;
        if (KLW) {
            float term = ex * (f[e] - other[e]);
            term = other[e] == -INFINITY ? INFINITY : term;      // the scored row gives this column no mass, the reference does
            term = f[e] == -INFINITY ? 0.0f : term;              // no reference mass: contributes nothing
            ct += term;
        }
    }
    st.s += cs;
    if (KLW) st.t += ct;
}

// 8 fp16 from an address that is only 2-byte aligned (the compiler picks the widest loads the target allows for that alignment)
struct __attribute__((packed, aligned(2))) LpVec2 {
    uint32_t x, y, z, w;
};

// the row walk: whole vectors of 8 columns (two loads in flight), then the V % 8 tail columns.  f(N, fx, fr, i0) sees N = 1 or 8
// consecutive columns from i0 on; a thread's i0 values only grow.  Which thread sees which columns, and in what order, depends on V
// alone -- never on the row's address: ALIGNED (the rows start on a 16-byte boundary) only selects 16-byte loads over narrower ones,
// so a row gives the same bits wherever it lies.
template <int NT, bool REF, bool ALIGNED, typename F>
__device__ __forceinline__ void lp_row_walk(const uint16_t* __restrict__ xrow, const uint16_t* __restrict__ rrow, int V, int tid,
                                            F&& f) {
    using I1 = std::integral_constant<int, 1>;
    using I8 = std::integral_constant<int, 8>;
    float fx[8], fr[8];
    const int nvec = V >> 3;
    auto ld8 = [](const uint16_t* row, int v) -> uint4 {
        if (ALIGNED) return ((const uint4*)row)[v];
        const LpVec2 u = ((const LpVec2*)row)[v];
        return uint4{u.x, u.y, u.z, u.w};
    };
    for (int v = tid; v < nvec; v += 2 * NT) {
        const bool two = v + NT < nvec;
        const uint4 a0 = ld8(xrow, v), a1 = two ? ld8(xrow, v + NT) : a0;
        uint4 b0 = a0, b1 = a0;
        if (REF) {
            b0 = ld8(rrow, v);
            b1 = two ? ld8(rrow, v + NT) : b0;
        }
        unpack8(a0, fx);
        if (REF) unpack8(b0, fr);
        f(I8{}, fx, fr, 8 * v);
        if (two) {
            unpack8(a1, fx);
            if (REF) unpack8(b1, fr);
            f(I8{}, fx, fr, 8 * (v + NT));
        }
    }
    for (int i = 8 * nvec + tid; i < V; i += NT) {
        fx[0] = h2f_bits(xrow[i]);
        if (REF) fr[0] = h2f_bits(rrow[i]);
        f(I1{}, fx, fr, i);
    }
}

template <int NT, bool REF>
__global__ __launch_bounds__(NT) void token_logprobs_kernel(LpArgs a) {
    constexpr int NW = NT / GEAR_WAVE;
    __shared__ LpStat red_x[NW], red_r[NW];
    __shared__ int red_cnt[NW];
    __shared__ float prev_v;
    __shared__ int prev_i;
    const int tid = threadIdx.x, lane = tid % GEAR_WAVE, wave = tid / GEAR_WAVE;
    const int64_t row = blockIdx.x;
    const int V = a.V;
    const uint16_t* xrow = a.x + row * a.ld;
    const uint16_t* rrow = REF ? a.r + row * a.ld : xrow;
    const int64_t id = a.ids[row];
    const bool valid = id >= 0 && id < (int64_t)V;
    const float xt = valid ? h2f_bits(xrow[id]) : INFINITY;      // (the id indexes a read only when it is inside the row)
    const bool aligned = ((((uintptr_t)xrow) | ((uintptr_t)rrow)) & 15u) == 0;       // (uniform over the workgroup)
    LpStat sx = lp_stat_init(), sr = lp_stat_init();
    int cnt = 0;
    auto main_body = [&](auto n, const float* fx, const float* fr, int i0) {
        constexpr int N = decltype(n)::value;
        lp_accum<N, false>(sx, fx, fx, i0);
        if (REF) lp_accum<N, true>(sr, fr, fx, i0);
#pragma unroll
        for (int e = 0; e < N; ++e) cnt += fx[e] > xt ? 1 : 0;
    };
    if (aligned)
        lp_row_walk<NT, REF, true>(xrow, rrow, V, tid, main_body);
    else
        lp_row_walk<NT, REF, false>(xrow, rrow, V, tid, main_body);
    sx = lp_wave_merge(sx);
    if (REF) sr = lp_wave_merge(sr);
#pragma unroll
    for (int o = GEAR_WAVE / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) {
        red_x[wave] = sx;
        if (REF) red_r[wave] = sr;
        red_cnt[wave] = cnt;
    }
    __syncthreads();
    const int k_top = a.k_top;
    double lse_d = 0.0;
    bool dead = false;
    if (tid == 0) {
        sx = red_x[0];
        if (REF) sr = red_r[0];
        cnt = red_cnt[0];
        for (int w = 1; w < NW; ++w) {                 // fixed order
            sx = lp_merge(sx, red_x[w]);
            if (REF) sr = lp_merge(sr, red_r[w]);
            cnt += red_cnt[w];
        }
        dead = sx.m == -INFINITY;                      // nothing finite in the row
        lse_d = dead ? (double)NAN : (double)sx.m + log((double)sx.s);
        float lpv;
        if (id < 0) lpv = 0.0f;
        else if (!valid || dead) lpv = NAN;
        else if (xt == -INFINITY) lpv = -INFINITY;
        else lpv = (float)((double)xt - lse_d);
        a.lp[row] = lpv;
        if (a.lse) a.lse[row] = (float)lse_d;
        if (a.rank) a.rank[row] = valid ? cnt : -1;
        if (REF) {
            if (a.kl) {
                const bool bad = dead || sr.m == -INFINITY;
                a.kl[row] = bad ? NAN
                                : (float)(((double)sr.t / (double)sr.s - ((double)sr.m - (double)sx.m)) -
                                          log((double)sr.s / (double)sx.s));
            }
            if (a.agree) a.agree[row] = sx.bi == sr.bi ? 1 : 0;
        }
        if (k_top > 0) {
            if (a.top_idx) a.top_idx[row * k_top] = sx.bi;
            if (a.top_lp) a.top_lp[row * k_top] = dead ? NAN : sx.bv == -INFINITY ? -INFINITY : (float)((double)sx.bv - lse_d);
            prev_v = sx.bv;
            prev_i = sx.bi;
        }
    }
    // ---- the rest of the top-k: pass j takes the best entry behind pass j - 1's in (value descending, index ascending) order
    for (int j = 1; j < k_top; ++j) {
        __syncthreads();
        const float pv = prev_v;
        const int pi = prev_i;
        float cv = -INFINITY;
        int ci = INT_MAX;
        auto top_body = [&](auto n, const float* fx, const float*, int i0) {
            constexpr int N = decltype(n)::value;
#pragma unroll
            for (int e = 0; e < N; ++e) {
                const float x = fx[e];
                const int i = i0 + e;
                const bool behind = x < pv || (x == pv && i > pi);
                if (behind && (x > cv || ci == INT_MAX)) {
                    cv = x;
                    ci = i;
                }
            }
        };
        if (aligned)
            lp_row_walk<NT, false, true>(xrow, xrow, V, tid, top_body);
        else
            lp_row_walk<NT, false, false>(xrow, xrow, V, tid, top_body);
#pragma unroll
        for (int o = GEAR_WAVE / 2; o > 0; o >>= 1) {
            const float nv = __shfl_xor(cv, o);
            const int ni = __shfl_xor(ci, o);
            const bool take = lp_better(nv, ni, cv, ci);
            cv = take ? nv : cv;
            ci = take ? ni : ci;
        }
        if (lane == 0) {
            red_x[wave].bv = cv;
            red_x[wave].bi = ci;
        }
        __syncthreads();
        if (tid == 0) {
            cv = red_x[0].bv;
            ci = red_x[0].bi;
            for (int w = 1; w < NW; ++w)
                if (lp_better(red_x[w].bv, red_x[w].bi, cv, ci)) {
                    cv = red_x[w].bv;
                    ci = red_x[w].bi;
                }
            if (a.top_idx) a.top_idx[row * k_top + j] = ci;
            if (a.top_lp) a.top_lp[row * k_top + j] = dead ? NAN : cv == -INFINITY ? -INFINITY : (float)((double)cv - lse_d);
            prev_v = cv;
            prev_i = ci;
        }
    }
}

template <int NT>
void lp_launch(const LpArgs& a, int64_t N, hipStream_t st) {
    if (a.r)
        hipLaunchKernelGGL((token_logprobs_kernel<NT, true>), dim3((unsigned)N), dim3(NT), 0, st, a);
    else
        hipLaunchKernelGGL((token_logprobs_kernel<NT, false>), dim3((unsigned)N), dim3(NT), 0, st, a);
}

}  // namespace

extern "C" int gear_token_logprobs(const void* logits, const void* ref_logits, const int64_t* ids, int64_t N, int V, int64_t ld,
                                   int k_top, float* lp, float* lse, int32_t* rank, float* kl, int32_t* agree, int32_t* top_idx,
                                   float* top_lp, void* stream) {
    GEAR_CHECK_ARG(logits && ids && lp, "gear_token_logprobs: null logits / ids / lp pointer");
    GEAR_CHECK_ARG(V > 0, "gear_token_logprobs: V = %d <= 0", V);
    GEAR_CHECK_ARG(N >= 0 && N <= (int64_t)INT_MAX, "gear_token_logprobs: N = %lld outside [0, 2^31 - 1]", (long long)N);
    GEAR_CHECK_ARG(ld >= V, "gear_token_logprobs: row pitch ld = %lld < V = %d", (long long)ld, V);
    GEAR_CHECK_ARG(k_top >= 0 && k_top <= LP_KMAX, "gear_token_logprobs: k_top = %d outside [0, %d]", k_top, LP_KMAX);
    GEAR_CHECK_ARG(k_top <= V, "gear_token_logprobs: k_top = %d > V = %d", k_top, V);
    GEAR_CHECK_ARG(ref_logits || !(kl || agree), "gear_token_logprobs: kl / agree requested without ref_logits");
    if (N == 0) return 0;
    LpArgs a;
    a.x = (const uint16_t*)logits;
    a.r = (const uint16_t*)ref_logits;
    a.ids = ids;
    a.V = V;
    a.k_top = (top_idx || top_lp) ? k_top : 0;
    a.ld = ld;
    a.lp = lp;
    a.lse = lse;
    a.kl = kl;
    a.top_lp = top_lp;
    a.rank = rank;
    a.agree = agree;
    a.top_idx = top_idx;
    const hipStream_t st = (hipStream_t)stream;
    if (V <= LP_V_SMALL)
        lp_launch<256>(a, N, st);
    else
        lp_launch<1024>(a, N, st);
    GEAR_CHECK_LAUNCH("gear_token_logprobs");
    return 0;
}
