// sample.hip -- token selection for the decoders in ONE launch (gfx950): temperature, top-k, top-p, a counter-based draw and the
// accept / residual rule of speculative sampling with a one-hot (deterministic) drafter.
//
// One 1024-thread workgroup per logits row.  Thread t owns a contiguous run of elements (index order matters for the draw).  The
// order keys are read from memory once and kept: in registers up to 4096 columns, in LDS up to 32768 (runs padded to an odd pitch,
// so that the lanes' run walks hit distinct banks); beyond that every pass re-reads the run (L2-resident: a 128256-column fp16 row
// is 250 KiB).  Passes over a row:
//   1. order keys of x = fp32(logit) / temperature (-0 folded into +0; -inf and padding = key 0 = never kept) and the block max
//      (key, first index) -- that is also the greedy answer;
//   2. top-k: radix select of the k-th largest key, 4 x 8-bit digits, integer counts in an LDS histogram;
//   3. top-p: the same radix descent over the masses e = exp(x - max) as 32.32 fixed-point integers (uint64 LDS histogram);
//   4. the draw: per-thread fixed-point sums, a block exclusive scan, and the one thread whose run holds the crossing of u * Z
//      walks its run.
// Every sum is an integer sum (LDS integer atomics and shuffles), so results are bit-identical from run to run whatever the order
// of arrival; there are no float atomics.  A 32.32 mass differs from the exact term by at most 2^-33 of the row's largest term.
#include <math.h>

#include "common.h"

namespace {

constexpr int SNT = 1024;              // threads per row
constexpr int SNW = SNT / GEAR_WAVE;   // waves per row
constexpr int S_REG = 4;               // register-resident elements per thread (V <= 4096)
constexpr int S_LDS_MAX = 32;          // LDS-resident elements per thread (V <= 32768: 132 KiB of keys)
constexpr int S_V_MAX = 262144;

// ------------------------------------------------------------------------------------------------- Philox4x32-10 (Random123)
struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += W0;
        k1 += W1;
    }
    return c;
}

// u = (out[0] >> 8) * 2^-24 of counter (P, b, purpose, 0), key (seed lo, seed hi)
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint32_t P, uint32_t b, uint32_t purpose) {
    const U4 o = philox4x32_10(U4{P, b, purpose, 0u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (float)(o.x >> 8) * 5.9604644775390625e-08f;
}

// ------------------------------------------------------------------------------------------------- order keys, masses
// Monotone map fp32 -> uint32 (a < b  <=>  key(a) < key(b)); -0 is folded into +0 so that equal values share a key.  Valid keys are
// >= 0x00800000 (that of -FLT_MAX); -inf gets 0.
__device__ __forceinline__ uint32_t order_key(float x) {
    uint32_t u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;
    const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return x == -INFINITY ? 0u : k;
}
__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
// exp(x - max) as a 32.32 fixed-point integer (x <= max, so the value is <= 2^32; a row of 2^18 terms sums to <= 2^50, exact in
// a double)
__device__ __forceinline__ unsigned long long fixed_mass(float x, float xmax) {
    const float dx = x - xmax;                  // exp(dx) < 2^-33 below -33 ln 2 = -22.87: the mass rounds to 0
    return dx < -23.0f ? 0ull : (unsigned long long)rintf(ldexpf(expf(dx), 32));
}

struct SampleSmem {
    uint32_t hist[256];
    unsigned long long hist64[256];
    unsigned long long red64[SNW];
    unsigned long long bcast64;
    uint32_t bcast;
    int tok;
};

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < GEAR_WAVE; o <<= 1) {
        const T n = __shfl_up(v, o);
        if (lane >= o) v += n;
    }
    return v;
}

__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, SampleSmem& sm, int lane, int wave) {
#pragma unroll
    for (int o = GEAR_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                       // red64 may still be read by the previous reduction
    if (lane == 0) sm.red64[wave] = v;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < SNW; ++w) s += sm.red64[w];
    return s;
}

// max over (key << 32 | ~index): the largest key, the first index among equal keys (torch.argmax)
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, SampleSmem& sm, int lane, int wave) {
#pragma unroll
    for (int o = GEAR_WAVE / 2; o > 0; o >>= 1) {
        const unsigned long long n = __shfl_xor(v, o);
        v = n > v ? n : v;
    }
    __syncthreads();
    if (lane == 0) sm.red64[wave] = v;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < SNW; ++w) s = sm.red64[w] > s ? sm.red64[w] : s;
    return s;
}

// Wave 0 walks the 256 bins of `hist` from the top (bin 255) down to the first bin whose inclusive running total reaches `target`:
// bcast = that bin (0xFFFFFFFF: none), bcast64 = the total of the bins above it.
template <typename T, typename TT>
__device__ __forceinline__ void find_crossing(const T* hist, TT target, SampleSmem& sm, int lane, int wave) {
    if (wave != 0) return;
    T v[4];
    T tot = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[q] = hist[255 - 4 * lane - q];
        tot += v[q];
    }
    const T incl = wave_incl_scan(tot, lane);
    const unsigned long long m = __ballot((TT)incl >= target);
    if (m == 0) {
        if (lane == 0) sm.bcast = 0xFFFFFFFFu;
        return;
    }
    if (lane == __ffsll((unsigned long long)m) - 1) {
        T c = incl - tot;
        for (int q = 0; q < 4; ++q) {
            if ((TT)(c + v[q]) >= target) {
                sm.bcast = (uint32_t)(255 - 4 * lane - q);
                sm.bcast64 = (unsigned long long)c;
                break;
            }
            c += v[q];
        }
    }
}

struct SampleArgs {
    const void* logits;
    int fp32, V, chunk;
    int64_t ld;
    int n_per_seq;
    float temperature;
    int top_k;
    float top_p;
    uint64_t seed;
    const int* pos_dev;
    int pos0;
    const int64_t* draft;
    const float* u;
    int64_t* token_out;
    int32_t* accepted_out;
    float* logprob_out;
};

__device__ __forceinline__ float load_logit(const SampleArgs& a, int64_t row, int i) {
    return a.fp32 ? ((const float*)a.logits)[row * a.ld + i] : h2f_bits(((const uint16_t*)a.logits)[row * a.ld + i]);
}

// NPER > 0: each thread's run of NPER elements is held in registers; NPER < 0: the runs of a.chunk elements are held in LDS
// (dynamic, SNT x pitch words); NPER == 0: the run is re-read every pass.
template <int NPER>
__global__ __launch_bounds__(SNT) void sample_tokens_kernel(SampleArgs a) {
    __shared__ SampleSmem sm;
    extern __shared__ uint32_t skeys[];
    const int tid = threadIdx.x, lane = tid % GEAR_WAVE, wave = tid / GEAR_WAVE;
    const int64_t row = blockIdx.x;
    const int n = NPER > 0 ? NPER : a.chunk;
    const int i0 = tid * n;
    const bool greedy = a.temperature == 0.0f;

    auto key_at = [&](int j) -> uint32_t {        // order key of element i0 + j (0 past the row)
        const int i = i0 + j;
        if (i >= a.V) return 0u;
        const float l = load_logit(a, row, i);
        return order_key(greedy ? l : l / a.temperature);
    };
    uint32_t kr[NPER > 0 ? NPER : 1];
    const int pitch = n | 1;
    if constexpr (NPER > 0) {
        for (int j = 0; j < NPER; ++j) kr[j] = key_at(j);
    } else if constexpr (NPER < 0) {
        float l[S_LDS_MAX];                               // coalesced reads, all in flight at once; element i -> run i / n, slot i % n
#pragma unroll
        for (int q = 0; q < S_LDS_MAX; ++q) {
            const int i = q * SNT + tid;
            l[q] = (q < n && i < a.V) ? load_logit(a, row, i) : -INFINITY;
        }
#pragma unroll
        for (int q = 0; q < S_LDS_MAX; ++q) {
            const int i = q * SNT + tid, t = i / n;
            if (q < n) skeys[t * pitch + (i - t * n)] = order_key(greedy ? l[q] : l[q] / a.temperature);
        }
        __syncthreads();
    }
    auto KEY = [&](int j) -> uint32_t {
        if constexpr (NPER > 0) return kr[j];
        else if constexpr (NPER < 0) return skeys[tid * pitch + j];
        else return key_at(j);
    };
    // body(j, key) over the run, SB keys fetched before any is used (the LDS / L2 reads of a batch are in flight together)
    constexpr int SB = NPER > 0 ? NPER : (NPER < 0 ? 8 : 16);
    auto each = [&](auto&& body) {
        for (int j0 = 0; j0 < n; j0 += SB) {
            uint32_t kb[SB];
#pragma unroll
            for (int q = 0; q < SB; ++q) kb[q] = j0 + q < n ? KEY(j0 + q) : 0u;
#pragma unroll
            for (int q = 0; q < SB; ++q)
                if (j0 + q < n) body(j0 + q, kb[q]);
        }
    };

    // ---- 1. the largest key, first index
    unsigned long long best = 0;
    each([&](int j, uint32_t k) {
        const unsigned long long c = ((unsigned long long)k << 32) | (0xFFFFFFFFu - (uint32_t)(i0 + j));
        best = (k != 0u && c > best) ? c : best;
    });
    best = block_max_u64(best, sm, lane, wave);
    const int arg = best ? (int)(0xFFFFFFFFu - (uint32_t)best) : 0;
    const float xmax = key_value((uint32_t)(best >> 32));

    const int64_t d = a.draft ? a.draft[row] : -1;
    if (greedy) {
        if (tid == 0) {
            a.token_out[row] = arg;
            if (a.accepted_out) a.accepted_out[row] = d == (int64_t)arg ? 1 : 0;
            if (a.logprob_out) a.logprob_out[row] = 0.0f;
        }
        return;
    }

    // ---- 2. top-k: keep every key >= the k-th largest (ties at the edge all kept)
    uint32_t thr = 1u;                                     // kept: key >= thr (excludes -inf)
    if (a.top_k > 0) {
        uint32_t prefix = 0u, mask = 0u, remaining = (uint32_t)a.top_k;
        bool on = true;
        for (int shift = 24; shift >= 0 && on; shift -= 8) {
            for (int i = tid; i < 256; i += SNT) sm.hist[i] = 0u;
            __syncthreads();
            each([&](int, uint32_t k) {
                if (k != 0u && (k & mask) == prefix) atomicAdd(&sm.hist[(k >> shift) & 255u], 1u);
            });
            __syncthreads();
            find_crossing<uint32_t, uint32_t>(sm.hist, remaining, sm, lane, wave);
            __syncthreads();
            const uint32_t bin = sm.bcast;
            if (bin == 0xFFFFFFFFu) {
                on = false;                               // fewer than k finite logits: all of them stay
            } else {
                prefix |= bin << shift;
                mask |= 255u << shift;
                remaining -= (uint32_t)sm.bcast64;
            }
            __syncthreads();
        }
        if (on) thr = prefix;
    }

    // ---- 3. top-p over the tokens kept so far: keep x_i iff the mass of the kept values > x_i is < top_p
    if (a.top_p < 1.0f) {
        unsigned long long z = 0;
        each([&](int, uint32_t k) { z += k >= thr ? fixed_mass(key_value(k), xmax) : 0ull; });
        z = block_sum_u64(z, sm, lane, wave);
        const double target = (double)a.top_p * (double)z;
        uint32_t prefix = 0u, mask = 0u;
        double above = 0.0;
        bool found = true;
        for (int shift = 24; shift >= 0 && found; shift -= 8) {
            for (int i = tid; i < 256; i += SNT) sm.hist64[i] = 0ull;
            __syncthreads();
            each([&](int, uint32_t k) {
                if (k >= thr && (k & mask) == prefix) atomicAdd(&sm.hist64[(k >> shift) & 255u], fixed_mass(key_value(k), xmax));
            });
            __syncthreads();
            find_crossing<unsigned long long, double>(sm.hist64, target - above, sm, lane, wave);
            __syncthreads();
            const uint32_t bin = sm.bcast;
            if (bin == 0xFFFFFFFFu) {
                found = false;                            // unreachable (the kept total is >= top_p * Z): keep the top-k set
            } else {
                prefix |= bin << shift;
                mask |= 255u << shift;
                above += (double)sm.bcast64;
            }
            __syncthreads();
        }
        if (found && prefix > thr) thr = prefix;
    }

    // ---- 4. the kept masses, the accept test of a draft, the draw
    unsigned long long s = 0;
    each([&](int, uint32_t k) { s += k >= thr ? fixed_mass(key_value(k), xmax) : 0ull; });
    const unsigned long long Z = block_sum_u64(s, sm, lane, wave);
    const double logZ = log(ldexp((double)Z, -32));
    const int b = (int)(row / a.n_per_seq);
    const int pos = a.pos0 + (a.pos_dev ? a.pos_dev[0] : 0);
    const uint32_t P = (uint32_t)(pos + (int)(row % a.n_per_seq));
    unsigned long long ed = 0;                             // e_d (0 when d is not kept)
    float xd = 0.0f;
    if (d >= 0 && d < a.V) {
        const uint32_t k = order_key(load_logit(a, row, (int)d) / a.temperature);
        xd = key_value(k);
        ed = (k != 0u && k >= thr) ? fixed_mass(xd, xmax) : 0ull;
    }
    if (d >= 0) {
        const float u_acc = a.u ? a.u[2 * row + 1] : philox_uniform(a.seed, P, (uint32_t)b, 1u);
        if ((double)u_acc * (double)Z < (double)ed) {     // accept with probability p(d) = e_d / Z
            if (tid == 0) {
                a.token_out[row] = d;
                if (a.accepted_out) a.accepted_out[row] = 1;
                if (a.logprob_out) a.logprob_out[row] = (float)(((double)xd - (double)xmax) - logZ);
            }
            return;
        }
    }
    // no draft, or rejected: the draw over the kept set without d (Z' = Z - e_d)
    const float u_draw = a.u ? a.u[2 * row] : philox_uniform(a.seed, P, (uint32_t)b, 0u);
    if (d >= i0 && d < i0 + n) s -= ed;
    const double t = (double)u_draw * (double)(Z - ed);
    const unsigned long long incl = wave_incl_scan(s, lane);   // block exclusive scan of the run sums (integers: order-free)
    __syncthreads();
    if (lane == GEAR_WAVE - 1) sm.red64[wave] = incl;
    if (tid == 0) sm.tok = -1;
    __syncthreads();
    unsigned long long excl = incl - s;
    for (int w = 0; w < wave; ++w) excl += sm.red64[w];
    if (s != 0 && (double)excl <= t && t < (double)(excl + s)) {     // exactly one run holds the first C_i > t
        unsigned long long c = excl;
        int tok = -1;
        each([&](int j, uint32_t k) {                   // no early exit: kr[] must stay statically indexed (registers)
            if (tok < 0 && (int64_t)(i0 + j) != d && k >= thr) {
                c += fixed_mass(key_value(k), xmax);
                if ((double)c > t) tok = i0 + j;
            }
        });
        sm.tok = tok;
    }
    __syncthreads();
    if (tid == 0) {
        const int tok = sm.tok >= 0 ? sm.tok : arg;
        a.token_out[row] = tok;
        if (a.accepted_out) a.accepted_out[row] = 0;
        if (a.logprob_out)
            a.logprob_out[row] = (float)(((double)key_value(order_key(load_logit(a, row, tok) / a.temperature)) - (double)xmax) - logZ);
    }
}

}  // namespace

extern "C" int gear_sample_tokens(const void* logits, int logits_fp32, int rows, int V, int64_t ld, int n_per_seq,
                                  const gear_sample_params* p, const int* pos_dev, int pos0, const int64_t* draft, const float* u,
                                  int64_t* token_out, int32_t* accepted_out, float* logprob_out, void* stream) {
    GEAR_CHECK_ARG(p, "gear_sample_tokens: null params");
    GEAR_CHECK_ARG(logits && token_out, "gear_sample_tokens: null logits / token_out pointer");
    GEAR_CHECK_ARG(V >= 1 && V <= S_V_MAX, "gear_sample_tokens: V = %d outside [1, %d]", V, S_V_MAX);
    GEAR_CHECK_ARG(rows >= 1 && rows <= (1 << 24), "gear_sample_tokens: rows = %d outside [1, 2^24]", rows);
    GEAR_CHECK_ARG(ld >= V, "gear_sample_tokens: row stride ld = %lld < V = %d", (long long)ld, V);
    GEAR_CHECK_ARG(n_per_seq >= 1, "gear_sample_tokens: n_per_seq = %d < 1", n_per_seq);
    GEAR_CHECK_ARG(p->temperature >= 0.0f && isfinite(p->temperature), "gear_sample_tokens: temperature = %g must be finite and >= 0",
                   (double)p->temperature);
    GEAR_CHECK_ARG(p->top_k >= 0, "gear_sample_tokens: top_k = %d < 0", p->top_k);
    GEAR_CHECK_ARG(p->top_p > 0.0f && p->top_p <= 1.0f, "gear_sample_tokens: top_p = %g outside (0, 1]", (double)p->top_p);
    SampleArgs a;
    a.logits = logits;
    a.fp32 = logits_fp32 ? 1 : 0;
    a.V = V;
    a.chunk = (V + SNT - 1) / SNT;
    a.ld = ld;
    a.n_per_seq = n_per_seq;
    a.temperature = p->temperature;
    a.top_k = p->top_k >= V ? 0 : p->top_k;
    a.top_p = p->top_p;
    a.seed = p->seed;
    a.pos_dev = pos_dev;
    a.pos0 = pos0;
    a.draft = draft;
    a.u = u;
    a.token_out = token_out;
    a.accepted_out = accepted_out;
    a.logprob_out = logprob_out;
    const hipStream_t st = (hipStream_t)stream;
    if (a.chunk <= S_REG) {
        hipLaunchKernelGGL(sample_tokens_kernel<S_REG>, dim3((unsigned)rows), dim3(SNT), 0, st, a);
    } else if (a.chunk <= S_LDS_MAX) {
        const size_t shmem = (size_t)SNT * (a.chunk | 1) * sizeof(uint32_t);
        static bool attr_set = false;      // (idempotent; set once for the largest size)
        if (!attr_set) {
            (void)hipFuncSetAttribute((const void*)sample_tokens_kernel<-1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)((size_t)SNT * (S_LDS_MAX | 1) * sizeof(uint32_t)));
            attr_set = true;
        }
        hipLaunchKernelGGL(sample_tokens_kernel<-1>, dim3((unsigned)rows), dim3(SNT), shmem, st, a);
    } else
        hipLaunchKernelGGL(sample_tokens_kernel<0>, dim3((unsigned)rows), dim3(SNT), 0, st, a);
    GEAR_CHECK_LAUNCH("gear_sample_tokens");
    return 0;
}
