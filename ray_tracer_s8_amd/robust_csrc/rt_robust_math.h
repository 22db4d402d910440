// rt_robust_math.h — the per-pixel arithmetic of the robust-film library (rt_robust.h): the fold of a pixel's records
// into its buckets, and the median-of-means estimate of a pixel from its buckets.  Plain C++ that compiles as HIP device code
// (rt_robust.hip.h) and under g++ -ffp-contract=off (tests/host/robust_host.cpp), so the kernels and the CPU harness run the same
// lines.  Every operation is one IEEE f32 rounding in the order rt_robust.h writes it: no fused multiply-add, correctly rounded
// division, no transcendental function.
//
// Every loop over buckets is marked RTR_UNROLL: the build has -fno-unroll-loops, and a per-lane array that a loop indexes at run time
// goes to scratch memory.  Unrolled, every m, y, key and rank below is a register of its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HOST_DEVICE __host__ __device__ inline
#else
#define RT_HOST_DEVICE inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define RTR_UNROLL _Pragma("unroll")
#else
#define RTR_UNROLL
#endif

namespace rtrm {

constexpr uint32_t MIN_BUCKETS = 3u, MAX_BUCKETS = 15u;
constexpr uint32_t MODE_GINI = 0u, MODE_TRIM = 1u;

constexpr bool buckets_ok(uint32_t K) { return K >= MIN_BUCKETS && K <= MAX_BUCKETS && (K & 1u) != 0u; }

// ---- the fold -----------------------------------------------------------------------------------------------------------------------
// The records of pixel p, rec[n][3] (record j is sample first + j), into the pixel's entries of the K buckets, B + k stride.  Per
// bucket a sample of the call falls into: one load, the bucket's samples in ascending order, one store.
RT_HOST_DEVICE void fold_pixel(const float* rec, uint32_t n, uint32_t first_mod_K, uint32_t K, float* B, size_t stride) {
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t j0 = k >= first_mod_K ? k - first_mod_K : k + K - first_mod_K;      // the first record of bucket k
        if (j0 >= n) continue;
        float* b = B + (size_t)k * stride;
        float s0 = b[0], s1 = b[1], s2 = b[2];
        for (uint32_t j = j0; j < n; j += K) {
            s0 += rec[3 * (size_t)j + 0];
            s1 += rec[3 * (size_t)j + 1];
            s2 += rec[3 * (size_t)j + 2];
        }
        b[0] = s0, b[1] = s1, b[2] = s2;
    }
}

// ---- the estimate -------------------------------------------------------------------------------------------------------------------
// What is uniform over a call: the count and its split over the buckets, the mode and the caller's width.
struct Call {
    uint32_t q, rem;              // e div K, e mod K
    float e_f;                    // (float)e
    uint32_t mode, c;
};

inline Call make_call(uint32_t K, uint32_t e, uint32_t mode, uint32_t c) { return Call{e / K, e % K, (float)e, mode, c}; }

struct Pixel {
    float r[3];                   // out_linear
    float G;                      // out_gini
    int32_t kept;                 // out_kept
    float v;                      // out_variance
    float accum[3];               // out_accum
    float S1, S2;                 // out_moments
};

RT_HOST_DEVICE uint32_t bits_of(float x) { return __builtin_bit_cast(uint32_t, x); }

// the key of a y: ascends with the value, -0 < +0, every NaN the largest
RT_HOST_DEVICE uint32_t key_of(float y) {
    const uint32_t u = bits_of(y);
    const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return y != y ? 0xffffffffu : k;
}

// The estimate of one pixel.  B(k, c): channel c of the pixel's sum in bucket k.
template <int K, class Buckets>
RT_HOST_DEVICE void resolve_pixel(const Call& a, const Buckets& B, Pixel& o) {
    static_assert(buckets_ok((uint32_t)K), "K is odd, 3 ... 15");
    constexpr int h = (K - 1) / 2;
    constexpr float K_f = (float)K;
    float m[K][3], y[K];
    uint32_t key[K];
    int rank[K];
    // bucket means
    RTR_UNROLL
    for (int k = 0; k < K; k++) {
        const float n_f = (float)(a.q + ((uint32_t)k < a.rem ? 1u : 0u));
        m[k][0] = B(k, 0) / n_f;
        m[k][1] = B(k, 1) / n_f;
        m[k][2] = B(k, 2) / n_f;
        y[k] = (m[k][0] + m[k][1]) + m[k][2];
        key[k] = key_of(y[k]);
    }
    // order: rank counting, ties by k
    RTR_UNROLL
    for (int k = 0; k < K; k++) {
        int rk = 0;
        RTR_UNROLL
        for (int j = 0; j < K; j++) {
            if (j < k) rk += key[j] <= key[k] ? 1 : 0;
            if (j > k) rk += key[j] < key[k] ? 1 : 0;
        }
        rank[k] = rk;
    }
    // Gini
    float T = 0.0f, g = 0.0f;
    RTR_UNROLL
    for (int k = 0; k < K; k++) {
        const float ys = y[k] > 0.0f ? y[k] : 0.0f;
        T += ys;
        g += (float)(2 * rank[k] - (K - 1)) * ys;
    }
    float G = T > 0.0f ? g / (K_f * T) : 0.0f;
    G = G > 0.0f ? G : 0.0f;
    G = G < 1.0f ? G : 1.0f;
    // width
    int c = (int)a.c;
    if (a.mode == MODE_GINI) c = (int)__builtin_floorf((1.0f - G) * (float)h);
    // estimate
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    RTR_UNROLL
    for (int k = 0; k < K; k++) {
        const bool kept = h - c <= rank[k] && rank[k] <= h + c;
        s0 = kept ? s0 + m[k][0] : s0;
        s1 = kept ? s1 + m[k][1] : s1;
        s2 = kept ? s2 + m[k][2] : s2;
    }
    const float kept_f = (float)(2 * c + 1);
    o.r[0] = s0 / kept_f;
    o.r[1] = s1 / kept_f;
    o.r[2] = s2 / kept_f;
    o.G = G;
    o.kept = 2 * c + 1;
    // variance of the estimate
    const int cw = c > 1 ? c : 1;
    float lo = 0.0f, hi = 0.0f;
    RTR_UNROLL
    for (int k = 0; k < K; k++) {
        lo = rank[k] == h - cw ? y[k] : lo;
        hi = rank[k] == h + cw ? y[k] : hi;
    }
    float w[K];
    float sw = 0.0f;
    RTR_UNROLL
    for (int k = 0; k < K; k++) {
        w[k] = y[k] < lo ? lo : (y[k] < hi ? y[k] : hi);
        sw += w[k];
    }
    const float mw = sw / K_f;
    float dw = 0.0f;
    RTR_UNROLL
    for (int k = 0; k < K; k++) {
        const float d = w[k] - mw;
        dw += d * d;
    }
    o.v = (dw / (K_f - 1.0f)) / K_f;
    // restated sums
    o.accum[0] = o.r[0] * a.e_f;
    o.accum[1] = o.r[1] * a.e_f;
    o.accum[2] = o.r[2] * a.e_f;
    const float yr = (o.r[0] + o.r[1]) + o.r[2];
    o.S1 = yr * a.e_f;
    o.S2 = (o.v * (a.e_f - 1.0f) + yr * yr) * a.e_f;
}

}  // namespace rtrm
