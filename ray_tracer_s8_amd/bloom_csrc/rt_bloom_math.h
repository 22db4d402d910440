// rt_bloom_math.h — the arithmetic of the bloom library (rt_bloom.h): the level shapes and the scratch layout, the
// sanitised input, the threshold, the taps and sums of a down step and of an up step, the accumulation, the two mixes, the rule that
// places the tail, and what the host refuses of the settings.  Plain C++ that compiles as HIP device code (rt_bloom.hip.h) and under
// g++ -ffp-contract=off (tests/host/bloom_host.cpp), so the kernels and the CPU harness run the same lines.  Every operation is one
// IEEE f32 rounding in the order rt_bloom.h writes it: no fused multiply-add, correctly rounded division, no transcendental function.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HOST_DEVICE __host__ __device__ inline
#else
#define RT_HOST_DEVICE inline
#endif

namespace rtbm {

constexpr uint32_t MAX_LEVELS = 8u;
constexpr uint32_t MODE_MIX = 0u, MODE_ADD = 1u;
constexpr uint32_t FORM_LEVELS = 0u, FORM_TAIL = 1u;
constexpr float MAX_CAP = 4611686018427387904.0f;          // 2^62: twice a cap, squared, is a finite float
constexpr uint64_t LDS_BUDGET = 160u * 1024u;               // the LDS of a compute unit: the tail kernel has no static LDS
constexpr uint64_t MAX_PIXELS = 0x7fffffffull;

// ---- levels -------------------------------------------------------------------------------------------------------------------------
RT_HOST_DEVICE uint32_t half_up(uint32_t n) { return (n + 1u) >> 1; }

// the side of level k of a side n
RT_HOST_DEVICE uint32_t level_side(uint32_t n, uint32_t k) {
    for (uint32_t j = 0; j < k; j++) n = half_up(n);
    return n;
}

// the bytes level k takes in the scratch: its pixels, rounded up to 16 bytes
RT_HOST_DEVICE uint64_t level_bytes(uint32_t W, uint32_t R, uint32_t k) {
    return ((uint64_t)level_side(W, k) * level_side(R, k) * 12u + 15u) & ~(uint64_t)15u;
}

// where level k (1 ... levels) begins in the scratch; k = levels + 1 gives the scratch's size
RT_HOST_DEVICE uint64_t level_offset(uint32_t W, uint32_t R, uint32_t k) {
    uint64_t at = 0;
    for (uint32_t j = 1; j < k; j++) at += level_bytes(W, R, j);
    return at;
}

// The least k >= 1 whose levels k ... levels lie in `budget` bytes of LDS together, 12 bytes a pixel; levels + 1 if the last level
// alone does not.  (The sum only grows as k falls, so it is taken from the last level down.)
RT_HOST_DEVICE uint32_t tail_from(uint32_t W, uint32_t R, uint32_t levels, uint64_t budget) {
    uint64_t sum = 0;
    uint32_t k = levels + 1u;
    while (k > 1u) {
        sum += (uint64_t)level_side(W, k - 1u) * level_side(R, k - 1u) * 12u;
        if (sum > budget) break;
        k--;
    }
    return k;
}

// ---- what the host refuses ----------------------------------------------------------------------------------------------------------
RT_HOST_DEVICE bool finite(float v) { return v - v == 0.0f; }

struct Settings {
    uint32_t levels, mode;
    float spread, strength, norm, cap, T, K;
};

RT_HOST_DEVICE bool settings_ok(const Settings& s) {
    if (s.levels < 1u || s.levels > MAX_LEVELS) return false;
    if (!(s.spread > 0.0f && s.spread <= 1.0f)) return false;
    if (s.mode == MODE_MIX) {
        if (!(s.strength > 0.0f && s.strength < 1.0f)) return false;
    } else if (s.mode == MODE_ADD) {
        if (!(s.strength > 0.0f) || !finite(s.strength)) return false;
    } else {
        return false;
    }
    if (!(s.norm > 0.0f) || !finite(s.norm)) return false;
    if (!finite(s.cap) || !finite(s.T) || !finite(s.K)) return false;
    if (!(s.cap > 0.0f) || s.cap > MAX_CAP) return false;
    if (s.T < 0.0f || s.T > s.cap || s.K < 0.0f || s.K > s.T) return false;
    return true;
}

// ---- the input ----------------------------------------------------------------------------------------------------------------------
// q: a NaN, both zeros and every negative give +0
RT_HOST_DEVICE float positive(float c) { return c > 0.0f ? c : 0.0f; }
// p: q under the cap, so +inf becomes the cap
RT_HOST_DEVICE float sanitise(float c, float cap) {
    const float q = positive(c);
    return q < cap ? q : cap;
}

RT_HOST_DEVICE float max_of(float a, float b) { return a > b ? a : b; }

// the factor f of a sanitised pixel under the threshold T with the knee K
RT_HOST_DEVICE float threshold_factor(float p0, float p1, float p2, float T, float K) {
    const float m = max_of(max_of(p0, p1), p2);
    float s = m - (T - K);
    s = s > 0.0f ? s : 0.0f;
    const float k2 = K + K;
    s = s < k2 ? s : k2;
    float g = (s * s) / ((k2 + k2) + 1e-5f);
    const float e = m - T;
    g = g > e ? g : e;
    g = g > 0.0f ? g : 0.0f;
    return g / (m > 1e-5f ? m : 1e-5f);
}

// the pixel a pyramid starts from: sanitised, and with THRESH under the threshold
template <bool THRESH>
RT_HOST_DEVICE void source_pixel(const float* c, float cap, float T, float K, float* p) {
    p[0] = sanitise(c[0], cap), p[1] = sanitise(c[1], cap), p[2] = sanitise(c[2], cap);
    if (THRESH) {
        const float f = threshold_factor(p[0], p[1], p[2], T, K);
        p[0] = p[0] * f, p[1] = p[1] * f, p[2] = p[2] * f;
    }
}

// ---- down ---------------------------------------------------------------------------------------------------------------------------
// tap a = 0 ... 3 of output index i over a side of n: clamp(2 i - 1 + a, 0, n - 1)
RT_HOST_DEVICE uint32_t down_tap(uint32_t i, uint32_t a, uint32_t n) {
    const int64_t t = 2 * (int64_t)i - 1 + (int64_t)a;
    return t < 0 ? 0u : (t > (int64_t)n - 1 ? n - 1u : (uint32_t)t);
}

// the 1 3 3 1 sum, of a row's four taps (h_a) and of the four rows (v)
RT_HOST_DEVICE float sum_1331(float s0, float s1, float s2, float s3) { return (s0 + 3.0f * s1) + (3.0f * s2 + s3); }
RT_HOST_DEVICE float down_value(float h0, float h1, float h2, float h3) { return sum_1331(h0, h1, h2, h3) * 0.015625f; }

// D_{k+1}[i][j] from a level of R x W pixels that `fetch(row, column, float[3])` reads
template <class F>
RT_HOST_DEVICE void down_pixel(const F& fetch, uint32_t i, uint32_t j, uint32_t R, uint32_t W, float* out) {
    float h[4][3];
#pragma unroll
    for (uint32_t a = 0; a < 4u; a++) {
        float s[4][3];
#pragma unroll
        for (uint32_t b = 0; b < 4u; b++) fetch(down_tap(i, a, R), down_tap(j, b, W), s[b]);
#pragma unroll
        for (uint32_t c = 0; c < 3u; c++) h[a][c] = sum_1331(s[0][c], s[1][c], s[2][c], s[3][c]);
    }
#pragma unroll
    for (uint32_t c = 0; c < 3u; c++) out[c] = down_value(h[0][c], h[1][c], h[2][c], h[3][c]);
}

// ---- up -----------------------------------------------------------------------------------------------------------------------------
struct UpTap {
    uint32_t a, b;                // the two coarse indices, clamped
    float wa, wb;                 // their weights, chosen before the clamp
};

// the taps of fine index y over a coarse side of n
RT_HOST_DEVICE UpTap up_tap(uint32_t y, uint32_t n) {
    const int64_t ya = (int64_t)((y + 1u) / 2u) - 1, yb = ya + 1;
    UpTap t;
    t.wa = (y & 1u) ? 3.0f : 1.0f;
    t.wb = 4.0f - t.wa;
    t.a = ya < 0 ? 0u : (ya > (int64_t)n - 1 ? n - 1u : (uint32_t)ya);
    t.b = yb > (int64_t)n - 1 ? n - 1u : (uint32_t)yb;
    return t;
}

// u from the four coarse values X[row][column]
RT_HOST_DEVICE float up_value(float Xaa, float Xab, float Xba, float Xbb, float wxa, float wxb, float wya, float wyb) {
    const float ga = wxa * Xaa + wxb * Xab;
    const float gb = wxa * Xba + wxb * Xbb;
    return (wya * ga + wyb * gb) * 0.0625f;
}

// up(X)[y][x] of a coarse level of R x W pixels, [R][W][3] in memory
RT_HOST_DEVICE void up_pixel(const float* X, uint32_t R, uint32_t W, uint32_t y, uint32_t x, float* out) {
    const UpTap ty = up_tap(y, R), tx = up_tap(x, W);
    const float* aa = X + 3u * ((size_t)ty.a * W + tx.a);
    const float* ab = X + 3u * ((size_t)ty.a * W + tx.b);
    const float* ba = X + 3u * ((size_t)ty.b * W + tx.a);
    const float* bb = X + 3u * ((size_t)ty.b * W + tx.b);
#pragma unroll
    for (uint32_t c = 0; c < 3u; c++) out[c] = up_value(aa[c], ab[c], ba[c], bb[c], tx.wa, tx.wb, ty.wa, ty.wb);
}

// U_k = D_k + spread up(U_{k+1})
RT_HOST_DEVICE float accumulate(float d, float spread, float u) { return d + spread * u; }

// ---- combine ------------------------------------------------------------------------------------------------------------------------
RT_HOST_DEVICE float bloom_value(float u, float norm) { return u * norm; }

// `keep` is 1 - strength, one subtraction the caller makes once
template <uint32_t MODE>
RT_HOST_DEVICE float mix(float q, float b, float strength, float keep) {
    return MODE == MODE_MIX ? keep * q + strength * b : q + strength * b;
}

}  // namespace rtbm
