// rt_denoise_math.h — the per-pixel and per-tap arithmetic of the a-trous denoiser (rt_tile.h "denoiser"): the entry
// transform, the edge-stopping weight, one iteration step of a pixel and the output transform.  Plain C++ that compiles as HIP device
// code (rt_denoise.hip.h) and under g++ -ffp-contract=off (tests/host/denoise_host.cpp), so the kernels and the CPU harness run the
// same lines.  Every operation is one IEEE f32 rounding in the order rt_tile.h writes it: no fused multiply-add (the build's
// -ffp-contract=off), correctly rounded division and sqrt (hipcc's default, SSE on the host), no transcendental function.
#pragma once
#include <stdint.h>

#include "rt_consts.h"

#if defined(__HIPCC__)
#define RT_DN_UNROLL _Pragma("unroll")
#else
#define RT_DN_UNROLL
#endif

namespace rtdn {

constexpr uint32_t MAX_ITER = 8;                 // RT_DENOISE_MAX_ITERATIONS
// the planes a call reads (the same set for every strip of a call)
constexpr uint32_t P_ALBEDO = 1u, P_NORMAL = 2u, P_DEPTH = 4u, P_HITS = 8u;
// the B3-spline taps 1/16, 1/4, 3/8, 1/4, 1/16 (exact in f32, and so is every product of two)
constexpr float H[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};

// The packed guide of a pixel: the unit normal (0 without one) and zg = g ? z : -1 (z >= 0, so g is zg >= 0).
struct Guide {
    float nx, ny, nz, zg;
};

// The constants of one iteration.
struct Step {
    float kc;          // k_color of this iteration
    float kn, kd;      // k_normal, k_depth
    int s;             // step 2^i
    uint32_t planes;   // P_* of the call
};

// Rust `as u8` from f32 (the tile kernel's f32_as_u8): truncate, saturate, NaN -> 0
RT_HOST_DEVICE uint8_t as_u8(float v) {
    if (!(v == v)) return 0;
    if (v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)(int)v;
}

// ---- entry transform --------------------------------------------------------------------------------------------------------------
// d = A / k + eps per channel: the albedo the colour is demodulated by, and remodulated by at the end
RT_HOST_DEVICE void albedo_d(const float A[3], float k_f, float eps, float d[3]) {
    for (int c = 0; c < 3; c++) d[c] = A[c] / k_f + eps;
}

// r0 of a pixel: c = C / e, divided by d when the albedo is given (d: nullptr otherwise)
RT_HOST_DEVICE void entry_color(const float C[3], float e_f, const float* d, float r[3]) {
    for (int c = 0; c < 3; c++) {
        const float cc = C[c] / e_f;
        r[c] = d ? cc / d[c] : cc;
    }
}

// the guide of a pixel from its planes (nullptr: not given); hits given or not decides g
RT_HOST_DEVICE Guide entry_guide(const float* N, const float* D, const uint32_t* hits) {
    Guide gd = {0.0f, 0.0f, 0.0f, 0.0f};
    if (N) {
        const float L = __builtin_sqrtf((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
        if (L > 0.0f) {
            gd.nx = N[0] / L;
            gd.ny = N[1] / L;
            gd.nz = N[2] / L;
        }
    }
    float z = 0.0f;
    if (D && hits && *hits > 0u) z = *D / (float)*hits;
    const bool g = hits ? *hits > 0u : true;
    gd.zg = g ? z : -1.0f;
    return gd;
}

// q = 1 / z of a pixel's depth (0 where z is 0)
RT_HOST_DEVICE float inv_depth(float zg) { return zg > 0.0f ? 1.0f / zg : 0.0f; }

// ---- one tap ----------------------------------------------------------------------------------------------------------------------
// The Tukey factor t of a tap other than the centre (rt_tile.h): colour, then normal, then depth, in that order.
RT_HOST_DEVICE float tap_t(const Step& st, const float rp[3], const Guide& gp, float qp, const float rq[3], const Guide& gq) {
    const float d0 = rq[0] - rp[0], d1 = rq[1] - rp[1], d2 = rq[2] - rp[2];
    float x = ((d0 * d0 + d1 * d1) + d2 * d2) * st.kc;
    if (st.planes & P_NORMAL) {
        const bool zp = gp.nx == 0.0f && gp.ny == 0.0f && gp.nz == 0.0f;
        const bool zq = gq.nx == 0.0f && gq.ny == 0.0f && gq.nz == 0.0f;
        if (!(zp && zq)) {
            const float dot = (gp.nx * gq.nx + gp.ny * gq.ny) + gp.nz * gq.nz;
            x = x + (1.0f - dot) * st.kn;
        }
    }
    if (st.planes & P_DEPTH) {
        const float zq = gq.zg > 0.0f ? gq.zg : 0.0f, zp = gp.zg > 0.0f ? gp.zg : 0.0f;
        const float dz = zq - zp;
        x = x + ((dz < 0.0f ? -dz : dz) * qp) * st.kd;
    }
    const float u = 1.0f - x;
    return u > 0.0f ? u : 0.0f;
}

// ---- one iteration step of pixel (px, py) of the W x R image ------------------------------------------------------------------------
// load(x, y, r, g): the colour r[3] and guide of pixel (x, y) (in bounds).  The guide is read only when the call has one.
template <class Load>
RT_HOST_DEVICE void step_pixel(const Step& st, int px, int py, int W, int R, const Load& load, float out[3]) {
    const bool guided = (st.planes & (P_NORMAL | P_DEPTH | P_HITS)) != 0;
    float rp[3];
    Guide gp = {0.0f, 0.0f, 0.0f, 0.0f};
    load(px, py, rp, gp);
    const float qp = (st.planes & P_DEPTH) ? inv_depth(gp.zg) : 0.0f;
    float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    RT_DN_UNROLL
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = py + st.s * dy;
        if (qy < 0 || qy >= R) continue;
        RT_DN_UNROLL
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = px + st.s * dx;
            if (qx < 0 || qx >= W) continue;
            float w = H[dy + 2] * H[dx + 2];
            float rq[3];
            if (dx == 0 && dy == 0) {
                rq[0] = rp[0];
                rq[1] = rp[1];
                rq[2] = rp[2];
            } else {
                Guide gq = {0.0f, 0.0f, 0.0f, 0.0f};
                load(qx, qy, rq, gq);
                if (guided && ((gq.zg >= 0.0f) != (gp.zg >= 0.0f))) continue;
                const float t = tap_t(st, rp, gp, qp, rq, gq);
                w = w * (t * t);
            }
            sw = sw + w;
            s0 = s0 + w * rq[0];
            s1 = s1 + w * rq[1];
            s2 = s2 + w * rq[2];
        }
    }
    out[0] = s0 / sw;
    out[1] = s1 / sw;
    out[2] = s2 / sw;
}

// ---- output transform ---------------------------------------------------------------------------------------------------------------
// m = r * d (d: nullptr without albedo) and what each output holds; any output pointer may be nullptr
RT_HOST_DEVICE void output_pixel(const float r[3], const float* d, float* lin, float* f32, uint8_t* rgb) {
    for (int c = 0; c < 3; c++) {
        const float m = d ? r[c] * d[c] : r[c];
        const float f = __builtin_sqrtf(m);
        if (lin) lin[c] = m;
        if (f32) f32[c] = f;
        if (rgb) rgb[c] = as_u8(f * 255.999f);
    }
}

}  // namespace rtdn
