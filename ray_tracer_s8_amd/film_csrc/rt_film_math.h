// rt_film_math.h — the per-pixel and per-tap arithmetic of the film library (rt_film.h): the moments fold of a pixel's
// records, the entry variance, the variance prefilter, the luminance edge-stop, one guided iteration step of a pixel.  Plain C++ that
// compiles as HIP device code (rt_film.hip.h) and under g++ -ffp-contract=off (tests/host/film_host.cpp), so the kernels and the CPU
// harness run the same lines.  Every operation is one IEEE f32 rounding in the order rt_film.h writes it: no fused multiply-add,
// correctly rounded division and sqrt, no transcendental function.  The entry guide, the B3 taps, the normal and depth terms' inputs
// and the output transform are csrc/rt_denoise_math.h's, unchanged.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rt_consts.h"
#include "rt_denoise_math.h"

namespace rtfm {

// the prefilter's taps 1/4, 1/2, 1/4 (exact in f32, and so is every product of two)
constexpr float G[3] = {0.25f, 0.5f, 0.25f};

// The constants of one iteration.
struct Step {
    float sigma_l, var_eps;   // the luminance edge-stop: a_p = 1 / (sigma_l sqrt(gv_p) + var_eps)
    float kn, kd;             // k_normal, k_depth
    int s;                    // step 2^i
    uint32_t planes;          // rtdn::P_NORMAL | P_DEPTH | P_HITS of the call (never P_ALBEDO)
};

// y of a colour
RT_HOST_DEVICE float lum(const float c[3]) { return (c[0] + c[1]) + c[2]; }

// ---- the fold -----------------------------------------------------------------------------------------------------------------------
// n records (3 floats each, in sample order) into the pixel's running sums: acc += c per channel, mom[0] += y, mom[1] += y y
RT_HOST_DEVICE void fold_pixel(const float* rec, uint32_t n, float acc[3], float mom[2]) {
    for (uint32_t j = 0; j < n; j++) {
        const float* c = rec + 3 * (size_t)j;
        acc[0] = acc[0] + c[0];
        acc[1] = acc[1] + c[1];
        acc[2] = acc[2] + c[2];
        const float y = lum(c);
        mom[0] = mom[0] + y;
        mom[1] = mom[1] + y * y;
    }
}

// ---- entry --------------------------------------------------------------------------------------------------------------------------
// v0: the variance of the mean of y from the sums S1, S2 over e samples (e >= 2)
RT_HOST_DEVICE float entry_variance(float S1, float S2, float e_f) {
    const float m = S1 / e_f;
    const float a = S2 / e_f;
    float d = a - m * m;
    d = d > 0.0f ? d : 0.0f;
    return d / (e_f - 1.0f);
}

// ---- one tap ------------------------------------------------------------------------------------------------------------------------
// The Tukey factor t of a tap other than the centre: the luminance term scaled by the pixel's a_p, then rtdn::tap_t's normal and
// depth terms, in that order.
RT_HOST_DEVICE float tap_t(const Step& st, float yp, float ap, const rtdn::Guide& gp, float qp, float yq, const rtdn::Guide& gq) {
    float x = __builtin_fabsf(yq - yp) * ap;
    if (st.planes & rtdn::P_NORMAL) {
        const bool zp = gp.nx == 0.0f && gp.ny == 0.0f && gp.nz == 0.0f;
        const bool zq = gq.nx == 0.0f && gq.ny == 0.0f && gq.nz == 0.0f;
        if (!(zp && zq)) {
            const float dot = (gp.nx * gq.nx + gp.ny * gq.ny) + gp.nz * gq.nz;
            x = x + (1.0f - dot) * st.kn;
        }
    }
    if (st.planes & rtdn::P_DEPTH) {
        const float zq = gq.zg > 0.0f ? gq.zg : 0.0f, zp = gp.zg > 0.0f ? gp.zg : 0.0f;
        const float dz = zq - zp;
        x = x + ((dz < 0.0f ? -dz : dz) * qp) * st.kd;
    }
    const float u = 1.0f - x;
    return u > 0.0f ? u : 0.0f;
}

// ---- one iteration step of pixel (px, py) of the W x R image ------------------------------------------------------------------------
// load(x, y, r, g): the record r[4] (colour, variance in r[3]) and guide of pixel (x, y) (in bounds).  The guide is read only when
// the call has one.  out[4]: r_{i+1} and v_{i+1}.
template <class Load>
RT_HOST_DEVICE void step_pixel(const Step& st, int px, int py, int W, int R, const Load& load, float out[4]) {
    const bool guided = (st.planes & (rtdn::P_NORMAL | rtdn::P_DEPTH | rtdn::P_HITS)) != 0;
    float rp[4];
    rtdn::Guide gp = {0.0f, 0.0f, 0.0f, 0.0f};
    load(px, py, rp, gp);
    // the prefilter: the 3 x 3 Gaussian of the variance at distance 1, over the taps of the pixel's own side
    float gw = 0.0f, gvs = 0.0f;
    RT_DN_UNROLL
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = py + dy;
        if (qy < 0 || qy >= R) continue;
        RT_DN_UNROLL
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = px + dx;
            if (qx < 0 || qx >= W) continue;
            const float g = G[dy + 1] * G[dx + 1];
            float vq = rp[3];
            if (!(dx == 0 && dy == 0)) {
                float rq[4];
                rtdn::Guide gq = {0.0f, 0.0f, 0.0f, 0.0f};
                load(qx, qy, rq, gq);
                if (guided && ((gq.zg >= 0.0f) != (gp.zg >= 0.0f))) continue;
                vq = rq[3];
            }
            gw = gw + g;
            gvs = gvs + g * vq;
        }
    }
    const float gv = gvs / gw;
    const float ap = 1.0f / (st.sigma_l * __builtin_sqrtf(gv) + st.var_eps);
    const float yp = lum(rp);
    const float qp = (st.planes & rtdn::P_DEPTH) ? rtdn::inv_depth(gp.zg) : 0.0f;
    float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sv = 0.0f;
    RT_DN_UNROLL
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = py + st.s * dy;
        if (qy < 0 || qy >= R) continue;
        RT_DN_UNROLL
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = px + st.s * dx;
            if (qx < 0 || qx >= W) continue;
            float w = rtdn::H[dy + 2] * rtdn::H[dx + 2];
            float rq[4];
            if (dx == 0 && dy == 0) {
                rq[0] = rp[0];
                rq[1] = rp[1];
                rq[2] = rp[2];
                rq[3] = rp[3];
            } else {
                rtdn::Guide gq = {0.0f, 0.0f, 0.0f, 0.0f};
                load(qx, qy, rq, gq);
                if (guided && ((gq.zg >= 0.0f) != (gp.zg >= 0.0f))) continue;
                const float t = tap_t(st, yp, ap, gp, qp, lum(rq), gq);
                w = w * (t * t);
            }
            sw = sw + w;
            s0 = s0 + w * rq[0];
            s1 = s1 + w * rq[1];
            s2 = s2 + w * rq[2];
            sv = sv + (w * w) * rq[3];
        }
    }
    out[0] = s0 / sw;
    out[1] = s1 / sw;
    out[2] = s2 / sw;
    out[3] = sv / (sw * sw);
}

}  // namespace rtfm
