// rt_film_math.h — the per-pixel and per-tap arithmetic of the film library (rt_film.h): the moments fold of a pixel's
// records, the entry variance, the variance prefilter, the luminance edge-stop, one guided iteration step of a pixel; and the pieces of
// the regression resolve: a pixel's entry and features, the Cholesky fit of a node and a pixel's blend.  Plain C++ that
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

// ---- the regression resolve (rt_film.h "Regression resolve") ---------------------------------------------------------
constexpr int RG_T = 16;                      // the node pitch; a window is 2T x 2T
constexpr int RG_M = 8;                       // features
constexpr int RG_NA = 36;                     // the entries A_ab, a <= b
constexpr int RG_NS = 60;                     // window sums: A, then B_ac at RG_NA + 3a + c
constexpr int RG_RECORD = 32;                 // floats of a node's record

RT_HOST_DEVICE uint32_t rg_nodes(uint32_t n) { return (n - 1u) / (uint32_t)RG_T + 2u; }

// the place of A_ab (a <= b) among the window sums: row by row of the upper triangle
RT_HOST_DEVICE int rg_ai(int a, int b) { return a * RG_M - (a * (a - 1)) / 2 + (b - a); }

// What the planes give of a pixel.  Any plane pointer may be nullptr; i: the pixel's index in the frame.
struct RgPlanes {
    const float* accum;
    const float* albedo;
    const float* normal;
    const float* depth;
    const uint32_t* hits;
    float e_f, k_f, albedo_eps;
};

struct RgPixel {
    float r[3];            // the entry colour
    float d[3];            // the albedo divisor (read only with an albedo plane)
    rtdn::Guide g;
    float z;               // g.zg > 0 ? g.zg : +0
    bool valid;            // g.zg >= 0
};

RT_HOST_DEVICE RgPixel rg_entry(const RgPlanes& pl, size_t i) {
    RgPixel px;
    px.d[0] = px.d[1] = px.d[2] = 0.0f;
    if (pl.albedo) rtdn::albedo_d(pl.albedo + 3 * i, pl.k_f, pl.albedo_eps, px.d);
    rtdn::entry_color(pl.accum + 3 * i, pl.e_f, pl.albedo ? px.d : nullptr, px.r);
    px.g = rtdn::entry_guide(pl.normal ? pl.normal + 3 * i : nullptr, pl.depth ? pl.depth + i : nullptr, pl.hits ? pl.hits + i : nullptr);
    px.valid = px.g.zg >= 0.0f;
    px.z = px.g.zg > 0.0f ? px.g.zg : 0.0f;
    return px;
}

// phi of pixel (x, y) in node (i, j) whose window has zlo and s
RT_HOST_DEVICE void rg_features(const RgPixel& px, int x, int y, int i, int j, float zlo, float s, float phi[RG_M]) {
    phi[0] = 1.0f;
    phi[1] = px.g.nx;
    phi[2] = px.g.ny;
    phi[3] = px.g.nz;
    const float zeta = s > 0.0f ? (px.z - zlo) / s : 0.0f;
    phi[4] = zeta;
    phi[5] = zeta * zeta;
    phi[6] = ((float)(x - RG_T * i) + 0.5f) / 16.0f;
    phi[7] = ((float)(y - RG_T * j) + 0.5f) / 16.0f;
}

// The Cholesky factor of a node's normal equations from its window sums S [RG_NS] (A without the ridge) and n.  L: 64 floats, the
// lower triangle row major.  Returns whether the fit stands (false: n = 0 or a pivot that is not > 0).  S and L may be LDS.
RT_HOST_DEVICE bool rg_cholesky(const float* S, uint32_t n, float ridge, float* L) {
    if (n == 0u) return false;
    const float rn = ridge * (float)n;
    for (int a = 0; a < RG_M; a++) {
        float p = S[rg_ai(a, a)];
        if (a >= 1) p = p + rn;
        for (int t = 0; t < a; t++) p = p - L[a * RG_M + t] * L[a * RG_M + t];
        if (!(p > 0.0f)) return false;
        const float laa = __builtin_sqrtf(p);
        L[a * RG_M + a] = laa;
        for (int b = a + 1; b < RG_M; b++) {
            float q = S[rg_ai(a, b)];
            for (int t = 0; t < a; t++) q = q - L[b * RG_M + t] * L[a * RG_M + t];
            L[b * RG_M + a] = q / laa;
        }
    }
    return true;
}

// The weights of channel c into the node's record rec (w_ac at 3a + c): the two solves, or the constant fallback.
RT_HOST_DEVICE void rg_solve(const float* S, uint32_t n, bool ok, const float* L, int c, float* rec) {
    if (ok) {
        for (int a = 0; a < RG_M; a++) {                         // forward: y in the place of w
            float y = S[RG_NA + 3 * a + c];
            for (int t = 0; t < a; t++) y = y - L[a * RG_M + t] * rec[3 * t + c];
            rec[3 * a + c] = y / L[a * RG_M + a];
        }
        for (int a = RG_M - 1; a >= 0; a--) {                    // back
            float w = rec[3 * a + c];
            for (int t = a + 1; t < RG_M; t++) w = w - L[t * RG_M + a] * rec[3 * t + c];
            rec[3 * a + c] = w / L[a * RG_M + a];
        }
    } else {
        rec[c] = n > 0u ? S[RG_NA + c] / (float)n : 0.0f;
        for (int a = 1; a < RG_M; a++) rec[3 * a + c] = 0.0f;
    }
}

// words 24 ... 31 of the record
RT_HOST_DEVICE void rg_record_tail(uint32_t n, float zlo, float s, bool ok, float* rec) {
    rec[24] = zlo;
    rec[25] = s;
    rec[26] = (float)n;
    rec[27] = ok ? 1.0f : 0.0f;
    rec[28] = 0.0f;
    rec[29] = 0.0f;
    rec[30] = 0.0f;
    rec[31] = 0.0f;
}

// r' of a valid pixel (x, y): the blend of its four nodes' models.  model: the records, NX to a row.
RT_HOST_DEVICE void rg_apply(const RgPixel& px, int x, int y, const float* model, uint32_t NX, float out[3]) {
    const int ci = x >> 4, cj = y >> 4;
    const float fx = ((float)(x & 15) + 0.5f) / 16.0f, fy = ((float)(y & 15) + 0.5f) / 16.0f;
    const float wt[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
    float acc[3] = {0.0f, 0.0f, 0.0f};
    RT_DN_UNROLL
    for (int k = 0; k < 4; k++) {
        const int i = ci + (k & 1), j = cj + (k >> 1);
        const float* rec = model + ((size_t)j * NX + (size_t)i) * RG_RECORD;
        float phi[RG_M];
        rg_features(px, x, y, i, j, rec[24], rec[25], phi);
        RT_DN_UNROLL
        for (int c = 0; c < 3; c++) {
            float m = 0.0f;
            RT_DN_UNROLL
            for (int a = 0; a < RG_M; a++) m = m + rec[3 * a + c] * phi[a];
            acc[c] = acc[c] + wt[k] * m;
        }
    }
    out[0] = acc[0] > 0.0f ? acc[0] : 0.0f;
    out[1] = acc[1] > 0.0f ? acc[1] : 0.0f;
    out[2] = acc[2] > 0.0f ? acc[2] : 0.0f;
}

}  // namespace rtfm
