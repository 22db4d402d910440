// rt_upsample_math.h — the per-pixel arithmetic of the film-upsampler library (rt_upsample.h): the position of an
// output pixel in the low film, the admission of a tap, the weighted sums with their bilinear fall-back, and the exit.  Plain C++ that
// compiles as HIP device code (rt_upsample.hip.h) and under g++ -ffp-contract=off (tests/host/upsample_host.cpp), so the kernel and the
// CPU harness run the same lines.  Every operation is one IEEE f32 rounding in the order rt_upsample.h writes it: no fused
// multiply-add, correctly rounded division and sqrt, no transcendental function.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rt_consts.h"
#include "rt_denoise_math.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define RT_UP_UNROLL _Pragma("unroll")
#else
#define RT_UP_UNROLL
#endif

namespace rtum {

// the planes a call has, on both sides together: the kernel's template argument
constexpr uint32_t P_ALBEDO = 1u, P_NORMAL = 2u, P_DEPTH = 4u, P_HITS = 8u, P_INDEX = 16u, P_ALL = 31u;

// whether a plane set is one a call may have: depth needs hits
constexpr bool planes_ok(uint32_t planes) { return planes <= P_ALL && (!(planes & P_DEPTH) || (planes & P_HITS)); }

// The two frames and the constants of a call (rt_upsample.h "The two frames").
struct Frame {
    uint32_t Wl, Rl, Hl, y0l;
    uint32_t Wh, Rh, Hh, y0h;
    float u_den_l, v_den_l, u_den_h, v_den_h;
    float kd, kn2;                // k_depth, and k_normal k_normal rounded once
    float eps, kl_f, kh_f;        // the albedo's eps and the two sample counts as floats
};

// u_den and v_den of a W x H frame, as rtplan::fill_camera forms them.  Host.
inline void frame_dens(uint32_t W, uint32_t H, float& u_den, float& v_den) {
    const float aspect_ratio = (float)W / (float)H;
    const float image_height = (float)H;
    u_den = aspect_ratio * image_height - 1.0f;
    v_den = image_height - 1.0f;
}

// What the CPU harness counts (tests/test_upsample_host.py: none may stay at zero over its cases): the test that rejected a tap,
// the taps admitted, and the class of a pixel.
enum Branch { BR_INDEX, BR_HITS, BR_DEPTH, BR_NORMAL, BR_ADMIT, BR_CLASS0, BR_CLASS1, BR_COUNT };
struct NoCount {
    RT_HOST_DEVICE void operator()(int) const {}
};

RT_HOST_DEVICE float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// The high side's values at the output pixel.  Only the members whose planes the call has are read.
struct Guide {
    float A[3], n[3];
    float D;
    uint32_t hits, index;
};

// Steps 1 to 5 of output pixel (x, r): V[3] and the class.  lo: the low side, read through
//     lo.colour(i, L[3])     the linear colour of film pixel i = y Wl + x (always inside the film)
//     lo.albedo(i, A[3]), lo.normal(i, n[3]), lo.depth(i), lo.hits(i), lo.index(i)     its feature sums; only those in PLANES are called
template <uint32_t PLANES, class Lo, class Count>
RT_HOST_DEVICE void gather_pixel(const Frame& f, uint32_t x, uint32_t r, const Guide& g, const Lo& lo, const Count& count, float V[3],
                                 uint32_t& cls) {
    static_assert(planes_ok(PLANES), "depth needs hits");
    constexpr bool ALBEDO = (PLANES & P_ALBEDO) != 0, NORMAL = (PLANES & P_NORMAL) != 0, DEPTH = (PLANES & P_DEPTH) != 0,
                   HITS = (PLANES & P_HITS) != 0, INDEX = (PLANES & P_INDEX) != 0;
    // 1
    const bool hit_h = HITS ? g.hits > 0u : true;
    float zh = 0.0f;
    if (DEPTH && hit_h) zh = g.D / (float)g.hits;
    const float zlim = DEPTH ? f.kd * zh : 0.0f;
    const float nn = NORMAL ? dot3(g.n, g.n) : 0.0f;
    // 2: fx and fy are finite and lie within a pixel of the film (u_den_h, v_den_h >= 1 and every size is below 2^24), so the
    // conversions are exact
    const float u = ((float)x + 0.5f) / f.u_den_h;
    const float fx = u * f.u_den_l - 0.5f;
    const float v = ((float)(f.Hh - (f.y0h + r) - 1u) + 0.5f) / f.v_den_h;
    const float cv = v * f.v_den_l - 0.5f;
    const float fy = ((float)(f.Hl - 1u) - cv) - (float)f.y0l;
    const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
    const int x0 = (int)flx, y0t = (int)fly;
    const float ax = fx - flx, ay = fy - fly;
    // 3, 4
    float b[4], Vq[4][3];
    bool adm[4];
    RT_UP_UNROLL
    for (int dy = 0; dy <= 1; dy++) {
        RT_UP_UNROLL
        for (int dx = 0; dx <= 1; dx++) {
            const int q = 2 * dy + dx;
            int qx = x0 + dx, qy = y0t + dy;
            qx = qx < 0 ? 0 : (qx > (int)f.Wl - 1 ? (int)f.Wl - 1 : qx);
            qy = qy < 0 ? 0 : (qy > (int)f.Rl - 1 ? (int)f.Rl - 1 : qy);
            const size_t i = (size_t)qy * f.Wl + (size_t)qx;
            b[q] = (dx ? ax : 1.0f - ax) * (dy ? ay : 1.0f - ay);
            lo.colour(i, Vq[q]);
            if (ALBEDO) {
                float Al[3], d[3];
                lo.albedo(i, Al);
                rtdn::albedo_d(Al, f.kl_f, f.eps, d);
                for (int k = 0; k < 3; k++) Vq[q][k] = Vq[q][k] / d[k];
            }
            bool ok = true;
            if (INDEX && ok && lo.index(i) != g.index) {
                count(BR_INDEX);
                ok = false;
            }
            uint32_t hl = 1u;
            if (HITS && ok) {
                hl = lo.hits(i);
                if ((hl == 0u) != (g.hits == 0u)) {
                    count(BR_HITS);
                    ok = false;
                }
            }
            if (DEPTH && ok && hit_h) {                           // (past the hits test: both hit, or neither)
                const float zl = lo.depth(i) / (float)hl;
                if (!(__builtin_fabsf(zh - zl) <= zlim)) {
                    count(BR_DEPTH);
                    ok = false;
                }
            }
            if (NORMAL && ok && hit_h) {
                float nl[3];
                lo.normal(i, nl);
                const float c = dot3(g.n, nl);
                if (!(c > 0.0f && c * c >= f.kn2 * (nn * dot3(nl, nl)))) {
                    count(BR_NORMAL);
                    ok = false;
                }
            }
            if (ok) count(BR_ADMIT);
            adm[q] = ok;
        }
    }
    // 5
    float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    RT_UP_UNROLL
    for (int q = 0; q < 4; q++)
        if (adm[q]) {
            sw = sw + b[q];
            s0 = s0 + b[q] * Vq[q][0];
            s1 = s1 + b[q] * Vq[q][1];
            s2 = s2 + b[q] * Vq[q][2];
        }
    cls = 0u;
    if (!(sw > 0.0f)) {
        cls = 1u;
        sw = s0 = s1 = s2 = 0.0f;
        RT_UP_UNROLL
        for (int q = 0; q < 4; q++) {
            sw = sw + b[q];
            s0 = s0 + b[q] * Vq[q][0];
            s1 = s1 + b[q] * Vq[q][1];
            s2 = s2 + b[q] * Vq[q][2];
        }
    }
    count(cls ? BR_CLASS1 : BR_CLASS0);
    V[0] = s0 / sw;
    V[1] = s1 / sw;
    V[2] = s2 / sw;
}

// Steps 6 and 7: V, remodulated by the high side's albedo in a call that has it, through the denoiser's exit (rtdn::output_pixel).
template <uint32_t PLANES>
RT_HOST_DEVICE void exit_pixel(const Frame& f, const Guide& g, const float V[3], float lin[3], float f32[3], uint8_t rgb[3]) {
    if (PLANES & P_ALBEDO) {
        float d[3];
        rtdn::albedo_d(g.A, f.kh_f, f.eps, d);
        rtdn::output_pixel(V, d, lin, f32, rgb);
    } else {
        rtdn::output_pixel(V, nullptr, lin, f32, rgb);
    }
}

}  // namespace rtum
