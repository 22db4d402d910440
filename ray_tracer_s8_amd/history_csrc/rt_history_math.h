// rt_history_math.h — the per-pixel and per-tap arithmetic of the film-history library (rt_history.h): the centre ray
// of a pixel, its reprojection into the previous camera, the admission of a tap, the weighted sums, the optional clip to the current
// frame's colour box and the blend.  Plain C++ that
// compiles as HIP device code (rt_history.hip.h) and under g++ -ffp-contract=off (tests/host/history_host.cpp), so the kernel and the
// CPU harness run the same lines.  Every operation is one IEEE f32 rounding in the order rt_history.h writes it: no fused
// multiply-add, correctly rounded division and sqrt, no transcendental function.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rt_consts.h"
#include "rt_plan.h"

namespace rthm {

constexpr uint32_t NONE = 0xffffffffu;       // RT_HIT_NONE

// The current frame's camera vectors (rtplan::fill_camera) and the previous frame's basis and plane (rt_history.h "Cameras").
struct Cur {
    float org[3], llc[3], hor[3], ver[3];
    float u_den, v_den;
};
struct Prev {
    float org[3], u[3], v[3], w[3];
    float f, vw, vh;
    float u_den, v_den;
};
struct Frame {
    Cur cur;
    Prev prev;
    uint32_t W, R;             // the film
    uint32_t H, y0;            // the frame's rows and the film's first global row
    uint32_t have_prev;        // 0: the first frame of a history
    uint32_t normals;          // 1: a call with normals
    float alpha, n_max, kd, kn2;
};

// The branches of accumulate_pixel, counted by the CPU harness (tests/test_history_host.py: none may stay at zero).
enum Branch {
    BR_NO_HITS, BR_FIRST, BR_CUR_NONE, BR_BEHIND, BR_OUTSIDE, BR_TAP_OUT, BR_TAP_EMPTY, BR_TAP_NONE, BR_TAP_INDEX, BR_TAP_DEPTH,
    BR_TAP_NORMAL, BR_TAP_OK, BR_NO_TAP, BR_BLEND, BR_N_MAX, BR_N_BELOW, BR_ALPHA, BR_RCP_N, BR_COUNT
};
struct NoCount {
    RT_HOST_DEVICE void operator()(int) const {}
};

RT_HOST_DEVICE float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Step 3: the direction of the centre ray of pixel (x, global row yg).  All zero or NaN when the camera is degenerate.
RT_HOST_DEVICE void centre_ray(const Cur& c, uint32_t H, uint32_t x, uint32_t yg, float d[3]) {
    const float u = ((float)x + 0.5f) / c.u_den;
    const float v = ((float)(H - yg - 1u) + 0.5f) / c.v_den;
    float e[3];
    for (int i = 0; i < 3; i++) e[i] = ((c.llc[i] + u * c.hor[i]) + v * c.ver[i]) - c.org[i];
    const float k = 1.0f / __builtin_sqrtf(dot3(e, e));
    const bool ok = k > 0.0f && k < __builtin_inff();
    float e1[3];
    for (int i = 0; i < 3; i++) e1[i] = ok ? e[i] * k : 0.0f;
    const float l = __builtin_sqrtf(dot3(e1, e1));
    for (int i = 0; i < 3; i++) d[i] = e1[i] / l;
}

// Step 4: the point at distance z along d, seen from the previous camera.  false: behind it (counted BR_BEHIND) or no tap of the
// footprint can lie inside the film (BR_OUTSIDE); then fx, fy, zp are not to be read.
template <class Count>
RT_HOST_DEVICE bool reproject(const Frame& f, const float d[3], float z, const Count& count, float& fx, float& fy, float& zp) {
    float q[3];
    for (int i = 0; i < 3; i++) q[i] = (f.cur.org[i] + z * d[i]) - f.prev.org[i];
    const float cx = dot3(q, f.prev.u), cy = dot3(q, f.prev.v), cz = -dot3(q, f.prev.w);
    if (!(cz > 0.0f)) {
        count(BR_BEHIND);
        return false;
    }
    const float t = f.prev.f / cz;
    const float sx = cx * t, sy = cy * t;
    fx = (sx / f.prev.vw + 0.5f) * f.prev.u_den - 0.5f;
    const float cv = (sy / f.prev.vh + 0.5f) * f.prev.v_den - 0.5f;
    fy = ((float)(f.H - 1u) - cv) - (float)f.y0;
    if (!(fx > -1.0f && fx < (float)f.W && fy > -1.0f && fy < (float)f.R)) {
        count(BR_OUTSIDE);
        return false;
    }
    zp = __builtin_sqrtf(dot3(q, q));
    return true;
}

// What steps 1 to 5 leave of a pixel that reached the blend: the history's colour sums, moments and length at the pixel.
struct History {
    float C[3], S1, S2, N;
};

// Steps 1 to 5 of one pixel: its z to store, and the bilinear gather of the previous state.  depth, hits, idx, n (3 floats, read only
// when f.normals): the feature sums.  prev: the previous state, read through
//     prev.guard(i, N, index, z)    the stored length, index and z of pixel i = y W + x (always inside the film)
//     prev.normal(i, n[3])          its stored normal sum (calls with normals only)
//     prev.values(i, C[3], M[2])    its stored colour sums and moments (admitted taps only)
// false: "no history" (the branch is counted), and h is not to be read.
template <class PrevState, class Count>
RT_HOST_DEVICE bool gather_pixel(const Frame& f, uint32_t x, uint32_t r, float depth, uint32_t hits, uint32_t idx, const float* n,
                                 const PrevState& prev, const Count& count, History& h, float& outZ) {
    outZ = 0.0f;
    if (hits == 0u) {
        count(BR_NO_HITS);
        return false;
    }
    const float z = depth / (float)hits;
    outZ = z;
    if (!f.have_prev) {
        count(BR_FIRST);
        return false;
    }
    if (idx == NONE) {
        count(BR_CUR_NONE);
        return false;
    }
    float d[3], fx, fy, zp;
    centre_ray(f.cur, f.H, x, f.y0 + r, d);
    if (!reproject(f, d, z, count, fx, fy, zp)) return false;
    // fx in (-1, W) and fy in (-1, R): the conversions are exact and x0, y0t lie in [-1, W - 1], [-1, R - 1]
    const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
    const int x0 = (int)flx, y0t = (int)fly;
    const float ax = fx - flx, ay = fy - fly;
    const float zlim = f.kd * zp;
    const float nn = f.normals ? dot3(n, n) : 0.0f;
    float sw = 0.0f, sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f, s1 = 0.0f, s2 = 0.0f, sn = 0.0f;
    bool any = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dy = 0; dy <= 1; dy++) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int dx = 0; dx <= 1; dx++) {
            const int qx = x0 + dx, qy = y0t + dy;
            if (qx < 0 || qx >= (int)f.W || qy < 0 || qy >= (int)f.R) {
                count(BR_TAP_OUT);
                continue;
            }
            const size_t i = (size_t)qy * f.W + (size_t)qx;
            float Nq, zq;
            uint32_t iq;
            prev.guard(i, Nq, iq, zq);
            if (!(Nq >= 1.0f)) {
                count(BR_TAP_EMPTY);
                continue;
            }
            if (iq == NONE) {
                count(BR_TAP_NONE);
                continue;
            }
            if (iq != idx) {
                count(BR_TAP_INDEX);
                continue;
            }
            if (!(__builtin_fabsf(zp - zq) <= zlim)) {
                count(BR_TAP_DEPTH);
                continue;
            }
            if (f.normals) {
                float nq[3];
                prev.normal(i, nq);
                const float c = dot3(n, nq);
                if (!(c > 0.0f && c * c >= f.kn2 * (nn * dot3(nq, nq)))) {
                    count(BR_TAP_NORMAL);
                    continue;
                }
            }
            count(BR_TAP_OK);
            float Cq[3], Mq[2];
            prev.values(i, Cq, Mq);
            const float w = (dx ? ax : 1.0f - ax) * (dy ? ay : 1.0f - ay);
            any = true;
            sw = sw + w;
            sc0 = sc0 + w * Cq[0];
            sc1 = sc1 + w * Cq[1];
            sc2 = sc2 + w * Cq[2];
            s1 = s1 + w * Mq[0];
            s2 = s2 + w * Mq[1];
            sn = sn + w * Nq;
        }
    }
    if (!any || !(sw > 0.0f)) {
        count(BR_NO_TAP);
        return false;
    }
    h.C[0] = sc0 / sw;
    h.C[1] = sc1 / sw;
    h.C[2] = sc2 / sw;
    h.S1 = s1 / sw;
    h.S2 = s2 / sw;
    h.N = sn / sw;
    return true;
}

// Step 6: the history h blended with the current sums C, M.
template <class Count>
RT_HOST_DEVICE void blend_pixel(const Frame& f, const float C[3], const float M[2], const History& h, const Count& count,
                                float outC[3], float outM[2], float& outN) {
    count(BR_BLEND);
    float N = h.N + 1.0f;
    if (N > f.n_max) {
        N = f.n_max;
        count(BR_N_MAX);
    } else {
        count(BR_N_BELOW);
    }
    float a = 1.0f / N;
    if (f.alpha > a) {
        a = f.alpha;
        count(BR_ALPHA);
    } else {
        count(BR_RCP_N);
    }
    const float b = 1.0f - a;
    outC[0] = b * h.C[0] + a * C[0];
    outC[1] = b * h.C[1] + a * C[1];
    outC[2] = b * h.C[2] + a * C[2];
    outM[0] = b * h.S1 + a * M[0];
    outM[1] = b * h.S2 + a * M[1];
    outN = N;
}

// One pixel of one frame: the gather, then the blend.  C, M: the film's sums.  Outputs: the blended sums, the length N and the z to
// store; "no history" leaves the current sums and N = 1.
template <class PrevState, class Count>
RT_HOST_DEVICE void accumulate_pixel(const Frame& f, uint32_t x, uint32_t r, const float C[3], const float M[2], float depth,
                                     uint32_t hits, uint32_t idx, const float* n, const PrevState& prev, const Count& count,
                                     float outC[3], float outM[2], float& outN, float& outZ) {
    outC[0] = C[0];
    outC[1] = C[1];
    outC[2] = C[2];
    outM[0] = M[0];
    outM[1] = M[1];
    outN = 1.0f;
    History h;
    if (!gather_pixel(f, x, r, depth, hits, idx, n, prev, count, h, outZ)) return;
    blend_pixel(f, C, M, h, count, outC, outM, outN);
}

// ---- step 5a: the clip of the history to the current frame's colour box -------------------------------------------
// gamma > 0 and e = (float)samples, as rt_history.h "5a" names them; the radius is a template argument of what follows.
struct Clip {
    float gamma, e;
};

// The branches of clip_history, counted by the CPU harness (tests/test_history_clip_host.py: none may stay at zero).  Its own enum:
// Branch and BR_COUNT stay as they are.
enum ClipBranch {
    CB_TAP_OUT, CB_TAP_IN, CB_SPREAD_ZERO, CB_SPREAD_POS, CB_LO, CB_HI, CB_INSIDE, CB_UNTOUCHED, CB_TOUCHED, CB_S1_ZERO, CB_S1_POS,
    CB_S2_ZERO, CB_S2_POS, CB_COUNT
};

// Step 5a on the history h of pixel (x, r).  cur: the current frame's accum around the pixel, read through
//     cur.colour(i, inside, C[3])   the colour sums of the window's record i, or (+0, +0, +0) for a tap that is not inside
// with the pixel itself at record `centre` and its lower neighbour at centre + pitch (the film's planes on the host: centre = r W + x,
// pitch = W, and a record that is not inside is not read; the workgroup's staged window on the device, whose records outside the
// film hold +0).  The text skips a tap outside the film; here such a tap adds +0 to A and B and nothing to n, which leaves the
// same bits without a branch a tap: A and B start at +0 and are never -0 (a sum that cancels rounds to +0), and x + (+0) = x for
// every other x.  Returns the amount; h is changed only if a channel was clipped.
template <int RADIUS, class CurWindow, class ClipCount>
RT_HOST_DEVICE float clip_history(const Frame& f, const Clip& clip, uint32_t x, uint32_t r, const CurWindow& cur, size_t centre,
                                  size_t pitch, const ClipCount& count, History& h) {
    uint32_t n = 0u;
    float A[3] = {0.0f, 0.0f, 0.0f}, B[3] = {0.0f, 0.0f, 0.0f};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dy = -RADIUS; dy <= RADIUS; dy++) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int dx = -RADIUS; dx <= RADIUS; dx++) {
            const int qx = (int)x + dx, qy = (int)r + dy;
            const bool inside = qx >= 0 && qx < (int)f.W && qy >= 0 && qy < (int)f.R;
            count(inside ? CB_TAP_IN : CB_TAP_OUT);
            float Cq[3];
            cur.colour(centre + (size_t)dy * pitch + (size_t)dx, inside, Cq);         // (modulo 2^64: a step back is a step back)
            n += inside ? 1u : 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 0; k < 3; k++) {
                A[k] = A[k] + Cq[k];
                B[k] = B[k] + Cq[k] * Cq[k];
            }
        }
    }
    const float nf = (float)n;
    float Cc[3];
    bool touched = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 3; k++) {
        const float mu = A[k] / nf;
        float d = B[k] / nf - mu * mu;
        if (d > 0.0f) {
            count(CB_SPREAD_POS);
        } else {
            d = 0.0f;
            count(CB_SPREAD_ZERO);
        }
        const float s = clip.gamma * __builtin_sqrtf(d);
        const float lo = mu - s, hi = mu + s;
        if (h.C[k] < lo) {                                        // (a NaN bound fails both comparisons)
            Cc[k] = lo;
            touched = true;
            count(CB_LO);
        } else if (h.C[k] > hi) {
            Cc[k] = hi;
            touched = true;
            count(CB_HI);
        } else {
            Cc[k] = h.C[k];
            count(CB_INSIDE);
        }
    }
    if (!touched) {
        count(CB_UNTOUCHED);
        return 0.0f;
    }
    count(CB_TOUCHED);
    const float y = (h.C[0] + h.C[1]) + h.C[2], yc = (Cc[0] + Cc[1]) + Cc[2];
    float S1 = h.S1 + (yc - y);
    if (S1 > 0.0f) {
        count(CB_S1_POS);
    } else {
        S1 = 0.0f;
        count(CB_S1_ZERO);
    }
    float S2 = h.S2 + (S1 * S1 - h.S1 * h.S1) / clip.e;
    if (S2 > 0.0f) {
        count(CB_S2_POS);
    } else {
        S2 = 0.0f;
        count(CB_S2_ZERO);
    }
    const float amount = (__builtin_fabsf(h.C[0] - Cc[0]) + __builtin_fabsf(h.C[1] - Cc[1])) + __builtin_fabsf(h.C[2] - Cc[2]);
    h.C[0] = Cc[0];
    h.C[1] = Cc[1];
    h.C[2] = Cc[2];
    h.S1 = S1;
    h.S2 = S2;
    return amount;
}

// One pixel of one frame of a clipping call: the gather, the clip, then the blend.  accumulate_pixel's arguments, the clip's, and
// the amount (+0 for a pixel with no history).
template <int RADIUS, class PrevState, class CurWindow, class Count, class ClipCount>
RT_HOST_DEVICE void accumulate_pixel_clip(const Frame& f, const Clip& clip, uint32_t x, uint32_t r, const float C[3], const float M[2],
                                          float depth, uint32_t hits, uint32_t idx, const float* n, const PrevState& prev,
                                          const CurWindow& cur, size_t centre, size_t pitch, const Count& count,
                                          const ClipCount& clip_count, float outC[3], float outM[2], float& outN, float& outZ,
                                          float& amount) {
    outC[0] = C[0];
    outC[1] = C[1];
    outC[2] = C[2];
    outM[0] = M[0];
    outM[1] = M[1];
    outN = 1.0f;
    amount = 0.0f;
    History h;
    if (!gather_pixel(f, x, r, depth, hits, idx, n, prev, count, h, outZ)) return;
    amount = clip_history<RADIUS>(f, clip, x, r, cur, centre, pitch, clip_count, h);
    blend_pixel(f, C, M, h, count, outC, outM, outN);
}

// ---- host: the two cameras of a frame (rt_history.h "Cameras") ---------------------------------------------------------------------
// what rtplan::fill_camera writes
struct CamFill {
    float org[3], hor[3], ver[3], llc[3];
    float lens_radius, focus_distance, u_den, v_den;
};

// H, y0, the current camera's vectors and, with a previous request pq, the previous camera's basis and plane, into f (have_prev is
// set accordingly).  cam, pcam: nullptr for the reference camera.  false: a pose make_pose refuses.
inline bool set_cameras(Frame& f, const rt_tile_request& rq, const rt_camera* cam, const rt_tile_request* pq, const rt_camera* pcam) {
    f.H = rq.height;
    f.y0 = rq.division_no * (rq.height / rq.divisions);
    rtplan::Pose ps;
    if (cam && !rtplan::make_pose(*cam, ps)) return false;
    CamFill c;
    rtplan::fill_camera(rq, cam ? &ps : nullptr, c);
    for (int i = 0; i < 3; i++) {
        f.cur.org[i] = c.org[i];
        f.cur.llc[i] = c.llc[i];
        f.cur.hor[i] = c.hor[i];
        f.cur.ver[i] = c.ver[i];
    }
    f.cur.u_den = c.u_den;
    f.cur.v_den = c.v_den;
    f.have_prev = pq ? 1u : 0u;
    if (!pq) return true;
    rt_camera ref = {};                                           // rt_camera_defaults' pose
    ref.target[2] = -1.0f;
    ref.up[1] = 1.0f;
    if (!rtplan::make_pose(pcam ? *pcam : ref, ps)) return false;
    rtplan::fill_camera(*pq, &ps, c);                             // (u_den, v_den)
    for (int i = 0; i < 3; i++) {
        f.prev.org[i] = ps.origin[i];
        f.prev.u[i] = ps.u[i];
        f.prev.v[i] = ps.v[i];
        f.prev.w[i] = ps.w[i];
    }
    const float aspect_ratio = (float)pq->width / (float)pq->height;
    f.prev.vh = 2.0f * std::tan(pq->fov / 2.0f);                  // as fill_camera takes them
    f.prev.vw = aspect_ratio * f.prev.vh;
    f.prev.f = pq->focal_length;
    f.prev.u_den = c.u_den;
    f.prev.v_den = c.v_den;
    return true;
}

}  // namespace rthm
