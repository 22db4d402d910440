// rt_direct_math.h — the sampling arithmetic of direct lighting (rt_tile.h "direct lighting"): the emitter pick, the
// point on a sphere or a triangle light, the two cosines and the weight of the estimate.  Plain C++ that compiles as HIP device code
// (rt_direct.hip.h) and under g++ -ffp-contract=off (tests/host/direct_host.cpp), so the kernel and the CPU harness run the same
// lines.  Every operation is one IEEE f32 rounding in the order rt_tile.h writes it: no fused multiply-add (the build's
// -ffp-contract=off), correctly rounded division and sqrt (hipcc's default, SSE on the host), no transcendental function.  The draws
// themselves (u01, the UnitSphere pair) and the triangle's normal come from the caller: the kernel takes them from the shared path
// steps, the harness from its input records.
#pragma once
#include <stdint.h>

#include "rt_consts.h"

namespace rtdl {

constexpr uint32_t MAX_LIGHTS = 1u << 23;        // every M up to here is an exact f32, and u * (float)M truncates to a pick <= M
constexpr float PI_F32 = 3.14159274101257324f;   // std::f32::consts::PI

struct Vec {
    float x, y, z;
};

// glam's dot3 order, as everywhere in the library: (x x' + y y') + z z'
RT_HOST_DEVICE float dot3(Vec a, Vec b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RT_HOST_DEVICE Vec sub3(Vec a, Vec b) { return Vec{a.x - b.x, a.y - b.y, a.z - b.z}; }

// k = min((uint32_t)(u * (float)M), M - 1) for u in [0, 1) and 1 <= M <= MAX_LIGHTS (the product is below 2^23 + 1: the cast is exact)
RT_HOST_DEVICE uint32_t pick_light(float u, uint32_t M) {
    const uint32_t k = (uint32_t)(u * (float)M);
    return k < M - 1u ? k : M - 1u;
}

// ---- light selection by power (RT_FLAG_LIGHTS_BY_POWER): the table arithmetic the host runs once per scene
// (rtscene::light_table) and the pick the kernels run per sample.
// lum = ((ar + ag) + ab) * emission
RT_HOST_DEVICE float light_luminance(Vec albedo, float emission) { return ((albedo.x + albedo.y) + albedo.z) * emission; }

// area of a sphere light: (4 (r r)) PI
RT_HOST_DEVICE float sphere_light_area(float r) { return (4.0f * (r * r)) * PI_F32; }

// q = lum * area, and 0 unless q > 0: a NaN, a zero or negative albedo sum, a zero radius and a degenerate triangle have no power
RT_HOST_DEVICE float light_power(float lum, float area) {
    const float q = lum * area;
    return q > 0.0f ? q : 0.0f;
}

// The table is degenerate unless its total is positive and finite: then the pick is the uniform one and p_k = 1 / M.
RT_HOST_DEVICE bool table_degenerate(float total) { return !(total > 0.0f && total < __builtin_inff()); }

// p = 0.5 (1 / (float)M) + 0.5 (w / total): half uniform, half by power, so p >= 1 / (2M) whatever the running sum rounded away
RT_HOST_DEVICE float mixture_probability(float w, float total, uint32_t M) {
    return 0.5f * (1.0f / (float)M) + 0.5f * (w / total);
}

// The pick by power from one u in [0, 1) over the running sums c[0 .. M - 1] (non-decreasing, total = c[M - 1]), 1 <= M <= MAX_LIGHTS.
// u < 0.5: the uniform pick of u + u (exact).  Otherwise x = ((u - 0.5) + (u - 0.5)) * total (the subtraction and the doubling are
// exact for a 24-bit u) and k is the smallest index with x < c[k], or M - 1 when there is none: ceil(log2 M) halvings whatever x is,
// so the lanes of a wave leave the loop together, then one comparison.  A degenerate table takes pick_light(u, M), the undoubled draw.
RT_HOST_DEVICE uint32_t pick_light_power(float u, uint32_t M, const float* c, float total) {
    if (table_degenerate(total)) return pick_light(u, M);
    if (u < 0.5f) return pick_light(u + u, M);
    const float x = ((u - 0.5f) + (u - 0.5f)) * total;
    uint32_t base = 0, len = M;
    while (len > 1u) {                                   // the answer is in [base, base + len]
        const uint32_t half = len >> 1;
        if (!(x < c[base + half - 1u])) base += half;
        len -= half;
    }
    const uint32_t k = x < c[base] ? base : base + 1u;
    return k < M - 1u ? k : M - 1u;
}

// L = c + r * us, the point of the UnitSphere draw `us` on the sphere (c, r); its outward normal there is us itself
RT_HOST_DEVICE Vec sphere_point(Vec c, float r, Vec us) { return Vec{c.x + r * us.x, c.y + r * us.y, c.z + r * us.z}; }

// The fold of the two triangle draws onto the half of the unit square that maps to the triangle: if u1 + u2 > 1, both become 1 - u.
RT_HOST_DEVICE void fold_pair(float& u1, float& u2) {
    if (u1 + u2 > 1.0f) {
        u1 = 1.0f - u1;
        u2 = 1.0f - u2;
    }
}

// L = a + (u1 * (b - a) + u2 * (c - a)) for the folded pair
RT_HOST_DEVICE Vec triangle_point(Vec a, Vec b, Vec c, float u1, float u2) {
    const Vec e1 = sub3(b, a), e2 = sub3(c, a);
    return Vec{a.x + (u1 * e1.x + u2 * e2.x), a.y + (u1 * e1.y + u2 * e2.y), a.z + (u1 * e1.z + u2 * e2.z)};
}

// A = 0.5 * |(a - b) x (a - c)|, the cross product as hit_normal forms it
RT_HOST_DEVICE float triangle_area(Vec a, Vec b, Vec c) {
    const Vec p = sub3(a, b), q = sub3(a, c);
    const Vec n = Vec{p.y * q.z - p.z * q.y, p.z * q.x - p.x * q.z, p.x * q.y - p.y * q.x};
    return 0.5f * __builtin_sqrtf(dot3(n, n));
}

// The geometry of one sample: from the hit point P with the record's normal n (as given, not flipped) to the light point L with the
// light's normal nl.
struct Geometry {
    Vec v;             // L - P: the shadow ray is Ray::new(P, v)
    float d2;          // (vx vx + vy vy) + vz vz
    Vec w;             // v / sqrt(d2), which is the direction Ray::new gives the shadow ray
    float cs, cl;      // n . w;  -(nl . w) for a sphere light, |nl . w| for a triangle light
    bool facing;       // cs > 0 and cl > 0 and d2 finite and not 0: only then is a shadow ray traced
};

RT_HOST_DEVICE Geometry light_geometry(Vec P, Vec n, Vec L, Vec nl, bool sphere) {
    Geometry g;
    g.v = sub3(L, P);
    g.d2 = dot3(g.v, g.v);
    const float len = __builtin_sqrtf(g.d2);
    g.w = Vec{g.v.x / len, g.v.y / len, g.v.z / len};
    g.cs = dot3(n, g.w);
    const float c = dot3(nl, g.w);
    g.cl = sphere ? -c : __builtin_fabsf(c);
    g.facing = g.cs > 0.0f && g.cl > 0.0f && g.d2 > 0.0f && g.d2 < __builtin_inff();
    return g;
}

// W of a sphere light of radius r: ((cs cl) ((4 (r r)) (float)M)) / d2.  Area 4 pi r^2 over the Lambertian pi: the pi cancel.
RT_HOST_DEVICE float sphere_weight(float cs, float cl, float r, uint32_t M, float d2) {
    return ((cs * cl) * ((4.0f * (r * r)) * (float)M)) / d2;
}

// W of a triangle light of area A: ((cs cl) (A (float)M)) / (PI d2)
RT_HOST_DEVICE float triangle_weight(float cs, float cl, float A, uint32_t M, float d2) {
    return ((cs * cl) * (A * (float)M)) / (PI_F32 * d2);
}

// ... and with the inverse probability ip of the emitter picked in the place of (float)M (RT_FLAG_LIGHTS_BY_POWER; the uniform pick
// has ip = (float)M): ((cs cl) ((4 (r r)) ip)) / d2 and ((cs cl) (A ip)) / (PI d2)
RT_HOST_DEVICE float sphere_weight_ip(float cs, float cl, float r, float ip, float d2) { return ((cs * cl) * ((4.0f * (r * r)) * ip)) / d2; }
RT_HOST_DEVICE float triangle_weight_ip(float cs, float cl, float A, float ip, float d2) { return ((cs * cl) * (A * ip)) / (PI_F32 * d2); }

// ---- cone sampling of sphere lights (RT_LIGHTS_CONE; rt_tile.h "cone sampling of sphere lights"): a direction in the
// cone the sphere (c, r) subtends from P, from the accepted pair (x1, x2) of the UnitSphere draw and s = x1 x1 + x2 x2 — s is uniform
// on [0, 1) and (x1, x2) / sqrt(s) a uniform azimuth, so the sample takes no draw of its own and no transcendental function.
constexpr float CONE_Q_MIN = 0.0009765625f;      // 2^-10: below it (r / dc < 1/32) the area sample, which has no rim, is used

// The sample of a point with q = r2 / dc2 is a cone sample when 2^-10 <= q < 1; a NaN, a point inside or on the sphere, radius 0,
// dc2 = 0 or inf are not.
RT_HOST_DEVICE bool cone_regime(float q) { return q >= CONE_Q_MIN && q < 1.0f; }

// The point as the light sees it: a = c - P, dc2 = a.a, r2 = r r, q = r2 / dc2
struct ConeAxis {
    Vec a;
    float dc2, r2, q;
};
RT_HOST_DEVICE ConeAxis cone_axis(Vec P, Vec c, float r) {
    ConeAxis x;
    x.a = sub3(c, P);
    x.dc2 = dot3(x.a, x.a);
    x.r2 = r * r;
    x.q = x.r2 / x.dc2;
    return x;
}

// omc = 1 - cos(theta_max) without cancellation: ctm = sqrt(1 - q); omc = q / (1 + ctm)
RT_HOST_DEVICE float cone_omc(float q) {
    const float ctm = __builtin_sqrtf(1.0f - q);
    return q / (1.0f + ctm);
}

struct Cone {
    Vec v;             // the direction, |v.v - 1| <= 2^-18 while dc2 >= 2^-130 (w takes on a subnormal dc2's lost bits): Ray::new(P, v)
    float omc;         // 1 - cos(theta_max)
    float dc2, dc;     // a.a and its root
    float ct, st;      // cosine and sine of the angle to the axis
};

// In the regime (cone_regime(cone_axis(P, c, r).q)).  The frame about the axis w = a / dc is Duff et al. 2017, branch-free.
RT_HOST_DEVICE Cone cone_sample(Vec P, Vec c, float r, float x1, float x2, float s) {
    const ConeAxis ax = cone_axis(P, c, r);
    Cone k;
    k.dc2 = ax.dc2;
    k.omc = cone_omc(ax.q);
    const float e = s * k.omc;
    k.ct = 1.0f - e;
    k.st = __builtin_sqrtf(e * (2.0f - e));
    const float rs = __builtin_sqrtf(s);
    const float cp = s > 0.0f ? x1 / rs : 0.0f;
    const float sp = s > 0.0f ? x2 / rs : 0.0f;
    k.dc = __builtin_sqrtf(ax.dc2);
    const Vec w{ax.a.x / k.dc, ax.a.y / k.dc, ax.a.z / k.dc};
    const float sg = __builtin_copysignf(1.0f, w.z);
    const float A = -1.0f / (sg + w.z);
    const float B = (w.x * w.y) * A;
    const Vec t1{1.0f + (sg * (w.x * w.x)) * A, sg * B, -(sg * w.x)};
    const Vec t2{B, sg + (w.y * w.y) * A, -w.y};
    const float ka = k.st * cp, kb = k.st * sp;
    k.v = Vec{(ka * t1.x + kb * t2.x) + k.ct * w.x, (ka * t1.y + kb * t2.y) + k.ct * w.y, (ka * t1.z + kb * t2.z) + k.ct * w.z};
    return k;
}

// The geometry of a cone sample: wn = v / sqrt(v.v) is the direction Ray::new gives the shadow ray, cs = n.wn, and the sample faces the
// light exactly when cs > 0 — every direction of the cone meets the front of the sphere, so there is no cl (it is set to 1, unread).
RT_HOST_DEVICE Geometry cone_geometry(Vec n, Vec v) {
    Geometry g;
    g.v = v;
    g.d2 = dot3(v, v);
    const float len = __builtin_sqrtf(g.d2);
    g.w = Vec{v.x / len, v.y / len, v.z / len};
    g.cs = dot3(n, g.w);
    g.cl = 1.0f;
    g.facing = g.cs > 0.0f;
    return g;
}

// W = (cs (omc + omc)) ip: cs Omega / pi over p_k, Omega = 2 pi omc the cone's solid angle; at most 2 ip.  ip = (float)M for the
// uniform pick.
RT_HOST_DEVICE float cone_weight(float cs, float omc, float ip) { return (cs * (omc + omc)) * ip; }

// Where the direction wn meets the sphere: h = r2 - dc2 (st st), clamped at 0; ts = dc ct - sqrt(h); L = P + ts wn
RT_HOST_DEVICE Vec cone_point(Vec P, Vec wn, float r, const Cone& k) {
    float h = r * r - k.dc2 * (k.st * k.st);
    h = h > 0.0f ? h : 0.0f;
    const float ts = k.dc * k.ct - __builtin_sqrtf(h);
    return Vec{P.x + ts * wn.x, P.y + ts * wn.y, P.z + ts * wn.z};
}

// rgb = (albedo * emission) * W per channel
RT_HOST_DEVICE Vec radiance(Vec albedo, float emission, float W) {
    return Vec{(albedo.x * emission) * W, (albedo.y * emission) * W, (albedo.z * emission) * W};
}

}  // namespace rtdl
