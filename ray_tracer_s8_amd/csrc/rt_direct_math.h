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

// rgb = (albedo * emission) * W per channel
RT_HOST_DEVICE Vec radiance(Vec albedo, float emission, float W) {
    return Vec{(albedo.x * emission) * W, (albedo.y * emission) * W, (albedo.z * emission) * W};
}

}  // namespace rtdl
