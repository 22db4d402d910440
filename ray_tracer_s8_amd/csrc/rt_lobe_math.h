// rt_lobe_math.h — the density of the reference's scatter at a glossy hit (rt_tile.h "next-event estimation", "Light samples at glossy
// hits"), which RT_GLOSSY_MIS puts in the place of the Lambertian cs of a light sample's weight.  Plain C++ that
// compiles as HIP device code (rt_nee.hip.h) and under g++ -ffp-contract=off (tests/host/lobe_host.cpp), like rt_nee_math.h beside
// it.  Every operation is one IEEE f32 rounding in the order rt_tile.h writes it.
//
// ray_color scatters along pre = diffuse + rho (glossy - diffuse) = c + r us with us uniform on the unit sphere, r = 1 - rho and
// c = r n + rho g: the direction from the origin to a uniform point of the sphere of radius r about c.  With b = c.w and
// kappa = |c|^2 - r^2 the ray of direction w meets that sphere when b > 0 and D = b^2 - kappa > 0, at t = b -+ sqrt(D), each
// intersection with the density t^2 / |cos| / (4 pi r^2), which sums to p(w) = (b^2 + D) / (2 pi r sqrt(D)).  cg = pi p(w).
#pragma once
#include "rt_direct_math.h"

namespace rtlobe {

// What the light strategy does at a scattering hit of roughness rho whose mirrored direction g has gn = n.g
enum { CLASS_NONE = 0u, CLASS_DIFFUSE = 1u, CLASS_LOBE = 2u };

// rho == 0: the diffuse sample (cs), as without the setting.  0 < rho < 1 and gn >= 0: lobe-sampled.  Anything else — rho >= 1,
// rho < 0, a NaN, a back-face hit (gn < 0, where the origin may lie inside the sphere) — takes no light sample and no draw.
RT_HOST_DEVICE uint32_t sampled_class(float rho, float gn) {
    if (rho == 0.0f) return CLASS_DIFFUSE;
    return (0.0f < rho && rho < 1.0f && gn >= 0.0f) ? CLASS_LOBE : CLASS_NONE;
}

// g = d - (2 (d.n)) n: the glossy_dir of the path step (rt_path_steps.hip.h scattered_dir), the same operations, so the same bits
RT_HOST_DEVICE rtdl::Vec glossy_dir(rtdl::Vec d, rtdl::Vec n) {
    const float k = 2.0f * rtdl::dot3(d, n);
    return rtdl::Vec{d.x - k * n.x, d.y - k * n.y, d.z - k * n.z};
}

struct Lobe {
    rtdl::Vec c;       // r n + rho g per component: two products and one sum
    float r;           // 1 - rho
    float kappa;       // |c|^2 - r^2 without cancellation: rho (rho gg + (r + r) gn)
};

// The lobe of a lobe-sampled hit: n the rt_hit normal, g the glossy_dir the step formed (d - (2 (d.n)) n), rho the roughness
RT_HOST_DEVICE Lobe lobe_of(rtdl::Vec n, rtdl::Vec g, float rho) {
    Lobe l;
    l.r = 1.0f - rho;
    l.c = rtdl::Vec{l.r * n.x + rho * g.x, l.r * n.y + rho * g.y, l.r * n.z + rho * g.z};
    const float gn = rtdl::dot3(n, g), gg = rtdl::dot3(g, g);
    l.kappa = rho * (rho * gg + (l.r + l.r) * gn);
    return l;
}

struct LobeFactor {
    float b, D;        // c.w;  b b - kappa
    bool in_lobe;      // b > 0 and D > 0: the scatter can take the direction w
    float cg;          // pi p(w) = (b b + D) / ((r + r) sqrt(D)); 0 outside the lobe
};

// The lobe factor of the unit direction w
RT_HOST_DEVICE LobeFactor lobe_factor(const Lobe& l, rtdl::Vec w) {
    LobeFactor f;
    f.b = rtdl::dot3(l.c, w);
    f.D = f.b * f.b - l.kappa;
    f.in_lobe = f.b > 0.0f && f.D > 0.0f;
    f.cg = f.in_lobe ? (f.b * f.b + f.D) / ((l.r + l.r) * __builtin_sqrtf(f.D)) : 0.0f;
    return f;
}

// The lobe factor of the direction the scatter itself took, from its UnitSphere vector us (the scattered point is X = c + r us).  In
// exact arithmetic this is lobe_factor of X / |X|; it is formed from the draw because D = b b - kappa cancels on the rim of the lobe, where
// the rounding of the direction alone puts up to 2^-9 of the scatter's own directions at D <= 0.  With q = c.us + r:
// sqrt(D) = r |q| / t, b = (kappa + r q) / t and t^2 = |X|^2 = kappa + 2 r q, none of which cancels there:
//   m = r q;  t = sqrt(kappa + (m + m));  cg = ((kappa + m) (kappa + m) + m m) / (((r + r) |m|) t),  in the lobe iff cg > 0.
// (m == 0, a NaN and an overflowing scatter give cg = 0 or NaN: not in the lobe.)
struct ScatterFactor {
    float m, t;        // r (c.us + r);  sqrt(kappa + (m + m))
    float cg;          // pi p(X / |X|)
    bool in_lobe;      // cg > 0
};

RT_HOST_DEVICE ScatterFactor lobe_factor_scatter(const Lobe& l, rtdl::Vec us) {
    ScatterFactor f;
    f.m = l.r * (rtdl::dot3(l.c, us) + l.r);
    f.t = __builtin_sqrtf(l.kappa + (f.m + f.m));
    const float km = l.kappa + f.m;
    f.cg = (km * km + f.m * f.m) / (((l.r + l.r) * __builtin_fabsf(f.m)) * f.t);
    f.in_lobe = f.cg > 0.0f;
    return f;
}

// A light sample of weight W at a lobe-sampled hit is taken only when its direction is in the lobe and W < inf (a NaN is not)
RT_HOST_DEVICE bool lobe_sample_taken(const LobeFactor& f, float W) { return f.in_lobe && W < __builtin_inff(); }

}  // namespace rtlobe
