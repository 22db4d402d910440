// rt_nee_math.h — what the next-event-estimation integrator adds to the sampling arithmetic of rt_direct_math.h (rt_tile.h "next-event
// estimation"): the two weights of the balance heuristic and the light strategy's view of a hit point the bounce
// reached by itself.  Plain C++ that compiles as HIP device code (rt_nee.hip.h) and under g++ -ffp-contract=off
// (tests/host/nee_host.cpp), so the kernel and the CPU harness run the same lines.  Every operation is one IEEE f32 rounding in the
// order rt_tile.h writes it.
#pragma once
#include "rt_direct_math.h"

namespace rtnee {

// W of a light sample is (cs / pi) / p_light = p_bsdf / p_light, so the balance heuristic's weight of the LIGHT sample,
// p_light / (p_light + p_bsdf), is 1 / (1 + W): 1 at W = 0, 0 at W = +inf, never NaN for W >= 0.
RT_HOST_DEVICE float light_weight(float W) { return 1.0f / (1.0f + W); }

// ... and the weight of the BOUNCE that found the emitter, p_bsdf / (p_light + p_bsdf), is 1 - 1 / (1 + W'): 0 at W' = 0, 1 at +inf.
RT_HOST_DEVICE float bounce_weight(float W) { return 1.0f - 1.0f / (1.0f + W); }

// An emitter hit by the bounce, as the light sample of the hit before would have seen the same point: n the normal of the hit before
// (as rt_hit reports it), d the unit direction of the segment, nh this hit's rt_hit normal, distance its rt_hit.distance.
struct View {
    float cs, cl, d2;   // n . d;  -(nh . d) for a sphere, |nh . d| for a triangle;  distance * distance
    bool samplable;     // cs > 0 and cl > 0 and d2 finite and not 0: the light sample could have drawn this point (Geometry::facing)
};

RT_HOST_DEVICE View emitter_view(rtdl::Vec n, rtdl::Vec d, rtdl::Vec nh, float distance, bool sphere) {
    View v;
    v.cs = rtdl::dot3(n, d);
    const float c = rtdl::dot3(nh, d);
    v.cl = sphere ? -c : __builtin_fabsf(c);
    v.d2 = distance * distance;
    v.samplable = v.cs > 0.0f && v.cl > 0.0f && v.d2 > 0.0f && v.d2 < __builtin_inff();
    return v;
}

// W' of that point: the weight rt_direct_math.h gives a light sample with this geometry (size: the radius, or the triangle's area)
RT_HOST_DEVICE float view_weight(const View& v, bool sphere, float size, uint32_t M) {
    return sphere ? rtdl::sphere_weight(v.cs, v.cl, size, M, v.d2) : rtdl::triangle_weight(v.cs, v.cl, size, M, v.d2);
}

// ... and under RT_FLAG_LIGHTS_BY_POWER, with the inverse probability ip of the emitter hit
RT_HOST_DEVICE float view_weight_ip(const View& v, bool sphere, float size, float ip) {
    return sphere ? rtdl::sphere_weight_ip(v.cs, v.cl, size, ip, v.d2) : rtdl::triangle_weight_ip(v.cs, v.cl, size, ip, v.d2);
}

// ---- cone sampling of sphere lights (RT_LIGHTS_CONE): the view of an emissive sphere (c, r) the bounce reached from
// the point o with the normal n there, d the unit direction of the segment.  The regime depends on o and the sphere alone, so the
// light sample taken at o and this view speak of the same p_light.  Not in the regime: the caller takes emitter_view above.
struct ConeView {
    float cs, omc;      // n . d;  1 - cos(theta_max) of the sphere seen from o
    bool in_regime;     // rtdl::cone_regime(q') of q' = r2 / dc2'
    bool samplable;     // in the regime and cs > 0: the cone sample could have drawn this direction
};

RT_HOST_DEVICE ConeView emitter_view_cone(rtdl::Vec o, rtdl::Vec n, rtdl::Vec d, rtdl::Vec c, float r) {
    ConeView v;
    const rtdl::ConeAxis ax = rtdl::cone_axis(o, c, r);
    v.in_regime = rtdl::cone_regime(ax.q);
    v.cs = rtdl::dot3(n, d);
    v.omc = v.in_regime ? rtdl::cone_omc(ax.q) : 0.0f;
    v.samplable = v.in_regime && v.cs > 0.0f;
    return v;
}

// W' of that view: (cs' (omc' + omc')) ip_j, ip = (float)M for the uniform pick
RT_HOST_DEVICE float cone_view_weight(const ConeView& v, float ip) { return rtdl::cone_weight(v.cs, v.omc, ip); }

}  // namespace rtnee
