// rt_nee.hip.h — gfx950 next-event-estimation integrator for caller rays (rt_scene_trace_nee*, rt_tile.h "next-event estimation";
// DESIGN.md 4.18).
//
// One lane per caller ray: `spp` samples of a path of at most max_bounces + 1 segments, with one light sample after every hit of
// roughness 0 but the last, summed in f32 in sample order.  Persistent waves stride over the batch as in rt_trace_kernel.  What the
// composed loop of rt_scene_bounce and rt_scene_direct writes to memory between its launches — rays, states, hit records, bounce
// records, samples, lists — stays in registers here, and the fold is FORWARD: the throughput T and the colour c are carried along,
// so there is no path stack.
//
// ONE closest_hit site.  A lane is in one of two phases: its ray (o, d) is a path segment, or it is the shadow ray of the light
// sample it has just drawn, in which case the scattered direction the path goes on with waits in `nd` (both rays start at the hit
// point) and the sample's contribution, already weighted, waits in `add`.  Every trip of the loop walks the lane's ray through the
// one site, whichever kind it is, and then resolves it.  A wave therefore never runs a walk for its path segments with the lanes
// that have a shadow ray idle, and then another for the shadow rays with the rest idle: lanes in different phases share the walk.
// A lane whose sample faces away, or whose hit is rough, goes straight on to its next segment.  In the LOBE instances (the scene's
// RT_GLOSSY_MIS, mode RT_NEE_MIS only) a hit of roughness 0 < rho < 1 seen from its front takes the light sample too, weighted by the
// density of the reference's scatter lobe (rt_lobe_math.h), and the lane keeps the lobe factor of the direction the
// scatter took for the emitter the bounce may reach next.
//
// Every step is a shared one, so the bits are those of the composed entry points: closest_hit, hit_normal, sky_colour,
// unit_sphere_pair, scattered_dir, u01 and the RNG load / store / seed of rt_path_steps.hip.h; the light
// sample is light_sample, rtdl::light_geometry and sample_weight, the steps rt_direct_kernel calls; the two MIS weights and the
// samplable test of rt_nee_math.h; the lobe, its factor and the sampled-class rule of rt_lobe_math.h.
//
// LDS per lane (rtplan::plan_nee): the walk's stack, (bvh depth + 1) u32 entries (engine 2); entry e of lane tid at [e * 256 + tid].
// No per-scene scratch: launches on different streams may overlap.
#pragma once
#include "rt_lobe_math.h"
#include "rt_nee_math.h"
#include "rt_path_steps.hip.h"

namespace rtk {

struct NParams : SceneRefs {
    const float4* rays;          // [2 n]: rt_ray (o, t_min) (d, t_max)
    float* rgb;                  // [3 n]: the f32 sum of the ray's sample colours
    uint32_t* segments;          // [n] path segments, or nullptr
    uint32_t* shadow;            // [n] shadow rays, or nullptr
    uint64_t* rng_state;         // [4 n] xoshiro256++ state per ray (read and written back), or nullptr: the seeded streams
    uint64_t n;
    uint64_t seed;               // rng_state == nullptr: sample s of ray i draws from seed_from_u64(seed + 4 PHI (i spp + s))
    uint32_t spp, max_bounces;
    uint32_t as_given;           // 1: the first direction is taken bit for bit (RT_TRACE_RAY_AS_GIVEN), 0: Ray::new normalises it
    uint32_t mis;                // 1: RT_NEE_MIS, 0: RT_NEE_LIGHT_ONLY
    const float4* mat;           // [n_sph + n_tri] (albedo r, g, b, roughness)
    const float* emis;           // [n_sph + n_tri]
    const uint32_t* lights;      // [n_lights] the emitters (library primitive numbers) in ascending world position
    uint32_t n_lights;           // M <= rtdl::MAX_LIGHTS
    LightTableRefs table;        // RT_FLAG_LIGHTS_BY_POWER (PICK_POWER instances only)
};

// The size rt_direct_math.h's weights take for primitive `prim`: a sphere's radius, a triangle's area.
template <class P>
__device__ __forceinline__ float light_size(const P& p, uint32_t prim) {
    if (prim < p.n_sph) return at32(p.geom_r, prim).w;
    const float* tv = p.tri + 9 * (size_t)(prim - p.n_sph);
    return rtdl::triangle_area(rtdl::Vec{tv[0], tv[1], tv[2]}, rtdl::Vec{tv[3], tv[4], tv[5]}, rtdl::Vec{tv[6], tv[7], tv[8]});
}

// ENGINE 2: the walk; 1: the scan with consider<MODE> (MODE 0 plain linear semantics, 2 BVH semantics).  PICK: the pick rule, which
// also decides what stands for (float)M in W and in W' (the inverse probability of the emitter sampled, and of the emitter hit).
// SHAPE: how a sphere light is sampled (the scene's rt_scene_set_light_sampling); SHAPE_CONE also views an emissive sphere the bounce
// reached from the segment's origin o — exactly the previous hit point — so that W' speaks of the p_light the sample there had.
// LOBE: 1 under the scene's RT_GLOSSY_MIS in mode RT_NEE_MIS (rt_scene_set_glossy_sampling); the LOBE = 0 instances are the code they
// were before the setting existed.
template <int ENGINE, int MODE, int PICK, int SHAPE, int LOBE>
__global__ __launch_bounds__(256) void rt_nee_kernel(const NParams p) {
    extern __shared__ uint32_t nstack[];                 // [depth + 1][256] (engine 2)
    const uint32_t tid = threadIdx.x, bs = blockDim.x;
    unsigned long long n_rays = 0, n_tests = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * bs + tid; i < p.n; i += (uint64_t)gridDim.x * bs) {
        const CallerRay r = load_caller_ray(p.rays + 2 * i, p.as_given != 0);
        Rng rng;
        if (p.rng_state) load_rng(p.rng_state + 4 * i, rng);
        float sum_r = 0.f, sum_g = 0.f, sum_b = 0.f;
        uint32_t segs = 0, shad = 0;
        for (uint32_t smp = 0; smp < p.spp; smp++) {
            if (!p.rng_state) rng = sample_seed(p, i, smp);
            V3 o = r.o, d = r.d;                         // the ray the next trip walks
            V3 T = mk(1.f, 1.f, 1.f), c = mk(0.f, 0.f, 0.f);
            V3 n_prev = mk(0.f, 0.f, 0.f);               // the normal of the last hit that scattered
            V3 nd = mk(0.f, 0.f, 0.f), add = mk(0.f, 0.f, 0.f);   // shadow phase: the path's next direction; the sample's T * D (* wl)
            uint32_t k = 0, lprim = 0;
            bool sampled = false, shadow = false;
            bool lobed = false;                          // LOBE: the last hit that scattered was lobe-sampled, and this is the lobe factor
            float cg_prev = 0.f;                         //   of the direction its scatter took (0 or NaN: not in the lobe)
            for (;;) {
                const RayAux aux = ray_aux(d, p.full_chain != 0);
                const Hit h = closest_hit<ENGINE, MODE, false>(p, o, d, r.t_min, r.t_max, aux, nstack, tid, bs, n_tests);
                if (shadow) {
                    // ================= the shadow ray resolved: LIT exactly when it reaches the emitter sampled =================
                    shad++;
                    if (h.idx == (int)lprim) {
                        c.x = c.x + add.x;
                        c.y = c.y + add.y;
                        c.z = c.z + add.z;
                    }
                    d = nd;                                                            // on with the path, from the same point
                    shadow = false;
                    continue;
                }
                // ================= one path step, as rt_scene_bounce specifies it =================
                segs++;
                if (h.idx < 0) {                                                       // MISSED
                    const V3 sky = sky_colour(d);
                    c.x = c.x + T.x * sky.x;
                    c.y = c.y + T.y * sky.y;
                    c.z = c.z + T.z * sky.z;
                    break;
                }
                const uint32_t prim = (uint32_t)h.idx;
                const V3 hp = o + h.t * d;                                             // Ray::at (ray.rs:147-149)
                const V3 nh = hit_normal(p, prim, hp);
                const float em = at32(p.emis, prim);
                const float4 ma = at32(p.mat, prim);
                if (em > 0.0f) {                                                       // EMITTED
                    float ex = ma.x * em, ey = ma.y * em, ez = ma.z * em;
                    bool add_it = true;
                    if (k != 0 && sampled) {
                        // the light strategy's view of this point: could the sample of the step before have drawn it?
                        const bool sphere = prim < p.n_sph;
                        bool cone_view = false;
                        const bool in_lobe = cg_prev > 0.0f;                            // LOBE: cg(d) takes the place of cs', and d must be in the lobe
                        if (SHAPE == SHAPE_CONE && sphere) {
                            const float4 g = at32(p.geom_r, prim);
                            rtnee::ConeView cv = rtnee::emitter_view_cone(dvec(o), dvec(n_prev), dvec(d), rtdl::Vec{g.x, g.y, g.z}, g.w);
                            cone_view = cv.in_regime;
                            if constexpr (LOBE != 0) {
                                if (lobed) {
                                    cv.samplable = cv.samplable && in_lobe;
                                    cv.cs = cg_prev;
                                }
                            }
                            if (cv.samplable) {
                                add_it = p.mis != 0;                                   // LIGHT_ONLY: that sample stood for it
                                if (add_it) {
                                    const float wb = rtnee::bounce_weight(
                                        rtnee::cone_view_weight(cv, PICK == PICK_POWER ? p.table.light_ip[prim] : (float)p.n_lights));
                                    ex = ex * wb;
                                    ey = ey * wb;
                                    ez = ez * wb;
                                }
                            }
                        }
                        rtnee::View v = rtnee::emitter_view(dvec(n_prev), dvec(d), dvec(nh), h.dist, sphere);
                        if constexpr (LOBE != 0) {
                            if (lobed) {
                                v.samplable = v.samplable && in_lobe;
                                v.cs = cg_prev;
                            }
                        }
                        if (!cone_view && v.samplable) {
                            add_it = p.mis != 0;                                       // LIGHT_ONLY: that sample stood for it
                            if (add_it) {
                                const float size = light_size(p, prim);
                                const float Wv = PICK == PICK_POWER ? rtnee::view_weight_ip(v, sphere, size, p.table.light_ip[prim])
                                                                    : rtnee::view_weight(v, sphere, size, p.n_lights);
                                const float wb = rtnee::bounce_weight(Wv);
                                ex = ex * wb;
                                ey = ey * wb;
                                ez = ez * wb;
                            }
                        }
                    }
                    if (add_it) {
                        c.x = c.x + T.x * ex;
                        c.y = c.y + T.y * ey;
                        c.z = c.z + T.z * ez;
                    }
                    break;
                }
                T.x = T.x * ma.x;                                                      // SCATTERED
                T.y = T.y * ma.y;
                T.z = T.z * ma.z;
                float x1, x2, sm;
                unit_sphere_pair(rng, x1, x2, sm);                                     // drawn also at the last depth (main.rs:119)
                if (k == p.max_bounces) break;
                k++;
                const V3 dn = scattered_dir(d, nh, ma.w, x1, x2, sm);
                rtlobe::Lobe lobe{rtdl::Vec{0.f, 0.f, 0.f}, 0.f, 0.f};
                if constexpr (LOBE != 0) {
                    const rtdl::Vec gd = rtlobe::glossy_dir(dvec(d), dvec(nh));        // the glossy_dir scattered_dir formed, the same bits
                    const uint32_t cls = p.n_lights > 0 ? rtlobe::sampled_class(ma.w, rtdl::dot3(dvec(nh), gd)) : (uint32_t)rtlobe::CLASS_NONE;
                    sampled = cls != rtlobe::CLASS_NONE;
                    lobed = cls == rtlobe::CLASS_LOBE;
                    if (lobed) {
                        lobe = rtlobe::lobe_of(dvec(nh), gd, ma.w);
                        cg_prev = rtlobe::lobe_factor_scatter(lobe, dvec(unit_sphere_vec(x1, x2, sm))).cg;   // the us scattered_dir used
                    }
                } else {
                    sampled = ma.w == 0.0f && p.n_lights > 0;
                }
                o = hp;                                                                // origin exactly P, of either ray
                d = dn;
                n_prev = nh;
                if (!sampled) continue;
                // ================= one light sample, as rt_scene_direct specifies it for the record (P, n, prim) =================
                const typename SampleOf<SHAPE>::type ls = light_sample<PICK, SHAPE>(p, rng, hp, nh);
                const rtdl::Geometry g = sample_geometry(ls, hp, nh);
                if (!g.facing) continue;                                               // FACING_AWAY: no ray, straight on
                const float4 la = at32(p.mat, ls.prim);
                float W;
                if constexpr (LOBE != 0) {
                    if (lobed) {                                                       // cg(wn) in the place of cs; outside the lobe: no ray
                        const rtlobe::LobeFactor lfs = rtlobe::lobe_factor(lobe, g.w);
                        rtdl::Geometry gl = g;
                        gl.cs = lfs.cg;
                        W = sample_weight<PICK, SHAPE>(ls, gl, p.n_lights);
                        if (!rtlobe::lobe_sample_taken(lfs, W)) continue;
                    } else {
                        W = sample_weight<PICK, SHAPE>(ls, g, p.n_lights);
                    }
                } else {
                    W = sample_weight<PICK, SHAPE>(ls, g, p.n_lights);
                }
                rtdl::Vec D = rtdl::radiance(rtdl::Vec{la.x, la.y, la.z}, at32(p.emis, ls.prim), W);
                if (p.mis) {
                    const float wl = rtnee::light_weight(W);
                    D = rtdl::Vec{D.x * wl, D.y * wl, D.z * wl};
                }
                add = mk(T.x * D.x, T.y * D.y, T.z * D.z);                             // added if the shadow ray is LIT
                lprim = ls.prim;
                nd = dn;
                d = v3of(g.w);                                                         // Ray::new(P, L - P)
                shadow = true;
            }
            sum_r = sum_r + c.x;
            sum_g = sum_g + c.y;
            sum_b = sum_b + c.z;
        }
        p.rgb[3 * i + 0] = sum_r;
        p.rgb[3 * i + 1] = sum_g;
        p.rgb[3 * i + 2] = sum_b;
        if (p.segments) p.segments[i] = segs;
        if (p.shadow) p.shadow[i] = shad;
        if (p.rng_state) store_rng(p.rng_state + 4 * i, rng);
        n_rays += (unsigned long long)segs + shad;
    }
    flush_counters(p.counters, n_rays, n_tests, tid);
}

using NeeFn = void (*)(const NParams);
// rt_kernels_nee.hip; cone: the scene's setting is RT_LIGHTS_CONE; lobe: it is RT_GLOSSY_MIS and the mode RT_NEE_MIS; nullptr for a
// combination that does not exist
NeeFn nee_kernel(int engine, int scan_mode, bool by_power, bool cone, bool lobe);

}  // namespace rtk
