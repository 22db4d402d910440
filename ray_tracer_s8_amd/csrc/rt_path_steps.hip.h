// rt_path_steps.hip.h — the path steps the caller-ray kernels share (DESIGN.md 1 "Device-side steps").
//
// The kernels beside the tile renderer (rt_query.hip.h, rt_trace.hip.h, rt_bounce.hip.h, rt_direct.hip.h, rt_nee.hip.h, rt_aov.hip.h,
// rt_camera.hip.h) each walk a part of the reference's path: the camera ray, the closest hit and its record, the shade, the scattered
// ray; two of them add a light sample.  Every such part is written ONCE, here, with the operations of the tile kernel
// (rt_kernel.hip.h) in the same order — so the same bits — and inlined into its callers.  A kernel derives its parameter block from
// SceneRefs (and CameraRefs), calls the steps and adds only what is its own.  The tile kernel keeps its merged camera / bounce arm
// and its single shared normalisation (measured divergence optimisations); what it shares with these steps is the device primitives
// they are made of.
#pragma once
#include "rt_direct_math.h"
#include "rt_kernel.hip.h"
#include "rt_tile.h"

namespace rtk {

// ------------------------------------------------------------------ parameter-block bases
// The scene as closest_hit / query_root read it: the base of every parameter block that finds first hits (QParams, TParams, BParams,
// AParams).  The host fills it in one place (rt_api.hip scene_refs).
struct SceneRefs {
    uint32_t n_sph, n_tri;
    uint32_t root_ref;           // root reference (LEAF_BIT | prim when the tree is a single leaf)
    uint32_t full_chain;         // the crate's literal slab test and the whole box chain
    const float4* trav;          // [4 n_internal] rtbvh::TravNode
    const float4* bvh_nodes;     // rtbvh::FlatNode (box chain of bvh_reaches)
    const uint32_t* leaf_of;     // primitive -> depth-first leaf rank
    const uint32_t* world_rank;  // primitive -> position in RenderInfo.world, or nullptr (= primitive order)
    const float4* geom_r;        // [n_sph] (cx, cy, cz, radius)
    const float* tri;            // [9 n_tri]
    unsigned long long* counters;   // [0] rays (ray_segments), [1] exact root tests (broad_candidates)
};

// The camera of a kernel that generates camera rays (AParams, CParams): the fields rtplan::fill_camera writes, the ray window and the
// image size.  KParams has the same fields among its own.
struct CameraRefs {
    float org[3], llc[3], hor[3], ver[3];   // Camera::new (camera.rs:19-47), host-computed by rtplan::fill_camera
    float lens_radius, focus_distance;
    float lens_u[3], lens_v[3];  // the lens disc's axes (as KParams)
    float u_den, v_den;          // aspect*H_f - 1, H_f - 1 (camera.rs:115-117)
    float t_min, t_max;
    uint32_t W, H;               // image size
};

// ------------------------------------------------------------------ the closest hit
// The reference's exact root test of primitive `prim` (sphere.rs:42-47 / mesh.rs:109-161 -> shapes/mod.rs:106-129).  P: a parameter
// block derived from SceneRefs.
template <class P>
__device__ __forceinline__ bool query_root(const P& p, uint32_t prim, V3 o, V3 d, float t_min, float t_max, float& t) {
    if (prim < p.n_sph) {
        const float4 g = at32(p.geom_r, prim);
        return exact_sphere(o, 2.0f * d, mk(g.x, g.y, g.z), g.w * g.w, t_min, t_max, t);    // (2f32 * ray.direction), radius.powi(2)
    }
    return exact_triangle(o, d, p.tri + 9 * (size_t)(prim - p.n_sph), t_min, t_max, t);
}

// The closest hit of one ray (ENGINE 2: the walk; 1: the scan with consider<MODE>; ANY: stop at the first admitted hit).  stack: the
// per-lane walk stack, entry e of lane `tid` at stack[e * stride + tid] ((bvh depth + 1) entries); n_tests counts the exact root tests.
template <int ENGINE, int MODE, bool ANY, class P>
__device__ __forceinline__ Hit closest_hit(const P& p, V3 o, V3 d, float t_min, float t_max, const RayAux& aux, uint32_t* stack,
                                           uint32_t tid, uint32_t stride, unsigned long long& n_tests) {
    Hit h{-1, 0.f, 0.f};
    if (ENGINE == 2) {
        uint32_t ref = p.root_ref, sp = 0;
        for (;;) {
            if (ref & LEAF_BIT) {
                const uint32_t prim = ref & ~LEAF_BIT;
                float t;
                n_tests++;
                if (query_root(p, prim, o, d, t_min, t_max, t)) {
                    const V3 pt = o + t * d;             // Ray::at, then |P - o| (consider)
                    const float dist = vlength(pt - o);
                    if (h.idx < 0 || h.dist > dist) {    // depth-first order: the first minimum wins
                        h.idx = (int)prim;
                        h.dist = dist;
                        h.t = t;
                    }
                    if (ANY) break;
                }
                if (sp == 0) break;
                ref = stack[--sp * stride + tid];
                continue;
            }
            // Ray::intersects_aabb (ray.rs:174-194) on both child boxes (TravNode: (l_lo, left) (l_hi, right) (r_lo, -) (r_hi, -))
            const float4* nd = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.trav) + ((size_t)ref << 6));
            const float4 n0 = nd[0], n1 = nd[1], n2 = nd[2], n3 = nd[3];
            const bool hl = aux.finite ? intersects_aabb_finite(o, aux, n0, n1) : intersects_aabb(o, aux, n0, n1);
            const bool hr = aux.finite ? intersects_aabb_finite(o, aux, n2, n3) : intersects_aabb(o, aux, n2, n3);
            const uint32_t cl = __float_as_uint(n0.w), cr = __float_as_uint(n1.w);
            if (hl && hr) stack[sp++ * stride + tid] = cr;   // the right subtree after the whole left one
            if (hl || hr) {
                ref = hl ? cl : cr;
            } else {
                if (sp == 0) break;
                ref = stack[--sp * stride + tid];
            }
        }
    } else {
        const uint32_t n_prims = p.n_sph + p.n_tri;
        for (uint32_t prim = 0; prim < n_prims; prim++) {
            float t;
            n_tests++;
            if (!query_root(p, prim, o, d, t_min, t_max, t)) continue;
            if (MODE == 0) {
                if (p.world_rank) consider<1>(h, (int)prim, o, d, t, aux, p.bvh_nodes, p.world_rank);
                else consider<0>(h, (int)prim, o, d, t, aux, p.bvh_nodes, p.leaf_of);
            } else {
                consider<2>(h, (int)prim, o, d, t, aux, p.bvh_nodes, p.leaf_of);
            }
            if (ANY && h.idx >= 0) break;
        }
    }
    return h;
}

// ------------------------------------------------------------------ the hit record (shapes/mod.rs:15-21, :184-190)
// The normal of a hit of primitive `prim` at the point pt: normalize_or_zero of P - centre (sphere.rs:49-51) or of
// the cross product of the edges from A (mesh.rs:163-165).
template <class P>
__device__ __forceinline__ V3 hit_normal(const P& p, uint32_t prim, V3 pt) {
    V3 nv;
    if (prim < p.n_sph) {
        const float4 g = at32(p.geom_r, prim);
        nv = pt - mk(g.x, g.y, g.z);
    } else {
        const float* tv = p.tri + 9 * (size_t)(prim - p.n_sph);
        const V3 A = mk(tv[0], tv[1], tv[2]), B = mk(tv[3], tv[4], tv[5]), C = mk(tv[6], tv[7], tv[8]);
        nv = cross(A - B, A - C);
    }
    return normalize_or_zero(nv);
}

// The position of primitive `prim` in RenderInfo.world, which rt_hit.index and the index plane report.
template <class P>
__device__ __forceinline__ uint32_t world_position(const P& p, uint32_t prim) {
    return p.world_rank ? p.world_rank[prim] : prim;
}

// rt_hit as two uint4, (P, distance) (normal, index) as bits: the record of a ray that hit nothing ...
__device__ __forceinline__ void hit_none(uint4& w0, uint4& w1) {
    w0 = make_uint4(0u, 0u, 0u, __float_as_uint(__builtin_inff()));
    w1 = make_uint4(0u, 0u, 0u, RT_HIT_NONE);
}

// ... and of the hit h (h.idx >= 0) at the point pt = o + h.t * d with the normal n = hit_normal(p, h.idx, pt)
template <class P>
__device__ __forceinline__ void hit_record(const P& p, const Hit& h, V3 pt, V3 n, uint4& w0, uint4& w1) {
    w0 = make_uint4(__float_as_uint(pt.x), __float_as_uint(pt.y), __float_as_uint(pt.z), __float_as_uint(h.dist));
    w1 = make_uint4(__float_as_uint(n.x), __float_as_uint(n.y), __float_as_uint(n.z), world_position(p, (uint32_t)h.idx));
}

// ------------------------------------------------------------------ the shade (main.rs:114-145)
// The sky a ray of direction d sees (main.rs:135-144), as (r, g, b).
__device__ __forceinline__ V3 sky_colour(V3 d) {
    const V3 nn = normalize_or_zero(d);
    float t = nn.y * 0.5f + 1.0f;
    float omt = 1.0f - t;
    return mk(1.0f * t + 0.3f * omt, 1.0f * t + 0.3f * omt, 1.0f * t + 0.8f * omt);
}

// The UnitSphere draw of a hit (main.rs:119), up to its accepted pair: Marsaglia's rejection loop.  The reference draws it before
// ray_color(.., 0) returns black (main.rs:119 then :109-111), so a kernel that counts depth draws, tests the depth, and only then ...
__device__ __forceinline__ void unit_sphere_pair(Rng& rng, float& x1, float& x2, float& sm) {
    for (;;) {
        x1 = uniform_m1_1(rng);
        x2 = uniform_m1_1(rng);
        sm = x1 * x1 + x2 * x2;
        if (!(sm >= 1.0f)) break;
    }
}

// The UnitSphere vector of an accepted pair (main.rs:119): a scattering hit adds it to the normal, a sphere light takes it as the
// normal of the sampled point.
__device__ __forceinline__ V3 unit_sphere_vec(float x1, float x2, float sm) {
    const float factor = 2.0f * RT_SQRT(1.0f - sm);
    return mk(x1 * factor, x2 * factor, 1.0f - 2.0f * sm);
}

// ... forms the direction of the scattered ray (main.rs:119-127) from the incoming direction d, the hit's normal n, the material's
// roughness and the accepted pair.  Its origin is the hit point, exactly.
__device__ __forceinline__ V3 scattered_dir(V3 d, V3 n, float roughness, float x1, float x2, float sm) {
    const V3 diffuse_dir = unit_sphere_vec(x1, x2, sm) + n;
    const V3 glossy_dir = d - (2.0f * dot(d, n)) * n;                      // main.rs:120-121
    const V3 pre = diffuse_dir + roughness * (glossy_dir - diffuse_dir);   // main.rs:122
    V3 xdir;
    if (!try_normalize(pre, xdir)) xdir = n;                               // main.rs:126
    return normalize(xdir);                                                // Ray::new (ray.rs:134)
}

// ------------------------------------------------------------------ the light sample (rt_tile.h "direct lighting")
// The arithmetic is rt_direct_math.h, which the CPU harness runs too; the draws, the triangle's normal and the scene are the kernel's.
__device__ __forceinline__ rtdl::Vec dvec(V3 a) { return rtdl::Vec{a.x, a.y, a.z}; }
__device__ __forceinline__ V3 v3of(rtdl::Vec a) { return mk(a.x, a.y, a.z); }

struct LightSample {
    uint32_t prim;               // the emitter picked (library primitive number)
    bool sphere;
    rtdl::Vec L, nl;             // the point on it and the emitter's normal there
    float size;                  // the radius, or the triangle's area
    float ip;                    // PICK_POWER: the inverse of the probability the emitter was picked with
};

// How the emitter is picked: uniformly, or by the scene's light table under RT_FLAG_LIGHTS_BY_POWER.  A template
// parameter of the kernels that sample lights, so the instances that run without the flag are the code they were before it existed.
enum { PICK_UNIFORM = 0, PICK_POWER = 1 };

// The scene's light table (rtscene::light_table), the last fields of a parameter block that samples lights; read by PICK_POWER only.
struct LightTableRefs {
    const float* light_c;        // [n_lights] running sums of the emitters' powers, in the list's order
    const float* light_ip;       // [n_sph + n_tri] by primitive number: 1 / p of an emitter
    float light_total;           // light_c[n_lights - 1]; not positive and finite: the table is degenerate, the pick uniform
};

// How a sphere light is sampled: over its whole area, or over the cone it subtends from the hit point when the scene's setting is
// RT_LIGHTS_CONE (rt_scene_set_light_sampling).  A template parameter beside PICK for the same reason: the SHAPE_AREA
// instances are the code they were before the setting existed; the regime test exists in the SHAPE_CONE instances only.
enum { SHAPE_AREA = 0, SHAPE_CONE = 1 };

// The sample of a SHAPE_CONE instance.  Its geometry g is formed inside the arm that drew it — rtdl::cone_geometry of the direction for a
// sphere light in the cone regime (cone; omc its 1 - cos(theta_max); L where the direction meets the sphere), rtdl::light_geometry of
// the point otherwise — so that only g, not the operands of both arms, is live where the arms meet.
struct ConeLightSample : LightSample {
    bool cone;
    float omc;
    rtdl::Geometry g;
};
template <int SHAPE>
struct SampleOf {
    using type = LightSample;
};
template <>
struct SampleOf<SHAPE_CONE> {
    using type = ConeLightSample;
};

// One light sample for the hit point P, drawn from rng (p.n_lights > 0): the emitter picked with one u01 — uniformly, or by power — then a point on it: the
// UnitSphere draw of a scattering hit for a sphere light, two u01 for a triangle light.  P: a parameter block with lights / n_lights
// (and, for PICK_POWER, table: LightTableRefs).  SHAPE_CONE takes the same draws — the cone arm reuses the accepted pair — so the state
// a sample leaves never depends on SHAPE; the hit (hp, n) is read by SHAPE_CONE only.
template <int PICK, int SHAPE, class P>
__device__ __forceinline__ typename SampleOf<SHAPE>::type light_sample(const P& p, Rng& rng, V3 hp, V3 n) {
    typename SampleOf<SHAPE>::type s;
    if constexpr (SHAPE == SHAPE_CONE) s.cone = false;
    const float u = u01(rng);
    uint32_t pick;
    if (PICK == PICK_POWER) pick = rtdl::pick_light_power(u, p.n_lights, p.table.light_c, p.table.light_total);
    else pick = rtdl::pick_light(u, p.n_lights);
    s.prim = p.lights[pick];
    s.ip = PICK == PICK_POWER ? p.table.light_ip[s.prim] : 0.0f;
    s.sphere = s.prim < p.n_sph;
    if (s.sphere) {
        const float4 g = at32(p.geom_r, s.prim);
        float x1, x2, sm;
        unit_sphere_pair(rng, x1, x2, sm);
        if constexpr (SHAPE == SHAPE_CONE) {
            if (rtdl::cone_regime(rtdl::cone_axis(dvec(hp), rtdl::Vec{g.x, g.y, g.z}, g.w).q)) {
                const rtdl::Cone cn = rtdl::cone_sample(dvec(hp), rtdl::Vec{g.x, g.y, g.z}, g.w, x1, x2, sm);
                s.cone = true;
                s.omc = cn.omc;
                s.g = rtdl::cone_geometry(dvec(n), cn.v);
                s.L = rtdl::cone_point(dvec(hp), s.g.w, g.w, cn);
                s.size = g.w;
                return s;
            }
        }
        s.nl = dvec(unit_sphere_vec(x1, x2, sm));
        s.L = rtdl::sphere_point(rtdl::Vec{g.x, g.y, g.z}, g.w, s.nl);
        s.size = g.w;
    } else {
        const float* tv = p.tri + 9 * (size_t)(s.prim - p.n_sph);
        const rtdl::Vec A{tv[0], tv[1], tv[2]}, B{tv[3], tv[4], tv[5]}, C{tv[6], tv[7], tv[8]};
        float u1 = u01(rng), u2 = u01(rng);
        rtdl::fold_pair(u1, u2);
        s.L = rtdl::triangle_point(A, B, C, u1, u2);
        s.nl = dvec(hit_normal(p, s.prim, mk(0.f, 0.f, 0.f)));                         // (a triangle's normal does not read the point)
        s.size = rtdl::triangle_area(A, B, C);
    }
    if constexpr (SHAPE == SHAPE_CONE) s.g = rtdl::light_geometry(dvec(hp), dvec(n), s.L, s.nl, s.sphere);
    return s;
}

// The geometry of the sample s at the hit (P, n): rtdl::light_geometry of its point, or rtdl::cone_geometry of its direction.
__device__ __forceinline__ rtdl::Geometry sample_geometry(const LightSample& s, V3 hp, V3 n) {
    return rtdl::light_geometry(dvec(hp), dvec(n), s.L, s.nl, s.sphere);
}
__device__ __forceinline__ rtdl::Geometry sample_geometry(const ConeLightSample& s, V3, V3) { return s.g; }

// W of the sample s seen under the geometry g = sample_geometry(s, P, n): radiance(albedo, emission, W) is the estimate, and the MIS
// weight of the light strategy reads W itself.  PICK_POWER: s.ip in the place of (float)n_lights.
template <int PICK, int SHAPE>
__device__ __forceinline__ float sample_weight(const typename SampleOf<SHAPE>::type& s, const rtdl::Geometry& g, uint32_t n_lights) {
    if constexpr (SHAPE == SHAPE_CONE) {
        if (s.cone) return rtdl::cone_weight(g.cs, s.omc, PICK == PICK_POWER ? s.ip : (float)n_lights);
    }
    if (PICK == PICK_POWER)
        return s.sphere ? rtdl::sphere_weight_ip(g.cs, g.cl, s.size, s.ip, g.d2) : rtdl::triangle_weight_ip(g.cs, g.cl, s.size, s.ip, g.d2);
    return s.sphere ? rtdl::sphere_weight(g.cs, g.cl, s.size, n_lights, g.d2) : rtdl::triangle_weight(g.cs, g.cl, s.size, n_lights, g.d2);
}

// ------------------------------------------------------------------ the camera ray (Camera::get_ray, camera.rs:109-129)
// The four vectors of Camera::new, formed once per lane outside its loop.
struct CameraBasis {
    V3 org, llc, hor, ver;
};
__device__ __forceinline__ CameraBasis camera_basis(const CameraRefs& cam) {
    return {mk(cam.org[0], cam.org[1], cam.org[2]), mk(cam.llc[0], cam.llc[1], cam.llc[2]), mk(cam.hor[0], cam.hor[1], cam.hor[2]),
            mk(cam.ver[0], cam.ver[1], cam.ver[2])};
}

// The ray of pixel (px, global row pyg) drawn from rng, as the tile kernel's camera arm (rt_kernel.hip.h, "next ray of the lane", the
// !bounce branch) makes it: the UnitDisc rejection pair (accept x1^2 + x2^2 <= 1); the lens offset; the u and v jitter draws;
// normalize_or_zero(llc + u hor + v ver - org), Ray::new's normalize, the focal point; try_normalize(focal - o) falling back to zero,
// then Ray::new's normalize.  o: the lens point; d: the direction as it is handed to ray_color; rng: the state after the draws.
__device__ __forceinline__ void camera_ray(const CameraRefs& cam, const CameraBasis& b, uint32_t px, uint32_t pyg, Rng& rng, V3& o, V3& d) {
    float x1, x2, sm;
    for (;;) {
        x1 = uniform_m1_1(rng);
        x2 = uniform_m1_1(rng);
        sm = x1 * x1 + x2 * x2;
        if (sm <= 1.0f) break;                                             // UnitDisc
    }
    const V3 offset = lens_offset(cam, x1, x2);                            // (the reference camera: same `o` bit for bit, see the tile kernel)
    const float u = ((float)px + gen_range_01(rng)) / cam.u_den;
    const float v = ((float)(cam.H - pyg - 1) + gen_range_01(rng)) / cam.v_den;   // camera row, main.rs:71
    const V3 dir0 = normalize_or_zero(b.llc + u * b.hor + v * b.ver - b.org);
    const V3 d1 = normalize(dir0);                                         // Ray::new re-normalises (ray.rs:134)
    const V3 focal_point = b.org + cam.focus_distance * d1;
    o = b.org + offset;
    const V3 pre = focal_point - o;
    V3 xdir;
    if (!try_normalize(pre, xdir)) xdir = mk(0.f, 0.f, 0.f);                // normalize_or_zero
    d = normalize(xdir);                                                   // Ray::new (ray.rs:134)
}

// ------------------------------------------------------------------ caller rays, RNG states, indices, counters
// The caller ray of the rt_ray record at `ray`, (o, t_min) (d, t_max): Ray::new normalises the direction (glam normalize, a division by
// the length; ray.rs:134), or — as_given — it is taken bit for bit, as a camera or a bounce hands it over.  The caller passes the
// record's address, rays + 2 * i (DESIGN.md 1 "Device-side steps").
struct CallerRay {
    V3 o, d;
    float t_min, t_max;
};
__device__ __forceinline__ CallerRay load_caller_ray(const float4* ray, bool as_given) {
    const float4 r0 = ray[0], r1 = ray[1];
    const V3 dr = mk(r1.x, r1.y, r1.z);
    return {mk(r0.x, r0.y, r0.z), as_given ? dr : normalize(dr), r0.w, r1.w};
}

// An xoshiro256++ state as four consecutive words of the caller's.
__device__ __forceinline__ void load_rng(const uint64_t* s, Rng& rng) {
    rng.s0 = s[0];
    rng.s1 = s[1];
    rng.s2 = s[2];
    rng.s3 = s[3];
}
__device__ __forceinline__ void store_rng(uint64_t* s, const Rng& rng) {
    s[0] = rng.s0;
    s[1] = rng.s1;
    s[2] = rng.s2;
    s[3] = rng.s3;
}

// The active list of a step (BParams, DParams): the number of entries taken, min(count, *n_active), and the index entry k names.  The
// kernel guards it with i < p.n itself: an index beyond the batch touches nothing.
template <class P>
__device__ __forceinline__ uint64_t active_count(const P& p) {
    uint64_t m = p.count;
    if (p.n_active) {
        const uint64_t listed = *p.n_active;
        m = listed < m ? listed : m;
    }
    return m;
}
template <class P>
__device__ __forceinline__ uint64_t active_index(const P& p, uint64_t k) {
    return p.active ? (uint64_t)p.active[k] : k;
}

// The stream of sample smp of ray i in a kernel that sums `spp` seeded samples per caller ray (TParams, NParams without caller states).
template <class P>
__device__ __forceinline__ Rng sample_seed(const P& p, uint64_t i, uint32_t smp) {
    return seed_state(p.seed + (i * p.spp + smp) * (4ull * PHI));
}

// i -> (q, r) = (i / n, i % n), q < 2^32: a 32-bit division while i fits (every launch of fewer than 2^32 items)
__device__ __forceinline__ void split_index(uint64_t i, uint32_t n, uint32_t& q, uint32_t& r) {
    if (i <= 0xffffffffull) {
        q = (uint32_t)i / n;
        r = (uint32_t)i - q * n;
    } else {
        q = (uint32_t)(i / n);
        r = (uint32_t)(i - (uint64_t)q * n);
    }
}

// A kernel's two counts (rays or segments, exact root tests) into counters[0..1]: one atomic per wave.  Reached by whole waves.
__device__ __forceinline__ void flush_counters(unsigned long long* counters, unsigned long long a, unsigned long long b, uint32_t tid) {
    a = wave_sum(a);
    b = wave_sum(b);
    if ((tid & 63u) == 0) {
        if (a) atomicAdd(counters + 0, a);
        if (b) atomicAdd(counters + 1, b);
    }
}

}  // namespace rtk
