// rt_aov.hip.h — gfx950 feature buffers of a strip (rt_scene_render_aov*, rt_tile.h "feature buffers").
//
// One lane per pixel of a batch of strips: the lane loops over the samples [s_begin, s_end) of its pixel, generates each sample's
// camera ray as the tile kernel does, finds its first hit with the query path's closest_hit (rt_query.hip.h: the exact-node walk or
// the scan, the same operations as rt_scene_intersect) and adds the hit's albedo, normal and distance to sums held in registers, in
// sample order — no cross-lane reduction.  Neighbouring lanes hold neighbouring pixels of a row, whose camera rays are coherent.
// Persistent waves stride over (strip, pixel) with 64-bit offsets.  Each plane is read at most once (s_begin > 0) and written once
// per pixel; a plane not asked for is neither read, nor summed, nor written.
//
// The camera ray restates the tile kernel's camera arm (rt_kernel.hip.h, "next ray of the lane", the !bounce branch) with the same
// operations in the same order: the stream seed + 4 PHI ((y W + x) S + s); the UnitDisc rejection pair (accept x1^2 + x2^2 <= 1);
// the lens offset; the u and v jitter draws; normalize_or_zero(llc + u hor + v ver - org), Ray::new's normalize, the focal point;
// try_normalize(focal - o) falling back to zero, then Ray::new's normalize.  That direction is traced as it is.  So the planes
// come from exactly the rays the beauty image averages.  The sky of a miss is the trace kernel's normalize_or_zero(d).y form.
//
// LDS: the walk's per-lane stack, (bvh depth + 1) u32 entries at [e * 256 + tid] (engine 2; rtplan::plan_query).  No other
// per-scene scratch: launches on different streams may overlap.
#pragma once
#include "rt_query.hip.h"

namespace rtk {

constexpr uint32_t AOV_ALBEDO = 1u, AOV_NORMAL = 2u, AOV_DEPTH = 4u, AOV_HITS = 8u, AOV_INDEX = 16u;   // AParams::planes

struct AovStrip {
    uint64_t seed;
    float* albedo;               // [Hs*W*3] or nullptr (as `planes` says: the same set for every strip of a launch)
    float* normal;               // [Hs*W*3]
    float* depth;                // [Hs*W]
    uint32_t* hits;              // [Hs*W]
    uint32_t* index;             // [Hs*W]
    uint32_t y0;                 // first global row of the strip = Hs * division_no
    uint32_t pad;
};

struct AParams : SceneRefs {
    float org[3], llc[3], hor[3], ver[3];   // Camera::new (camera.rs:19-47), host-computed by rtplan::fill_camera
    float lens_radius, focus_distance;
    float lens_u[3], lens_v[3];  // the lens disc's axes (as KParams)
    float u_den, v_den;          // aspect*H_f - 1, H_f - 1 (camera.rs:115-117)
    float t_min, t_max;
    uint32_t W, H;               // image size
    uint32_t npix;               // pixels of a strip, Hs * W
    uint32_t spp_all;            // S: samples of the job (the stream stride)
    uint32_t s_begin, s_end;     // the samples of this launch
    uint32_t n_strips;
    uint32_t planes;             // AOV_* bits of the planes computed
    const float4* mat;           // [n_sph + n_tri] (albedo r, g, b, roughness)
    AovStrip strips[MAX_BATCH];
};
static_assert(sizeof(AParams) <= 4096, "AParams must fit the kernel argument segment");

// ENGINE 2: the walk; 1: the scan with consider<MODE> (MODE 0 plain linear semantics, 2 BVH semantics).
template <int ENGINE, int MODE>
__global__ __launch_bounds__(256) void rt_aov_kernel(const AParams p) {
    extern __shared__ uint32_t astack[];                 // [depth + 1][256] (engine 2)
    const uint32_t tid = threadIdx.x;
    const V3 corg = mk(p.org[0], p.org[1], p.org[2]);
    const V3 llc = mk(p.llc[0], p.llc[1], p.llc[2]);
    const V3 hor = mk(p.hor[0], p.hor[1], p.hor[2]);
    const V3 ver = mk(p.ver[0], p.ver[1], p.ver[2]);
    const bool cont = p.s_begin > 0;
    unsigned long long n_rays = 0, n_tests = 0;
    const uint64_t total = (uint64_t)p.n_strips * p.npix;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + tid; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        // the strip and the pixel in it: a 32-bit division while the offset fits (every launch of fewer than 2^32 pixels)
        uint32_t si, pix;
        if (i <= 0xffffffffull) {
            si = (uint32_t)i / p.npix;
            pix = (uint32_t)i - si * p.npix;
        } else {
            si = (uint32_t)(i / p.npix);
            pix = (uint32_t)(i - (uint64_t)si * p.npix);
        }
        const uint32_t row = pix / p.W, px = pix - row * p.W;
        const AovStrip& sd = p.strips[si];
        const uint32_t pyg = sd.y0 + row;
        // SplitMix64 state of the pixel's first stream of the launch: seed + 4 PHI ((y W + x) S + s_begin)
        const uint64_t seed0 = sd.seed + (((uint64_t)pyg * p.W + px) * p.spp_all + p.s_begin) * (4ull * PHI);
        float al_r = 0.f, al_g = 0.f, al_b = 0.f, n_x = 0.f, n_y = 0.f, n_z = 0.f, dep = 0.f;
        uint32_t nh = 0, idx0 = RT_HIT_NONE;
        if (cont) {
            if (p.planes & AOV_ALBEDO) {
                al_r = sd.albedo[3 * (size_t)pix + 0];
                al_g = sd.albedo[3 * (size_t)pix + 1];
                al_b = sd.albedo[3 * (size_t)pix + 2];
            }
            if (p.planes & AOV_NORMAL) {
                n_x = sd.normal[3 * (size_t)pix + 0];
                n_y = sd.normal[3 * (size_t)pix + 1];
                n_z = sd.normal[3 * (size_t)pix + 2];
            }
            if (p.planes & AOV_DEPTH) dep = sd.depth[pix];
            if (p.planes & AOV_HITS) nh = sd.hits[pix];
        }
        for (uint32_t s = p.s_begin; s < p.s_end; s++) {
            Rng rng = seed_state(seed0 + (uint64_t)(s - p.s_begin) * (4ull * PHI));
            // ---- the camera ray (Camera::get_ray, camera.rs:109-129), as the tile kernel's camera arm
            float x1, x2, sm;
            for (;;) {
                x1 = uniform_m1_1(rng);
                x2 = uniform_m1_1(rng);
                sm = x1 * x1 + x2 * x2;
                if (sm <= 1.0f) break;                                         // UnitDisc
            }
            const V3 offset = lens_offset(p, x1, x2);                          // (the reference camera: same `o` bit for bit, see the tile kernel)
            const float u = ((float)px + gen_range_01(rng)) / p.u_den;
            const float v = ((float)(p.H - pyg - 1) + gen_range_01(rng)) / p.v_den;   // camera row, main.rs:71
            const V3 dir0 = normalize_or_zero(llc + u * hor + v * ver - corg);
            const V3 d1 = normalize(dir0);                                     // Ray::new re-normalises (ray.rs:134)
            const V3 focal_point = corg + p.focus_distance * d1;
            const V3 o = corg + offset;
            const V3 pre = focal_point - o;
            V3 xdir;
            if (!try_normalize(pre, xdir)) xdir = mk(0.f, 0.f, 0.f);            // normalize_or_zero
            const V3 d = normalize(xdir);                                      // Ray::new (ray.rs:134)
            // ---- its first hit (shapes/mod.rs:158-191)
            n_rays++;
            const RayAux aux = ray_aux(d, p.full_chain != 0);
            const Hit h = closest_hit<ENGINE, MODE, false>(p, o, d, p.t_min, p.t_max, aux, astack, tid, 256u, n_tests);
            if (h.idx < 0) {
                if (p.planes & AOV_ALBEDO) {
                    const V3 nn = normalize_or_zero(d);                        // sky (main.rs:135-144)
                    float t = nn.y * 0.5f + 1.0f;
                    float omt = 1.0f - t;
                    al_r = al_r + (1.0f * t + 0.3f * omt);
                    al_g = al_g + (1.0f * t + 0.3f * omt);
                    al_b = al_b + (1.0f * t + 0.8f * omt);
                }
                continue;
            }
            const uint32_t prim = (uint32_t)h.idx;
            if (p.planes & AOV_ALBEDO) {
                const float4 m = at32(p.mat, prim);                            // p_albedo_at
                al_r = al_r + m.x;
                al_g = al_g + m.y;
                al_b = al_b + m.z;
            }
            if (p.planes & AOV_NORMAL) {
                // the normal of the hit record (sphere.rs:49-51 / mesh.rs:163-165), as rt_query_kernel forms it
                const V3 pt = o + h.t * d;
                V3 nv;
                if (prim < p.n_sph) {
                    const float4 g = at32(p.geom_r, prim);
                    nv = pt - mk(g.x, g.y, g.z);
                } else {
                    const float* tv = p.tri + 9 * (size_t)(prim - p.n_sph);
                    const V3 A = mk(tv[0], tv[1], tv[2]), B = mk(tv[3], tv[4], tv[5]), C = mk(tv[6], tv[7], tv[8]);
                    nv = cross(A - B, A - C);
                }
                const V3 nn = normalize_or_zero(nv);
                n_x = n_x + nn.x;
                n_y = n_y + nn.y;
                n_z = n_z + nn.z;
            }
            dep = dep + h.dist;                                                // |P - o|
            nh++;
            if (s == 0) idx0 = p.world_rank ? p.world_rank[prim] : prim;
        }
        if (p.planes & AOV_ALBEDO) {
            sd.albedo[3 * (size_t)pix + 0] = al_r;
            sd.albedo[3 * (size_t)pix + 1] = al_g;
            sd.albedo[3 * (size_t)pix + 2] = al_b;
        }
        if (p.planes & AOV_NORMAL) {
            sd.normal[3 * (size_t)pix + 0] = n_x;
            sd.normal[3 * (size_t)pix + 1] = n_y;
            sd.normal[3 * (size_t)pix + 2] = n_z;
        }
        if (p.planes & AOV_DEPTH) sd.depth[pix] = dep;
        if (p.planes & AOV_HITS) sd.hits[pix] = nh;
        if ((p.planes & AOV_INDEX) && !cont) sd.index[pix] = idx0;
    }
    // counters: one atomic per wave
    n_rays = wave_sum(n_rays);
    n_tests = wave_sum(n_tests);
    if ((tid & 63u) == 0) {
        if (n_rays) atomicAdd(p.counters + 0, n_rays);
        if (n_tests) atomicAdd(p.counters + 1, n_tests);
    }
}

using AovFn = void (*)(const AParams);
AovFn aov_kernel(int engine, int scan_mode);    // rt_kernels_aov.hip; nullptr for a combination that does not exist

}  // namespace rtk
