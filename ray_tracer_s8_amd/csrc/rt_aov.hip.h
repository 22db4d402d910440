// rt_aov.hip.h — gfx950 feature buffers of a strip (rt_scene_render_aov*, rt_tile.h "feature buffers").
//
// One lane per pixel of a batch of strips: the lane loops over the samples [s_begin, s_end) of its pixel, generates each sample's
// camera ray as the tile kernel does, finds its first hit with the query path's closest_hit (the exact-node walk or the scan, the
// same operations as rt_scene_intersect) and adds the hit's albedo, normal and distance to sums held in registers, in
// sample order — no cross-lane reduction.  Neighbouring lanes hold neighbouring pixels of a row, whose camera rays are coherent.
// Persistent waves stride over (strip, pixel) with 64-bit offsets.  Each plane is read at most once (s_begin > 0) and written once
// per pixel; a plane not asked for is neither read, nor summed, nor written.
//
// The camera ray, the first hit, the normal and the sky of a miss are the shared steps of rt_path_steps.hip.h (camera_ray on the stream
// seed + 4 PHI ((y W + x) S + s), closest_hit, hit_normal, sky_colour); the direction is traced as it is.  So the planes come from
// exactly the rays the beauty image averages.
//
// LDS: the walk's per-lane stack, (bvh depth + 1) u32 entries at [e * 256 + tid] (engine 2; rtplan::plan_query).  No other
// per-scene scratch: launches on different streams may overlap.
#pragma once
#include "rt_path_steps.hip.h"

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

struct AParams : SceneRefs, CameraRefs {
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
    const CameraBasis basis = camera_basis(p);
    const bool cont = p.s_begin > 0;
    unsigned long long n_rays = 0, n_tests = 0;
    const uint64_t total = (uint64_t)p.n_strips * p.npix;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + tid; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t si, pix;                                                      // the strip and the pixel in it
        split_index(i, p.npix, si, pix);
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
            // ---- the camera ray (Camera::get_ray, camera.rs:109-129)
            V3 o, d;
            camera_ray(p, basis, px, pyg, rng, o, d);
            // ---- its first hit (shapes/mod.rs:158-191)
            n_rays++;
            const RayAux aux = ray_aux(d, p.full_chain != 0);
            const Hit h = closest_hit<ENGINE, MODE, false>(p, o, d, p.t_min, p.t_max, aux, astack, tid, 256u, n_tests);
            if (h.idx < 0) {
                if (p.planes & AOV_ALBEDO) {
                    const V3 sky = sky_colour(d);                              // main.rs:135-144
                    al_r = al_r + sky.x;
                    al_g = al_g + sky.y;
                    al_b = al_b + sky.z;
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
                const V3 nn = hit_normal(p, prim, o + h.t * d);                // the normal of the hit record
                n_x = n_x + nn.x;
                n_y = n_y + nn.y;
                n_z = n_z + nn.z;
            }
            dep = dep + h.dist;                                                // |P - o|
            nh++;
            if (s == 0) idx0 = world_position(p, prim);
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
    flush_counters(p.counters, n_rays, n_tests, tid);
}

using AovFn = void (*)(const AParams);
AovFn aov_kernel(int engine, int scan_mode);    // rt_kernels_aov.hip; nullptr for a combination that does not exist

}  // namespace rtk
