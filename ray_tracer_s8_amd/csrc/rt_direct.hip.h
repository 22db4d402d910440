// rt_direct.hip.h — gfx950 direct lighting of caller rays (rt_scene_direct*, rt_tile.h "direct lighting").
//
// One lane per ACTIVE hit record (the rt_hit a path step writes), one light sample per lane: an emitter picked from the
// scene's emitter list (uniformly, or by power under RT_FLAG_LIGHTS_BY_POWER) with one u01 of the ray's own RNG state, a point on it (the UnitSphere draw of the shared path steps for a
// sphere light, two u01 for a triangle light), the two cosines, the shadow ray through the shared closest_hit, and the Lambertian
// estimate without the surface albedo.  The arithmetic of the pick, the point, the cosines and the weight is rt_direct_math.h, which the
// CPU harness runs too; the sample (light_sample, sample_weight: the draws, the point, the normal of a triangle light) and the
// closest hit are the steps of rt_path_steps.hip.h, so the sample is rt_nee_kernel's and the shadow ray's hit is rt_scene_intersect's
// bit for bit.
//
// Persistent waves stride over the active list (or over all n records) exactly as rt_bounce_kernel does; the device form reads the
// list's length from device memory.  Lanes whose sample faces away trace nothing: the walk runs under one branch that the lanes with
// a shadow ray enter together.  Nothing is read or written through an index >= n.
//
// LDS per lane (rtplan::plan_query): the walk's stack, (bvh depth + 1) u32 entries (engine 2); entry e of lane tid at [e * 256 + tid].
// No per-scene scratch: launches on different streams may overlap.
#pragma once
#include "rt_path_steps.hip.h"

namespace rtk {

struct DParams : SceneRefs {
    const uint4* hits;           // [2 n]: rt_hit (P, distance) (normal, index), as bits
    uint64_t* rng_state;         // [4 n] xoshiro256++ state per ray: read, and written back by a record that drew
    const uint32_t* active;      // [count] record indices < n, or nullptr: records 0 .. count - 1
    const uint32_t* n_active;    // device word that holds the list's length (the call takes min(count, *n_active)), or nullptr
    uint4* out;                  // [2 n]: rt_direct (r, g, b, light) (lx, ly, lz, status), as bits
    uint64_t n;                  // records in the batch: every index is below it
    uint64_t count;              // upper bound of the entries taken (the grid is sized from it)
    const float4* mat;           // [n_sph + n_tri] (albedo r, g, b, roughness)
    const float* emis;           // [n_sph + n_tri]
    const uint32_t* lights;      // [n_lights] the emitters (library primitive numbers) in ascending world position
    uint32_t n_lights;           // M <= rtdl::MAX_LIGHTS
    float t_min, t_max;          // the shadow rays' window
    LightTableRefs table;        // RT_FLAG_LIGHTS_BY_POWER (PICK_POWER instances only)
};

// ENGINE 2: the walk; 1: the scan with consider<MODE> (MODE 0 plain linear semantics, 2 BVH semantics).  PICK: the pick rule.  SHAPE: how
// a sphere light is sampled (the scene's rt_scene_set_light_sampling).  A cone sample has its l* — where its direction meets the
// sphere — formed before the walk, by light_sample, and its W after it from cs, omc and ip.
template <int ENGINE, int MODE, int PICK, int SHAPE>
__global__ __launch_bounds__(256) void rt_direct_kernel(const DParams p) {
    extern __shared__ uint32_t dstack[];                 // [depth + 1][256] (engine 2)
    const uint32_t tid = threadIdx.x;
    const uint64_t m = active_count(p);
    unsigned long long n_rays = 0, n_tests = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + tid; k < m; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = active_index(p, k);
        if (i >= p.n) continue;                                                        // (an index beyond the batch touches nothing)
        const uint4 h0 = p.hits[2 * i], h1 = p.hits[2 * i + 1];
        if (h1.w == RT_HIT_NONE || p.n_lights == 0) {                                  // no draw, the state unchanged
            p.out[2 * i] = make_uint4(0u, 0u, 0u, RT_HIT_NONE);
            p.out[2 * i + 1] = make_uint4(0u, 0u, 0u, h1.w == RT_HIT_NONE ? RT_DIRECT_SKIPPED : RT_DIRECT_NO_LIGHTS);
            continue;
        }
        const V3 P = mk(__uint_as_float(h0.x), __uint_as_float(h0.y), __uint_as_float(h0.z));
        const V3 n = mk(__uint_as_float(h1.x), __uint_as_float(h1.y), __uint_as_float(h1.z));
        // ================= the draws: the emitter, then the point on it =================
        Rng rng;
        load_rng(p.rng_state + 4 * i, rng);
        const typename SampleOf<SHAPE>::type ls = light_sample<PICK, SHAPE>(p, rng, P, n);
        store_rng(p.rng_state + 4 * i, rng);
        // ================= the cosines; the shadow ray Ray::new(P, L - P) =================
        const rtdl::Geometry g = sample_geometry(ls, P, n);
        uint32_t status = RT_DIRECT_FACING_AWAY;
        rtdl::Vec rgb{0.0f, 0.0f, 0.0f};
        if (g.facing) {
            const V3 d = v3of(g.w);                                                    // v / |v|: Ray::new's division (ray.rs:134)
            const RayAux aux = ray_aux(d, p.full_chain != 0);
            n_rays++;
            const Hit h = closest_hit<ENGINE, MODE, false>(p, P, d, p.t_min, p.t_max, aux, dstack, tid, 256u, n_tests);
            status = RT_DIRECT_OCCLUDED;
            if (h.idx == (int)ls.prim) {
                status = RT_DIRECT_LIT;
                const float4 ma = at32(p.mat, ls.prim);
                const float W = sample_weight<PICK, SHAPE>(ls, g, p.n_lights);
                rgb = rtdl::radiance(rtdl::Vec{ma.x, ma.y, ma.z}, at32(p.emis, ls.prim), W);
            }
        }
        p.out[2 * i] = make_uint4(__float_as_uint(rgb.x), __float_as_uint(rgb.y), __float_as_uint(rgb.z), world_position(p, ls.prim));
        p.out[2 * i + 1] = make_uint4(__float_as_uint(ls.L.x), __float_as_uint(ls.L.y), __float_as_uint(ls.L.z), status);
    }
    flush_counters(p.counters, n_rays, n_tests, tid);
}

using DirectFn = void (*)(const DParams);
// rt_kernels_direct.hip; cone: the scene's setting is RT_LIGHTS_CONE; nullptr for a combination that does not exist
DirectFn direct_kernel(int engine, int scan_mode, bool by_power, bool cone);

}  // namespace rtk
