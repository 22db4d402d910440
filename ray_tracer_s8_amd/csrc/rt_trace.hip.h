// rt_trace.hip.h — gfx950 path tracing of caller rays (rt_scene_trace*, rt_tile.h "path tracing of caller rays").
//
// One lane per caller ray: `spp` samples of ray_color(ray, max_bounces + 1, rng) (main.rs:108-146), summed in f32 in sample order.
// Persistent waves stride over the batch; each lane loops over its samples and, within a sample, over the segments of the path.
// The closest hit of every segment, the normal, the sky and the scattered ray are the shared steps of rt_path_steps.hip.h (closest_hit:
// the exact-node walk or the scan, the same operations as rt_scene_intersect; hit_normal, sky_colour, unit_sphere_pair, scattered_dir);
// the kernel's own are emission em * albedo, the UnitSphere draw of a hit at the last depth and the right-to-left albedo product
// a1 (a2 (... (ak term))).  So a ray the tile renderer traces gives the same bits here.
//
// LDS per lane (rtplan::plan_trace): the walk's stack, (bvh depth + 1) u32 entries (engine 2), then the path stack, max_bounces + 1
// primitive indices (u16 when the scene has at most 65 536 primitives, as the tile's path32 rule).  Entry e of lane tid sits at
// [e * blockDim.x + tid].  No other per-scene scratch: launches on different streams may overlap.
#pragma once
#include "rt_path_steps.hip.h"

namespace rtk {

struct TParams : SceneRefs {
    const float4* rays;          // [2 n]: rt_ray (o, t_min) (d, t_max)
    float* rgb;                  // [3 n]: the f32 sum of the ray's sample colours
    uint32_t* segments;          // [n] ray_color entries with depth > 0, or nullptr
    uint64_t* rng_state;         // [4 n] xoshiro256++ state per ray (read and written back), or nullptr: the seeded streams
    uint64_t n;
    uint64_t seed;               // rng_state == nullptr: sample s of ray i draws from seed_from_u64(seed + 4 PHI (i spp + s))
    uint32_t spp, depth;         // samples per ray; ray_color entry depth = max_bounces + 1
    uint32_t as_given;           // 1: the direction is taken bit for bit (RT_TRACE_RAY_AS_GIVEN), 0: Ray::new normalises it
    uint32_t path32;             // 1: path stack entries are u32, 0: u16
    uint32_t lds_path_off;       // byte offset of the path stack in dynamic LDS
    const float4* mat;           // [n_sph + n_tri] (albedo r, g, b, roughness)
    const float* emis;           // [n_sph + n_tri]
};

// ENGINE 2: the walk; 1: the scan with consider<MODE> (MODE 0 plain linear semantics, 2 BVH semantics).
template <int ENGINE, int MODE>
__global__ __launch_bounds__(256) void rt_trace_kernel(const TParams p) {
    extern __shared__ uint32_t tlds[];
    const uint32_t tid = threadIdx.x, bs = blockDim.x;
    char* const lpath = reinterpret_cast<char*>(tlds) + p.lds_path_off;
    auto path_set = [&](uint32_t e, uint32_t prim) {
        if (p.path32) reinterpret_cast<uint32_t*>(lpath)[e * bs + tid] = prim;
        else reinterpret_cast<uint16_t*>(lpath)[e * bs + tid] = (uint16_t)prim;
    };
    auto path_idx = [&](uint32_t e) -> uint32_t {
        return p.path32 ? reinterpret_cast<const uint32_t*>(lpath)[e * bs + tid] : (uint32_t) reinterpret_cast<const uint16_t*>(lpath)[e * bs + tid];
    };
    unsigned long long n_segs = 0, n_tests = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * bs + tid; i < p.n; i += (uint64_t)gridDim.x * bs) {
        const CallerRay r = load_caller_ray(p.rays + 2 * i, p.as_given != 0);
        Rng rng;
        if (p.rng_state) load_rng(p.rng_state + 4 * i, rng);
        float sum_r = 0.f, sum_g = 0.f, sum_b = 0.f;
        uint32_t segs = 0;
        for (uint32_t smp = 0; smp < p.spp; smp++) {
            if (!p.rng_state) rng = sample_seed(p, i, smp);
            V3 o = r.o, d = r.d;
            uint32_t k = 0, depth_left = p.depth;
            float term_r, term_g, term_b;
            for (;;) {
                // ================= one ray_color entry with depth > 0: the closest hit (shapes/mod.rs:158-191) =================
                segs++;
                const RayAux aux = ray_aux(d, p.full_chain != 0);
                const Hit h = closest_hit<ENGINE, MODE, false>(p, o, d, r.t_min, r.t_max, aux, tlds, tid, bs, n_tests);
                // ================= shade (main.rs:114-145) =================
                if (h.idx < 0) {
                    const V3 sky = sky_colour(d);                                      // main.rs:135-144
                    term_r = sky.x;
                    term_g = sky.y;
                    term_b = sky.z;
                    break;
                }
                const float em = at32(p.emis, (uint32_t)h.idx);
                const float4 m = at32(p.mat, (uint32_t)h.idx);
                if (em > 0.0f) {                                                       // main.rs:116-117
                    term_r = m.x * em;
                    term_g = m.y * em;
                    term_b = m.z * em;
                    break;
                }
                const V3 hp = o + h.t * d;                                             // Ray::at (ray.rs:147-149), as in consider
                const V3 n = hit_normal(p, (uint32_t)h.idx, hp);
                path_set(k, (uint32_t)h.idx);                                          // the albedo product is applied back to front
                k++;
                depth_left--;
                // the scattered ray (main.rs:119-127) — drawn also when the depth has run out: the reference draws UnitSphere
                // before ray_color(.., 0) returns black (main.rs:119 then :109-111)
                float x1, x2, sm;
                unit_sphere_pair(rng, x1, x2, sm);
                if (depth_left == 0) {
                    term_r = term_g = term_b = 0.0f;
                    break;
                }
                d = scattered_dir(d, n, m.w, x1, x2, sm);
                o = hp;                                                                // origin exactly P
            }
            // a1 (.) (a2 (.) ( ... (ak (.) terminal))) : right-to-left (main.rs:123)
#pragma clang loop unroll(disable)
            for (uint32_t e = k; e-- > 0;) {
                const float4 ma = at32(p.mat, path_idx(e));
                term_r = ma.x * term_r;
                term_g = ma.y * term_g;
                term_b = ma.z * term_b;
            }
            sum_r = sum_r + term_r;                                                    // pix_color += ray_color(..) (main.rs:75)
            sum_g = sum_g + term_g;
            sum_b = sum_b + term_b;
        }
        p.rgb[3 * i + 0] = sum_r;
        p.rgb[3 * i + 1] = sum_g;
        p.rgb[3 * i + 2] = sum_b;
        if (p.segments) p.segments[i] = segs;
        if (p.rng_state) store_rng(p.rng_state + 4 * i, rng);
        n_segs += segs;
    }
    flush_counters(p.counters, n_segs, n_tests, tid);
}

using TraceFn = void (*)(const TParams);
TraceFn trace_kernel(int engine, int scan_mode);    // rt_kernels_trace.hip; nullptr for a combination that does not exist

}  // namespace rtk
