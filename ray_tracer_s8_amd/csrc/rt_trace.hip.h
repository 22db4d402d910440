// rt_trace.hip.h — gfx950 path tracing of caller rays (rt_scene_trace*, rt_tile.h "path tracing of caller rays").
//
// One lane per caller ray: `spp` samples of ray_color(ray, max_bounces + 1, rng) (main.rs:108-146), summed in f32 in sample order.
// Persistent waves stride over the batch; each lane loops over its samples and, within a sample, over the segments of the path.
// The closest hit of every segment is the query path's (rt_query.hip.h closest_hit: the exact-node walk or the scan, the same
// operations as rt_scene_intersect), the shading restates the tile kernel's (rt_kernel.hip.h, "shade" and the scattered ray at the
// top of its round) with the same operations in the same order: the Marsaglia rejection loop, diffuse + roughness (glossy -
// diffuse), try_normalize falling back to the normal, then Ray::new's normalize; emission em * albedo; the sky of
// normalize_or_zero(d).y; the UnitSphere draw of a hit at the last depth; the right-to-left albedo product a1 (a2 (... (ak term))).
// So a ray the tile renderer traces gives the same bits here.
//
// LDS per lane (rtplan::plan_trace): the walk's stack, (bvh depth + 1) u32 entries (engine 2), then the path stack, max_bounces + 1
// primitive indices (u16 when the scene has at most 65 536 primitives, as the tile's path32 rule).  Entry e of lane tid sits at
// [e * blockDim.x + tid].  No other per-scene scratch: launches on different streams may overlap.
#pragma once
#include "rt_query.hip.h"

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
        const float4 r0 = p.rays[2 * i], r1 = p.rays[2 * i + 1];
        const V3 o0 = mk(r0.x, r0.y, r0.z);
        const V3 dr = mk(r1.x, r1.y, r1.z);
        const V3 d0 = p.as_given ? dr : normalize(dr);         // Ray::new (ray.rs:134), or the direction a camera / bounce hands over
        const float t_min = r0.w, t_max = r1.w;
        Rng rng;
        if (p.rng_state) {
            const uint64_t* s = p.rng_state + 4 * i;
            rng.s0 = s[0];
            rng.s1 = s[1];
            rng.s2 = s[2];
            rng.s3 = s[3];
        }
        float sum_r = 0.f, sum_g = 0.f, sum_b = 0.f;
        uint32_t segs = 0;
        for (uint32_t smp = 0; smp < p.spp; smp++) {
            if (!p.rng_state) rng = seed_state(p.seed + (i * p.spp + smp) * (4ull * PHI));
            V3 o = o0, d = d0;
            uint32_t k = 0, depth_left = p.depth;
            float term_r, term_g, term_b;
            for (;;) {
                // ================= one ray_color entry with depth > 0: the closest hit (shapes/mod.rs:158-191) =================
                segs++;
                const RayAux aux = ray_aux(d, p.full_chain != 0);
                const Hit h = closest_hit<ENGINE, MODE, false>(p, o, d, t_min, t_max, aux, tlds, tid, bs, n_tests);
                // ================= shade (main.rs:114-145) =================
                if (h.idx < 0) {
                    const V3 nn = normalize_or_zero(d);                                // sky (main.rs:135-144)
                    float t = nn.y * 0.5f + 1.0f;
                    float omt = 1.0f - t;
                    term_r = 1.0f * t + 0.3f * omt;
                    term_g = 1.0f * t + 0.3f * omt;
                    term_b = 1.0f * t + 0.8f * omt;
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
                V3 nv;
                if ((uint32_t)h.idx < p.n_sph) {
                    const float4 g = at32(p.geom_r, (uint32_t)h.idx);
                    nv = hp - mk(g.x, g.y, g.z);                                       // sphere.rs:49-51
                } else {
                    const float* tv = p.tri + 9 * (size_t)(h.idx - p.n_sph);
                    V3 A = mk(tv[0], tv[1], tv[2]), B = mk(tv[3], tv[4], tv[5]), C = mk(tv[6], tv[7], tv[8]);
                    nv = cross(A - B, A - C);                                          // mesh.rs:163-165
                }
                const V3 n = normalize_or_zero(nv);
                path_set(k, (uint32_t)h.idx);                                          // the albedo product is applied back to front
                k++;
                depth_left--;
                // the scattered ray (main.rs:119-127) — drawn also when the depth has run out: the reference draws UnitSphere
                // before ray_color(.., 0) returns black (main.rs:119 then :109-111)
                float x1, x2, sm;
                for (;;) {
                    x1 = uniform_m1_1(rng);
                    x2 = uniform_m1_1(rng);
                    sm = x1 * x1 + x2 * x2;
                    if (!(sm >= 1.0f)) break;
                }
                if (depth_left == 0) {
                    term_r = term_g = term_b = 0.0f;
                    break;
                }
                const float factor = 2.0f * RT_SQRT(1.0f - sm);                        // UnitSphere, main.rs:119
                const V3 us = mk(x1 * factor, x2 * factor, 1.0f - 2.0f * sm);
                const V3 diffuse_dir = us + n;
                const V3 glossy_dir = d - (2.0f * dot(d, n)) * n;                      // main.rs:120-121
                const V3 pre = diffuse_dir + m.w * (glossy_dir - diffuse_dir);         // main.rs:122
                V3 xdir;
                if (!try_normalize(pre, xdir)) xdir = n;                               // main.rs:126
                d = normalize(xdir);                                                   // Ray::new (ray.rs:134)
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
        if (p.rng_state) {
            uint64_t* s = p.rng_state + 4 * i;
            s[0] = rng.s0;
            s[1] = rng.s1;
            s[2] = rng.s2;
            s[3] = rng.s3;
        }
        n_segs += segs;
    }
    // counters: one atomic per wave
    n_segs = wave_sum(n_segs);
    n_tests = wave_sum(n_tests);
    if ((tid & 63u) == 0) {
        if (n_segs) atomicAdd(p.counters + 0, n_segs);
        if (n_tests) atomicAdd(p.counters + 1, n_tests);
    }
}

using TraceFn = void (*)(const TParams);
TraceFn trace_kernel(int engine, int scan_mode);    // rt_kernels_trace.hip; nullptr for a combination that does not exist

}  // namespace rtk
