// rt_bounce.hip.h — gfx950 path steps of caller rays (rt_scene_bounce*, rt_tile.h "path steps").
//
// One lane per ACTIVE caller ray, one ray_color entry with depth > 0 (main.rs:108-146) per lane: the closest hit of the segment, its
// shade, and — when the ray scatters — the UnitSphere draw from the ray's own RNG state and the scattered ray, written back over the
// ray and the state.  What rt_trace.hip.h does between two segments of its loop, operation for operation: the closest hit is the query
// path's (rt_query.hip.h closest_hit: the exact-node walk or the scan), the hit record is the query kernel's, the shade and the
// scatter are the trace kernel's (the Marsaglia rejection loop, diffuse + roughness (glossy - diffuse), try_normalize falling back to
// the normal, then Ray::new's normalize; emission em * albedo; the sky of normalize_or_zero(d).y).  The albedo product and the
// termination rule are the caller's: a step returns the segment's own factor (rt_bounce.rgb) and its status.
//
// Persistent waves stride over the active list (or over all n rays).  The device form reads the list's length from device memory, so
// consecutive steps need no host synchronisation.  Compaction: the lanes of a wave that scattered are counted by a ballot, ranked by
// mbcnt, and appended to next_active behind ONE atomicAdd per wave on *n_next; every per-ray result lives at the ray's own index, so
// nothing depends on the order of that list.
//
// LDS per lane (rtplan::plan_query): the walk's stack, (bvh depth + 1) u32 entries (engine 2); entry e of lane tid at [e * 256 + tid].
// No per-scene scratch: launches on different streams may overlap.
#pragma once
#include "rt_query.hip.h"

namespace rtk {

struct BParams : SceneRefs {
    float4* rays;                // [2 n]: rt_ray (o, t_min) (d, t_max); a scattered ray is written over its slot
    uint64_t* rng_state;         // [4 n] xoshiro256++ state per ray: read, and written back by a ray that scattered (or was seeded)
    const uint32_t* active;      // [count] ray indices < n, or nullptr: rays 0 .. count - 1
    const uint32_t* n_active;    // device word that holds the list's length (the step takes min(count, *n_active)), or nullptr
    uint4* bounce;               // [n]: rt_bounce (r, g, b, status), as bits
    uint4* hits;                 // [2 n]: rt_hit of the incoming ray, or nullptr
    uint32_t* next_active;       // [n] indices of the rays that scattered, in no particular order, or nullptr (n_next alone: count only)
    uint32_t* n_next;            // their number (zeroed on the stream before the launch), or nullptr: no compaction
    uint64_t n;                  // rays in the batch: every index is below it
    uint64_t count;              // upper bound of the entries stepped (the grid is sized from it)
    uint64_t seed;               // seed_states: state i = seed_from_u64(seed + 4 PHI i) is written first
    uint32_t as_given;           // 1: the direction is taken bit for bit (RT_TRACE_RAY_AS_GIVEN), 0: Ray::new normalises it
    uint32_t seed_states;
    const float4* mat;           // [n_sph + n_tri] (albedo r, g, b, roughness)
    const float* emis;           // [n_sph + n_tri]
};

// ENGINE 2: the walk; 1: the scan with consider<MODE> (MODE 0 plain linear semantics, 2 BVH semantics).
template <int ENGINE, int MODE>
__global__ __launch_bounds__(256) void rt_bounce_kernel(const BParams p) {
    extern __shared__ uint32_t bstack[];                 // [depth + 1][256] (engine 2)
    const uint32_t tid = threadIdx.x;
    uint64_t m = p.count;
    if (p.n_active) {
        const uint64_t listed = *p.n_active;
        m = listed < m ? listed : m;
    }
    unsigned long long n_rays = 0, n_tests = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + tid; k < m; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = p.active ? (uint64_t)p.active[k] : k;
        bool scattered = false;
        if (i < p.n) {                                                                 // (an index beyond the batch touches nothing)
            const float4 r0 = p.rays[2 * i], r1 = p.rays[2 * i + 1];
            const V3 o = mk(r0.x, r0.y, r0.z);
            const V3 dr = mk(r1.x, r1.y, r1.z);
            const V3 d = p.as_given ? dr : normalize(dr);                              // Ray::new (ray.rs:134), or the direction as handed over
            const float t_min = r0.w, t_max = r1.w;
            const RayAux aux = ray_aux(d, p.full_chain != 0);
            n_rays++;
            // ================= one ray_color entry with depth > 0: the closest hit (shapes/mod.rs:158-191) =================
            const Hit h = closest_hit<ENGINE, MODE, false>(p, o, d, t_min, t_max, aux, bstack, tid, 256u, n_tests);
            uint4 w0 = make_uint4(0u, 0u, 0u, __float_as_uint(__builtin_inff())), w1 = make_uint4(0u, 0u, 0u, RT_HIT_NONE);
            float cr, cg, cb;
            uint32_t status;
            Rng rng;
            if (p.seed_states) rng = seed_state(p.seed + i * (4ull * PHI));
            if (h.idx < 0) {
                const V3 nn = normalize_or_zero(d);                                    // sky (main.rs:135-144)
                float t = nn.y * 0.5f + 1.0f;
                float omt = 1.0f - t;
                cr = 1.0f * t + 0.3f * omt;
                cg = 1.0f * t + 0.3f * omt;
                cb = 1.0f * t + 0.8f * omt;
                status = RT_BOUNCE_MISSED;
            } else {
                const uint32_t prim = (uint32_t)h.idx;
                // the hit record (shapes/mod.rs:184-190), as rt_query_kernel fills it
                const V3 hp = o + h.t * d;                                             // Ray::at (ray.rs:147-149)
                V3 nv;
                if (prim < p.n_sph) {
                    const float4 g = at32(p.geom_r, prim);
                    nv = hp - mk(g.x, g.y, g.z);                                       // sphere.rs:49-51
                } else {
                    const float* tv = p.tri + 9 * (size_t)(prim - p.n_sph);
                    const V3 A = mk(tv[0], tv[1], tv[2]), B = mk(tv[3], tv[4], tv[5]), C = mk(tv[6], tv[7], tv[8]);
                    nv = cross(A - B, A - C);                                          // mesh.rs:163-165
                }
                const V3 n = normalize_or_zero(nv);
                w0 = make_uint4(__float_as_uint(hp.x), __float_as_uint(hp.y), __float_as_uint(hp.z), __float_as_uint(h.dist));
                w1 = make_uint4(__float_as_uint(n.x), __float_as_uint(n.y), __float_as_uint(n.z), p.world_rank ? p.world_rank[prim] : prim);
                // ================= shade (main.rs:114-127) =================
                const float em = at32(p.emis, prim);
                const float4 ma = at32(p.mat, prim);
                if (em > 0.0f) {                                                       // main.rs:116-117
                    cr = ma.x * em;
                    cg = ma.y * em;
                    cb = ma.z * em;
                    status = RT_BOUNCE_EMITTED;
                } else {
                    cr = ma.x;
                    cg = ma.y;
                    cb = ma.z;
                    status = RT_BOUNCE_SCATTERED;
                    scattered = true;
                    if (!p.seed_states) {
                        const uint64_t* s = p.rng_state + 4 * i;
                        rng.s0 = s[0];
                        rng.s1 = s[1];
                        rng.s2 = s[2];
                        rng.s3 = s[3];
                    }
                    float x1, x2, sm;
                    for (;;) {                                                         // UnitSphere, main.rs:119
                        x1 = uniform_m1_1(rng);
                        x2 = uniform_m1_1(rng);
                        sm = x1 * x1 + x2 * x2;
                        if (!(sm >= 1.0f)) break;
                    }
                    const float factor = 2.0f * RT_SQRT(1.0f - sm);
                    const V3 us = mk(x1 * factor, x2 * factor, 1.0f - 2.0f * sm);
                    const V3 diffuse_dir = us + n;
                    const V3 glossy_dir = d - (2.0f * dot(d, n)) * n;                  // main.rs:120-121
                    const V3 pre = diffuse_dir + ma.w * (glossy_dir - diffuse_dir);    // main.rs:122
                    V3 xdir;
                    if (!try_normalize(pre, xdir)) xdir = n;                           // main.rs:126
                    const V3 d2 = normalize(xdir);                                     // Ray::new (ray.rs:134)
                    p.rays[2 * i] = make_float4(hp.x, hp.y, hp.z, t_min);              // origin exactly P, the window kept
                    p.rays[2 * i + 1] = make_float4(d2.x, d2.y, d2.z, t_max);
                }
            }
            if (scattered || p.seed_states) {
                uint64_t* s = p.rng_state + 4 * i;
                s[0] = rng.s0;
                s[1] = rng.s1;
                s[2] = rng.s2;
                s[3] = rng.s3;
            }
            p.bounce[i] = make_uint4(__float_as_uint(cr), __float_as_uint(cg), __float_as_uint(cb), status);
            if (p.hits) {
                p.hits[2 * i] = w0;
                p.hits[2 * i + 1] = w1;
            }
        }
        // ================= compaction: one atomic per wave =================
        if (p.n_next) {
            const unsigned long long mask = __ballot(scattered);
            if (mask) {
                const int leader = (int)__builtin_ctzll(mask);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                uint32_t base = 0;
                if ((int)(tid & 63u) == leader) base = atomicAdd(p.n_next, (uint32_t)__builtin_popcountll(mask));
                base = (uint32_t)__shfl((int)base, leader, 64);
                // (base + rank < n unless the caller's list names a ray twice: such an entry is dropped, not written out of bounds)
                if (scattered && p.next_active && (uint64_t)base + rank < p.n) p.next_active[base + rank] = (uint32_t)i;
            }
        }
    }
    // counters: one atomic per wave
    n_rays = wave_sum(n_rays);
    n_tests = wave_sum(n_tests);
    if ((tid & 63u) == 0) {
        if (n_rays) atomicAdd(p.counters + 0, n_rays);
        if (n_tests) atomicAdd(p.counters + 1, n_tests);
    }
}

using BounceFn = void (*)(const BParams);
BounceFn bounce_kernel(int engine, int scan_mode);    // rt_kernels_bounce.hip; nullptr for a combination that does not exist

}  // namespace rtk
