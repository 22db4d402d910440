// rt_bounce.hip.h — gfx950 path steps of caller rays (rt_scene_bounce*, rt_tile.h "path steps").
//
// One lane per ACTIVE caller ray, one ray_color entry with depth > 0 (main.rs:108-146) per lane: the closest hit of the segment, its
// shade, and — when the ray scatters — the UnitSphere draw from the ray's own RNG state and the scattered ray, written back over the
// ray and the state.  What rt_trace.hip.h does between two segments of its loop, through the same shared steps of rt_path_steps.hip.h
// (closest_hit, hit_normal, hit_record, sky_colour, unit_sphere_pair, scattered_dir); emission is em * albedo.  The albedo product and
// the termination rule are the caller's: a step returns the segment's own factor (rt_bounce.rgb) and its status.
//
// Persistent waves stride over the active list (or over all n rays).  The device form reads the list's length from device memory, so
// consecutive steps need no host synchronisation.  Compaction: the lanes of a wave that scattered are counted by a ballot, ranked by
// mbcnt, and appended to next_active behind ONE atomicAdd per wave on *n_next; every per-ray result lives at the ray's own index, so
// nothing depends on the order of that list.
//
// LDS per lane (rtplan::plan_query): the walk's stack, (bvh depth + 1) u32 entries (engine 2); entry e of lane tid at [e * 256 + tid].
// No per-scene scratch: launches on different streams may overlap.
#pragma once
#include "rt_path_steps.hip.h"

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
    const uint64_t m = active_count(p);
    unsigned long long n_rays = 0, n_tests = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + tid; k < m; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = active_index(p, k);
        bool scattered = false;
        if (i < p.n) {                                                                 // (an index beyond the batch touches nothing)
            const CallerRay r = load_caller_ray(p.rays + 2 * i, p.as_given != 0);
            const V3 o = r.o, d = r.d;
            const RayAux aux = ray_aux(d, p.full_chain != 0);
            n_rays++;
            // ================= one ray_color entry with depth > 0: the closest hit (shapes/mod.rs:158-191) =================
            const Hit h = closest_hit<ENGINE, MODE, false>(p, o, d, r.t_min, r.t_max, aux, bstack, tid, 256u, n_tests);
            uint4 w0, w1;
            hit_none(w0, w1);
            float cr, cg, cb;
            uint32_t status;
            Rng rng;
            if (p.seed_states) rng = seed_state(p.seed + i * (4ull * PHI));
            if (h.idx < 0) {
                const V3 sky = sky_colour(d);                                          // main.rs:135-144
                cr = sky.x;
                cg = sky.y;
                cb = sky.z;
                status = RT_BOUNCE_MISSED;
            } else {
                const uint32_t prim = (uint32_t)h.idx;
                const V3 hp = o + h.t * d;                                             // Ray::at (ray.rs:147-149)
                const V3 n = hit_normal(p, prim, hp);
                hit_record(p, h, hp, n, w0, w1);                                       // shapes/mod.rs:184-190
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
                    if (!p.seed_states) load_rng(p.rng_state + 4 * i, rng);
                    float x1, x2, sm;
                    unit_sphere_pair(rng, x1, x2, sm);                                 // UnitSphere, main.rs:119
                    const V3 d2 = scattered_dir(d, n, ma.w, x1, x2, sm);
                    p.rays[2 * i] = make_float4(hp.x, hp.y, hp.z, r.t_min);            // origin exactly P, the window kept
                    p.rays[2 * i + 1] = make_float4(d2.x, d2.y, d2.z, r.t_max);
                }
            }
            if (scattered || p.seed_states) store_rng(p.rng_state + 4 * i, rng);
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
    flush_counters(p.counters, n_rays, n_tests, tid);
}

using BounceFn = void (*)(const BParams);
BounceFn bounce_kernel(int engine, int scan_mode);    // rt_kernels_bounce.hip; nullptr for a combination that does not exist

}  // namespace rtk
