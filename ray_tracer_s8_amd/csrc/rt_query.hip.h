// rt_query.hip.h — gfx950 ray-query kernels (rt_scene_intersect*, rt_tile.h "ray queries").
//
// One lane per caller ray: Ray::new (ray.rs:133-143), the closest hit WorldRefList::intersect picks among the candidates of
// BVH::traverse (shapes/mod.rs:158-191, bvh_impl.rs:373-398), and the hit record the reference fills (shapes/mod.rs:15-21).
// Persistent waves stride over the batch; nothing of the tile kernel's sample units, ring or commit.  The ray, the closest hit and
// the record are the shared steps of rt_path_steps.hip.h (load_caller_ray, closest_hit, hit_normal, hit_record).
//
// Engines (rt_tile_stats.engine, rtplan::plan_query):
//   2  walk of the exact 64-byte nodes (rtbvh::TravNode) from L2, depth first, left child first: the leaves are met in the order
//      BVH::traverse returns them, so the first strict minimum of |P - o| is the reference's winner (ties to the earlier leaf)
//      with no rank look-up.  Per-lane stack in LDS, (bvh depth + 1) entries.
//   1  scan of every primitive in storage order: MODE 0 plain linear semantics (ties to the earlier world position through
//      world_rank), MODE 2 BVH semantics (every improving hit validated by its box chain, ties by depth-first rank).  The
//      semantics path; not tuned.
// ANY: the same walk / scan, ended at the first admitted hit.
#pragma once
#include "rt_path_steps.hip.h"

namespace rtk {

struct QParams : SceneRefs {
    const float4* rays;          // [2 n]: rt_ray (o, t_min) (d, t_max)
    uint4* hits;                 // [2 n]: rt_hit (P, distance) (normal, index), as bits
    uint64_t n;
};

// ENGINE 2: the walk; 1: the scan with consider<MODE>.  ANY: stop at the first admitted hit.
template <int ENGINE, int MODE, bool ANY>
__global__ __launch_bounds__(256) void rt_query_kernel(const QParams p) {
    extern __shared__ uint32_t qstack[];                 // [depth + 1][256] (engine 2)
    const uint32_t tid = threadIdx.x;
    unsigned long long n_rays = 0, n_tests = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + tid; i < p.n; i += (uint64_t)gridDim.x * blockDim.x) {
        const CallerRay r = load_caller_ray(p.rays + 2 * i, false);
        const RayAux aux = ray_aux(r.d, p.full_chain != 0);
        n_rays++;
        const Hit h = closest_hit<ENGINE, MODE, ANY>(p, r.o, r.d, r.t_min, r.t_max, aux, qstack, tid, 256u, n_tests);
        uint4 w0, w1;
        hit_none(w0, w1);
        if (h.idx >= 0) {
            const V3 pt = r.o + h.t * r.d;
            hit_record(p, h, pt, hit_normal(p, (uint32_t)h.idx, pt), w0, w1);
        }
        p.hits[2 * i] = w0;
        p.hits[2 * i + 1] = w1;
    }
    flush_counters(p.counters, n_rays, n_tests, tid);
}

using QueryFn = void (*)(const QParams);
QueryFn query_kernel(int engine, int scan_mode, bool any);    // rt_kernels_query.hip; nullptr for a combination that does not exist

}  // namespace rtk
