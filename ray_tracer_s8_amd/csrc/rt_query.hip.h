// rt_query.hip.h — gfx950 ray-query kernels (rt_scene_intersect*, rt_tile.h "ray queries").
//
// One lane per caller ray: Ray::new (ray.rs:133-143), the closest hit WorldRefList::intersect picks among the candidates of
// BVH::traverse (shapes/mod.rs:158-191, bvh_impl.rs:373-398), and the hit record the reference fills (shapes/mod.rs:15-21).
// Persistent waves stride over the batch; nothing of the tile kernel's sample units, ring or commit.  The arithmetic is the
// tile kernel's own, through its device primitives (rt_kernel.hip.h: exact_sphere, exact_triangle, ray_aux, intersects_aabb[_finite],
// bvh_reaches, consider<MODE>): the same operations in the same order, so the same bits.
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
#include "rt_kernel.hip.h"
#include "rt_tile.h"

namespace rtk {

// The scene as closest_hit / query_root read it: the base of every parameter block that finds first hits (QParams, rt_trace.hip.h
// TParams, rt_aov.hip.h AParams).  The host fills it in one place (rt_api.hip scene_refs).
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

struct QParams : SceneRefs {
    const float4* rays;          // [2 n]: rt_ray (o, t_min) (d, t_max)
    uint4* hits;                 // [2 n]: rt_hit (P, distance) (normal, index), as bits
    uint64_t n;
};

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

// ENGINE 2: the walk; 1: the scan with consider<MODE>.  ANY: stop at the first admitted hit.
template <int ENGINE, int MODE, bool ANY>
__global__ __launch_bounds__(256) void rt_query_kernel(const QParams p) {
    extern __shared__ uint32_t qstack[];                 // [depth + 1][256] (engine 2)
    const uint32_t tid = threadIdx.x;
    unsigned long long n_rays = 0, n_tests = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + tid; i < p.n; i += (uint64_t)gridDim.x * blockDim.x) {
        const float4 r0 = p.rays[2 * i], r1 = p.rays[2 * i + 1];
        const V3 o = mk(r0.x, r0.y, r0.z);
        const V3 d = normalize(mk(r1.x, r1.y, r1.z));    // Ray::new: glam normalize, a division by the length
        const float t_min = r0.w, t_max = r1.w;
        const RayAux aux = ray_aux(d, p.full_chain != 0);
        n_rays++;
        const Hit h = closest_hit<ENGINE, MODE, ANY>(p, o, d, t_min, t_max, aux, qstack, tid, 256u, n_tests);
        // the hit record (shapes/mod.rs:184-190): P, |P - o|, the normal of sphere.rs:49-51 / mesh.rs:163-165, the world position
        uint4 w0 = make_uint4(0u, 0u, 0u, __float_as_uint(__builtin_inff())), w1 = make_uint4(0u, 0u, 0u, RT_HIT_NONE);
        if (h.idx >= 0) {
            const uint32_t prim = (uint32_t)h.idx;
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
            w0 = make_uint4(__float_as_uint(pt.x), __float_as_uint(pt.y), __float_as_uint(pt.z), __float_as_uint(h.dist));
            w1 = make_uint4(__float_as_uint(nn.x), __float_as_uint(nn.y), __float_as_uint(nn.z), p.world_rank ? p.world_rank[prim] : prim);
        }
        p.hits[2 * i] = w0;
        p.hits[2 * i + 1] = w1;
    }
    // counters: one atomic per wave
    n_rays = wave_sum(n_rays);
    n_tests = wave_sum(n_tests);
    if ((tid & 63u) == 0) {
        if (n_rays) atomicAdd(p.counters + 0, n_rays);
        if (n_tests) atomicAdd(p.counters + 1, n_tests);
    }
}

using QueryFn = void (*)(const QParams);
QueryFn query_kernel(int engine, int scan_mode, bool any);    // rt_kernels_query.hip; nullptr for a combination that does not exist

}  // namespace rtk
