// rt_plan.h — the plan of one batched launch (rt_api.hip launch_batch): which engine renders it, the LDS layout of its kernel,
// the camera, the sample units and the split of its queue.  A pure function of the scene's shape, the request and the launch-path
// knobs: plain C++, no HIP (also built by g++ in the CPU harness tests/host/plan_host.cpp, tests/test_launch_plan.py).
//
// The planner writes the kernel parameters it decides into `p`: rtk::KParams in rt_api.hip, a struct with the same scalar fields
// in the harness.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rt_consts.h"
#include "rt_tile.h"

namespace rtplan {

constexpr size_t LDS_LIMIT = 160 * 1024 - 3072;   // dynamic LDS budget; 3 KiB left for the kernels' static LDS (the queue words and
                                                  // one rtk::WaveQ per wave: 16 + 16 x 160 bytes in the 1024-thread kernel)
constexpr uint32_t RESIDENT_MAX = rtk::CHUNK;   // spheres kept wholly in LDS
constexpr uint32_t STREAM_CHUNK = 2048;         // chunk size when streaming through LDS
constexpr uint32_t STACK_LDS_MAX = 12;          // quantised-node kernel: stack entries per lane in LDS, deeper ones in HBM
constexpr uint32_t RT_QNODES_MIN_PRIMS = 4096;   // from here up the traversal walks the 32-byte quantised nodes (tools/crossover_q.py)
constexpr uint32_t DENSE_SCAN_MAX_PRIMS = 192;       // piles of up to this many spheres at a box density of at least ...
constexpr float DENSE_SCAN_MIN_DENSITY = 3.0f;       // ... this keep the linear scan (see `traverse`)
constexpr float DENSE_MID_MIN_DENSITY = 2.5f;        // dense sphere scenes of at least DENSE_MID_MIN_PRIMS whose tree does not fit LDS
constexpr uint32_t DENSE_MID_MIN_PRIMS = 512;        //   take the quantised nodes for the culled walk (see `dense_mid`)
constexpr float FIELD_MID_MIN_DENSITY = 0.15f;       // sphere fields below RT_QNODES_MIN_PRIMS take the quantised nodes from here up (`field_mid`)
constexpr float LT_CULL_MIN_DENSITY = 2.2f;          // the LDS-resident tree is walked nearer child first, with distance culling, from this box density up
                                                     // (tests/test_gpu_engine_rules.py: at 1.1 ... 1.8 a helix, a lattice and a colonnade of 700 ... 960
                                                     // spheres lose 7 ... 17 % to the culled step, piles at 1.8 / 2.7 gain 2 / 38 %)
constexpr uint32_t TRAVERSE_MIN_PRIMS = 2;      // from this many primitives up the BVH-traversal engine is the default.  (Rounds 1-3: 32, with a density rule below it;
                                                // with the sample units the LDS-resident tree leads the scan on every scene of tools/small_scene_matrix.py —
                                                // 2 ... 32 spheres, five families, 1.02 ... 1.36 x — but one pile of 32, and on c2's 16-sphere room by 5 ... 8 %.)

// The scalar facts of a scene the rules read (rt_scene_host.h build_host_scene computes them).
struct SceneShape {
    uint32_t n_sph = 0, n_sph_pad = 0, n_tri = 0;   // spheres (padded to rtk::UNROLL), triangles
    uint32_t bvh_depth = 0, n_internal = 0;         // the reference BVH: depth, internal nodes
    uint32_t root_ref = 0;                          //   root reference (LEAF_BIT | prim when the tree is a single leaf)
    float cull_density = 0.f;      // box density of the primitives outside the culled walks' `big` list
    bool cull_pays = false;        // host heuristic: the scene is dense enough for the culled walk
    bool xcull_pays = false;       //   ... the same for scenes with triangles
    bool quant_ok = false;         // quantised walk usable and worthwhile (grid step small against the primitives)
    bool tri_ok = false;           // every triangle has a finite culling bound or a place in the `big` list
    float r_slack = 0.f;           // largest radius among the spheres not in `big`
    bool inverted_boxes = false;   // a sphere of negative radius: its AABB has lo > hi (sphere.rs:65-72)
    bool expanded = false;         // expanded-form broad phase: margin small against r^2
    float leaf_density = 0.f;      // sum of primitive box areas / scene box area
};

// The launch-path knobs the plan reads (rt_api.hip DebugKnob: RT_LDS_TREE, RT_CULL_WALK, ...); the defaults are the product's.
struct Knobs {
    int lds_tree = 1;         // 0: never the LDS-resident tree engine
    int cull_walk = -1;       // 0 / 1: culled walks off / on wherever they are valid; -1: host rule
    int no_stage = 0;         // 1: no LDS output staging
    int slots = 0;            // pixel slots per wave; 0: host rule
    int commit_slots = 0;     // complete slots a commit waits for; 0: host rule
    int force_capped = 0;     // 1: quantised walks take the capped-stack kernel
    int stack_lds = 0;        // capped-stack kernel: stack entries per lane in LDS; 0: STACK_LDS_MAX
    int compact = 1;          // 0: per-lane root tests in the exact-node L2 kernel
    int refill_eighths = 0;   // refill threshold of the walks; 0: host rule
    int tail_tiles = -1;      // tiles at the end of the queue handed out in parts; -1: host rule
    int ltree_general = 0;    // 1: the LDS-tree engines take their general kernel (spheres and triangles) whatever the world holds
    int plain_frame = 1;      // 0: no launch counts as a plain frame (the LDS-tree kernels commit through their general path)
};

// The engines (rt_tile_stats.engine) and the kernels that run them: template argument ISECT of rtk::rt_tile_kernel, that of the
// capped-stack kernel where the engine has one, and the workgroup size.
struct Engine {
    int isect, isect_capped, block;
};
constexpr Engine ENGINES[8] = {
    {0, -1, rtk::BLOCK},         // 0 linear scan, scene resident in LDS
    {1, -1, rtk::BLOCK},         // 1 linear scan, scene streamed through LDS
    {2, -1, rtk::BLOCK},         // 2 BVH traversal, exact nodes from L2
    {3, 4, rtk::BLOCK},          // 3 BVH traversal, quantised nodes
    {5, -1, rtk::LTREE_BLOCK},   // 4 BVH traversal, exact nodes resident in LDS
    {7, 8, rtk::BLOCK},          // 5 BVH traversal, quantised nodes, nearer child first with distance culling (spheres only)
    {9, -1, rtk::BLOCK},         // 6 BVH traversal, exact nodes, nearer child first with distance culling
    {6, -1, rtk::LTREE_BLOCK},   // 7 BVH traversal, exact nodes resident in LDS, nearer child first with distance culling
};
constexpr int N_ISECT = 10;      // ISECT 0, 1: rtk::kernel_linear; 2 ... 9: rtk::kernel_traverse

// Samples [begin, end) of the request's spp; pass: a progressive pass (the strips' running sums are carried).
struct SampleRange {
    uint32_t begin, end;
    bool pass;
};

struct Plan {
    int status = RT_OK;          // RT_ERR_LIMIT: a budget is exceeded (`error` says which); nothing else below is meaningful then
    const char* error = nullptr;
    int engine = 0;              // rt_tile_stats.engine
    bool capped = false;         // the quantised walk keeps only p.stack_lds stack entries per lane in LDS
    int isect = 0;               // the kernel: ENGINES[engine], capped or not
    int block = rtk::BLOCK;      //   its workgroup size
    bool expanded = false;       //   linear engines: the expanded-form broad phase (rt_tile_stats.broad_form)
    bool count_steps = false;    //   traversal engines: the twin that counts node visits
    bool tris = true;            //   LDS-tree engines (4, 7): false picks the sphere-only instantiation — the world has no triangle
                                 //   (LT_SPHERE_ONLY_MAX_TRIS) and Knobs::ltree_general is 0; every other engine has one kernel: true
    bool plain_shape = false;    // the plan's part of a plain frame (plain_frame below)
    size_t lds = 0;              // dynamic LDS bytes
    uint32_t maxl_l2 = 0;        // leaf slots of an L2 walk (the RT_VERBOSE line's; the LDS tree's own are p.maxl)
    uint32_t ovf_entries = 0;    // capped stack: entries per thread in the HBM overflow area
    // plan_queue
    uint32_t blocks = 0;         // workgroups of the persistent grid
    size_t ring_bytes = 0;       // sample-unit ring: [waves][n_slots][slot_stride] 12-byte records
    size_t ovf_words = 0;        // stack overflow area
};

constexpr uint32_t LT_MAX_PRIMS = 0x7fffu;        // the LDS-tree engines' 16-bit references hold 15 bits of primitive number
constexpr uint32_t PATH16_MAX_PRIMS = 65536u;     // up to here a path stack entry is 16 bits (KParams::path32 == 0)
constexpr uint32_t LT_SPHERE_ONLY_MAX_TRIS = 0;   // the LDS-tree engines take their sphere-only kernel up to this many triangles: none —
                                                  // it rests on the world's contents, not on a measurement: that kernel has no triangle code

// A plain frame: every launch-uniform choice of the commit falls the flagship's way — all samples in one pass and no running sum
// in or out, one pixel per slot (8 samples per pixel and more), a power-of-two sample count (the mean is a product), 16-bit path
// entries — and no strip asks for an f32 plane or a per-strip cost.  The LDS-tree kernels then commit through a copy of the commit
// that carries none of those tests (rtk::KParams::plain); any other launch, and every other engine, takes the general path.
// any_f32 / strip_cost: what the launch's strips and its caller ask for (rt_api.hip launch_batch).
inline bool plain_frame(const Plan& pl, bool any_f32, bool strip_cost) { return pl.plain_shape && !any_f32 && !strip_cost; }

// An explicit request flag wins over the process-level knob (RT_CULL_WALK), the knob over the host rule.
inline bool cull_wanted(uint32_t flags, int knob, bool rule) {
    return (flags & RT_FLAG_NO_CULL_WALK) ? false : (flags & RT_FLAG_CULL_WALK) ? true : knob >= 0 ? knob != 0 : rule;
}

// ---- A placed camera (rt_camera, rt_tile.h "placed camera").  The pose is validated and turned into its basis once,
// by rt_scene_set_camera / rt_frame_ctx_set_camera; every launch forms its camera vectors from the basis and the request's knobs.  Each
// operation below is one f32 rounding in the order written (this header is compiled without contraction on both sides).
struct Pose {
    float origin[3];   // the eye
    float u[3], v[3], w[3];   // right, up, backward (the camera looks down -w)
};

inline float length3(const float a[3]) { return std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }
inline void cross3(const float a[3], const float b[3], float out[3]) {    // the two products of a component rounded separately
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// w = (origin - target) / |origin - target| (division by the length, as Ray::new), u = c / |c| with c = up x w, v = w x u.
// false, and `ps` untouched: a component that is not finite, a length that is 0 or not finite, flags or reserved not 0.
inline bool make_pose(const rt_camera& c, Pose& ps) {
    if (c.flags != 0 || c.reserved != 0) return false;
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(c.origin[i]) || !std::isfinite(c.target[i]) || !std::isfinite(c.up[i])) return false;
    Pose r;
    float d[3], x[3];
    for (int i = 0; i < 3; i++) d[i] = c.origin[i] - c.target[i];
    const float ld = length3(d);
    if (!(ld > 0.0f) || !std::isfinite(ld)) return false;
    for (int i = 0; i < 3; i++) r.w[i] = d[i] / ld;
    cross3(c.up, r.w, x);
    const float lx = length3(x);
    if (!(lx > 0.0f) || !std::isfinite(lx)) return false;
    for (int i = 0; i < 3; i++) r.u[i] = x[i] / lx;
    cross3(r.w, r.u, r.v);
    for (int i = 0; i < 3; i++) r.origin[i] = c.origin[i];
    ps = r;
    return true;
}

// The lens vectors of a parameter block that has them (rtk::KParams, rtk::AParams, rtk::CParams); a block without (the launch-plan
// harness's) gets none.
template <class KP>
auto set_lens(KP& p, const float lu[3], const float lv[3], int) -> decltype((void)p.lens_u[0]) {
    for (int i = 0; i < 3; i++) {
        p.lens_u[i] = lu[i];
        p.lens_v[i] = lv[i];
    }
}
template <class KP>
void set_lens(KP&, const float*, const float*, long) {}

// Camera::new with the slave's arguments (main.rs:42-50 -> camera.rs:19-47): the reference camera, Point3::ZERO looking down -z
template <class KP>
void fill_camera(const rt_tile_request& rq, KP& p) {
    const float origin[3] = {0.f, 0.f, 0.f};          // Point3::ZERO
    const float aspect_ratio = (float)rq.width / (float)rq.height;
    const float image_height = (float)rq.height;
    const float vh = 2.0f * std::tan(rq.fov / 2.0f);
    const float vw = aspect_ratio * vh;
    const float hor[3] = {vw, 0.f, 0.f}, ver[3] = {0.f, vh, 0.f};
    const float foc[3] = {0.f, 0.f, rq.focal_length};
    for (int i = 0; i < 3; i++) {
        p.org[i] = origin[i];
        p.hor[i] = hor[i];
        p.ver[i] = ver[i];
        // origin - horizontal / 2 - vertical / 2 - (0,0,focal_length)
        float v = origin[i] - hor[i] / 2.0f;
        v = v - ver[i] / 2.0f;
        v = v - foc[i];
        p.llc[i] = v;
    }
    p.lens_radius = rq.aperture / 2.0f;
    // the lens disc's axes, literally (no multiplication: an extreme aperture keeps its bits)
    const float lens_u[3] = {p.lens_radius, 0.f, 0.f}, lens_v[3] = {0.f, p.lens_radius, 0.f};
    set_lens(p, lens_u, lens_v, 0);
    p.focus_distance = rq.focus_distance;
    p.u_den = aspect_ratio * image_height - 1.0f;      // camera.rs:116
    p.v_den = image_height - 1.0f;                     // camera.rs:117
}

// The same camera placed by a pose (Camera::set_origin, camera.rs:73-83, and a look-at basis): hor = vw u, ver = vh v,
// foc = focal_length w, llc in fill_camera's order, the lens disc spanned by lens_radius u and lens_radius v.
template <class KP>
void fill_camera(const rt_tile_request& rq, const Pose& ps, KP& p) {
    const float aspect_ratio = (float)rq.width / (float)rq.height;
    const float image_height = (float)rq.height;
    const float vh = 2.0f * std::tan(rq.fov / 2.0f);
    const float vw = aspect_ratio * vh;
    p.lens_radius = rq.aperture / 2.0f;
    float lens_u[3], lens_v[3];
    for (int i = 0; i < 3; i++) {
        const float hor = vw * ps.u[i], ver = vh * ps.v[i], foc = rq.focal_length * ps.w[i];
        p.org[i] = ps.origin[i];
        p.hor[i] = hor;
        p.ver[i] = ver;
        float v = ps.origin[i] - hor / 2.0f;
        v = v - ver / 2.0f;
        v = v - foc;
        p.llc[i] = v;
        lens_u[i] = p.lens_radius * ps.u[i];
        lens_v[i] = p.lens_radius * ps.v[i];
    }
    set_lens(p, lens_u, lens_v, 0);
    p.focus_distance = rq.focus_distance;
    p.u_den = aspect_ratio * image_height - 1.0f;
    p.v_den = image_height - 1.0f;
}

// pose == nullptr: the reference camera, on exactly the code path it had before cameras could be placed
template <class KP>
void fill_camera(const rt_tile_request& rq, const Pose* pose, KP& p) {
    if (pose) fill_camera(rq, *pose, p);
    else fill_camera(rq, p);
}

// Everything of a launch of n_strips strips of request rq that does not depend on the device: engine, LDS plan, camera, sample
// units, tiles.  `p` must come zeroed.  pose: the scene's placed camera, nullptr for the reference camera; nothing but the camera
// vectors depends on it (the engine least of all).
template <class KP>
Plan plan_launch(const SceneShape& sh, const rt_tile_request& rq, uint32_t n_strips, const SampleRange& smp, const Knobs& kn, KP& p,
                 const Pose* pose = nullptr) {
    using namespace rtk;
    Plan pl;
    p.W = rq.width;
    p.H = rq.height;
    p.Hs = rq.height / rq.divisions;
    // Everything the launch's work is sized by — slots, magic divisors, queue parts, scratch, primary rays — follows the units per
    // pixel OF THIS LAUNCH; only the stream stride (spp_all) and the mean's divisor (s_end) see the job's whole sample count.
    const uint32_t s_begin = smp.begin, s_end = smp.end;
    p.upp = s_end - s_begin;
    p.spp_all = rq.spp;
    p.s_begin = s_begin;
    p.gap = rq.spp - p.upp;
    p.acc_out = smp.pass ? 1u : 0u;
    p.depth = rq.max_bounces + 1;
    p.n_sph = sh.n_sph;
    p.n_sph_pad = sh.n_sph_pad;
    p.n_tri = sh.n_tri;
    p.flags = rq.flags;
    // A sphere of negative radius has an AABB with lo > hi (Sphere::aabb = center -+ radius, sphere.rs:65-72): the reference's
    // sign-selected slab test rejects such a box for (almost) every ray, while the finite-direction shortcut of the kernels
    // (min / max of the two plane values, valid for lo <= hi) would enter it.  Such a scene is rendered with the crate's
    // literal test and the whole box chain throughout (the RT_FLAG_FULL_CHAIN path): slower, and exact.
    if (sh.inverted_boxes) p.flags |= RT_FLAG_FULL_CHAIN;
    const uint32_t fl = rq.flags;
    // Engine choice.  BVH traversal reproduces reference semantics only, needs the tree to fit the traversal
    // stack, and pays off once the scene is larger than a couple of LDS chunks; RT_FLAG_BVH_TRAVERSE /
    // RT_FLAG_LINEAR_SCAN force either engine for A/B runs and tests.
    const uint32_t n_prims = sh.n_sph + sh.n_tri;
    const bool trav_ok = !(fl & (RT_FLAG_EXACT_SCAN | RT_FLAG_NO_BVH_CULL | RT_FLAG_LINEAR_SCAN)) &&
                         sh.bvh_depth < (uint32_t)TRAV_STACK && n_prims > 0;   // LDS stack: (depth + 1) KiB per workgroup
    // (Small PILES of overlapping spheres keep the scan: at a box density of 3 and more a ray meets so many leaf boxes that up
    // to about 200 spheres the scan's 64 packed instructions per 8 spheres beat any walk — tools/dense_matrix.py, 48 ... 192 spheres at
    // density 3.3 ... 13: the culled LDS-tree walk of round 4 renders them at 0.67 ... 0.84 of the scan (the plain one: 0.59 ... 0.92), at
    // 256 it leads by 1.4 ... 1.5 x.  Round 3's two further pile rules — up to 384 spheres at densities 5 ... 12 to the scan, larger or
    // denser piles to the culled L2 walk although their tree fits LDS — are gone: the culled LDS-tree walk is the best engine in
    // every cell of tools/dense_mid_matrix.py, by 13 ... 30 %.)
    const bool dense_pile = sh.n_tri == 0 && n_prims <= DENSE_SCAN_MAX_PRIMS && sh.cull_density >= DENSE_SCAN_MIN_DENSITY;
    const bool traverse = trav_ok && ((fl & RT_FLAG_BVH_TRAVERSE) || (n_prims >= TRAVERSE_MIN_PRIMS && !dense_pile));
    // node format: from RT_QNODES_MIN_PRIMS primitives up the 32-byte quantised nodes (half the gather footprint, and an
    // LDS plan that keeps five workgroups per CU whatever the tree's depth): +14 % on sparse fields of every size, +17...29 %
    // on dense fields of 32 768+ spheres, within 2.5 % either way in between; below it the exact-node kernel's six
    // waves per SIMD win on the headline scene (c3 +1.5 %).  tools/crossover_q.py, DESIGN.md 4.7
    // (meshes keep the exact nodes: a quantised walk validates a triangle leaf by walking its box chain — two more gathers
    // per improving hit — and lost 2...16 % on the generated terrains of 7 200 and 100 352 triangles, tools/heuristics_matrix.py)
    // LDS-resident tree (engines 4 and 7): the exact 64-byte nodes of a small scene staged into LDS by one
    // 1024-thread workgroup per CU, 16-bit references / stack / leaf lists.  RT_FLAG_NO_LDS_TREE forces the
    // L2-gather kernel (A/B runs, tests).
    bool ltree_fits = false;
    const size_t lt_lane = ((size_t)MAXL_LTREE + (size_t)(rq.max_bounces + 1) + (size_t)(sh.bvh_depth + 2)) * sizeof(uint16_t);
    static_assert(LT_MAX_PRIMS <= PATH16_MAX_PRIMS, "the LDS-tree kernels compile the 32-bit path entries out (rt_kernel.hip.h path32())");
    if (traverse && kn.lds_tree != 0 && !(fl & RT_FLAG_NO_LDS_TREE) && sh.n_internal > 0 && n_prims <= LT_MAX_PRIMS &&
        ((size_t)sh.n_internal + 2) * LNODE_DW < 0x8000u) {
        const size_t fixed = (((size_t)sh.n_internal + 2) * LNODE_DW + n_prims) * 4 + 16 + lt_lane * LTREE_BLOCK;   // + node DONE and the NaN field
        ltree_fits = fixed <= LDS_LIMIT;
    }
    // (Below the threshold a DENSE sphere scene whose tree does not fit LDS also takes the quantised nodes, for the culled
    // walk below: tools/cull_matrix_small.py, 2 000...3 500 overlapping spheres 1.55...1.95 x over the exact-node walk, fields of
    // box density 1...2 0.87...0.98 — hence the higher bar of DENSE_MID_MIN_DENSITY here.)
    // (round 4: piles whose tree FITS LDS no longer need a rule — the LDS-resident tree has its own culled walk, below)
    const bool dense_mid = sh.cull_pays && !(fl & RT_FLAG_NO_CULL_WALK) && !ltree_fits && sh.cull_density >= DENSE_MID_MIN_DENSITY &&
                           n_prims >= DENSE_MID_MIN_PRIMS;
    // (... and so does a sphere FIELD between the LDS tree's limit and that threshold: at box densities of 0.15 and more the quantised
    // walk leads the exact one by 17...24 % there — tools/qnodes_mid_matrix.py, 1200...4000 spheres; flat sheets of small spheres,
    // 0.03...0.1, are the scenes the exact nodes win by up to 12 %, and clusters fail quant_ok)
    const bool field_mid = !ltree_fits && sh.n_tri == 0 && n_prims < RT_QNODES_MIN_PRIMS && sh.cull_density >= FIELD_MID_MIN_DENSITY;
    const bool qnodes = traverse && sh.quant_ok && !(fl & RT_FLAG_EXACT_NODES) &&
                        ((fl & RT_FLAG_QUANT_NODES) || (n_prims >= RT_QNODES_MIN_PRIMS && sh.n_tri <= sh.n_sph) || dense_mid ||
                         field_mid);
    const bool ltree = ltree_fits && !qnodes;
    // Culled walk (engine 5): the quantised walk nearer child first, subtrees beyond the running closest hit
    // skipped.  Spheres only (the bound is derived from the sphere root test's error terms).
    // Default where the host heuristic says it pays (cull_pays: DESIGN.md 4.7); RT_FLAG_CULL_WALK / RT_FLAG_NO_CULL_WALK
    // force it on / off (A/B runs, tests), RT_CULL_WALK=0/1 likewise for a whole process.
    const bool cull = qnodes && cull_wanted(fl, kn.cull_walk, sh.cull_pays) && sh.n_tri == 0 && std::isfinite(sh.r_slack);
    // ... and over the exact nodes (engine 6): scenes with triangles — the bound of cull_bound_tri — wherever the exact-node
    // L2 walk is the engine; default where the host heuristic says it pays (xcull_pays), forced by the same flags
    const bool xcull = traverse && !qnodes && !ltree && cull_wanted(fl, kn.cull_walk, sh.xcull_pays) && sh.n_tri > 0 && sh.tri_ok &&
                       std::isfinite(sh.r_slack) && !sh.inverted_boxes;
    // ... and in the LDS-resident tree (engine 7; round 4): the same bound, so the same premises (a finite slack
    // radius, triangles within the K limit or in the `big` list, no inverted boxes); default from a box density of LT_CULL_MIN_DENSITY
    // up — below it the rays meet so few leaf boxes that ordering the children costs more than the skipped subtrees save
    // (tools/dense_matrix.py, tools/dense_mid_matrix.py, tests/test_gpu_engine_rules.py)
    const bool lt_cull_ok = ltree && !sh.inverted_boxes && std::isfinite(sh.r_slack) && (sh.n_tri == 0 || sh.tri_ok);
    const bool ltcull = lt_cull_ok && cull_wanted(fl, kn.cull_walk, sh.cull_density >= LT_CULL_MIN_DENSITY);
    const bool streamed = !traverse && sh.n_sph_pad > RESIDENT_MAX;
    pl.engine = traverse ? (ltree ? (ltcull ? 7 : 4) : qnodes ? (cull ? 5 : 3) : xcull ? 6 : 2) : (streamed ? 1 : 0);
    const int bs = ENGINES[pl.engine].block;
    p.chunk = traverse ? 0 : (streamed ? STREAM_CHUNK : sh.n_sph_pad);
    p.n_chunks = p.chunk ? (sh.n_sph_pad + p.chunk - 1) / p.chunk : 0;
    p.path32 = (sh.n_sph + sh.n_tri) > PATH16_MAX_PRIMS ? 1u : 0u;
    size_t geom_bytes = traverse ? 0 : (size_t)(p.chunk ? p.chunk : 1) * 4 * sizeof(float);   // float4 records
    p.lds_cand_off = (uint32_t)geom_bytes;
    size_t path_bytes = (size_t)p.depth * BLOCK * (p.path32 ? 4 : 2);
    // ---- LDS plan of a traversal launch.  Occupancy is worth more than long leaf lists (c3: 6 workgroups per CU with
    // 7 slots +1.5 % over 5 with 8; c5: 5 with 5 slots +7.5 % over 4 with 8), and an uncapped stack more than either
    // (the HBM-overflow test on every push / pop costs 6...10 %).  So: the target number of workgroups per CU follows
    // from the kernel's registers (five waves per SIMD for both node formats).  The exact-node kernel has 7 slots, fixed; the quantised
    // kernel's lists shrink from MAXL down to MINL slots to reach its target, and a quantised walk whose whole stack still
    // does not fit takes the capped-stack kernel.
    // stack slots per lane: up to bvh_depth pending right children (+ 1 spare); the LDS-tree kernel's branch-free step
    // adds the DONE sentinel in slot 0 and needs the free slot its unconditional stores land in
    // output staging (one tile per wave): wherever the LDS plan has room for it
    const bool want_stage = kn.no_stage == 0 && ((traverse && !ltree) || streamed);     // the kernels it is compiled into (see there)
    const bool list16 = traverse && !ltree && n_prims <= 65536u;          // 16-bit leaf-list entries: half the LDS
    const size_t stage_bytes_wg = (size_t)STAGE_TILES * STAGE_TILE_BYTES * (bs / 64);
    const uint32_t stack_capped = sh.bvh_depth + 1;
    const uint32_t stack_need = sh.bvh_depth + (ltree ? 2u : 1u);
    uint32_t maxl = qnodes ? (uint32_t)MAXL : (uint32_t)MAXL_EXACT, stack_lds = stack_need;
    if (traverse && qnodes) {
        const size_t per_wg = (160u * 1024u - 4096u) / 5u - 512u;     // 4 KiB of slack, 464 B static LDS
        const size_t slot = (size_t)BLOCK * (list16 ? sizeof(uint16_t) : sizeof(uint32_t));
        const size_t fixed = path_bytes + (size_t)stack_need * BLOCK * sizeof(uint32_t) + (want_stage ? stage_bytes_wg : 0);
        // (force_capped / stack_lds: tests drive the capped-stack kernel with small trees)
        if (kn.force_capped == 0 && fixed + (size_t)MINL * slot <= per_wg) {
            maxl = (uint32_t)std::min<size_t>((size_t)MAXL, (per_wg - fixed) / slot);
        } else {
            const uint32_t cap = kn.stack_lds > 0 ? (uint32_t)kn.stack_lds : STACK_LDS_MAX;
            pl.capped = stack_capped > cap;
            stack_lds = pl.capped ? cap : stack_need;
        }
    }
    p.maxl = maxl;
    p.stack_lds = stack_lds;
    p.list16 = list16 ? 1u : 0u;
    size_t cand_bytes = traverse ? (size_t)maxl * BLOCK * (list16 ? sizeof(uint16_t) : sizeof(uint32_t))
                                 : (size_t)MAXC * BLOCK * sizeof(uint16_t);
    p.lds_path_off = (uint32_t)(geom_bytes + cand_bytes);
    const bool expanded = !traverse && sh.expanded && !(fl & RT_FLAG_OC_BROAD_PHASE);
    p.lds_rr_off = (uint32_t)(geom_bytes + cand_bytes + path_bytes);
    size_t rr_bytes = expanded ? (size_t)(p.chunk ? p.chunk : 1) * sizeof(float) : 0;
    p.lds_stack_off = (uint32_t)(geom_bytes + cand_bytes + path_bytes + rr_bytes);
    size_t stack_bytes = traverse ? (size_t)stack_lds * BLOCK * sizeof(uint32_t) : 0;
    size_t lds = geom_bytes + cand_bytes + path_bytes + rr_bytes + stack_bytes;
    p.n_internal = sh.n_internal;
    p.lds_node_off = 0;
    if (ltree) {
        // [nodes][leaf lists u16][path u16][stack u16]
        size_t off = ((((size_t)sh.n_internal + 2) * LNODE_DW + n_prims) * 4 + 15) & ~(size_t)15;    // nodes, DONE, NaN field of n_prims + 19 dwords
        p.lds_cand_off = (uint32_t)off;
        // leaf-list slots: MAXL_LTREE, and up to MAXL_LTREE_MAX where the tree leaves room (fewer flushes forced by a full list)
        uint32_t lt_maxl = MAXL_LTREE;
        while (lt_maxl < (uint32_t)MAXL_LTREE_MAX &&
               off + ((size_t)(lt_maxl + 1) + p.depth + stack_need) * bs * sizeof(uint16_t) <= LDS_LIMIT) lt_maxl++;
        p.maxl = lt_maxl;
        off += (size_t)lt_maxl * bs * sizeof(uint16_t);
        p.lds_path_off = (uint32_t)off;
        off += (size_t)p.depth * bs * sizeof(uint16_t);
        p.lds_stack_off = (uint32_t)off;
        off += (size_t)stack_need * bs * sizeof(uint16_t);
        lds = off;
    }
    // compacted root tests of the exact-node L2 kernel (1 KiB per wave; RT_COMPACT=0 keeps the per-lane flush for A/B runs)
    p.lds_cmp_off = 0xffffffffu;
    if (traverse && !qnodes && !ltree && kn.compact != 0 && lds + 1024u * (BLOCK / 64) + 16 <= LDS_LIMIT) {
        lds = (lds + 15) & ~(size_t)15;
        p.lds_cmp_off = (uint32_t)lds;
        lds += 1024u * (BLOCK / 64);
    }
    p.lds_stage_off = 0xffffffffu;
    if (want_stage && lds + stage_bytes_wg <= LDS_LIMIT) {
        lds = (lds + 15) & ~(size_t)15;
        p.lds_stage_off = (uint32_t)lds;
        lds += stage_bytes_wg;
    }
    pl.lds = lds;
    if (lds > LDS_LIMIT) {
        pl.status = RT_ERR_LIMIT;
        pl.error = "LDS budget exceeded (scene chunk + path stack)";
        return pl;
    }
    pl.isect = pl.capped ? ENGINES[pl.engine].isect_capped : ENGINES[pl.engine].isect;
    pl.block = bs;
    pl.expanded = expanded;
    pl.count_steps = traverse && (fl & RT_FLAG_COUNT_STEPS);
    pl.tris = !(ltree && sh.n_tri <= LT_SPHERE_ONLY_MAX_TRIS && kn.ltree_general == 0);
    pl.maxl_l2 = maxl;
    pl.ovf_entries = pl.capped ? stack_capped - stack_lds : 0u;
    fill_camera(rq, pose, p);
    p.t_min = rq.t_min;
    p.t_max = rq.t_max;
    p.spp_f = (float)s_end;
    p.spp_rcp = (s_end & (s_end - 1u)) == 0u ? 1.0f / (float)s_end : 0.0f;         // a power of two up to 2^31: exact in f32
    p.root_ref = sh.root_ref;
    if (ltree) p.root_ref = (p.root_ref & LEAF_BIT) ? (0x8000u | (p.root_ref & 0x7fffu)) : lt_r0(sh.n_internal) + p.root_ref * (uint32_t)LNODE_DW;
    // refill threshold: long walks (large scenes) want finished lanes replaced sooner, short walks amortise the
    // per-round shading / ray-generation code over more finished lanes (tools/variants_q.sh sweeps)
    p.refill_eighths = kn.refill_eighths > 0 ? (uint32_t)kn.refill_eighths : (n_prims >= RT_QNODES_MIN_PRIMS ? 4u : 2u);
    p.n_strips = n_strips;
    // Tile shape: 64x1 keeps each tile on whole 64-byte lines of the RGB8 strip (64 px * 3 B = 3 lines),
    // so one CU / one XCD L2 writes every byte of a line; 8x8 tiles split lines across XCDs and doubled the
    // HBM write traffic (profiles/r01_*).
    p.tiles_x = (p.W + 63u) / 64u;
    p.tiles_per_strip = p.tiles_x * p.Hs;
    // Sample units (rt_kernel.hip.h): pixel slots per wave, the commit threshold, the division by the units per pixel
    {
        p.grp = p.upp >= 8u ? 1u : (8u + p.upp - 1u) / p.upp;            // a slot is at least 8 units
        const uint64_t slot_units = (uint64_t)p.grp * p.upp;
        p.grp_magic = p.grp > 1u ? (uint32_t)((1ull << 32) / p.grp) + 1u : 0u;
        p.slot_stride = 1u + (uint32_t)slot_units;
        // enough slots for the pixels in flight (64 lanes' units, each pixel open as long as its longest path) plus the complete
        // ones a commit waits for.  The price of every slot is scratch that L2 has to keep between a sample's store and its pixel's
        // commit; what L2 does not keep goes out to HBM (c3, WRITE_SIZE per 23.7 MiB frame / Mrays/s: 32 slots 135 / 15 580, 24 slots
        // 88 / 15 330, 20 slots 40 / 15 270, 16 slots 33 / 14 300; c4 at 12 / 16 / 24 slots: 15 615 / 16 070 / 16 220 Mrays/s).  The
        // rate is what this path is measured by, HBM is idle either way (c3: 20 GB/s of 8 TB/s): 384 units per wave, at most 32 slots
        // — but never fewer than 16 pixels open while a pixel is at most 256 units: a slot is free again only when its LAST sample is in,
        // and with the 4 slots the 384 units gave the reference's literal 100 samples per pixel a wave stood still for want of a slot
        // (the mesh at 100 spp: 4 / 8 / 16 / 32 slots 6 990 / 7 250 / 7 340 / 7 370 Mrays/s); 8 up to 1 024 units, 4 beyond (scratch:
        // 12 bytes per unit and slot for every wave of the grid)
        const uint64_t fewest = slot_units <= 256u ? 16u : slot_units <= 1024u ? 8u : 4u;
        p.n_slots = kn.slots > 0 ? std::min<uint32_t>((uint32_t)kn.slots, SLOTS_MAX)
                                 : (uint32_t)std::min<uint64_t>(SLOTS_MAX, std::max<uint64_t>(fewest, 384u / slot_units));
        const uint32_t cs = kn.commit_slots > 0 ? (uint32_t)kn.commit_slots : std::max<uint32_t>(1u, p.n_slots / 4u);     // (c3: 4 ... 20 of 32 within 1 %)
        p.commit_slots = std::min<uint32_t>(cs, p.n_slots);
        // q / d == mulhi(q, floor(2^32 / d) + 1) whenever q * d < 2^32: q < 65 * upp with upp <= RT_MAX_SPP (4096)
        p.spp_magic = p.upp > 1u ? (uint32_t)((1ull << 32) / p.upp) + 1u : 0u;
        p.slotu_magic = (uint32_t)((1ull << 32) / slot_units) + 1u;
    }
    const uint64_t n_tiles = (uint64_t)p.tiles_per_strip * n_strips;
    if (n_tiles > 0x1fffffffull) {
        pl.status = RT_ERR_LIMIT;
        pl.error = "too many tiles in one launch";
        return pl;
    }
    p.tiles_total = (uint32_t)n_tiles;
    p.n_tiles = (uint32_t)n_tiles;             // (queue entries: the split into whole tiles and parts follows the grid, plan_queue)
    p.tiles_big = (uint32_t)n_tiles;
    pl.plain_shape = ltree && kn.plain_frame != 0 && p.s_begin == 0u && p.acc_out == 0u && p.grp == 1u && p.spp_rcp != 0.0f && p.path32 == 0u;
    return pl;
}

// The persistent grid of the launch — `blocks` workgroups as the chip holds them at the plan's LDS / register budget, fewer when the
// launch has fewer tiles than waves — its queue entries and the sizes of its scratch.
template <class KP>
void plan_queue(Plan& pl, uint32_t blocks, const Knobs& kn, KP& p) {
    const uint32_t waves_per_wg = (uint32_t)pl.block / 64u;
    const uint32_t useful = (p.n_tiles + waves_per_wg - 1) / waves_per_wg;   // a wave needs at least one tile
    if (blocks > useful) blocks = useful ? useful : 1;
    pl.blocks = blocks;
    // Queue entries.  Whole tiles (64 pixels x spp units) first, and the LAST ones — two tiles per wave of the grid — in parts: quarters
    // (16 pixels), so that the launch's tail is one short entry long.  Two cases take parts for EVERY tile (round 4, measured on the
    // 100 352-triangle mesh: 1080p / 4 spp +13 %, 100 spp +19 %): a launch with fewer than 16 tiles per wave — its expensive tiles
    // (handed out first: the bottom rows) are still being worked on when the cheap ones at the end of the queue have long run out, and
    // an expensive whole tile is a large share of such a launch — and more than 16 samples per pixel, where a whole tile is thousands of
    // units; from 33 samples per pixel up the parts are sixteenths (4 pixels).  The price where it is not needed: 1-2 % (c2, c4).
    const uint64_t waves = (uint64_t)blocks * waves_per_wg;
    const bool all_parts = p.tiles_total < 16ull * waves || p.upp > 16u;
    const uint64_t conv = std::min<uint64_t>(p.tiles_total, kn.tail_tiles >= 0 ? (uint64_t)kn.tail_tiles : all_parts ? (uint64_t)p.tiles_total : 2ull * waves);
    p.sub_shift = p.upp > 32u ? 4u : 2u;
    if ((((uint64_t)p.tiles_total - conv) + (conv << p.sub_shift)) > 0x7fffffffull) p.sub_shift = 2u;       // (entry numbers are 31 bits)
    p.tiles_big = p.tiles_total - (uint32_t)conv;
    p.n_tiles = p.tiles_big + ((uint32_t)conv << p.sub_shift);
    p.ovf_stride = blocks * (uint32_t)pl.block;
    pl.ovf_words = (size_t)pl.ovf_entries * p.ovf_stride;
    pl.ring_bytes = (size_t)blocks * waves_per_wg * p.n_slots * p.slot_stride * 12u;
}

// ---- Ray queries (rt_scene_intersect*, rt_query.hip.h).  One lane per caller ray, no sample units: the plan is the
// engine, the semantics of its scan and the slab test — a pure function of the scene's shape and the request flags.
constexpr int QUERY_BLOCK = 256;   // workgroup size of the query kernels

struct QueryPlan {
    int engine = 2;           // rt_tile_stats.engine: 2 the exact-node walk, 1 the scan in primitive order
    int scan_mode = 2;        // engine 1: rtk::consider MODE — 0 plain world order (RT_FLAG_NO_BVH_CULL), 2 BVH semantics, every
                              //   improving hit validated at once
    bool full_chain = false;  // the crate's literal slab test and the whole box chain (RT_FLAG_FULL_CHAIN, or inverted sphere boxes)
    size_t lds = 0;           // dynamic LDS bytes: the walk's per-lane stack
};

// Default: the walk, which reproduces BVH::traverse's depth-first candidate order (ties to the earlier leaf) for spheres and
// triangles alike.  The scan where the walk cannot serve: plain linear semantics (RT_FLAG_NO_BVH_CULL), an explicit scan
// (RT_FLAG_EXACT_SCAN / RT_FLAG_LINEAR_SCAN, BVH semantics), a tree deeper than the stack, an empty world.  Every other flag
// names an engine the query path does not have and changes nothing (rt_tile.h).
inline QueryPlan plan_query(const SceneShape& sh, uint32_t flags) {
    QueryPlan q;
    const uint32_t n_prims = sh.n_sph + sh.n_tri;
    const bool no_cull = (flags & RT_FLAG_NO_BVH_CULL) != 0;
    const bool walk = !no_cull && !(flags & (RT_FLAG_EXACT_SCAN | RT_FLAG_LINEAR_SCAN)) && n_prims > 0 &&
                      sh.bvh_depth < (uint32_t)rtk::TRAV_STACK;
    q.engine = walk ? 2 : 1;
    q.scan_mode = no_cull ? 0 : 2;
    q.full_chain = (flags & RT_FLAG_FULL_CHAIN) != 0 || sh.inverted_boxes;   // (as plan_launch: the finite-direction test needs lo <= hi)
    q.lds = walk ? ((size_t)sh.bvh_depth + 1) * QUERY_BLOCK * sizeof(uint32_t) : 0;
    return q;
}

// ---- Direct lighting of caller rays (rt_scene_direct*, rt_direct.hip.h).  One lane per active hit record; the shadow
// ray takes the query path's engine, so the plan is the query plan plus the one limit of the emitter pick: M up to 2^23, where
// every (float)M is exact and u * (float)M truncates to at most M.
constexpr uint32_t DIRECT_MAX_LIGHTS = 1u << 23;

struct DirectPlan {
    QueryPlan query;          // engine, scan mode, slab test and LDS of the shadow rays
    bool too_many = false;    // n_lights > DIRECT_MAX_LIGHTS: RT_ERR_LIMIT, nothing launched
};

inline DirectPlan plan_direct(const SceneShape& sh, uint32_t n_lights, uint32_t flags) {
    DirectPlan d;
    d.query = plan_query(sh, flags);
    d.too_many = n_lights > DIRECT_MAX_LIGHTS;
    return d;
}

// ---- Next-event estimation for caller rays (rt_scene_trace_nee*, rt_nee.hip.h).  One lane per caller ray; path
// segments and shadow rays take the query path's engine through one closest-hit site, and the fold is forward (no path stack), so
// the plan is the query plan plus the emitter limit of the pick, as plan_direct.
using NeePlan = DirectPlan;

inline NeePlan plan_nee(const SceneShape& sh, uint32_t n_lights, uint32_t flags) { return plan_direct(sh, n_lights, flags); }

// ---- Path tracing of caller rays (rt_scene_trace*, rt_trace.hip.h).  One lane per caller ray, its samples and bounces
// in a loop: the engine is the query path's, the plan adds the path stack and the workgroup size.
constexpr uint32_t TRACE_LDS_CU = 160 * 1024;   // LDS of one CU: the trace kernels have no static LDS
constexpr uint32_t TRACE_BLOCKS[] = {256, 128, 64};   // workgroup sizes, largest first

struct TracePlan {
    int engine = 2;           // as QueryPlan
    int scan_mode = 2;
    bool full_chain = false;
    uint32_t block = 256;     // workgroup size: the largest of TRACE_BLOCKS at which two workgroups share a CU's LDS (64 otherwise)
    bool path32 = false;      // path stack entries are u32 (more than 65 536 primitives, as the tile's path32), else u16
    size_t lds_path_off = 0;  // byte offset of the path stack: behind the walk's (bvh depth + 1) x block u32 entries (engine 2)
    size_t lds = 0;           // dynamic LDS bytes: walk stack + (max_bounces + 1) path entries per lane
};

// max_bounces <= RT_MAX_BOUNCES (checked by the caller).  The largest case, a 62-bounce trace over a tree of depth TRAV_STACK - 1,
// needs (64 + 63) x 4 bytes a lane: 127 KiB at 256 lanes, so it takes 128-lane workgroups (63.5 KiB, two per CU).
inline TracePlan plan_trace(const SceneShape& sh, uint32_t flags, uint32_t max_bounces) {
    const QueryPlan q = plan_query(sh, flags);
    TracePlan t;
    t.engine = q.engine;
    t.scan_mode = q.scan_mode;
    t.full_chain = q.full_chain;
    t.path32 = (sh.n_sph + sh.n_tri) > 65536u;
    const size_t stack_lane = q.engine == 2 ? ((size_t)sh.bvh_depth + 1) * sizeof(uint32_t) : 0;
    const size_t path_lane = ((size_t)max_bounces + 1) * (t.path32 ? 4 : 2);
    for (uint32_t b : TRACE_BLOCKS) {
        t.block = b;
        if (2 * (stack_lane + path_lane) * b <= TRACE_LDS_CU) break;
    }
    t.lds_path_off = stack_lane * t.block;
    t.lds = (stack_lane + path_lane) * t.block;
    return t;
}

// ---- The a-trous denoiser (rt_scene_denoise*, rt_denoise.hip.h).  One lane per pixel of the W x R image P in 64 x 4
// tiles of 256 lanes; the iterations ping-pong two colour buffers in the caller's scratch, next to one guide buffer.  Steps up to
// lds_max_step stage their tile's (64 + 4s) x (4 + 4s) window of colours (and guides) in LDS; larger steps gather through L2.
constexpr uint32_t DN_TILE_X = 64, DN_TILE_Y = 4, DN_BLOCK = DN_TILE_X * DN_TILE_Y;
constexpr uint32_t DN_MAX_ITER = 8;              // RT_DENOISE_MAX_ITERATIONS
constexpr uint32_t DN_LDS_MAX_STEP = 2;          // default: steps 1 and 2 through LDS (tools/denoise_bench.py --lds-step)
constexpr size_t DN_LDS_CU = 160 * 1024;         // LDS of one CU: the denoiser kernels have no static LDS
constexpr uint32_t DN_WG_PER_CU_MAX = 8;         // 2048 lanes of a CU / DN_BLOCK
constexpr size_t DN_REC = 16;                    // bytes of a colour or guide record (float4)
constexpr size_t DN_ALIGN = 256;

struct DenoisePlan {
    uint64_t npix = 0;            // W * R
    uint32_t tiles_x = 0;         // tiles per row band; the launches' grids are tiles_x x (row band height / DN_TILE_Y) workgroups
    size_t off_guide = 0;         // byte offsets in the scratch: the guide records, the two colour buffers
    size_t off_color[2] = {0, 0};
    size_t scratch_bytes = 0;     // rt_denoise_scratch_bytes: independent of the iteration count and the planes
    uint32_t step[DN_MAX_ITER] = {};       // per iteration: the step s
    size_t lds[DN_MAX_ITER] = {};          // per iteration: dynamic LDS bytes of its window, 0: gather through L2
    uint32_t wg_per_cu[DN_MAX_ITER] = {};  // per iteration: workgroups a CU holds by its LDS (at most DN_WG_PER_CU_MAX)
};

inline size_t dn_align(size_t b) { return (b + DN_ALIGN - 1) / DN_ALIGN * DN_ALIGN; }

// The LDS window of step s: (64 + 4s) x (4 + 4s) records of colour, and as many of guide when the call has one.
inline size_t dn_window_bytes(uint32_t s, bool guided) {
    return (size_t)(DN_TILE_X + 4 * s) * (DN_TILE_Y + 4 * s) * DN_REC * (guided ? 2 : 1);
}

// W, R >= 1 with W * R < 2^31 (the tile ABI's largest frame; checked by the caller), iterations <= DN_MAX_ITER.  lds_max_step: the
// largest step staged in LDS (0: none; a window that does not fit DN_LDS_CU gathers through L2 whatever it says).
inline DenoisePlan plan_denoise(uint32_t W, uint32_t R, uint32_t iterations, bool guided, uint32_t lds_max_step = DN_LDS_MAX_STEP) {
    DenoisePlan p;
    p.npix = (uint64_t)W * R;
    p.tiles_x = (W + DN_TILE_X - 1) / DN_TILE_X;
    const size_t buf = dn_align((size_t)p.npix * DN_REC);
    p.off_guide = 0;
    p.off_color[0] = buf;
    p.off_color[1] = 2 * buf;
    p.scratch_bytes = 3 * buf;
    for (uint32_t i = 0; i < iterations && i < DN_MAX_ITER; i++) {
        const uint32_t s = 1u << i;
        p.step[i] = s;
        const size_t b = dn_window_bytes(s, guided);
        if (s <= lds_max_step && b <= DN_LDS_CU) {
            p.lds[i] = b;
            p.wg_per_cu[i] = (uint32_t)std::min<size_t>(DN_WG_PER_CU_MAX, DN_LDS_CU / b);
        } else {
            p.wg_per_cu[i] = DN_WG_PER_CU_MAX;
        }
    }
    return p;
}

// ---- The staging of a host form (rt_api.hip Staging): the call's arrays in the order they lie in the scene's one staging buffer,
// each at a multiple of DN_ALIGN behind the one before.  An entry is present when it has a host side or is STAGE_DEVICE (device
// memory only: the filter's scratch); an absent one, an optional array the caller did not ask for, takes no room.
enum : unsigned { STAGE_UP = 1, STAGE_DOWN = 2, STAGE_DEVICE = 4 };
struct StageEntry {
    const void* host;
    size_t bytes;
    unsigned copy;           // STAGE_UP: uploaded before the launch, STAGE_DOWN: downloaded after it
    size_t off;              // stage_layout's
    bool present() const { return host || (copy & STAGE_DEVICE); }
};
// Sets every entry's offset; returns the bytes the list takes.
inline size_t stage_layout(StageEntry* e, size_t n) {
    size_t top = 0;
    for (size_t k = 0; k < n; k++) {
        e[k].off = top;
        if (e[k].present()) top += dn_align(e[k].bytes);
    }
    return top;
}

// The list of rt_scene_denoise: the scratch, then DN_STAGE_STRIP entries per strip (entry k of strip i is 1 + DN_STAGE_STRIP * i + k):
// its running sum, its guide planes and its outputs.  rgb, f32, lin: NULL or n arrays.
enum { DN_ACCUM, DN_ALBEDO, DN_NORMAL, DN_DEPTH, DN_HITS, DN_RGB, DN_F32, DN_LIN, DN_STAGE_STRIP };
inline std::vector<StageEntry> dn_stage_list(const rt_tile_request& rq, uint32_t n, const float* const* acc, const rt_aov_planes* planes,
                                             uint8_t* const* rgb, float* const* f32, float* const* lin) {
    const uint32_t Hs = rq.height / rq.divisions;
    const size_t npix = (size_t)Hs * rq.width, v3 = npix * 3 * sizeof(float), s1 = npix * sizeof(uint32_t), u8 = npix * 3;
    std::vector<StageEntry> e;
    e.reserve(1 + (size_t)DN_STAGE_STRIP * n);
    e.push_back({nullptr, plan_denoise(rq.width, Hs * n, 0, false).scratch_bytes, STAGE_DEVICE, 0});
    for (uint32_t i = 0; i < n; i++) {
        e.push_back({acc[i], v3, STAGE_UP, 0});
        e.push_back({planes[i].albedo, v3, STAGE_UP, 0});
        e.push_back({planes[i].normal, v3, STAGE_UP, 0});
        e.push_back({planes[i].depth, s1, STAGE_UP, 0});
        e.push_back({planes[i].hits, s1, STAGE_UP, 0});
        e.push_back({rgb ? rgb[i] : nullptr, u8, STAGE_DOWN, 0});
        e.push_back({f32 ? f32[i] : nullptr, v3, STAGE_DOWN, 0});
        e.push_back({lin ? lin[i] : nullptr, v3, STAGE_DOWN, 0});
    }
    return e;
}

}  // namespace rtplan
