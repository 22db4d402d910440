// rt_scene_host.h — everything rt_scene_create derives on the host from the primitive lists (rt_api.hip uploads it): the
// reference's candidate-filter BVH, the storage order, the device-layout arrays and the scene facts the engine rules read.
// Plain C++, no HIP: also built by g++ in the CPU harness tests/host/scene_host.cpp (tests/test_scene_host.py pins every
// byte and every SceneShape value of a scene corpus; a change to a threshold here re-records that golden on purpose).
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_bvh.h"
#include "rt_consts.h"
#include "rt_direct_math.h"
#include "rt_plan.h"
#include "rt_tile.h"

namespace rtscene {

struct alignas(16) F4 {               // the device's float4
    float x, y, z, w;
};

constexpr uint32_t REORDER_MIN_PRIMS = 64;      // from here up the primitive records are stored in the tree's depth-first leaf order

// Everything rt_scene_create derives on the host from the primitive lists: the device-layout arrays and the reference's
// candidate-filter BVH.  rt_render_frame builds it ONCE per job and uploads it to every device.
struct HostScene {
    rtplan::SceneShape shape;        // what the engine rules read (rt_plan.h); the rest is uploaded
    std::vector<F4> geom, geom_pk, geom_px, mat, tri_box, geom_r;
    std::vector<float> emis, tri;
    float bvh_build_ms = 0.f;
    rtbvh::FlatBVH bvh;
    std::vector<uint32_t> big;       // culled walk: spheres far larger than the rest (shape.r_slack: the largest radius among the others)
    uint32_t n_big = 0;
    float tri_k = 0.f, tri_diag = 0.f, tri_es = 0.f, tri_e = 0.f;
    std::vector<uint32_t> world_rank;   // the caller's world_index (one dummy entry when none came)
    bool has_order = false;
    std::vector<uint32_t> lights;       // direct lighting: the emitters, in ascending world position (one dummy entry when none)
    uint32_t n_lights = 0;
    // light selection by power (RT_FLAG_LIGHTS_BY_POWER), per emitter k of `lights`: the running sum of the powers, the
    // mixture probability and its inverse; light_ip_prim: that inverse by primitive number (0 for a primitive that does not emit), which
    // the kernels read for the emitter picked and for an emitter a bounce hit.  One dummy entry when there is no emitter.
    std::vector<float> light_c, light_p, light_ip, light_ip_prim;
    float light_total = 0.f;
    bool light_degenerate = true;       // !(total > 0 && total < inf): p = 1 / M, ip = (float)M, the uniform pick
};

// positions in RenderInfo.world: every one of 0 .. n - 1 exactly once
inline bool world_is_permutation(const uint32_t* world_index, uint32_t np) {
    std::vector<bool> seen(np, false);
    for (uint32_t i = 0; i < np; i++) {
        if (world_index[i] >= np || seen[world_index[i]]) return false;
        seen[world_index[i]] = true;
    }
    return true;
}

inline rtbvh::Box sphere_box(const rt_sphere& s) {              // Sphere::aabb, sphere.rs:65-72
    rtbvh::Box box;
    const float c[3] = {s.cx, s.cy, s.cz};
    for (int a = 0; a < 3; a++) {
        box.lo[a] = c[a] - s.radius;
        box.hi[a] = c[a] + s.radius;
    }
    return box;
}

inline rtbvh::Box tri_box(const rt_triangle& t) {               // Triangle::aabb, mesh.rs:46-96 (min_by / max_by order a,c,b)
    rtbvh::Box box;
    for (int a = 0; a < 3; a++) {
        const float va = t.a[a], vb = t.b[a], vc = t.c[a];
        const float m1 = va > vc ? vc : va;      // min_by(a, c): a unless a > c
        box.lo[a] = m1 > vb ? vb : m1;
        const float x1 = va > vc ? va : vc;      // max_by(a, c): c unless a > c
        box.hi[a] = x1 > vb ? x1 : vb;
    }
    return box;
}

// the reference's candidate-filter BVH (slave main.rs:60) is built from these, once per scene instead of per strip
inline std::vector<rtbvh::Box> prim_boxes(const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt) {
    std::vector<rtbvh::Box> boxes(ns + nt);
    for (uint32_t i = 0; i < ns; i++) boxes[i] = sphere_box(sp[i]);
    for (uint32_t i = 0; i < nt; i++) boxes[ns + i] = tri_box(tr[i]);
    return boxes;
}

inline void build_tree(const std::vector<rtbvh::Box>& boxes, const uint32_t* world_index, HostScene& hs) {
    const uint32_t np = (uint32_t)boxes.size();
    auto tb0 = std::chrono::steady_clock::now();
    {
        // BVH::build(&mut req.world) (slave main.rs:60) numbers the shapes by their position in `world`: start the build
        // from the primitives in that order (rt_bvh.h); ties between equal distances then fall as in the reference
        std::vector<uint32_t> order;
        if (hs.has_order) {
            order.resize(np);
            for (uint32_t i = 0; i < np; i++) order[world_index[i]] = i;
        }
        hs.bvh = rtbvh::build(boxes, hs.has_order ? order.data() : nullptr);
    }
    rtbvh::FlatBVH& bvh = hs.bvh;
    hs.bvh_build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - tb0).count();
    hs.shape.n_internal = (uint32_t)bvh.trav.size();        // before the placeholders below
    if (bvh.nodes.empty()) bvh.nodes.push_back(rtbvh::FlatNode{{0, 0, 0}, 0xffffffffu, {0, 0, 0}, 0});
    if (bvh.leaf_of.empty()) bvh.leaf_of.push_back(0);
    if (bvh.trav.empty()) bvh.trav.push_back(rtbvh::TravNode{});
    if (bvh.travq.empty()) bvh.travq.push_back(rtbvh::QNode{});
}

// ---- Storage order (round 3).  The records the kernels fetch per primitive — sphere (centre, radius), material, emission, triangle
// vertices — are laid out in the order in which the tree's depth-first walk meets the leaves, not in the caller's order: the
// primitives a ray (and the rays of a wave) touch are then neighbours in memory, four sphere records to a 64-byte line, instead of
// scattered over megabytes.  Only the library's INTERNAL primitive numbers change (spheres stay below n_sph, triangles above): leaf
// references, leaf ranks, the `big` list and the world positions are renumbered with them, and every rule that looks at a
// primitive's place in `world` (distance ties) goes through world_rank, which from here on always exists.
inline void reorder_storage(const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt, std::vector<rt_sphere>& sp_store,
                            std::vector<rt_triangle>& tr_store, std::vector<rtbvh::Box>& boxes, std::vector<uint32_t>& wi_store,
                            rtbvh::FlatBVH& bvh) {
    const uint32_t np = ns + nt;
    std::vector<uint32_t> old_of(np), new_of(np);
    for (uint32_t i = 0; i < np; i++) old_of[i] = i;
    std::stable_sort(old_of.begin(), old_of.begin() + ns, [&](uint32_t x, uint32_t y) { return bvh.leaf_of[x] < bvh.leaf_of[y]; });
    std::stable_sort(old_of.begin() + ns, old_of.end(), [&](uint32_t x, uint32_t y) { return bvh.leaf_of[x] < bvh.leaf_of[y]; });
    for (uint32_t i = 0; i < np; i++) new_of[old_of[i]] = i;
    sp_store.resize(ns);
    tr_store.resize(nt);
    std::vector<rtbvh::Box> boxes2(np);
    std::vector<uint32_t> leaf2(np), wi2(np);
    for (uint32_t i = 0; i < np; i++) {
        const uint32_t o = old_of[i];
        if (i < ns) sp_store[i] = sp[o];
        else tr_store[i - ns] = tr[o - ns];
        boxes2[i] = boxes[o];
        leaf2[i] = bvh.leaf_of[o];
        wi2[i] = wi_store[o];
    }
    boxes.swap(boxes2);
    bvh.leaf_of.swap(leaf2);
    wi_store.swap(wi2);
    auto remap = [&](uint32_t& ref) {
        if (ref & rtbvh::LEAF_BIT) ref = rtbvh::LEAF_BIT | new_of[ref & ~rtbvh::LEAF_BIT];
    };
    for (rtbvh::TravNode& t : bvh.trav) { remap(t.left); remap(t.right); }
    for (rtbvh::QNode& q : bvh.travq) { remap(q.left); remap(q.right); }
    remap(bvh.root_ref);
}

// the device arrays of the primitive records, in storage order
inline void pack_records(const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt, const std::vector<rtbvh::Box>& boxes,
                         HostScene& hs) {
    rtplan::SceneShape& sh = hs.shape;
    const uint32_t np = ns + nt;
    sh.n_sph_pad = (ns + rtk::UNROLL - 1) / rtk::UNROLL * rtk::UNROLL;
    std::vector<F4>& geom = hs.geom;
    std::vector<F4>& mat = hs.mat;
    std::vector<float>& emis = hs.emis;
    std::vector<float>& tri = hs.tri;
    geom.assign(sh.n_sph_pad ? sh.n_sph_pad : 1, F4{0.f, 0.f, 0.f, 0.f});
    mat.assign(np ? np : 1, F4{0.f, 0.f, 0.f, 0.f});
    emis.assign(np ? np : 1, 0.f);
    tri.assign((size_t)nt * 9 + 1, 0.f);
    for (uint32_t i = 0; i < ns; i++) {
        // rr = radius.powi(2) (sphere.rs:45): one rounded multiply
        volatile float rr = sp[i].radius * sp[i].radius;
        geom[i] = F4{sp[i].cx, sp[i].cy, sp[i].cz, rr};
        mat[i] = F4{sp[i].albedo_r, sp[i].albedo_g, sp[i].albedo_b, sp[i].roughness};
        emis[i] = sp[i].emission;
    }
    // padding spheres can never pass either phase: rr = -inf makes every discriminant -inf
    for (uint32_t i = ns; i < sh.n_sph_pad; i++) geom[i] = F4{0.f, 0.f, 0.f, -INFINITY};
    // pair layout for the packed-FP32 broad phase: (c0x,c1x,c0y,c1y) (c0z,c1z,rr0,rr1)
    std::vector<F4>& geom_pk = hs.geom_pk;
    geom_pk.assign(geom.size(), F4{0.f, 0.f, 0.f, 0.f});
    for (uint32_t i = 0; i + 1 < sh.n_sph_pad; i += 2) {
        geom_pk[i] = F4{geom[i].x, geom[i + 1].x, geom[i].y, geom[i + 1].y};
        geom_pk[i + 1] = F4{geom[i].z, geom[i + 1].z, geom[i].w, geom[i + 1].w};
    }
    for (uint32_t i = 0; i < nt; i++) {
        std::memcpy(&tri[(size_t)i * 9], tr[i].a, 9 * sizeof(float));
        mat[ns + i] = F4{tr[i].albedo_r, tr[i].albedo_g, tr[i].albedo_b, tr[i].roughness};
        emis[ns + i] = tr[i].emission;
    }
    hs.tri_box.assign((size_t)nt * 2 + 1, F4{0.f, 0.f, 0.f, 0.f});
    for (uint32_t i = 0; i < nt; i++) {
        const rtbvh::Box& b = boxes[ns + i];
        hs.tri_box[2 * (size_t)i] = F4{b.lo[0], b.lo[1], b.lo[2], 0.f};
        hs.tri_box[2 * (size_t)i + 1] = F4{b.hi[0], b.hi[1], b.hi[2], 0.f};
    }
    hs.geom_r.assign(ns ? ns : 1, F4{0.f, 0.f, 0.f, 0.f});
    for (uint32_t i = 0; i < ns; i++) {
        hs.geom_r[i] = F4{sp[i].cx, sp[i].cy, sp[i].cz, sp[i].radius};
        if (sp[i].radius < 0.0f) sh.inverted_boxes = true;
    }
}

// expanded-form broad phase records: w = |c|^2 - rr - 2^-16 (|c|^2 + rr), evaluated in
// double and rounded DOWN to f32 (conservative).
inline void expanded_records(const rt_sphere* sp, uint32_t ns, HostScene& hs) {
    rtplan::SceneShape& sh = hs.shape;
    const std::vector<F4>& geom = hs.geom;
    std::vector<F4>& geom_px = hs.geom_px;
    geom_px.assign(geom.size(), F4{0.f, 0.f, 0.f, 0.f});
    std::vector<F4> px(geom.size());
    std::vector<double> ratio;
    const double K = std::ldexp(1.0, -16);
    for (uint32_t i = 0; i < sh.n_sph_pad; i++) {
        if (i >= ns) {
            px[i] = F4{0.f, 0.f, 0.f, INFINITY};      // w = +inf: t = -inf, never a candidate
            continue;
        }
        const double cc = (double)sp[i].cx * sp[i].cx + (double)sp[i].cy * sp[i].cy + (double)sp[i].cz * sp[i].cz;
        const double rr = (double)geom[i].w;
        const double w = cc - rr - K * (cc + rr);
        float wf = (float)w;
        if ((double)wf > w) wf = std::nextafterf(wf, -INFINITY);
        px[i] = F4{sp[i].cx, sp[i].cy, sp[i].cz, wf};
        if (rr > 0) ratio.push_back(K * 2.0 * cc / rr);
    }
    for (uint32_t i = 0; i + 1 < sh.n_sph_pad; i += 2) {
        geom_px[i] = F4{px[i].x, px[i + 1].x, px[i].y, px[i + 1].y};
        geom_px[i + 1] = F4{px[i].z, px[i + 1].z, px[i].w, px[i + 1].w};
    }
    // heuristic: the expanded form's additive margin 2^-16 (|o|^2 + |c|^2 + rr) must stay small against rr
    // for the typical sphere, otherwise candidate lists blow up (c5-class scenes): then use the oc form.
    bool ok = !ratio.empty();
    if (ok) {
        std::nth_element(ratio.begin(), ratio.begin() + ratio.size() / 2, ratio.end());
        ok = ratio[ratio.size() / 2] < 0.5;
    }
    for (uint32_t i = 0; i < ns && ok; i++)
        ok = std::isfinite(px[i].x) && std::isfinite(px[i].y) && std::isfinite(px[i].z) && std::isfinite(px[i].w);
    sh.expanded = ok;
}

// worthwhile only if the grid step is small against the primitives (else the rounded boxes admit crowds of
// false leaves): median primitive box edge >= 8 steps on every axis
inline bool quant_rule(const std::vector<rtbvh::Box>& boxes, const rtbvh::QGrid& grid) {
    const uint32_t np = (uint32_t)boxes.size();
    bool ok = grid.ok && np > 1;
    if (ok) {
        std::vector<float> edge(np);
        for (uint32_t i = 0; i < np; i++) {
            float e = INFINITY;
            for (int a3 = 0; a3 < 3; a3++)
                e = fminf(e, (boxes[i].hi[a3] - boxes[i].lo[a3]) / grid.step[a3]);
            edge[i] = e;
        }
        std::nth_element(edge.begin(), edge.begin() + np / 2, edge.end());
        ok = edge[np / 2] >= 8.0f;
    }
    return ok;
}

// leaf density = sum of primitive box areas / area of the scene box ~ leaves a random ray reaches; above ~2
// the walk is bound by the exact leaf tests, where the lighter exact-node kernel (5 waves/SIMD) wins
inline float leaf_density(const std::vector<rtbvh::Box>& boxes) {
    const uint32_t np = (uint32_t)boxes.size();
    double area = 0.0, root = 0.0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = 0; i < np; i++) {
        const double ex = (double)boxes[i].hi[0] - boxes[i].lo[0], ey = (double)boxes[i].hi[1] - boxes[i].lo[1],
                     ez = (double)boxes[i].hi[2] - boxes[i].lo[2];
        area += ex * ey + ey * ez + ez * ex;
        for (int a3 = 0; a3 < 3; a3++) {
            lo[a3] = fminf(lo[a3], boxes[i].lo[a3]);
            hi[a3] = fmaxf(hi[a3], boxes[i].hi[a3]);
        }
    }
    if (np) {
        const double ex = (double)hi[0] - lo[0], ey = (double)hi[1] - lo[1], ez = (double)hi[2] - lo[2];
        root = ex * ey + ey * ez + ez * ex;
    }
    return root > 0.0 ? (float)(area / root) : INFINITY;
}

// culled walk: its distance bound carries sqrt(2) * (largest radius) of slack, so the few spheres far larger than the
// rest (a ground sphere) are listed apart and root-tested at every query start instead
// (area, lo, hi: the box areas and the common box of the spheres outside `big`, which the triangle rule goes on from)
inline void sphere_cull_rule(const rt_sphere* sp, uint32_t ns, uint32_t nt, HostScene& hs, double& area, float lo[3], float hi[3]) {
    rtplan::SceneShape& sh = hs.shape;
    std::vector<float> rad(ns);
    for (uint32_t i = 0; i < ns; i++) rad[i] = fabsf(sp[i].radius);
    float med = 0.f;
    if (ns) {
        std::vector<float> tmp(rad);
        std::nth_element(tmp.begin(), tmp.begin() + ns / 2, tmp.end());
        med = tmp[ns / 2];
    }
    std::vector<uint32_t> cand;
    for (uint32_t i = 0; i < ns; i++)
        if (rad[i] > 8.0f * med) cand.push_back(i);
    std::sort(cand.begin(), cand.end(), [&](uint32_t a, uint32_t b) { return rad[a] > rad[b] || (rad[a] == rad[b] && a < b); });
    if (cand.size() > 16) cand.resize(16);
    std::vector<char> is_big(ns ? ns : 1, 0);
    for (uint32_t i : cand) is_big[i] = 1;
    float rs = 0.f;
    for (uint32_t i = 0; i < ns; i++)
        if (!is_big[i] && rad[i] > rs) rs = rad[i];
    hs.big = cand;
    hs.n_big = (uint32_t)cand.size();
    sh.r_slack = rs;
    if (hs.big.empty()) hs.big.push_back(0);
    // Does it pay?  The ratio below is the expected number of (non-big) primitive boxes a random line through their
    // common box meets (Cauchy: box areas add up).  tools/cull_matrix.py, 2560x1440: sparse fields at 0.06...0.35 lose
    // 5...7 % to the ordering and the early root tests, c5 at 0.95 gains 12 %, fields / mixed radii / dense overlap at
    // 2...30 gain 1.35...3.5 x.  And the bound's slack (1.5 r_slack) must be small against the scene.
    for (uint32_t i = 0; i < ns; i++) {
        if (is_big[i]) continue;
        const double e = 2.0 * rad[i];
        area += 3.0 * e * e;
        const float c[3] = {sp[i].cx, sp[i].cy, sp[i].cz};
        for (int a3 = 0; a3 < 3; a3++) {
            lo[a3] = fminf(lo[a3], c[a3] - rad[i]);
            hi[a3] = fmaxf(hi[a3], c[a3] + rad[i]);
        }
    }
    const double ex = (double)hi[0] - lo[0], ey = (double)hi[1] - lo[1], ez = (double)hi[2] - lo[2];
    const double root = ex * ey + ey * ez + ez * ex, diag = std::sqrt(ex * ex + ey * ey + ez * ez);
    sh.cull_density = root > 0.0 ? (float)(area / root) : 0.f;
    sh.cull_pays = nt == 0 && root > 0.0 && std::isfinite(area / root) && area / root >= 0.7 && (double)rs <= 0.05 * diag;
}

// The maxima cull_bound_tri (rt_cull.h) takes, of one triangle: K = |e1||e2|, the box diagonal, |e1| + |e2| and the longest edge,
// in double, times 1.0001, rounded to f32.
struct TriMeasures {
    float kk, dg, es, em;
};
inline TriMeasures tri_measures(const rt_triangle& t, const rtbvh::Box& box) {
    double e1 = 0, e2 = 0, e3 = 0, d2 = 0;
    for (int a3 = 0; a3 < 3; a3++) {
        const double ab = (double)t.b[a3] - t.a[a3], ac = (double)t.c[a3] - t.a[a3], bc = (double)t.c[a3] - t.b[a3];
        e1 += ab * ab; e2 += ac * ac; e3 += bc * bc;
        const double ext = (double)box.hi[a3] - box.lo[a3];
        d2 += ext * ext;
    }
    e1 = std::sqrt(e1); e2 = std::sqrt(e2); e3 = std::sqrt(e3);
    TriMeasures m;
    m.dg = (float)(std::sqrt(d2) * 1.0001);
    m.kk = (float)(e1 * e2 * 1.0001);
    m.es = (float)((e1 + e2) * 1.0001);
    m.em = (float)(std::max(e1, std::max(e2, e3)) * 1.0001);
    return m;
}

// (What the bounds claim — no accepted root of a primitive outside the `big` list enters its box beyond cull_bound /
// cull_bound_tri of its compared distance — is tested by itself, on 1.8e7 seeded and adversarial (ray, primitive, box)
// triples incl. K -> 0.25, |det| -> 1e-5, origins at 1e3 and tangent rays: tests/test_cull_lemma.py with the bounds
// of csrc/rt_cull.h; reduced soaks against the oracle: tests/test_gpu_cull_soaks.py.)
// Scenes with triangles (culled walk over the EXACT nodes, cull_bound_tri in rt_cull.h): its bound needs every
// triangle outside the `big` list to have K = |e1||e2| <= 0.25 (with the reference's |det| >= 1e-5 that keeps the
// computed determinant within 1.5 % of the true one) and carries the largest box diagonal as slack, so triangles with
// a larger K, or a box diagonal of more than 8 x the median, join the list (16 entries with the spheres; more: no culling).
inline void triangle_cull_rule(const rt_triangle* tr, uint32_t ns, uint32_t nt, const std::vector<rtbvh::Box>& boxes, HostScene& hs,
                               double area, float lo[3], float hi[3]) {
    rtplan::SceneShape& sh = hs.shape;
    const float rs = sh.r_slack;
    std::vector<float> dg(nt), kk(nt), es(nt), em(nt);
    for (uint32_t i = 0; i < nt; i++) {
        const TriMeasures m = tri_measures(tr[i], boxes[ns + i]);
        dg[i] = m.dg;
        kk[i] = m.kk;
        es[i] = m.es;
        em[i] = m.em;
    }
    std::vector<float> tmp(dg);
    std::nth_element(tmp.begin(), tmp.begin() + nt / 2, tmp.end());
    const float med_d = tmp[nt / 2];
    std::vector<uint32_t> bigt;
    bool ok = true;
    for (uint32_t i = 0; i < nt && ok; i++) {
        const bool fin = std::isfinite(dg[i]) && std::isfinite(kk[i]);
        if (!fin) ok = false;
        else if (kk[i] > 0.25f || dg[i] > 8.0f * med_d) bigt.push_back(ns + i);
        if (bigt.size() + hs.n_big > 16) ok = false;
    }
    if (ok) {
        std::vector<char> isb(nt, 0);
        for (uint32_t q : bigt) isb[q - ns] = 1;
        double tarea = 0.0;
        for (uint32_t i = 0; i < nt; i++) {
            if (isb[i]) continue;
            hs.tri_k = fmaxf(hs.tri_k, kk[i]);
            hs.tri_diag = fmaxf(hs.tri_diag, dg[i]);
            hs.tri_es = fmaxf(hs.tri_es, es[i]);
            hs.tri_e = fmaxf(hs.tri_e, em[i]);
            const rtbvh::Box& b = boxes[ns + i];
            const double ex2 = (double)b.hi[0] - b.lo[0], ey2 = (double)b.hi[1] - b.lo[1], ez2 = (double)b.hi[2] - b.lo[2];
            tarea += ex2 * ey2 + ey2 * ez2 + ez2 * ex2;
            for (int a3 = 0; a3 < 3; a3++) {
                lo[a3] = fminf(lo[a3], b.lo[a3]);
                hi[a3] = fmaxf(hi[a3], b.hi[a3]);
            }
        }
        const double fx = (double)hi[0] - lo[0], fy = (double)hi[1] - lo[1], fz = (double)hi[2] - lo[2];
        const double root2 = fx * fy + fy * fz + fz * fx, diag2 = std::sqrt(fx * fx + fy * fy + fz * fz);
        const double dens = root2 > 0.0 ? (area + tarea) / root2 : 0.0;
        if (hs.n_big) hs.big.resize(hs.n_big); else hs.big.clear();
        for (uint32_t q : bigt) hs.big.push_back(q);
        hs.n_big = (uint32_t)hs.big.size();
        if (hs.big.empty()) hs.big.push_back(0);
        sh.cull_density = (float)dens;
        sh.xcull_pays = std::isfinite(dens) && dens >= 0.7 && (double)rs <= 0.05 * diag2 && (double)hs.tri_diag <= 0.05 * diag2;
    }
    sh.tri_ok = ok;
}

// The emitter list of direct lighting (rt_scene_direct*, rt_tile.h): the library's numbers of the primitives with emission > 0 (a NaN
// emits nothing, as `em > 0` in ray_color), in ascending world position — the order of the caller's world, whatever the storage
// order — so that pick k names the same light for every storage order.  Reads hs.emis and hs.world_rank (pack_records and
// build_host_scene before it); no launch but rt_direct_kernel reads the list.
inline void emitter_list(HostScene& hs) {
    const uint32_t np = hs.shape.n_sph + hs.shape.n_tri;
    std::vector<uint32_t>& lights = hs.lights;
    lights.clear();
    for (uint32_t i = 0; i < np; i++)
        if (hs.emis[i] > 0.0f) lights.push_back(i);
    if (hs.has_order)
        std::sort(lights.begin(), lights.end(), [&](uint32_t x, uint32_t y) { return hs.world_rank[x] < hs.world_rank[y]; });
    hs.n_lights = (uint32_t)lights.size();
    if (lights.empty()) lights.push_back(0);
}

// The light table of RT_FLAG_LIGHTS_BY_POWER (rt_tile.h "light selection by power"): per emitter of the list, in its order, the power
// q = luminance * area (rt_direct_math.h; 0 unless positive), the running f32 sum c, and from the width each emitter has IN that sum
// the mixture probability p = 0.5 / M + 0.5 w / total with its inverse ip.  One IEEE f32 rounding per operation, as the header writes
// them.  Reads hs.lights, hs.geom_r, hs.tri, hs.mat and hs.emis (emitter_list and pack_records before it); no launch without the flag
// reads the table.
inline void light_table(HostScene& hs) {
    const uint32_t ns = hs.shape.n_sph, np = ns + hs.shape.n_tri, M = hs.n_lights;
    hs.light_c.assign(M ? M : 1, 0.f);
    hs.light_p.assign(M ? M : 1, 0.f);
    hs.light_ip.assign(M ? M : 1, 0.f);
    hs.light_ip_prim.assign(np ? np : 1, 0.f);
    float run = 0.f;
    for (uint32_t k = 0; k < M; k++) {
        const uint32_t prim = hs.lights[k];
        const float lum = rtdl::light_luminance(rtdl::Vec{hs.mat[prim].x, hs.mat[prim].y, hs.mat[prim].z}, hs.emis[prim]);
        float area;
        if (prim < ns) {
            area = rtdl::sphere_light_area(hs.geom_r[prim].w);
        } else {
            const float* tv = &hs.tri[(size_t)(prim - ns) * 9];
            const float A = rtdl::triangle_area(rtdl::Vec{tv[0], tv[1], tv[2]}, rtdl::Vec{tv[3], tv[4], tv[5]}, rtdl::Vec{tv[6], tv[7], tv[8]});
            area = A + A;                                    // a triangle emits from both sides
        }
        run = run + rtdl::light_power(lum, area);
        hs.light_c[k] = run;
    }
    hs.light_total = run;
    hs.light_degenerate = rtdl::table_degenerate(run);
    for (uint32_t k = 0; k < M; k++) {
        if (hs.light_degenerate) {
            hs.light_p[k] = 1.0f / (float)M;
            hs.light_ip[k] = (float)M;
        } else {
            const float w = hs.light_c[k] - (k ? hs.light_c[k - 1] : 0.0f);
            hs.light_p[k] = rtdl::mixture_probability(w, run, M);
            hs.light_ip[k] = 1.0f / hs.light_p[k];
        }
        hs.light_ip_prim[hs.lights[k]] = hs.light_ip[k];
    }
}

// reorder: false keeps the primitive records in the caller's order (A/B)
inline void build_host_scene(const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt, const uint32_t* world_index,
                             bool reorder, HostScene& hs) {
    rtplan::SceneShape& sh = hs.shape;
    sh.n_sph = ns;
    sh.n_tri = nt;
    hs.has_order = world_index != nullptr && ns + nt > 0;
    const uint32_t np = ns + nt;
    std::vector<rtbvh::Box> boxes = prim_boxes(sp, ns, tr, nt);
    build_tree(boxes, world_index, hs);
    rtbvh::FlatBVH& bvh = hs.bvh;
    std::vector<rt_sphere> sp_store;
    std::vector<rt_triangle> tr_store;
    std::vector<uint32_t> wi_store(np ? np : 1, 0u);
    for (uint32_t i = 0; i < np; i++) wi_store[i] = world_index ? world_index[i] : i;
    if (np >= REORDER_MIN_PRIMS && reorder) {
        reorder_storage(sp, ns, tr, nt, sp_store, tr_store, boxes, wi_store, bvh);
        sp = sp_store.data();
        tr = tr_store.data();
        hs.has_order = true;                 // (ties of the plain linear-scan semantics: by place in `world`, no longer by number)
    }
    sh.bvh_depth = bvh.depth;
    sh.root_ref = bvh.root_ref;
    if (hs.has_order) hs.world_rank.assign(wi_store.begin(), wi_store.begin() + np);
    else hs.world_rank.assign(1, 0u);
    pack_records(sp, ns, tr, nt, boxes, hs);
    emitter_list(hs);
    light_table(hs);
    expanded_records(sp, ns, hs);
    sh.quant_ok = quant_rule(boxes, bvh.grid);
    sh.leaf_density = leaf_density(boxes);
    double area = 0.0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    sphere_cull_rule(sp, ns, nt, hs, area, lo, hi);
    if (nt > 0) triangle_cull_rule(tr, ns, nt, boxes, hs, area, lo, hi);
}

}  // namespace rtscene
