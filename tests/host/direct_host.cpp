// CPU harness of direct lighting (tests/test_direct_host.py): the product's sampling arithmetic (csrc/rt_direct_math.h) on records of
// inputs, the emitter list of the host's scene derivation (csrc/rt_scene_host.h emitter_list) and the plan (csrc/rt_plan.h
// plan_direct), built by g++ -ffp-contract=off as a shared library.  With -DDIRECT_HOST_MAIN it is a stand-alone program that runs the
// emitter list and the plan over a few scenes (for a sanitizer build: -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_direct_math.h"
#include "rt_scene_host.h"

using rtdl::Vec;

namespace {
constexpr int IN_WORDS = 28, OUT_WORDS = 16;

float f_of(uint32_t w) {
    float f;
    std::memcpy(&f, &w, 4);
    return f;
}
uint32_t w_of(float f) {
    uint32_t w;
    std::memcpy(&w, &f, 4);
    return w;
}
Vec vec_at(const uint32_t* r, int i) { return Vec{f_of(r[i]), f_of(r[i + 1]), f_of(r[i + 2])}; }
}  // namespace

extern "C" {

// Record i, IN_WORDS 32-bit words: [0] kind (0 sphere, 1 triangle), [1] M, [2] u, [3..5] P, [6..8] n; sphere: [9..11] c, [12] r,
// [13..15] us; triangle: [9..11] a, [12..14] b, [15..17] c, [18] u1, [19] u2, [20..22] nl; [23..25] albedo, [26] emission.
// Out, OUT_WORDS words: [0] k, [1..3] L, [4] d2, [5] cs, [6] cl, [7] facing, [8] W, [9..11] rgb, [12..14] w, [15] area (triangle).
__attribute__((visibility("default"))) void direct_math(uint32_t n, const uint32_t* in, uint32_t* out) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* r = in + (size_t)i * IN_WORDS;
        uint32_t* o = out + (size_t)i * OUT_WORDS;
        const bool sphere = r[0] == 0;
        const uint32_t M = r[1];
        o[0] = rtdl::pick_light(f_of(r[2]), M);
        const Vec P = vec_at(r, 3), nrm = vec_at(r, 6);
        Vec L, nl;
        float size, area = 0.0f;
        if (sphere) {
            nl = vec_at(r, 13);
            size = f_of(r[12]);
            L = rtdl::sphere_point(vec_at(r, 9), size, nl);
        } else {
            float u1 = f_of(r[18]), u2 = f_of(r[19]);
            rtdl::fold_pair(u1, u2);
            const Vec a = vec_at(r, 9), b = vec_at(r, 12), c = vec_at(r, 15);
            L = rtdl::triangle_point(a, b, c, u1, u2);
            nl = vec_at(r, 20);
            size = area = rtdl::triangle_area(a, b, c);
        }
        const rtdl::Geometry g = rtdl::light_geometry(P, nrm, L, nl, sphere);
        const float W = sphere ? rtdl::sphere_weight(g.cs, g.cl, size, M, g.d2) : rtdl::triangle_weight(g.cs, g.cl, size, M, g.d2);
        const Vec rgb = rtdl::radiance(vec_at(r, 23), f_of(r[26]), W);
        o[1] = w_of(L.x), o[2] = w_of(L.y), o[3] = w_of(L.z);
        o[4] = w_of(g.d2), o[5] = w_of(g.cs), o[6] = w_of(g.cl), o[7] = g.facing ? 1u : 0u, o[8] = w_of(W);
        o[9] = w_of(rgb.x), o[10] = w_of(rgb.y), o[11] = w_of(rgb.z);
        o[12] = w_of(g.w.x), o[13] = w_of(g.w.y), o[14] = w_of(g.w.z);
        o[15] = w_of(area);
    }
}

// The emitter list of build_host_scene for a world: per emitter, in list order, its world position (out_pos), whether it is a sphere
// (out_sphere) and its emission as bits (out_emis); returns M (cap: the capacity of the out arrays; M > cap writes only cap entries).
__attribute__((visibility("default"))) uint32_t direct_emitters(const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt,
                                                                const uint32_t* world_index, int reorder, uint32_t cap,
                                                                uint32_t* out_pos, uint32_t* out_sphere, uint32_t* out_emis) {
    rtscene::HostScene hs;
    rtscene::build_host_scene(sp, ns, tr, nt, world_index, reorder != 0, hs);
    for (uint32_t k = 0; k < hs.n_lights && k < cap; k++) {
        const uint32_t prim = hs.lights[k];
        out_pos[k] = hs.has_order ? hs.world_rank[prim] : prim;
        out_sphere[k] = prim < ns ? 1u : 0u;
        out_emis[k] = w_of(hs.emis[prim]);
    }
    return hs.lights.size() >= 1 ? hs.n_lights : 0xffffffffu;      // (the uploaded array is never empty)
}

// plan_direct for a shape (n_sph, n_tri, bvh_depth, inverted_boxes): out = (engine, scan_mode, full_chain, lds, too_many)
__attribute__((visibility("default"))) void direct_plan(const uint32_t* shape, uint32_t n_lights, uint32_t flags, uint64_t* out) {
    rtplan::SceneShape sh;
    sh.n_sph = shape[0];
    sh.n_tri = shape[1];
    sh.bvh_depth = shape[2];
    sh.inverted_boxes = shape[3] != 0;
    const rtplan::DirectPlan d = rtplan::plan_direct(sh, n_lights, flags);
    out[0] = (uint64_t)d.query.engine;
    out[1] = (uint64_t)d.query.scan_mode;
    out[2] = d.query.full_chain ? 1 : 0;
    out[3] = d.query.lds;
    out[4] = d.too_many ? 1 : 0;
}

__attribute__((visibility("default"))) uint32_t direct_max_lights() { return rtplan::DIRECT_MAX_LIGHTS; }
__attribute__((visibility("default"))) uint32_t direct_math_max_lights() { return rtdl::MAX_LIGHTS; }

}  // extern "C"

#ifdef DIRECT_HOST_MAIN
// The host side of the feature under a sanitizer: the emitter list over worlds with and without a world_index, below and above the
// storage-reorder threshold, with no emitter and with only emitters, an empty world; the plan over its flags.
int main() {
    int bad = 0;
    for (uint32_t np : {0u, 1u, 5u, 63u, 64u, 200u, 3000u}) {
        for (int mode = 0; mode < 3; mode++) {              // emitters: none, every third primitive, all
            const uint32_t ns = np - np / 3, nt = np / 3;
            std::vector<rt_sphere> sp(ns);
            std::vector<rt_triangle> tr(nt);
            uint32_t want = 0;
            for (uint32_t i = 0; i < np; i++) {
                const float x = (float)((i * 37u) % 101u) - 50.0f, y = (float)((i * 11u) % 17u), z = -5.0f - (float)((i * 7u) % 29u);
                const float em = mode == 2 || (mode == 1 && i % 3 == 0) ? 2.0f : 0.0f;
                want += em > 0.0f;
                if (i < ns) {
                    sp[i] = rt_sphere{x, y, z, 0.4f, 0.5f, 0.5f, 0.5f, 0.0f, em};
                } else {
                    rt_triangle t{};
                    const float a[3] = {x, y, z}, b[3] = {x + 0.5f, y, z}, c[3] = {x, y + 0.5f, z + 0.1f};
                    std::memcpy(t.a, a, 12), std::memcpy(t.b, b, 12), std::memcpy(t.c, c, 12);
                    t.albedo_r = t.albedo_g = t.albedo_b = 0.5f;
                    t.emission = em;
                    tr[i - ns] = t;
                }
            }
            std::vector<uint32_t> wi(np);
            for (uint32_t i = 0; i < np; i++) wi[i] = np - 1 - i;        // the world reversed
            for (int ordered = 0; ordered < 2; ordered++) {
                std::vector<uint32_t> pos(np + 1), sph(np + 1), emis(np + 1);
                const uint32_t m = direct_emitters(sp.data(), ns, tr.data(), nt, ordered ? wi.data() : nullptr, 1, np + 1, pos.data(),
                                                   sph.data(), emis.data());
                if (m != want) bad++;
                for (uint32_t k = 1; k < m && k < np + 1; k++) bad += !(pos[k - 1] < pos[k]);
                for (uint32_t k = 0; k < m && k < np + 1; k++) bad += !(f_of(emis[k]) > 0.0f);
                uint64_t out[5];
                const uint32_t shape[4] = {ns, nt, 12, 0};
                for (uint32_t flags : {0u, (uint32_t)RT_FLAG_NO_BVH_CULL, (uint32_t)RT_FLAG_EXACT_SCAN, (uint32_t)RT_FLAG_FULL_CHAIN}) {
                    direct_plan(shape, m, flags, out);
                    bad += out[4] != 0;
                }
            }
        }
    }
    uint64_t out[5];
    const uint32_t shape[4] = {10, 0, 3, 0};
    direct_plan(shape, rtplan::DIRECT_MAX_LIGHTS + 1u, 0, out);
    bad += out[4] != 1;
    std::printf(bad ? "DIRECT_HOST_FAILED %d\n" : "DIRECT_HOST_OK\n", bad);
    return bad ? 1 : 0;
}
#endif
