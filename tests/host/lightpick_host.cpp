// CPU harness of light selection by power (tests/test_lightpick_host.py): the light table of the host's scene derivation
// (csrc/rt_scene_host.h light_table), the pick and the weights with ip (csrc/rt_direct_math.h, csrc/rt_nee_math.h) and the plans
// (csrc/rt_plan.h plan_direct, plan_nee), built by g++ -ffp-contract=off as a shared library.  With -DLIGHTPICK_HOST_MAIN it is a
// stand-alone program that runs the table, the pick and the plans over a few scenes (for a sanitizer build:
// -fsanitize=address,undefined).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_direct_math.h"
#include "rt_nee_math.h"
#include "rt_scene_host.h"

namespace {
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
}  // namespace

extern "C" {

// The light table of build_host_scene for a world: per emitter, in list order, its world position, c, p and ip (f32 as bits; ip as the
// kernels read it, by primitive number); out_total[0] = total as bits, out_total[1] = degenerate.  Returns M, or 0xffffffff when the
// per-primitive ip is not the per-emitter one or a primitive that does not emit has one (cap: the capacity of the out arrays).
__attribute__((visibility("default"))) uint32_t lightpick_table(const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt,
                                                                const uint32_t* world_index, int reorder, uint32_t cap, uint32_t* out_pos,
                                                                uint32_t* out_c, uint32_t* out_p, uint32_t* out_ip, uint32_t* out_total) {
    rtscene::HostScene hs;
    rtscene::build_host_scene(sp, ns, tr, nt, world_index, reorder != 0, hs);
    const uint32_t M = hs.n_lights;
    if (hs.light_c.size() != (M ? M : 1) || hs.light_ip_prim.size() != (ns + nt ? ns + nt : 1)) return 0xffffffffu;
    uint32_t with_ip = 0;
    for (uint32_t i = 0; i < ns + nt; i++) with_ip += hs.light_ip_prim[i] != 0.0f;
    if (with_ip != M) return 0xffffffffu;
    for (uint32_t k = 0; k < M && k < cap; k++) {
        const uint32_t prim = hs.lights[k];
        if (w_of(hs.light_ip_prim[prim]) != w_of(hs.light_ip[k])) return 0xffffffffu;
        out_pos[k] = hs.has_order ? hs.world_rank[prim] : prim;
        out_c[k] = w_of(hs.light_c[k]);
        out_p[k] = w_of(hs.light_p[k]);
        out_ip[k] = w_of(hs.light_ip_prim[prim]);
    }
    out_total[0] = w_of(hs.light_total);
    out_total[1] = hs.light_degenerate ? 1u : 0u;
    return M;
}

// pick_light_power of n draws u (f32 as bits) over the running sums c[0 .. M - 1]
__attribute__((visibility("default"))) void lightpick_pick(uint32_t n, const uint32_t* u, uint32_t M, const float* c, uint32_t total,
                                                           uint32_t* out_k) {
    for (uint32_t i = 0; i < n; i++) out_k[i] = rtdl::pick_light_power(f_of(u[i]), M, c, f_of(total));
}

// ... and of every u01 there is, j / 2^24 for j = 0 .. 2^24 - 1: counts[k] = the draws that pick emitter k.  Returns the draws whose
// pick was not below M.
__attribute__((visibility("default"))) uint32_t lightpick_counts(uint32_t M, const float* c, uint32_t total, uint64_t* counts) {
    uint32_t bad = 0;
    const float t = f_of(total);
    for (uint32_t j = 0; j < (1u << 24); j++) {
        const uint32_t k = rtdl::pick_light_power((float)j * 0x1p-24f, M, c, t);
        if (k < M) counts[k]++;
        else bad++;
    }
    return bad;
}

// Record i, 20 words (the PICK_POWER records of csrc/rt_unit_sampling.hip.h): [0] u, [1] M (1 .. 16), [2] total, [3] M_big
// (1 .. 2^23), [4..19] the running sums c.  Out, 2 words: pick_light_power(u, M, c, total) and pick_light(u, M_big); an M or M_big
// outside its range writes 0, 0.
__attribute__((visibility("default"))) void lightpick_pick_records(uint32_t n, const uint32_t* in, uint32_t* out) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* r = in + (size_t)i * 20;
        const uint32_t M = r[1], M_big = r[3];
        out[2 * i] = out[2 * i + 1] = 0;
        if (M < 1u || M > 16u || M_big < 1u || M_big > rtdl::MAX_LIGHTS) continue;
        float c[16];
        std::memcpy(c, r + 4, sizeof c);
        out[2 * i] = rtdl::pick_light_power(f_of(r[0]), M, c, f_of(r[2]));
        out[2 * i + 1] = rtdl::pick_light(f_of(r[0]), M_big);
    }
}

// Record i, 6 words: [0] kind (0 sphere, 1 triangle), [1] cs, [2] cl, [3] size, [4] ip, [5] d2.  Out, 2 words: W of
// sphere_weight_ip / triangle_weight_ip, and W' of rtnee::view_weight_ip for the view (cs, cl, d2).
__attribute__((visibility("default"))) void lightpick_weights(uint32_t n, const uint32_t* in, uint32_t* out) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* r = in + (size_t)i * 6;
        const bool sphere = r[0] == 0;
        const float cs = f_of(r[1]), cl = f_of(r[2]), size = f_of(r[3]), ip = f_of(r[4]), d2 = f_of(r[5]);
        out[2 * i] = w_of(sphere ? rtdl::sphere_weight_ip(cs, cl, size, ip, d2) : rtdl::triangle_weight_ip(cs, cl, size, ip, d2));
        rtnee::View v;
        v.cs = cs, v.cl = cl, v.d2 = d2, v.samplable = true;
        out[2 * i + 1] = w_of(rtnee::view_weight_ip(v, sphere, size, ip));
    }
}

// plan_direct and plan_nee for a shape (n_sph, n_tri, bvh_depth, inverted_boxes): out[0..4] / out[5..9] = (engine, scan_mode,
// full_chain, lds, too_many)
__attribute__((visibility("default"))) void lightpick_plans(const uint32_t* shape, uint32_t n_lights, uint32_t flags, uint64_t* out) {
    rtplan::SceneShape sh;
    sh.n_sph = shape[0];
    sh.n_tri = shape[1];
    sh.bvh_depth = shape[2];
    sh.inverted_boxes = shape[3] != 0;
    const rtplan::DirectPlan plans[2] = {rtplan::plan_direct(sh, n_lights, flags), rtplan::plan_nee(sh, n_lights, flags)};
    for (int i = 0; i < 2; i++) {
        out[5 * i + 0] = (uint64_t)plans[i].query.engine;
        out[5 * i + 1] = (uint64_t)plans[i].query.scan_mode;
        out[5 * i + 2] = plans[i].query.full_chain ? 1 : 0;
        out[5 * i + 3] = plans[i].query.lds;
        out[5 * i + 4] = plans[i].too_many ? 1 : 0;
    }
}

}  // extern "C"

#ifdef LIGHTPICK_HOST_MAIN
// The host side of the feature under a sanitizer: the table over worlds of every size class (none, one, a few, above the
// storage-reorder threshold, a thousand emitters), ordinary and degenerate, with and without a world_index; on each table the pick at
// its ends and on a sweep of draws, every index it reads within the table; the plans over their flags.
int main() {
    int bad = 0;
    for (uint32_t np : {0u, 1u, 2u, 7u, 63u, 64u, 200u, 1500u}) {
        for (int mode = 0; mode < 4; mode++) {               // powers: spread over decades, all zero, overflowing, one infinite
            const uint32_t ns = np - np / 3, nt = np / 3;
            std::vector<rt_sphere> sp(ns);
            std::vector<rt_triangle> tr(nt);
            for (uint32_t i = 0; i < np; i++) {
                const float x = (float)((i * 37u) % 101u) - 50.0f, y = (float)((i * 11u) % 17u), z = -5.0f - (float)((i * 7u) % 29u);
                float em = i % 3 == 2 ? 0.0f : std::pow(10.0f, (float)(i % 13u) - 6.0f), alb = 0.5f;
                if (mode == 1) alb = 0.0f;
                if (mode == 2) em = em > 0.0f ? 3e37f : 0.0f;
                if (mode == 3 && i == 0) em = INFINITY;
                if (i < ns) {
                    sp[i] = rt_sphere{x, y, z, i % 5 == 4 ? 0.0f : 0.4f, alb, alb, alb, 0.0f, em};
                } else {
                    rt_triangle t{};
                    const float a[3] = {x, y, z}, b[3] = {x + 0.5f, y, z}, c[3] = {x, y + 0.5f, z + 0.1f};
                    std::memcpy(t.a, a, 12), std::memcpy(t.b, b, 12), std::memcpy(t.c, i % 7 == 0 ? a : c, 12);
                    t.albedo_r = t.albedo_g = t.albedo_b = alb;
                    t.emission = em;
                    tr[i - ns] = t;
                }
            }
            std::vector<uint32_t> wi(np);
            for (uint32_t i = 0; i < np; i++) wi[i] = np - 1 - i;        // the world reversed
            for (int ordered = 0; ordered < 2; ordered++) {
                std::vector<uint32_t> pos(np + 1), c(np + 1), p(np + 1), ip(np + 1);
                uint32_t tot[2] = {0, 0};
                const uint32_t M = lightpick_table(sp.data(), ns, tr.data(), nt, ordered ? wi.data() : nullptr, 1, np + 1, pos.data(),
                                                   c.data(), p.data(), ip.data(), tot);
                if (M > np) { bad++; continue; }
                if (mode == 1 && M && !tot[1]) bad++;
                double sum = 0.0;
                for (uint32_t k = 0; k < M; k++) {
                    sum += (double)f_of(p[k]);
                    bad += !(f_of(p[k]) >= 0.5f / (float)M * 0.999f) || !(f_of(ip[k]) > 0.0f);
                    if (k) bad += !(f_of(c[k]) >= f_of(c[k - 1])) && !tot[1];
                }
                if (M) bad += !(std::fabs(sum - 1.0) < 1e-3);
                if (M == 0) continue;
                // exactly M running sums on the heap: a read beyond them is the sanitizer's to find
                std::vector<float> cs(M);
                for (uint32_t k = 0; k < M; k++) cs[k] = f_of(c[k]);
                std::vector<uint32_t> us, ks;
                for (float u : {0.0f, 0.5f - 0x1p-25f, 0.5f, 1.0f - 0x1p-24f, 0.75f, 0.25f}) us.push_back(w_of(u));
                for (uint32_t j = 0; j < 4096; j++) us.push_back(w_of((float)(j * 4099u % (1u << 24)) * 0x1p-24f));
                ks.resize(us.size());
                lightpick_pick((uint32_t)us.size(), us.data(), M, cs.data(), tot[0], ks.data());
                for (uint32_t k : ks) bad += !(k < M);
            }
        }
    }
    uint64_t out[10];
    const uint32_t shape[4] = {10, 5, 3, 0};
    for (uint32_t flags : {0u, (uint32_t)RT_FLAG_NO_BVH_CULL, (uint32_t)RT_FLAG_EXACT_SCAN, (uint32_t)RT_FLAG_FULL_CHAIN}) {
        uint64_t with[10];
        lightpick_plans(shape, 33, flags, out);
        lightpick_plans(shape, 33, flags | RT_FLAG_LIGHTS_BY_POWER, with);
        bad += std::memcmp(out, with, sizeof out) != 0;
    }
    std::printf(bad ? "LIGHTPICK_HOST_FAILED %d\n" : "LIGHTPICK_HOST_OK\n", bad);
    return bad ? 1 : 0;
}
#endif
