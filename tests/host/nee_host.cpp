// CPU harness of the next-event-estimation integrator (tests/test_nee_host.py): the product's MIS weights and samplable test
// (csrc/rt_nee_math.h) on records of inputs and the plan (csrc/rt_plan.h plan_nee), built by g++ -ffp-contract=off as a shared
// library.  With -DNEE_HOST_MAIN it is a stand-alone program that runs the same entry points over constructed operands (for a
// sanitizer build: -fsanitize=address,undefined).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_nee_math.h"
#include "rt_scene_host.h"

using rtdl::Vec;

namespace {
constexpr int IN_WORDS = 13, OUT_WORDS = 6;

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

// W[i] as bits -> out[2 i] = light_weight(W), out[2 i + 1] = bounce_weight(W), as bits
__attribute__((visibility("default"))) void nee_weights(uint32_t n, const uint32_t* in, uint32_t* out) {
    for (uint32_t i = 0; i < n; i++) {
        out[2 * i] = w_of(rtnee::light_weight(f_of(in[i])));
        out[2 * i + 1] = w_of(rtnee::bounce_weight(f_of(in[i])));
    }
}

// Record i, IN_WORDS 32-bit words: [0] kind (0 sphere, 1 triangle), [1] M, [2..4] n, [5..7] d, [8..10] nh, [11] distance, [12] size.
// Out, OUT_WORDS words: [0] cs', [1] cl', [2] d2', [3] samplable, [4] W', [5] wb.
__attribute__((visibility("default"))) void nee_view(uint32_t n, const uint32_t* in, uint32_t* out) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* r = in + (size_t)i * IN_WORDS;
        uint32_t* o = out + (size_t)i * OUT_WORDS;
        const bool sphere = r[0] == 0;
        const rtnee::View v = rtnee::emitter_view(vec_at(r, 2), vec_at(r, 5), vec_at(r, 8), f_of(r[11]), sphere);
        const float W = rtnee::view_weight(v, sphere, f_of(r[12]), r[1]);
        o[0] = w_of(v.cs), o[1] = w_of(v.cl), o[2] = w_of(v.d2), o[3] = v.samplable ? 1u : 0u, o[4] = w_of(W);
        o[5] = w_of(rtnee::bounce_weight(W));
    }
}

// plan_nee for a shape (n_sph, n_tri, bvh_depth, inverted_boxes): out = (engine, scan_mode, full_chain, lds, too_many)
__attribute__((visibility("default"))) void nee_plan(const uint32_t* shape, uint32_t n_lights, uint32_t flags, uint64_t* out) {
    rtplan::SceneShape sh;
    sh.n_sph = shape[0];
    sh.n_tri = shape[1];
    sh.bvh_depth = shape[2];
    sh.inverted_boxes = shape[3] != 0;
    const rtplan::NeePlan d = rtplan::plan_nee(sh, n_lights, flags);
    out[0] = (uint64_t)d.query.engine;
    out[1] = (uint64_t)d.query.scan_mode;
    out[2] = d.query.full_chain ? 1 : 0;
    out[3] = d.query.lds;
    out[4] = d.too_many ? 1 : 0;
}

}  // extern "C"

#ifdef NEE_HOST_MAIN
// The host side of the feature under a sanitizer: the weights over W = 0, subnormal, 1, large, +inf and a sweep of magnitudes (no NaN,
// both in [0, 1], wl falling and wb rising); the view over facing and back-facing directions, a sphere hit from inside, zero normals,
// distances 0 and huge; the plan over its flags and the emitter limit.
int main() {
    int bad = 0;
    std::vector<float> Ws = {0.0f, 1e-45f, 1e-40f, 1e-8f, 0.5f, 1.0f, 2.0f, 1e8f, 3e38f, INFINITY};
    for (int e = -140; e <= 127; e += 3) Ws.push_back(std::ldexp(1.0f, e));
    std::vector<uint32_t> in(Ws.size()), out(2 * Ws.size());
    for (size_t i = 0; i < Ws.size(); i++) in[i] = w_of(Ws[i]);
    nee_weights((uint32_t)Ws.size(), in.data(), out.data());
    for (size_t i = 0; i < Ws.size(); i++) {
        const float wl = f_of(out[2 * i]), wb = f_of(out[2 * i + 1]);
        bad += !(wl >= 0.0f && wl <= 1.0f) + !(wb >= 0.0f && wb <= 1.0f);
    }
    bad += f_of(out[0]) != 1.0f || f_of(out[1]) != 0.0f;                                    // W = 0
    bad += f_of(out[2 * 9]) != 0.0f || f_of(out[2 * 9 + 1]) != 1.0f;                        // W = +inf
    const float dirs[][3] = {{0, 0, 1}, {0, 0, -1}, {0.6f, 0, 0.8f}, {1, 0, 0}, {0, 0, 0}};
    const float dists[] = {0.0f, 1e-30f, 1.0f, 7.5f, 1e19f, 3e19f, INFINITY};
    std::vector<uint32_t> rec, res;
    uint32_t n = 0;
    for (uint32_t kind = 0; kind < 2; kind++)
        for (const auto& nn : dirs)
            for (const auto& dd : dirs)
                for (const auto& nh : dirs)
                    for (float dist : dists) {
                        const uint32_t r[IN_WORDS] = {kind,        3u,          w_of(nn[0]), w_of(nn[1]), w_of(nn[2]), w_of(dd[0]), w_of(dd[1]),
                                                      w_of(dd[2]), w_of(nh[0]), w_of(nh[1]), w_of(nh[2]), w_of(dist),  w_of(0.5f)};
                        rec.insert(rec.end(), r, r + IN_WORDS);
                        n++;
                    }
    res.resize((size_t)n * OUT_WORDS);
    nee_view(n, rec.data(), res.data());
    uint32_t n_samplable = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* o = res.data() + (size_t)i * OUT_WORDS;
        if (!o[3]) continue;
        n_samplable++;
        const float W = f_of(o[4]), wb = f_of(o[5]);
        bad += !(f_of(o[0]) > 0.0f && f_of(o[1]) > 0.0f && f_of(o[2]) > 0.0f && std::isfinite(f_of(o[2])));
        bad += !(W >= 0.0f) + !(wb >= 0.0f && wb <= 1.0f);
    }
    bad += n_samplable == 0 || n_samplable == n;
    uint64_t plan[5];
    const uint32_t shape[4] = {10, 4, 3, 0};
    for (uint32_t flags : {0u, (uint32_t)RT_FLAG_NO_BVH_CULL, (uint32_t)RT_FLAG_EXACT_SCAN, (uint32_t)RT_FLAG_FULL_CHAIN}) {
        nee_plan(shape, 2, flags, plan);
        bad += plan[4] != 0;
    }
    nee_plan(shape, rtplan::DIRECT_MAX_LIGHTS + 1u, 0, plan);
    bad += plan[4] != 1;
    std::printf(bad ? "NEE_HOST_FAILED %d\n" : "NEE_HOST_OK\n", bad);
    return bad ? 1 : 0;
}
#endif
