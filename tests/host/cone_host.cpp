// CPU harness of cone sampling of sphere lights (tests/test_cone_host.py): the regime, the cone sample, its geometry, weight and
// point (csrc/rt_direct_math.h) and the cone view of an emitter the bounce reached (csrc/rt_nee_math.h), built by g++
// -ffp-contract=off as a shared library, so the lines the kernels run are compared with the numpy restatement bit for bit.  With
// -DCONE_HOST_MAIN it is a stand-alone program that runs the same functions over structured and seeded operands (for a sanitizer
// build: -fsanitize=address,undefined).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_direct_math.h"
#include "rt_nee_math.h"

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

constexpr uint32_t CONE_IN = 16, CONE_OUT = 20, VIEW_IN = 14, VIEW_OUT = 5;

// out[i] = cone_regime(q[i]) (f32 as bits)
__attribute__((visibility("default"))) void cone_regimes(uint32_t n, const uint32_t* q, uint32_t* out) {
    for (uint32_t i = 0; i < n; i++) out[i] = rtdl::cone_regime(f_of(q[i])) ? 1u : 0u;
}

// Record i, CONE_IN words (f32 as bits): [0..2] P, [3..5] c, [6] r, [7] x1, [8] x2, [9] s, [10..12] n, [13] ip, [14..15] unused.
// Out, CONE_OUT words: [0] q, [1] in the regime, and — in the regime only, otherwise 0 — [2..4] v, [5] omc, [6] dc2, [7] dc, [8] ct,
// [9] st, [10..12] wn, [13] cs, [14] facing, [15] W, [16..18] L, [19] v.v.
__attribute__((visibility("default"))) void cone_samples(uint32_t n, const uint32_t* in, uint32_t* out) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* r = in + (size_t)i * CONE_IN;
        uint32_t* o = out + (size_t)i * CONE_OUT;
        const rtdl::Vec P{f_of(r[0]), f_of(r[1]), f_of(r[2])}, c{f_of(r[3]), f_of(r[4]), f_of(r[5])};
        const rtdl::Vec nrm{f_of(r[10]), f_of(r[11]), f_of(r[12])};
        const float rad = f_of(r[6]);
        std::memset(o, 0, CONE_OUT * 4);
        const rtdl::ConeAxis ax = rtdl::cone_axis(P, c, rad);
        o[0] = w_of(ax.q);
        if (!rtdl::cone_regime(ax.q)) continue;
        o[1] = 1u;
        const rtdl::Cone k = rtdl::cone_sample(P, c, rad, f_of(r[7]), f_of(r[8]), f_of(r[9]));
        const rtdl::Geometry g = rtdl::cone_geometry(nrm, k.v);
        const rtdl::Vec L = rtdl::cone_point(P, g.w, rad, k);
        o[2] = w_of(k.v.x), o[3] = w_of(k.v.y), o[4] = w_of(k.v.z);
        o[5] = w_of(k.omc), o[6] = w_of(k.dc2), o[7] = w_of(k.dc), o[8] = w_of(k.ct), o[9] = w_of(k.st);
        o[10] = w_of(g.w.x), o[11] = w_of(g.w.y), o[12] = w_of(g.w.z);
        o[13] = w_of(g.cs);
        o[14] = g.facing ? 1u : 0u;
        o[15] = w_of(rtdl::cone_weight(g.cs, k.omc, f_of(r[13])));
        o[16] = w_of(L.x), o[17] = w_of(L.y), o[18] = w_of(L.z);
        o[19] = w_of(g.d2);
    }
}

// Record i, VIEW_IN words: [0..2] o, [3..5] n, [6..8] d, [9..11] c, [12] r, [13] ip.  Out, VIEW_OUT words: cs', omc', in_regime,
// samplable, W'.
__attribute__((visibility("default"))) void cone_views(uint32_t n, const uint32_t* in, uint32_t* out) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* r = in + (size_t)i * VIEW_IN;
        uint32_t* o = out + (size_t)i * VIEW_OUT;
        const rtnee::ConeView v = rtnee::emitter_view_cone(rtdl::Vec{f_of(r[0]), f_of(r[1]), f_of(r[2])}, rtdl::Vec{f_of(r[3]), f_of(r[4]), f_of(r[5])},
                                                           rtdl::Vec{f_of(r[6]), f_of(r[7]), f_of(r[8])},
                                                           rtdl::Vec{f_of(r[9]), f_of(r[10]), f_of(r[11])}, f_of(r[12]));
        o[0] = w_of(v.cs), o[1] = w_of(v.omc), o[2] = v.in_regime ? 1u : 0u, o[3] = v.samplable ? 1u : 0u;
        o[4] = w_of(rtnee::cone_view_weight(v, f_of(r[13])));
    }
}

}  // extern "C"

#ifdef CONE_HOST_MAIN
// The host side of the feature under a sanitizer: the regime at its two ends and their neighbours, degenerate spheres and points, the
// axis along every coordinate direction with both signs of zero, s at its ends, and a seeded sweep; in the regime no NaN,
// 0 <= W <= 2 ip for a facing sample and |v.v - 1| <= 2^-18.
int main() {
    int bad = 0;
    const float qs[] = {std::nextafterf(0x1p-10f, 0.f), 0x1p-10f, std::nextafterf(0x1p-10f, 1.f), std::nextafterf(1.f, 0.f), 1.f,
                        std::nextafterf(1.f, 2.f), 0.f, -0.f, INFINITY, NAN, 0.5f};
    const uint32_t want[] = {0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1};
    std::vector<uint32_t> q, reg(sizeof qs / sizeof *qs);
    for (float x : qs) q.push_back(w_of(x));
    cone_regimes((uint32_t)q.size(), q.data(), reg.data());
    for (size_t i = 0; i < q.size(); i++) bad += reg[i] != want[i];

    std::vector<uint32_t> in, views;
    auto add = [&](float px, float py, float pz, float cx, float cy, float cz, float r, float x1, float x2, float nx, float ny, float nz,
                   float ip) {
        const float rec[CONE_IN] = {px, py, pz, cx, cy, cz, r, x1, x2, x1 * x1 + x2 * x2, nx, ny, nz, ip, 0.f, 0.f};
        for (float f : rec) in.push_back(w_of(f));
        const float len = std::sqrt(cx * cx + cy * cy + cz * cz);
        const float v[VIEW_IN] = {px, py, pz, nx, ny, nz, (cx - px) / len, (cy - py) / len, (cz - pz) / len, cx, cy, cz, r, ip};
        for (float f : v) views.push_back(w_of(f));
    };
    const float axes[][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {1, 0, -0.f}, {0, 1, -0.f}, {0.6f, 0.8f, 0.f}};
    const float pairs[][2] = {{0.f, 0.f}, {0x1p-75f, 0.f}, {0.f, -0x1p-70f}, {0.70710677f, 0.70710671f}, {-0.999999f, 0.001f}, {0.3f, -0.4f}};
    for (const auto& a : axes)
        for (const auto& p : pairs)
            for (float r : {0.f, 1e-41f, 0.03125f, 0.0312f, 0.3f, 0.9f, 0.99999994f, 1.f, 1.5f, INFINITY})
                add(0.f, 0.f, 0.f, a[0], a[1], a[2], r, p[0], p[1], a[0], a[1], a[2], 33.f);
    for (float d : {0.f, INFINITY, NAN, 1e-30f, 1e30f}) add(0.f, 0.f, 0.f, d, 0.f, 0.f, 0.5f, 0.1f, 0.2f, 1.f, 0.f, 0.f, 2.f);
    uint64_t lcg = 12345;
    auto u = [&] {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((lcg >> 40) & 0xffffff) * 0x1p-24f;
    };
    for (int i = 0; i < 20000; i++) {
        float x1, x2;
        do {
            x1 = 2.f * u() - 1.f;
            x2 = 2.f * u() - 1.f;
        } while (x1 * x1 + x2 * x2 >= 1.f);
        const float cx = 8.f * u() - 4.f, cy = 8.f * u() - 4.f, cz = 8.f * u() - 4.f;
        add(u(), u(), u(), cx, cy, cz, 0.05f + 3.f * u(), x1, x2, 2.f * u() - 1.f, 2.f * u() - 1.f, 2.f * u() - 1.f, 1.f + 40.f * u());
    }
    const uint32_t n = (uint32_t)(in.size() / CONE_IN);
    std::vector<uint32_t> out((size_t)n * CONE_OUT), vout((size_t)n * VIEW_OUT);
    cone_samples(n, in.data(), out.data());
    cone_views(n, views.data(), vout.data());
    uint32_t in_regime = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* o = out.data() + (size_t)i * CONE_OUT;
        if (!o[1]) continue;
        in_regime++;
        const float ip = f_of(in[(size_t)i * CONE_IN + 13]);
        for (int k = 2; k < 14; k++) bad += std::isnan(f_of(o[k]));
        for (int k = 15; k < 20; k++) bad += std::isnan(f_of(o[k]));
        bad += !(std::fabs(f_of(o[19]) - 1.f) <= 0x1p-18f);
        if (o[14]) bad += !(f_of(o[15]) >= 0.f && f_of(o[15]) <= 2.f * ip);
        const uint32_t* v = vout.data() + (size_t)i * VIEW_OUT;
        bad += v[2] != 1u || std::isnan(f_of(v[1]));
    }
    bad += in_regime < 5000;
    if (bad) std::printf("CONE_HOST_FAILED %d\n", bad);
    else std::printf("CONE_HOST_OK %u of %u in the regime\n", in_regime, n);
    return bad ? 1 : 0;
}
#endif
