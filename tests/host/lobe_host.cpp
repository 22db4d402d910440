// CPU harness of the light samples at glossy hits (tests/test_lobe_host.py): the sampled-class rule, the glossy direction, the lobe and
// its factor (csrc/rt_lobe_math.h), built by g++ -ffp-contract=off as a shared library, so the lines the kernel runs are compared with
// the numpy restatement bit for bit.  With -DLOBE_HOST_MAIN it is a stand-alone program that runs the same functions over structured
// and seeded operands (for a sanitizer build: -fsanitize=address,undefined).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_lobe_math.h"

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

constexpr uint32_t LOBE_IN = 16, LOBE_OUT = 20;

// Record i, LOBE_IN words (f32 as bits): [0..2] n, [3..5] d (the incoming direction), [6] rho, [7..9] w, [10] W, [11..13] us,
// [14..15] unused.  Out, LOBE_OUT words: [0] sampled_class, [1..3] g, [4] gn, [5..7] c, [8] r, [9] kappa, [10] b, [11] D, [12] in the
// lobe, [13] cg, [14] lobe_sample_taken(W); of lobe_factor_scatter(us): [15] m, [16] t, [17] cg, [18] in the lobe; [19] 0.  The lobe and
// its factors are formed whatever the class is.
__attribute__((visibility("default"))) void lobe_records(uint32_t n, const uint32_t* in, uint32_t* out) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* r = in + (size_t)i * LOBE_IN;
        uint32_t* o = out + (size_t)i * LOBE_OUT;
        const rtdl::Vec nrm{f_of(r[0]), f_of(r[1]), f_of(r[2])}, d{f_of(r[3]), f_of(r[4]), f_of(r[5])};
        const rtdl::Vec w{f_of(r[7]), f_of(r[8]), f_of(r[9])};
        const float rho = f_of(r[6]);
        const rtdl::Vec g = rtlobe::glossy_dir(d, nrm);
        const float gn = rtdl::dot3(nrm, g);
        const rtlobe::Lobe l = rtlobe::lobe_of(nrm, g, rho);
        const rtlobe::LobeFactor f = rtlobe::lobe_factor(l, w);
        o[0] = rtlobe::sampled_class(rho, gn);
        o[1] = w_of(g.x), o[2] = w_of(g.y), o[3] = w_of(g.z);
        o[4] = w_of(gn);
        o[5] = w_of(l.c.x), o[6] = w_of(l.c.y), o[7] = w_of(l.c.z);
        o[8] = w_of(l.r), o[9] = w_of(l.kappa), o[10] = w_of(f.b), o[11] = w_of(f.D);
        o[12] = f.in_lobe ? 1u : 0u;
        o[13] = w_of(f.cg);
        o[14] = rtlobe::lobe_sample_taken(f, f_of(r[10])) ? 1u : 0u;
        const rtlobe::ScatterFactor s = rtlobe::lobe_factor_scatter(l, rtdl::Vec{f_of(r[11]), f_of(r[12]), f_of(r[13])});
        o[15] = w_of(s.m), o[16] = w_of(s.t), o[17] = w_of(s.cg);
        o[18] = s.in_lobe ? 1u : 0u;
        o[19] = 0u;
    }
}

}  // extern "C"

#ifdef LOBE_HOST_MAIN
// The host side of the feature under a sanitizer: the class rule on its boundaries, exceptional operands, and a seeded sweep of unit
// normals and directions at front-face hits; there kappa > 0, no NaN, and cg > 0 exactly in the lobe.
int main() {
    int bad = 0;
    std::vector<uint32_t> in;
    auto add = [&](float nx, float ny, float nz, float dx, float dy, float dz, float rho, float wx, float wy, float wz, float W) {
        const float rec[LOBE_IN] = {nx, ny, nz, dx, dy, dz, rho, wx, wy, wz, W, wz, -wx, wy, 0.f, 0.f};   // (us: w's components shuffled)
        for (float f : rec) in.push_back(w_of(f));
    };
    const float rhos[] = {0.f, -0.f, 0x1p-24f, 0.5f, 1.f - 0x1p-24f, 1.f, 1.5f, -0.5f, NAN, INFINITY, 1e-45f};
    const uint32_t cls_front[] = {1, 1, 2, 2, 2, 0, 0, 0, 0, 0, 2};
    for (float rho : rhos) {
        add(0.f, 1.f, 0.f, 0.6f, -0.8f, 0.f, rho, 0.6f, 0.8f, 0.f, 1.f);       // front: gn = 0.8
        add(0.f, 1.f, 0.f, 0.6f, 0.8f, 0.f, rho, 0.6f, -0.8f, 0.f, 1.f);       // back: gn = -0.8
        add(0.f, 1.f, 0.f, 1.f, 0.f, 0.f, rho, 1.f, 0.f, 0.f, INFINITY);       // grazing: gn = 0
    }
    const uint32_t n_dir = (uint32_t)(in.size() / LOBE_IN);
    for (float x : {0.f, NAN, INFINITY, 1e-30f, 1e30f}) add(0.f, 1.f, 0.f, x, -1.f, 0.f, 0.5f, 0.f, 1.f, x, x);
    uint64_t lcg = 424242;
    auto u = [&] {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((lcg >> 40) & 0xffffff) * 0x1p-24f;
    };
    auto unit = [&](float* v) {
        float s;
        do {
            v[0] = 2.f * u() - 1.f, v[1] = 2.f * u() - 1.f, v[2] = 2.f * u() - 1.f;
            s = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        } while (s >= 1.f || s < 0.01f);
        const float l = std::sqrt(s);
        v[0] /= l, v[1] /= l, v[2] /= l;
    };
    const uint32_t first_seeded = (uint32_t)(in.size() / LOBE_IN);
    for (int i = 0; i < 20000; i++) {
        float nn[3], dd[3], ww[3];
        unit(nn), unit(dd), unit(ww);
        if (nn[0] * dd[0] + nn[1] * dd[1] + nn[2] * dd[2] > 0.f) dd[0] = -dd[0], dd[1] = -dd[1], dd[2] = -dd[2];   // a front-face hit
        add(nn[0], nn[1], nn[2], dd[0], dd[1], dd[2], 0.01f + 0.98f * u(), ww[0], ww[1], ww[2], 40.f * u());
    }
    const uint32_t n = (uint32_t)(in.size() / LOBE_IN);
    std::vector<uint32_t> out((size_t)n * LOBE_OUT);
    lobe_records(n, in.data(), out.data());
    for (uint32_t i = 0; i < n_dir; i++) {
        const uint32_t want = i % 3 == 1 ? (cls_front[i / 3] == 1 ? 1u : 0u) : cls_front[i / 3];
        bad += out[(size_t)i * LOBE_OUT] != want;
    }
    uint32_t in_lobe = 0;
    for (uint32_t i = first_seeded; i < n; i++) {
        const uint32_t* o = out.data() + (size_t)i * LOBE_OUT;
        for (int k = 1; k < 12; k++) bad += std::isnan(f_of(o[k]));
        bad += std::isnan(f_of(o[13]));
        bad += o[0] == 2u && !(f_of(o[9]) > 0.f);                              // kappa > 0 at a lobe-sampled hit
        bad += (o[12] != 0u) != (f_of(o[13]) > 0.f);
        bad += o[14] != 0u && o[12] == 0u;
        bad += o[0] == 2u && f_of(o[9]) > 1e-6f && !(o[18] != 0u && f_of(o[17]) > 0.f);   // the scatter's own direction is in its lobe
        in_lobe += o[12];
    }
    bad += in_lobe < 1000;
    if (bad) std::printf("LOBE_HOST_FAILED %d\n", bad);
    else std::printf("LOBE_HOST_OK %u of %u in the lobe\n", in_lobe, n - first_seeded);
    return bad ? 1 : 0;
}
#endif
