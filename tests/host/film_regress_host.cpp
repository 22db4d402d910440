// Test harness (CPU only, built by tests/test_film_regress_host.py with g++ -ffp-contract=off): the film library's regression resolve
// (film_csrc/rt_film.h "Regression resolve") run with the product's own per-pixel and per-node lines (film_csrc/rt_film_math.h,
// csrc/rt_denoise_math.h) over plain arrays.  The window sum is the header's, written here as the plain tree: sixteen groups of 64
// lanes, adjacent pairs over six levels, the group totals added in order.  With a main() (-DFILM_REGRESS_MAIN) it is a stand-alone
// program that runs a seeded image of every size, for a run under a host sanitizer.
#include <cstdint>
#include <vector>

#include "rt_denoise_math.h"
#include "rt_film_math.h"

namespace {

// S(v) over the 1024 window lanes
float window_sum(const float* v) {
    float s = 0.0f;
    for (int k = 0; k < 16; k++) {
        float t[64];
        for (int m = 0; m < 64; m++) t[m] = v[64 * k + m];
        for (int width = 32; width >= 1; width >>= 1)
            for (int m = 0; m < width; m++) t[m] = t[2 * m] + t[2 * m + 1];
        s = s + t[0];
    }
    return s;
}

}  // namespace

extern "C" {

// C: R*W*3 sums; A, N: R*W*3 or NULL; D, hits: R*W or NULL.  fp: samples, aov_samples, albedo_eps, ridge.
// model: NY*NX*32 floats.  Outputs (any may be NULL): lin, f32 (R*W*3 floats), rgb (R*W*3 bytes).
void film_regress_host(uint32_t W, uint32_t R, const float* fp, const float* C, const float* A, const float* N, const float* D,
                       const uint32_t* hits, float* model, float* lin, float* f32, uint8_t* rgb) {
    const rtfm::RgPlanes pl = {C, A, N, D, hits, fp[0], fp[1], fp[2]};
    const float ridge = fp[3];
    const uint32_t NX = rtfm::rg_nodes(W), NY = rtfm::rg_nodes(R);
    std::vector<float> v(1024);
    for (uint32_t j = 0; j < NY; j++)
        for (uint32_t i = 0; i < NX; i++) {
            std::vector<rtfm::RgPixel> px(1024);
            std::vector<char> valid(1024, 0);
            uint32_t n = 0;
            float zlo = __builtin_inff(), zhi = 0.0f;
            for (int l = 0; l < 1024; l++) {
                const int x = 16 * (int)i - 16 + (l & 31), y = 16 * (int)j - 16 + (l >> 5);
                if (x < 0 || x >= (int)W || y < 0 || y >= (int)R) continue;
                px[l] = rtfm::rg_entry(pl, (size_t)y * W + x);
                if (!px[l].valid) continue;
                valid[l] = 1;
                n++;
                zlo = __builtin_fminf(zlo, px[l].z);
                zhi = __builtin_fmaxf(zhi, px[l].z);
            }
            if (n == 0 || !D) zlo = zhi = 0.0f;
            const float s = zhi - zlo;
            std::vector<float> phi(1024 * rtfm::RG_M, 0.0f);
            for (int l = 0; l < 1024; l++)
                if (valid[l]) rtfm::rg_features(px[l], 16 * (int)i - 16 + (l & 31), 16 * (int)j - 16 + (l >> 5), (int)i, (int)j, zlo, s, &phi[l * rtfm::RG_M]);
            float S[rtfm::RG_NS], L[64], *rec = model + ((size_t)j * NX + i) * rtfm::RG_RECORD;
            for (int a = 0; a < rtfm::RG_M; a++) {
                for (int b = a; b < rtfm::RG_M; b++) {
                    for (int l = 0; l < 1024; l++) v[l] = valid[l] ? phi[l * rtfm::RG_M + a] * phi[l * rtfm::RG_M + b] : 0.0f;
                    S[rtfm::rg_ai(a, b)] = window_sum(v.data());
                }
                for (int c = 0; c < 3; c++) {
                    for (int l = 0; l < 1024; l++) v[l] = valid[l] ? phi[l * rtfm::RG_M + a] * px[l].r[c] : 0.0f;
                    S[rtfm::RG_NA + 3 * a + c] = window_sum(v.data());
                }
            }
            const bool ok = rtfm::rg_cholesky(S, n, ridge, L);
            for (int c = 0; c < 3; c++) rtfm::rg_solve(S, n, ok, L, c, rec);
            rtfm::rg_record_tail(n, zlo, s, ok, rec);
        }
    for (uint32_t y = 0; y < R; y++)
        for (uint32_t x = 0; x < W; x++) {
            const size_t g = (size_t)y * W + x;
            const rtfm::RgPixel px = rtfm::rg_entry(pl, g);
            float r[3] = {px.r[0], px.r[1], px.r[2]};
            if (px.valid) rtfm::rg_apply(px, (int)x, (int)y, model, NX, r);
            rtdn::output_pixel(r, A ? px.d : nullptr, lin ? lin + 3 * g : nullptr, f32 ? f32 + 3 * g : nullptr, rgb ? rgb + 3 * g : nullptr);
        }
}
}

#ifdef FILM_REGRESS_MAIN
#include <cstdio>
int main() {
    const uint32_t sizes[5][2] = {{1, 1}, {16, 16}, {17, 16}, {33, 47}, {70, 9}};
    uint32_t state = 12345u;
    auto rnd = [&]() {
        state = state * 1664525u + 1013904223u;
        return (float)(state >> 8) / 16777216.0f;
    };
    for (auto& wr : sizes) {
        const uint32_t W = wr[0], R = wr[1];
        const size_t np = (size_t)W * R;
        std::vector<float> C(np * 3), A(np * 3), N(np * 3), D(np), lin(np * 3), f(np * 3);
        std::vector<uint32_t> hits(np);
        std::vector<uint8_t> rgb(np * 3);
        for (size_t i = 0; i < np; i++) {
            hits[i] = (uint32_t)(rnd() * 5.0f);
            D[i] = hits[i] * (2.0f + rnd());
            for (int c = 0; c < 3; c++) {
                C[3 * i + c] = rnd() * 8.0f;
                A[3 * i + c] = rnd() * 4.0f;
                N[3 * i + c] = (rnd() - 0.5f) * hits[i];
            }
        }
        std::vector<float> model((size_t)rtfm::rg_nodes(W) * rtfm::rg_nodes(R) * rtfm::RG_RECORD);
        const float fp[4] = {8.0f, 4.0f, 0.00390625f, 0.001f};
        film_regress_host(W, R, fp, C.data(), A.data(), N.data(), D.data(), hits.data(), model.data(), lin.data(), f.data(), rgb.data());
        film_regress_host(W, R, fp, C.data(), nullptr, nullptr, nullptr, nullptr, model.data(), lin.data(), nullptr, rgb.data());
        std::printf("%u x %u: model[0] %g, rgb[0] %u\n", W, R, model[0], rgb[0]);
    }
    return 0;
}
#endif
