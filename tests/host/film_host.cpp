// Test harness (CPU only, built by tests/test_film_guided_host.py with g++ -ffp-contract=off): the film library's moments fold and
// variance-guided a-trous (film_csrc/rt_film.h) run with the product's own per-pixel lines (film_csrc/rt_film_math.h,
// csrc/rt_denoise_math.h) over plain arrays.
#include <cstdint>
#include <vector>

#include "rt_denoise_math.h"
#include "rt_film_math.h"

extern "C" {

// accum [P*3], mom [P*2] += rec [P*n*3], pixel by pixel in record order
void film_fold_host(const float* rec, uint64_t P, uint32_t n, float* accum, float* mom) {
    for (uint64_t p = 0; p < P; p++) rtfm::fold_pixel(rec + p * n * 3, n, accum + p * 3, mom + p * 2);
}

// C: R*W*3 sums; M: R*W*2 sums; N: R*W*3 or NULL; D, hits: R*W or NULL.  fp: samples, sigma_l, var_eps, k_normal, k_depth.
// Outputs (any may be NULL): lin, f32 (R*W*3 floats), rgb (R*W*3 bytes), var (R*W floats).
void film_resolve_host(uint32_t W, uint32_t R, uint32_t iterations, const float* fp, const float* C, const float* M, const float* N,
                       const float* D, const uint32_t* hits, float* lin, float* f32, uint8_t* rgb, float* var) {
    const size_t np = (size_t)W * R;
    const uint32_t planes = (N ? rtdn::P_NORMAL : 0u) | (D ? rtdn::P_DEPTH : 0u) | (hits ? rtdn::P_HITS : 0u);
    std::vector<float> r(np * 4), r2(np * 4);
    std::vector<rtdn::Guide> g(np);
    for (size_t i = 0; i < np; i++) {
        rtdn::entry_color(C + 3 * i, fp[0], nullptr, &r[4 * i]);
        r[4 * i + 3] = rtfm::entry_variance(M[2 * i], M[2 * i + 1], fp[0]);
        g[i] = rtdn::entry_guide(N ? N + 3 * i : nullptr, D ? D + i : nullptr, hits ? hits + i : nullptr);
    }
    for (uint32_t it = 0; it < iterations; it++) {
        rtfm::Step st;
        st.sigma_l = fp[1];
        st.var_eps = fp[2];
        st.kn = fp[3];
        st.kd = fp[4];
        st.s = 1 << it;
        st.planes = planes;
        auto load = [&](int x, int y, float q[4], rtdn::Guide& gd) {
            const size_t i = (size_t)y * W + x;
            q[0] = r[4 * i];
            q[1] = r[4 * i + 1];
            q[2] = r[4 * i + 2];
            q[3] = r[4 * i + 3];
            gd = g[i];
        };
        for (uint32_t y = 0; y < R; y++)
            for (uint32_t x = 0; x < W; x++) rtfm::step_pixel(st, (int)x, (int)y, (int)W, (int)R, load, &r2[4 * ((size_t)y * W + x)]);
        r.swap(r2);
    }
    for (size_t i = 0; i < np; i++) {
        rtdn::output_pixel(&r[4 * i], nullptr, lin ? lin + 3 * i : nullptr, f32 ? f32 + 3 * i : nullptr, rgb ? rgb + 3 * i : nullptr);
        if (var) var[i] = r[4 * i + 3];
    }
}
}
