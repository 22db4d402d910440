// Test harness (CPU only, built by tests/test_denoise_host.py with g++ -ffp-contract=off): the a-trous denoiser of rt_tile.h run with
// the product's own per-pixel lines (csrc/rt_denoise_math.h) — the entry transform, step_pixel per iteration, the output transform —
// over the image P in plain arrays, and the product's plan (csrc/rt_plan.h plan_denoise).
#include <cstdint>
#include <vector>

#include "rt_denoise_math.h"
#include "rt_plan.h"

extern "C" {

// C: R*W*3 sums; A, N: R*W*3 or NULL; D, hits: R*W or NULL.  fp: color_samples, aov_samples, albedo_eps, k_color, color_step_scale,
// k_normal, k_depth.  Outputs (any may be NULL): lin, f32 (R*W*3 floats), rgb (R*W*3 bytes).
void dn_host(uint32_t W, uint32_t R, uint32_t iterations, const float* fp, const float* C, const float* A, const float* N,
             const float* D, const uint32_t* hits, float* lin, float* f32, uint8_t* rgb) {
    const size_t np = (size_t)W * R;
    const uint32_t planes = (A ? rtdn::P_ALBEDO : 0u) | (N ? rtdn::P_NORMAL : 0u) | (D ? rtdn::P_DEPTH : 0u) | (hits ? rtdn::P_HITS : 0u);
    std::vector<float> r(np * 3), r2(np * 3), d(A ? np * 3 : 0);
    std::vector<rtdn::Guide> g(np);
    for (size_t i = 0; i < np; i++) {
        if (A) rtdn::albedo_d(A + 3 * i, fp[1], fp[2], &d[3 * i]);
        rtdn::entry_color(C + 3 * i, fp[0], A ? &d[3 * i] : nullptr, &r[3 * i]);
        g[i] = rtdn::entry_guide(N ? N + 3 * i : nullptr, D ? D + i : nullptr, hits ? hits + i : nullptr);
    }
    float kc = fp[3];
    for (uint32_t it = 0; it < iterations; it++) {
        rtdn::Step st;
        st.kc = kc;
        st.kn = fp[5];
        st.kd = fp[6];
        st.s = 1 << it;
        st.planes = planes;
        auto load = [&](int x, int y, float q[3], rtdn::Guide& gd) {
            const size_t i = (size_t)y * W + x;
            q[0] = r[3 * i];
            q[1] = r[3 * i + 1];
            q[2] = r[3 * i + 2];
            gd = g[i];
        };
        for (uint32_t y = 0; y < R; y++)
            for (uint32_t x = 0; x < W; x++) rtdn::step_pixel(st, (int)x, (int)y, (int)W, (int)R, load, &r2[3 * ((size_t)y * W + x)]);
        r.swap(r2);
        kc = kc * fp[4];
    }
    for (size_t i = 0; i < np; i++)
        rtdn::output_pixel(&r[3 * i], A ? &d[3 * i] : nullptr, lin ? lin + 3 * i : nullptr, f32 ? f32 + 3 * i : nullptr,
                           rgb ? rgb + 3 * i : nullptr);
}

// plan_denoise: out = npix, tiles_x, off_guide, off_color0, off_color1, scratch_bytes, then per iteration step, lds, wg_per_cu
void dn_plan(uint32_t W, uint32_t R, uint32_t iterations, int guided, uint32_t lds_max_step, uint64_t* out) {
    const rtplan::DenoisePlan p = rtplan::plan_denoise(W, R, iterations, guided != 0, lds_max_step);
    out[0] = p.npix;
    out[1] = p.tiles_x;
    out[2] = p.off_guide;
    out[3] = p.off_color[0];
    out[4] = p.off_color[1];
    out[5] = p.scratch_bytes;
    for (uint32_t i = 0; i < rtplan::DN_MAX_ITER; i++) {
        out[6 + 3 * i] = p.step[i];
        out[7 + 3 * i] = p.lds[i];
        out[8 + 3 * i] = p.wg_per_cu[i];
    }
}

uint32_t dn_lds_max_step_default(void) { return rtplan::DN_LDS_MAX_STEP; }
uint64_t dn_lds_cu(void) { return rtplan::DN_LDS_CU; }
}
