// Test harness (CPU only, built by tests/test_bloom_host.py with g++ -ffp-contract=off): the bloom library's call (bloom_csrc/rt_bloom.h)
// run with the product's own lines (bloom_csrc/rt_bloom_math.h) over plain arrays, step by step and as a whole, with the scratch laid
// out as the library lays it out.  With -DBLOOM_HOST_MAIN it is a stand-alone program (its own main) that blooms exactly sized images
// that hold extreme values too, for a sanitizer build.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rt_bloom_math.h"

namespace {

void down_level(const float* src, uint32_t Ws, uint32_t Rs, float* dst) {
    const uint32_t Wd = rtbm::half_up(Ws), Rd = rtbm::half_up(Rs);
    const auto fetch = [&](uint32_t r, uint32_t c, float* s) {
        const float* q = src + 3 * ((size_t)r * Ws + c);
        s[0] = q[0], s[1] = q[1], s[2] = q[2];
    };
    for (uint32_t i = 0; i < Rd; i++)
        for (uint32_t j = 0; j < Wd; j++) rtbm::down_pixel(fetch, i, j, Rs, Ws, dst + 3 * ((size_t)i * Wd + j));
}

template <uint32_t MODE>
void combine(const float* img, uint32_t W, uint32_t R, const float* U1, float strength, float norm, float* out, float* out_bloom) {
    const float keep = 1.0f - strength;
    const uint32_t W1 = rtbm::half_up(W), R1 = rtbm::half_up(R);
    for (uint32_t y = 0; y < R; y++)
        for (uint32_t x = 0; x < W; x++) {
            float u[3];
            rtbm::up_pixel(U1, R1, W1, y, x, u);
            for (uint32_t c = 0; c < 3; c++) {
                const size_t at = 3 * ((size_t)y * W + x) + c;
                const float b = rtbm::bloom_value(u[c], norm);
                out[at] = rtbm::mix<MODE>(rtbm::positive(img[at]), b, strength, keep);
                if (out_bloom) out_bloom[at] = b;
            }
        }
}

}  // namespace

extern "C" {

// the pixels a pyramid starts from, n of them: sanitised, and under the threshold where T > 0
void bloom_source_host(const float* img, uint32_t n, float cap, float T, float K, float* out) {
    for (uint32_t i = 0; i < n; i++) {
        if (T > 0.0f)
            rtbm::source_pixel<true>(img + 3 * (size_t)i, cap, T, K, out + 3 * (size_t)i);
        else
            rtbm::source_pixel<false>(img + 3 * (size_t)i, cap, T, K, out + 3 * (size_t)i);
    }
}

// f of n sanitised pixels
void bloom_factor_host(const float* p, uint32_t n, float T, float K, float* f) {
    for (uint32_t i = 0; i < n; i++) f[i] = rtbm::threshold_factor(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2], T, K);
}

// D_{k+1} [ (Rs + 1) / 2 ][ (Ws + 1) / 2 ][3] of a level [Rs][Ws][3]
void bloom_down_host(const float* src, uint32_t Ws, uint32_t Rs, float* dst) { down_level(src, Ws, Rs, dst); }

// up(X) [Rf][Wf][3] of a level X [Rc][Wc][3]
void bloom_up_host(const float* X, uint32_t Wc, uint32_t Rc, uint32_t Wf, uint32_t Rf, float* out) {
    for (uint32_t y = 0; y < Rf; y++)
        for (uint32_t x = 0; x < Wf; x++) rtbm::up_pixel(X, Rc, Wc, y, x, out + 3 * ((size_t)y * Wf + x));
}

// the taps, for the clamp cases: down[4] of output index i over a side n, and (a, b, wa, wb) of fine index y over a coarse side n
void bloom_taps_host(uint32_t i, uint32_t n, uint32_t* down, uint32_t* up, float* w) {
    for (uint32_t a = 0; a < 4; a++) down[a] = rtbm::down_tap(i, a, n);
    const rtbm::UpTap t = rtbm::up_tap(i, n);
    up[0] = t.a, up[1] = t.b, w[0] = t.wa, w[1] = t.wb;
}

uint32_t bloom_tail_from_host(uint32_t W, uint32_t R, uint32_t levels, uint64_t budget) { return rtbm::tail_from(W, R, levels, budget); }
uint64_t bloom_lds_budget_host() { return rtbm::LDS_BUDGET; }

// the scratch: the offsets of levels 1 ... levels, and its size
uint64_t bloom_scratch_host(uint32_t W, uint32_t R, uint32_t levels, uint64_t* offsets) {
    for (uint32_t k = 1; k <= levels; k++) offsets[k - 1] = rtbm::level_offset(W, R, k);
    return rtbm::level_offset(W, R, levels + 1);
}

int bloom_settings_ok_host(uint32_t levels, uint32_t mode, float spread, float strength, float norm, float cap, float T, float K) {
    const rtbm::Settings s = {levels, mode, spread, strength, norm, cap, T, K};
    return rtbm::settings_ok(s) ? 1 : 0;
}

// rtb_apply.  `scratch` is laid out as the library's and holds U_1 ... U_L afterwards; `first` [R][W][3] is the caller's room for the
// pixels the pyramid starts from.  Returns 0, or 1 for settings the library refuses.
int bloom_apply_host(const float* img, uint32_t W, uint32_t R, uint32_t levels, uint32_t mode, float spread, float strength, float norm,
                     float cap, float T, float K, float* first, char* scratch, float* out, float* out_bloom) {
    const rtbm::Settings s = {levels, mode, spread, strength, norm, cap, T, K};
    if (!rtbm::settings_ok(s) || W == 0 || R == 0) return 1;
    const auto level = [&](uint32_t k) { return (float*)(scratch + rtbm::level_offset(W, R, k)); };
    bloom_source_host(img, W * R, cap, T, K, first);
    for (uint32_t k = 1; k <= levels; k++)
        down_level(k == 1 ? first : level(k - 1), rtbm::level_side(W, k - 1), rtbm::level_side(R, k - 1), level(k));
    for (uint32_t k = levels - 1; k >= 1; k--) {
        const uint32_t Wf = rtbm::level_side(W, k), Rf = rtbm::level_side(R, k);
        float* fine = level(k);
        for (uint32_t y = 0; y < Rf; y++)
            for (uint32_t x = 0; x < Wf; x++) {
                float u[3];
                rtbm::up_pixel(level(k + 1), rtbm::half_up(Rf), rtbm::half_up(Wf), y, x, u);
                float* d = fine + 3 * ((size_t)y * Wf + x);
                for (uint32_t c = 0; c < 3; c++) d[c] = rtbm::accumulate(d[c], spread, u[c]);
            }
    }
    if (mode == rtbm::MODE_MIX)
        combine<rtbm::MODE_MIX>(img, W, R, level(1), strength, norm, out, out_bloom);
    else
        combine<rtbm::MODE_ADD>(img, W, R, level(1), strength, norm, out, out_bloom);
    return 0;
}
}

#ifdef BLOOM_HOST_MAIN
// Images of 9 x 70, 5 x 37, 1 x 1 and 2 x 3 in exactly sized buffers, the scratch exactly rtb_scratch_bytes: seeded values over
// 2^-20 ... 2^20 with subnormal, huge, negative and non-finite values (the classes of tests/_extreme_planes.py) written over some.
// Each is bloomed at every level count it admits and at 8, in both modes, with and without a threshold and the second output:
// whatever the image holds, no line reads or writes outside its buffer, no conversion is undefined, no NaN comes out, a +inf stays
// +inf and the bloom alone is finite.
int main() {
    uint32_t lcg = 2463534242u;
    auto rnd = [&] { return (float)((lcg = lcg * 1664525u + 1013904223u) >> 8) / 16777216.0f; };
    const float special[] = {1e-45f, -1e-45f, 5.9e-39f, 1.1754942e-38f, -0.0f, 0.0f, 1e-30f, 1.9e19f, 3e38f, 3.4028235e38f, -3.4028235e38f,
                             __builtin_inff(), -__builtin_inff(), __builtin_nanf(""), -__builtin_nanf(""), -1.5f, 65536.0f, 61440.0f};
    const size_t n_special = sizeof special / sizeof *special;
    unsigned long long bloomed = 0;
    const uint32_t sizes[4][2] = {{70, 9}, {37, 5}, {1, 1}, {3, 2}};
    for (const auto& size : sizes) {
        const uint32_t W = size[0], R = size[1], n = W * R;
        std::vector<float> img((size_t)n * 3);
        for (float& v : img) {
            const float e = 40.0f * rnd() - 20.0f;
            v = (rnd() < 0.1f ? -1.0f : 1.0f) * __builtin_ldexpf(1.0f + rnd(), (int)e);
        }
        for (size_t j = 0; j < 4 * n_special; j++) img[(7 * j + 3) % img.size()] = special[j % n_special];
        for (size_t j = 0; j < n_special && j < n; j++)                                        // and whole pixels of them
            for (int c = 0; c < 3; c++) img[3 * ((size_t)n - 1 - j) + c] = special[j];
        for (uint32_t levels = 1; levels <= rtbm::MAX_LEVELS; levels++) {
            uint64_t offsets[rtbm::MAX_LEVELS];
            const uint64_t bytes = bloom_scratch_host(W, R, levels, offsets);
            if (bytes % 16 != 0 || bloom_tail_from_host(W, R, levels, rtbm::LDS_BUDGET) != 1) return 2;
            std::vector<char> scratch(bytes);
            double total = 0.0, term = 1.0;
            for (uint32_t k = 0; k < levels; k++) total += term, term *= (double)0.7f;
            const float norm = (float)(1.0 / total);
            std::vector<float> first(img.size()), out(img.size()), b(img.size());
            for (uint32_t mode = 0; mode < 2; mode++)
                for (int thresh = 0; thresh < 2; thresh++)
                    for (int second = 0; second < 2; second++) {
                        if (bloom_apply_host(img.data(), W, R, levels, mode, 0.7f, mode ? 2.5f : 0.05f, norm, 65536.0f, thresh ? 1.0f : 0.0f,
                                             thresh ? 0.5f : 0.0f, first.data(), scratch.data(), out.data(), second ? b.data() : nullptr))
                            return 1;
                        for (size_t i = 0; i < img.size(); i++) {
                            const bool inf_in = img[i] == __builtin_inff();
                            if (out[i] != out[i] || !(out[i] >= 0.0f) || (inf_in && out[i] != __builtin_inff()) ||
                                (second && !(b[i] >= 0.0f && b[i] < __builtin_inff()))) {
                                std::printf("bloom_host: %u x %u, %u levels at %zu: in %g out %g\n", W, R, levels, i, (double)img[i], (double)out[i]);
                                return 4;
                            }
                        }
                        bloomed += n;
                    }
        }
        if (bloom_apply_host(img.data(), W, R, 9, 0, 0.7f, 0.05f, 0.5f, 65536.0f, 0, 0, nullptr, nullptr, nullptr, nullptr) != 1) return 1;
    }
    std::printf("bloom_host: %llu pixels bloomed\n", bloomed);
    return 0;
}
#endif
