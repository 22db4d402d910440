// Test harness (CPU only, built by tests/test_display_host.py with g++ -ffp-contract=off): the three calls of the display library
// (display_csrc/rt_display.h) run with the product's own per-pixel and per-histogram lines (display_csrc/rt_display_math.h) over plain
// arrays.  With -DDISPLAY_HOST_MAIN it is a stand-alone program (its own main) that meters, exposes and applies exactly sized images
// that hold extreme values too, for a sanitizer build.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rt_display_math.h"

namespace {

template <uint32_t CURVE>
void apply(const float* img, uint32_t W, uint32_t R, float scale, float white, bool dither, float* t, float* f, uint8_t* rgb) {
    const float w2 = white * white;
    for (uint32_t row = 0; row < R; row++)
        for (uint32_t col = 0; col < W; col++)
            for (uint32_t c = 0; c < 3; c++) {
                const size_t at = 3 * ((size_t)row * W + col) + c;
                const float v = rtdm::display_value<CURVE>(img[at], scale, w2);
                if (t) t[at] = rtdm::tone<CURVE>(img[at], scale, w2);
                if (f) f[at] = v;
                if (rgb) rgb[at] = dither ? rtdm::quantise_dithered(v, rtdm::dither_offset(row, col)) : rtdm::quantise(v);
            }
}

}  // namespace

extern "C" {

// bin_of over n luminances: 0 ... 255, or 256 for the excluded.
void display_bins_host(const float* y, uint32_t n, uint32_t* bin) {
    for (uint32_t i = 0; i < n; i++) bin[i] = rtdm::bin_of(y[i]);
}

// rtd_meter over n pixels [n][3]: H[257] cleared and counted.
void display_meter_host(const float* img, uint32_t n, uint32_t* H) {
    for (uint32_t w = 0; w < rtdm::HIST_WORDS; w++) H[w] = 0;
    for (uint32_t i = 0; i < n; i++) H[rtdm::bin_of(rtdm::luminance(img[3 * (size_t)i], img[3 * (size_t)i + 1], img[3 * (size_t)i + 2]))]++;
}

// rtd_expose: the record's eight words read and written.  Returns 0, or 1 for arguments the library refuses.  The scan and the two
// searches are the definition's (the kernel's run in parallel); the record's lines are the product's.
int display_expose_host(const uint32_t* H, uint32_t* record, uint32_t mode, float key, uint32_t key_q16, uint32_t white_q16, float rate,
                        float scale_min, float scale_max, float scale, float white) {
    const rtdm::Exposure e = {mode, key, key_q16, white_q16, rate, scale_min, scale_max, scale, white};
    if (!rtdm::exposure_ok(e)) return 1;
    rtdm::Record prev;
    prev.scale = rtdm::float_of(record[0]), prev.white = rtdm::float_of(record[1]), prev.target = rtdm::float_of(record[2]);
    prev.bin_key = record[3], prev.bin_white = record[4], prev.counted = record[5], prev.excluded = record[6], prev.frames = record[7];
    rtdm::Record r;
    if (mode == rtdm::MODE_MANUAL) {
        r = rtdm::manual_record(e, prev);
    } else {
        uint32_t N = 0;
        for (uint32_t b = 0; b < rtdm::BINS; b++) N += H[b];
        const uint32_t t[2] = {rtdm::rank_of(N, key_q16), rtdm::rank_of(N, white_q16)};
        uint32_t found[2] = {0, 0};
        for (int k = 0; k < 2; k++) {
            uint32_t cum = 0;
            for (uint32_t b = 0; b < rtdm::BINS; b++) {
                cum += H[b];
                if (cum > t[k]) {
                    found[k] = b;
                    break;
                }
            }
        }
        r = rtdm::auto_record(e, prev, N, H[rtdm::EXCLUDED], found[0], found[1]);
    }
    record[0] = rtdm::bits_of(r.scale), record[1] = rtdm::bits_of(r.white), record[2] = rtdm::bits_of(r.target);
    record[3] = r.bin_key, record[4] = r.bin_white, record[5] = r.counted, record[6] = r.excluded, record[7] = r.frames;
    return 0;
}

// rtd_apply over an image [R][W][3] under (scale, white): t (steps 1 and 2), f (step 3) and rgb (step 4), each written unless NULL.
// Returns 0, or 1 for a curve the library refuses.
int display_apply_host(const float* img, uint32_t W, uint32_t R, uint32_t curve, uint32_t dither, float scale, float white, float* t,
                       float* f, uint8_t* rgb) {
    switch (curve) {
        case rtdm::CURVE_NONE: apply<rtdm::CURVE_NONE>(img, W, R, scale, white, dither != 0, t, f, rgb); return 0;
        case rtdm::CURVE_REINHARD: apply<rtdm::CURVE_REINHARD>(img, W, R, scale, white, dither != 0, t, f, rgb); return 0;
        case rtdm::CURVE_FILMIC: apply<rtdm::CURVE_FILMIC>(img, W, R, scale, white, dither != 0, t, f, rgb); return 0;
        default: return 1;
    }
}
}

#ifdef DISPLAY_HOST_MAIN
// Images of 9 x 70 and 5 x 37 in exactly sized buffers: seeded values over 2^-20 ... 2^20 with subnormal, huge, negative and
// non-finite values (the classes of tests/_extreme_planes.py) written over some.  Each is metered (the counts sum to the pixels),
// exposed five times at rate 0.25 from a fresh record, then under manual values, and applied under every curve with and without
// dither: whatever the image holds, no line reads or writes outside its buffer, and no conversion is undefined.
int main() {
    uint32_t lcg = 2463534242u;
    auto rnd = [&] { return (float)((lcg = lcg * 1664525u + 1013904223u) >> 8) / 16777216.0f; };
    const float special[] = {1e-45f, -1e-45f, 5.9e-39f, 1.1754942e-38f, -0.0f, 0.0f, 1e-30f, 1.9e19f, 3e38f, 3.4028235e38f, -3.4028235e38f,
                             __builtin_inff(), -__builtin_inff(), __builtin_nanf(""), -__builtin_nanf(""), -1.5f, 65536.0f, 61440.0f};
    const size_t n_special = sizeof special / sizeof *special;
    unsigned long long shown = 0;
    const uint32_t sizes[2][2] = {{70, 9}, {37, 5}};
    for (const auto& size : sizes) {
        const uint32_t W = size[0], R = size[1], n = W * R;
        std::vector<float> img((size_t)n * 3);
        for (float& v : img) {
            const float e = 40.0f * rnd() - 20.0f;
            v = (rnd() < 0.1f ? -1.0f : 1.0f) * __builtin_ldexpf(1.0f + rnd(), (int)e);
        }
        for (size_t j = 0; j < 4 * n_special; j++) img[(7 * j + 3) % img.size()] = special[j % n_special];
        for (size_t j = 0; j < n_special; j++)                                                 // and whole pixels of them
            for (int c = 0; c < 3; c++) img[3 * ((size_t)n - 1 - j) + c] = special[j];
        std::vector<uint32_t> H(rtdm::HIST_WORDS);
        display_meter_host(img.data(), n, H.data());
        uint64_t sum = 0;
        for (uint32_t h : H) sum += h;
        if (sum != n) {
            std::printf("display_host: %u x %u: the counts sum to %llu\n", W, R, (unsigned long long)sum);
            return 2;
        }
        std::vector<uint32_t> rec = {0x3F800000u, 0x7F800000u, 0x3F800000u, 0, 0, 0, 0, 0};
        for (int frame = 0; frame < 5; frame++) {
            if (display_expose_host(H.data(), rec.data(), rtdm::MODE_AUTO, 0.54f, 32768, 64880, 0.25f, 1.0f / 256, 256.0f, 0, 0)) return 1;
            if (rec[7] != (uint32_t)frame + 1 || rec[3] > 255 || rec[4] > 255 || rec[4] < rec[3]) return 3;
        }
        std::vector<float> t(img.size()), f(img.size());
        std::vector<uint8_t> rgb(img.size());
        for (int manual = 0; manual < 3; manual++) {
            if (manual && display_expose_host(nullptr, rec.data(), rtdm::MODE_MANUAL, 0, 0, 0, 0, 0, 0, manual == 1 ? 0.37f : __builtin_inff(),
                                              manual == 1 ? 4.0f : __builtin_inff()))
                return 1;
            for (uint32_t curve = 0; curve < 3; curve++)
                for (uint32_t dither = 0; dither < 2; dither++) {
                    if (display_apply_host(img.data(), W, R, curve, dither, rtdm::float_of(rec[0]), rtdm::float_of(rec[1]), t.data(), f.data(),
                                           rgb.data()))
                        return 1;
                    for (size_t i = 0; i < img.size(); i++)
                        if (t[i] != t[i] || f[i] != f[i] || (curve != rtdm::CURVE_NONE && !(t[i] >= 0.0f && t[i] <= 1.0f))) {
                            std::printf("display_host: curve %u at %zu: t %g\n", curve, i, (double)t[i]);
                            return 4;
                        }
                    shown += n;
                }
        }
        if (display_apply_host(img.data(), W, R, 3, 0, 1.0f, 1.0f, nullptr, nullptr, rgb.data()) != 1) return 1;
    }
    std::printf("display_host: %llu pixels shown\n", shown);
    return 0;
}
#endif
