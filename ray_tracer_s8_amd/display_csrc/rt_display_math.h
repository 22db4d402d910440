// rt_display_math.h — the per-pixel and per-histogram arithmetic of the display library (rt_display.h): the bin of a
// luminance, the exposure record from the two bins a histogram's percentiles fall into, the tone curves and the two quantisations.
// Plain C++ that compiles as HIP device code (rt_display.hip.h) and under g++ -ffp-contract=off (tests/host/display_host.cpp), so the
// kernels and the CPU harness run the same lines.  Every operation is one IEEE f32 rounding in the order rt_display.h writes it: no
// fused multiply-add, correctly rounded division and square root, no transcendental function.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HOST_DEVICE __host__ __device__ inline
#else
#define RT_HOST_DEVICE inline
#endif

namespace rtdm {

constexpr uint32_t BINS = 256u, HIST_WORDS = 257u, EXCLUDED = 256u, RECORD_WORDS = 8u;
constexpr uint32_t BIN_BASE = 888u;               // (127 - 16) << 3: the q of 2^-16
constexpr uint32_t MODE_AUTO = 0u, MODE_MANUAL = 1u;
constexpr uint32_t CURVE_NONE = 0u, CURVE_REINHARD = 1u, CURVE_FILMIC = 2u;
constexpr uint32_t MAX_Q16 = 65535u;

RT_HOST_DEVICE uint32_t bits_of(float x) { return __builtin_bit_cast(uint32_t, x); }
RT_HOST_DEVICE float float_of(uint32_t u) { return __builtin_bit_cast(float, u); }

// ---- metering -----------------------------------------------------------------------------------------------------------------------
RT_HOST_DEVICE float luminance(float c0, float c1, float c2) { return (c0 + c1) + c2; }

// the histogram word of a luminance: 0 ... 255, or EXCLUDED for a NaN, a zero and a negative
RT_HOST_DEVICE uint32_t bin_of(float y) {
    if (y != y || !(y > 0.0f)) return EXCLUDED;
    const uint32_t q = bits_of(y) >> 20;
    const uint32_t b = q < BIN_BASE ? 0u : q - BIN_BASE;
    return b < BINS - 1u ? b : BINS - 1u;
}

// ---- exposure -----------------------------------------------------------------------------------------------------------------------
struct Record {
    float scale, white, target;
    uint32_t bin_key, bin_white, counted, excluded, frames;
};
static_assert(sizeof(Record) == 4 * RECORD_WORDS, "eight 32-bit words");

// what is uniform over an rtd_expose
struct Exposure {
    uint32_t mode;
    float key;
    uint32_t key_q16, white_q16;
    float rate, scale_min, scale_max;
    float scale, white;           // MODE_MANUAL
};

RT_HOST_DEVICE bool finite_positive(float v) { return v > 0.0f && v < __builtin_inff(); }

// what the host refuses of an Exposure
RT_HOST_DEVICE bool exposure_ok(const Exposure& e) {
    if (e.mode == MODE_MANUAL) return e.scale > 0.0f && e.white >= 1.0f;        // (a NaN fails both; +inf passes)
    if (e.mode != MODE_AUTO) return false;
    if (!finite_positive(e.key) || !finite_positive(e.rate) || !finite_positive(e.scale_min) || !finite_positive(e.scale_max)) return false;
    if (e.scale_min > e.scale_max || e.rate > 1.0f) return false;
    return e.key_q16 <= MAX_Q16 && e.white_q16 <= MAX_Q16 && e.white_q16 >= e.key_q16;
}

// the rank of a percentile among N counted pixels: below N whenever N > 0
RT_HOST_DEVICE uint32_t rank_of(uint32_t N, uint32_t q16) { return (uint32_t)(((uint64_t)N * q16) >> 16); }

// the middle of bin b
RT_HOST_DEVICE float rep(uint32_t b) { return float_of(((b + BIN_BASE) << 20) | 0x80000u); }

RT_HOST_DEVICE uint32_t next_frame(uint32_t frames) { return frames == 0xffffffffu ? frames : frames + 1u; }

// The record after a metered frame: N counted pixels, the two bins the percentiles fall into (anything where N == 0).
RT_HOST_DEVICE Record auto_record(const Exposure& e, const Record& prev, uint32_t N, uint32_t excluded, uint32_t bin_key, uint32_t bin_white) {
    Record r = prev;
    if (N == 0u) {
        r.bin_key = r.bin_white = 0u;
        if (prev.frames == 0u) r.scale = 1.0f, r.white = __builtin_inff(), r.target = 1.0f;
    } else {
        float target = e.key / rep(bin_key);
        target = target < e.scale_min ? e.scale_min : target;
        target = target < e.scale_max ? target : e.scale_max;
        float scale = target;
        if (!(prev.frames == 0u || e.rate >= 1.0f)) {
            const float d = target - prev.scale;
            scale = prev.scale + e.rate * d;
        }
        float white = (rep(bin_white) * scale) / 3.0f;
        white = white > 1.0f ? white : 1.0f;
        r.scale = scale, r.white = white, r.target = target;
        r.bin_key = bin_key, r.bin_white = bin_white;
    }
    r.counted = N, r.excluded = excluded;
    r.frames = next_frame(prev.frames);
    return r;
}

RT_HOST_DEVICE Record manual_record(const Exposure& e, const Record& prev) {
    Record r = prev;
    r.scale = e.scale, r.white = e.white, r.target = e.scale;
    r.bin_key = r.bin_white = 0u;
    r.frames = next_frame(prev.frames);
    return r;
}

// ---- display ------------------------------------------------------------------------------------------------------------------------
// steps 1 and 2: t of a channel value under the record's scale and w2 = white white
template <uint32_t CURVE>
RT_HOST_DEVICE float tone(float c, float scale, float w2) {
    static_assert(CURVE <= CURVE_FILMIC, "one of the three curves");
    float x = c * scale;
    x = x > 0.0f ? x : 0.0f;
    if (CURVE == CURVE_NONE) return x;
    float t;
    if (CURVE == CURVE_REINHARD) {
        t = (x * (1.0f + x / w2)) / (1.0f + x);
    } else {
        const float n = x * (2.51f * x + 0.03f);
        const float d = x * (2.43f * x + 0.59f) + 0.14f;
        t = n / d;
    }
    return t < 1.0f ? t : 1.0f;
}

// step 3
template <uint32_t CURVE>
RT_HOST_DEVICE float display_value(float c, float scale, float w2) { return __builtin_sqrtf(tone<CURVE>(c, scale, w2)); }

// Rust `as u8` from f32 (the tile's): truncate, saturate, NaN -> 0
RT_HOST_DEVICE uint8_t as_u8(float v) {
    if (!(v == v)) return 0;
    if (v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)(int)v;
}

// B[row & 3][col & 3] of the 4 x 4 Bayer matrix {0, 8, 2, 10; 12, 4, 14, 6; 3, 11, 1, 9; 15, 7, 13, 5}: entry 4 r + c is nibble 4 r + c
// of one 64-bit constant, so there is no table to index
constexpr uint64_t BAYER_NIBBLES = 0x5D7F91B36E4CA280ull;
RT_HOST_DEVICE uint32_t bayer(uint32_t row, uint32_t col) { return (uint32_t)(BAYER_NIBBLES >> (16u * (row & 3u) + 4u * (col & 3u))) & 15u; }

// what the dither adds ahead of the truncation: ((float)B + 0.5f) / 16, exact
RT_HOST_DEVICE float dither_offset(uint32_t row, uint32_t col) { return ((float)bayer(row, col) + 0.5f) / 16.0f; }

// step 4
RT_HOST_DEVICE uint8_t quantise(float f) { return as_u8(f * 255.999f); }
RT_HOST_DEVICE uint8_t quantise_dithered(float f, float offset) { return as_u8(f * 255.0f + offset); }

}  // namespace rtdm
