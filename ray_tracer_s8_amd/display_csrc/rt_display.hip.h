// rt_display.hip.h — the gfx950 kernels of the display library (rt_display.h), wave64, every per-pixel and
// per-histogram operation taken from rt_display_math.h (the lines the CPU harness runs too).  No inline assembly; every address comes
// from the sizes alone, and a histogram index is at most 256 by bin_of's clamp.
//
// rtd_meter_kernel<FORM>: blocks of 1 024 lanes; a block takes a chunk of 4 096 neighbouring pixels a trip, a lane four of them 1 024
//   apart, loaded before any is counted, and at most MAX_GRID blocks, one a compute unit, stride over the image, so that a trip is
//   uniform over the block and its waves can vote.  (Blocks of 256 lanes under a grid of 1 024 took twice as long: what a block adds
//   to the caller's words at its end is serialised per word, and there were four times as many blocks: DESIGN.md 4.30.)  A lane past the end loads
//   the last pixel and counts nothing.  A wave counts into an LDS histogram of its own (257 words), so waves never meet on a word.
//   RTD_HIST_WAVE: one LDS atomic add a pixel.  RTD_HIST_MATCH: the lanes of a wave that hold the first unserved lane's bin are found
//   with one ballot and served with one add of their number, until no lane is left: one add a wave for a constant image, up to 64
//   rounds for noise.  At the end the sixteen histograms are summed, and the block adds every non-empty word to the caller's with one
//   global integer atomic: integer adds commute, so the counts are deterministic.
// rtd_expose_kernel: one block of 256 lanes, a bin each.  The inclusive scan runs in the wave by shifts and across the four waves
//   through LDS; the lane whose bin holds a percentile's rank (exclusive sum <= rank < inclusive sum: exactly one lane where N > 0)
//   posts its bin in LDS; lane 0 reads the record, takes the record's lines and writes the eight words with plain vector stores.
// rtd_apply_kernel<CURVE, DITHER>: the arithmetic is per channel, so the image is a flat float array and a lane takes a group of four
//   floats: one 16-byte load, one 16-byte store of out_f32, one 4-byte store of out_rgb.  Only the dither needs the pixel: a group
//   lies in at most two neighbouring pixels, the first of which is g + g div 3 for group g.  The lane of the last, partial group
//   works float by float.  The record is read through a uniform address.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_display_math.h"

namespace rtdk {

constexpr uint32_t BLOCK = 256, WAVES = BLOCK / 64;
// the meter's blocks: 16 waves, so that one block a compute unit fills it and a histogram word takes at most MAX_GRID global adds
constexpr uint32_t METER_BLOCK = 1024, METER_WAVES = METER_BLOCK / 64;
constexpr uint32_t PER_LANE = 4, CHUNK = METER_BLOCK * PER_LANE;
constexpr uint32_t MAX_GRID = 256;                // a block a compute unit: a trip of 1 048 576 pixels
constexpr uint32_t FORM_WAVE = 0u, FORM_MATCH = 1u;

struct MeterParams {
    uint32_t pixels;
    const float* linear;
    uint32_t* hist;
};

template <uint32_t FORM>
__global__ __launch_bounds__(1024) void rtd_meter_kernel(const MeterParams p) {
    __shared__ uint32_t h[METER_WAVES * rtdm::HIST_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t* mine = h + (tid >> 6) * rtdm::HIST_WORDS;
    for (uint32_t w = tid; w < METER_WAVES * rtdm::HIST_WORDS; w += METER_BLOCK) h[w] = 0u;
    __syncthreads();
    const uint32_t stride = gridDim.x * CHUNK;
    for (uint32_t base = blockIdx.x * CHUNK; base < p.pixels; base += stride) {       // (base < 2^31 and stride <= 2^20: no wrap)
        uint32_t bin[PER_LANE];
        bool valid[PER_LANE];
#pragma unroll
        for (uint32_t k = 0; k < PER_LANE; k++) {
            const uint32_t i = base + k * METER_BLOCK + tid;
            valid[k] = i < p.pixels;
            const float* c = p.linear + 3u * (size_t)(valid[k] ? i : p.pixels - 1u);
            bin[k] = rtdm::bin_of(rtdm::luminance(c[0], c[1], c[2]));
        }
#pragma unroll
        for (uint32_t k = 0; k < PER_LANE; k++) {
            if (FORM == FORM_WAVE) {
                if (valid[k]) atomicAdd(mine + bin[k], 1u);
            } else {
                unsigned long long todo = __ballot(valid[k]);
                while (todo != 0ull) {                                                  // uniform over the wave
                    const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
                    const uint32_t served = (uint32_t)__builtin_amdgcn_readlane((int)bin[k], (int)leader);
                    const unsigned long long same = __ballot(valid[k] && bin[k] == served) & todo;
                    if (lane == leader) atomicAdd(mine + served, (uint32_t)__popcll(same));
                    todo &= ~same;
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t w = tid; w < rtdm::HIST_WORDS; w += METER_BLOCK) {
        uint32_t s = 0u;
        for (uint32_t k = 0; k < METER_WAVES; k++) s += h[k * rtdm::HIST_WORDS + w];
        if (s != 0u) atomicAdd(p.hist + w, s);
    }
}

struct ExposeParams {
    rtdm::Exposure e;
    const uint32_t* hist;
    uint32_t* record;
};

__device__ __forceinline__ rtdm::Record load_record(const uint32_t* w) {
    rtdm::Record r;
    r.scale = rtdm::float_of(w[0]), r.white = rtdm::float_of(w[1]), r.target = rtdm::float_of(w[2]);
    r.bin_key = w[3], r.bin_white = w[4], r.counted = w[5], r.excluded = w[6], r.frames = w[7];
    return r;
}

__device__ __forceinline__ void store_record(uint32_t* w, const rtdm::Record& r) {
    w[0] = rtdm::bits_of(r.scale), w[1] = rtdm::bits_of(r.white), w[2] = rtdm::bits_of(r.target);
    w[3] = r.bin_key, w[4] = r.bin_white, w[5] = r.counted, w[6] = r.excluded, w[7] = r.frames;
}

__global__ __launch_bounds__(256) void rtd_expose_kernel(const ExposeParams p) {
    __shared__ uint32_t wave_sum[WAVES];
    __shared__ uint32_t found[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (p.e.mode == rtdm::MODE_MANUAL) {                                               // (uniform: the whole block leaves)
        if (tid == 0u) store_record(p.record, rtdm::manual_record(p.e, load_record(p.record)));
        return;
    }
    const uint32_t own = p.hist[tid];
    uint32_t c = own;
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t below = (uint32_t)__shfl_up((int)c, d);
        if (lane >= d) c += below;
    }
    if (lane == 63u) wave_sum[wave] = c;
    if (tid < 2u) found[tid] = 0u;
    __syncthreads();
    uint32_t before = 0u, N = 0u;
#pragma unroll
    for (uint32_t k = 0; k < WAVES; k++) {
        const uint32_t s = wave_sum[k];
        before += k < wave ? s : 0u;
        N += s;
    }
    c += before;
    const uint32_t first = c - own;                                                    // the exclusive sum
    const uint32_t t_key = rtdm::rank_of(N, p.e.key_q16), t_white = rtdm::rank_of(N, p.e.white_q16);
    if (first <= t_key && t_key < c) found[0] = tid;
    if (first <= t_white && t_white < c) found[1] = tid;
    __syncthreads();
    if (tid == 0u)
        store_record(p.record, rtdm::auto_record(p.e, load_record(p.record), N, p.hist[rtdm::EXCLUDED], found[0], found[1]));
}

struct ApplyParams {
    uint32_t W;
    uint32_t groups;              // ceil(floats / 4)
    uint64_t floats;              // 3 R W
    const float* linear;
    const uint32_t* record;
    float* out_f32;
    uint8_t* out_rgb;
};

template <uint32_t CURVE, bool DITHER>
__global__ __launch_bounds__(256) void rtd_apply_kernel(const ApplyParams p) {
    const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= p.groups) return;
    const float scale = rtdm::float_of(p.record[0]), white = rtdm::float_of(p.record[1]);
    const float w2 = white * white;
    // the pixels of the group's floats: float 4 g is channel g mod 3 of pixel g + g div 3, and float 4 g + j lies in the next pixel
    // once g mod 3 + j reaches 3
    const uint32_t third = g / 3u, ch = g - 3u * third;
    float o0 = 0.0f, o1 = 0.0f;
    if (DITHER) {
        const uint32_t pixel = g + third, row = pixel / p.W, col = pixel - row * p.W;
        const bool wraps = col + 1u == p.W;
        o0 = rtdm::dither_offset(row, col);
        o1 = rtdm::dither_offset(wraps ? row + 1u : row, wraps ? 0u : col + 1u);
    }
    const uint64_t at = 4ull * g;
    if (at + 4u <= p.floats) {
        const float4 v = reinterpret_cast<const float4*>(p.linear)[g];
        const float c[4] = {v.x, v.y, v.z, v.w};
        float f[4];
        uint32_t bytes = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            f[j] = rtdm::display_value<CURVE>(c[j], scale, w2);
            const uint8_t b = DITHER ? rtdm::quantise_dithered(f[j], ch + j >= 3u ? o1 : o0) : rtdm::quantise(f[j]);
            bytes |= (uint32_t)b << (8u * j);
        }
        if (p.out_f32) reinterpret_cast<float4*>(p.out_f32)[g] = make_float4(f[0], f[1], f[2], f[3]);
        if (p.out_rgb) reinterpret_cast<uint32_t*>(p.out_rgb)[g] = bytes;
    } else {
        const uint32_t left = (uint32_t)(p.floats - at);                                // 1 ... 3 floats of the last group
        for (uint32_t j = 0; j < left; j++) {
            const float f = rtdm::display_value<CURVE>(p.linear[at + j], scale, w2);
            if (p.out_f32) p.out_f32[at + j] = f;
            if (p.out_rgb) p.out_rgb[at + j] = DITHER ? rtdm::quantise_dithered(f, ch + j >= 3u ? o1 : o0) : rtdm::quantise(f);
        }
    }
}

}  // namespace rtdk
