// rt_upsample.hip.h — the gfx950 kernel of the film-upsampler library (rt_upsample.h), wave64, every per-pixel
// operation taken from rt_upsample_math.h (the lines the CPU harness runs too).
//
// One lane an output pixel, 64 x 4 tiles of 256 lanes as the film's resolve and the history: a wave is 64 neighbouring pixels of an
// output row, so the high side's guides are read once a pixel and out_linear and out_f32 written in whole runs (768 contiguous bytes
// a wave for a three-float plane, 256 for a dword plane), and the taps of neighbouring lanes are the same or neighbouring records of
// the low film: of the 64 lanes of a wave about 64 / s + 1 distinct columns of two low rows are touched, each record by about four
// of the s^2 output pixels it covers, and the sharing is left to the caches (the direct form; DESIGN.md 4.27 says why no staged form
// is kept).  The plane set is the template argument: no lane tests a plane pointer.  The four outputs are tested, once a lane, on
// kernel arguments, which are uniform.  out_rgb is three byte stores a lane, as the denoiser's.  No LDS, no barrier, no atomics, no
// inline assembly.  Out-of-image lanes do nothing; every tap address is clamped into the low film.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_upsample_math.h"

namespace rtuk {

constexpr uint32_t TILE_X = 64, TILE_Y = 4, BLOCK = TILE_X * TILE_Y;

struct Side {
    const float* albedo;
    const float* normal;
    const float* depth;
    const uint32_t* hits;
    const uint32_t* index;
};

struct Params {
    rtum::Frame f;
    const float* linear;
    Side lo, hi;
    float* out_linear;
    float* out_f32;
    uint8_t* out_rgb;
    uint8_t* out_class;
};

struct LowFilm {
    const float* linear;
    const Side& s;
    __device__ __forceinline__ void colour(size_t i, float L[3]) const {
        L[0] = linear[3 * i + 0];
        L[1] = linear[3 * i + 1];
        L[2] = linear[3 * i + 2];
    }
    __device__ __forceinline__ void albedo(size_t i, float A[3]) const {
        A[0] = s.albedo[3 * i + 0];
        A[1] = s.albedo[3 * i + 1];
        A[2] = s.albedo[3 * i + 2];
    }
    __device__ __forceinline__ void normal(size_t i, float n[3]) const {
        n[0] = s.normal[3 * i + 0];
        n[1] = s.normal[3 * i + 1];
        n[2] = s.normal[3 * i + 2];
    }
    __device__ __forceinline__ float depth(size_t i) const { return s.depth[i]; }
    __device__ __forceinline__ uint32_t hits(size_t i) const { return s.hits[i]; }
    __device__ __forceinline__ uint32_t index(size_t i) const { return s.index[i]; }
};

template <uint32_t PLANES>
__global__ __launch_bounds__(256) void rtu_upsample_kernel(const Params p) {
    const uint32_t tx = threadIdx.x & (TILE_X - 1u), ty = threadIdx.x / TILE_X;
    const uint32_t x = blockIdx.x * TILE_X + tx;
    const uint32_t r = blockIdx.y * TILE_Y + ty;
    if (x >= p.f.Wh || r >= p.f.Rh) return;
    const size_t i = (size_t)r * p.f.Wh + x;
    rtum::Guide g = {};
    if constexpr ((PLANES & rtum::P_ALBEDO) != 0) {
        g.A[0] = p.hi.albedo[3 * i + 0];
        g.A[1] = p.hi.albedo[3 * i + 1];
        g.A[2] = p.hi.albedo[3 * i + 2];
    }
    if constexpr ((PLANES & rtum::P_NORMAL) != 0) {
        g.n[0] = p.hi.normal[3 * i + 0];
        g.n[1] = p.hi.normal[3 * i + 1];
        g.n[2] = p.hi.normal[3 * i + 2];
    }
    if constexpr ((PLANES & rtum::P_DEPTH) != 0) g.D = p.hi.depth[i];
    if constexpr ((PLANES & rtum::P_HITS) != 0) g.hits = p.hi.hits[i];
    if constexpr ((PLANES & rtum::P_INDEX) != 0) g.index = p.hi.index[i];
    float V[3];
    uint32_t cls;
    rtum::gather_pixel<PLANES>(p.f, x, r, g, LowFilm{p.linear, p.lo}, rtum::NoCount{}, V, cls);
    float lin[3], f32[3];
    uint8_t rgb[3];
    rtum::exit_pixel<PLANES>(p.f, g, V, lin, f32, rgb);
    if (p.out_linear) {
        p.out_linear[3 * i + 0] = lin[0];
        p.out_linear[3 * i + 1] = lin[1];
        p.out_linear[3 * i + 2] = lin[2];
    }
    if (p.out_f32) {
        p.out_f32[3 * i + 0] = f32[0];
        p.out_f32[3 * i + 1] = f32[1];
        p.out_f32[3 * i + 2] = f32[2];
    }
    if (p.out_rgb) {
        p.out_rgb[3 * i + 0] = rgb[0];
        p.out_rgb[3 * i + 1] = rgb[1];
        p.out_rgb[3 * i + 2] = rgb[2];
    }
    if (p.out_class) p.out_class[i] = (uint8_t)cls;
}

}  // namespace rtuk
