// rt_history.hip.h — the gfx950 kernel of the film-history library (rt_history.h), wave64, every per-pixel operation
// taken from rt_history_math.h (the lines the CPU harness runs too).
//
// One lane a pixel, 64 x 4 tiles of 256 lanes as the film's resolve: a wave is 64 neighbouring pixels of a row, so the current
// frame's planes are read and the next state's planes written in whole runs (768, 512 and 256 contiguous bytes a wave), and under a
// coherent camera motion the four taps of neighbouring lanes are neighbouring pixels of the previous state.  Out-of-image lanes do
// nothing.  A tap reads the three guard planes first (length, index, z: one dword each) and the colour sums and moments (a 12-byte
// and an 8-byte load) only once it is admitted.  State is film-shaped planes, so next.accum and next.moments ARE the resolve's
// inputs: nothing is written twice (the packed-record form that was measured against this one is in DESIGN.md 4.24 "Measured").
// No atomics, no LDS, no inline assembly.  A tap outside the film is skipped before any address is formed.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_history_math.h"

namespace rthk {

constexpr uint32_t TILE_X = 64, TILE_Y = 4, BLOCK = TILE_X * TILE_Y;

struct State {
    float* accum;
    float* moments;
    float* length;
    float* depth;
    uint32_t* index;
    float* normal;
};

struct Params {
    rthm::Frame f;
    const float* accum;
    const float* moments;
    const float* depth;
    const uint32_t* hits;
    const uint32_t* index;
    const float* normal;
    State prev, next;
};

struct PrevState {
    const State& s;
    __device__ __forceinline__ void guard(size_t i, float& N, uint32_t& index, float& z) const {
        N = s.length[i];
        index = s.index[i];
        z = s.depth[i];
    }
    __device__ __forceinline__ void normal(size_t i, float n[3]) const {
        n[0] = s.normal[3 * i + 0];
        n[1] = s.normal[3 * i + 1];
        n[2] = s.normal[3 * i + 2];
    }
    __device__ __forceinline__ void values(size_t i, float C[3], float M[2]) const {
        C[0] = s.accum[3 * i + 0];
        C[1] = s.accum[3 * i + 1];
        C[2] = s.accum[3 * i + 2];
        const float2 m = reinterpret_cast<const float2*>(s.moments)[i];
        M[0] = m.x;
        M[1] = m.y;
    }
};

__global__ __launch_bounds__(256) void rth_accumulate_kernel(const Params p) {
    const uint32_t x = blockIdx.x * TILE_X + (threadIdx.x & (TILE_X - 1u));
    const uint32_t r = blockIdx.y * TILE_Y + (threadIdx.x / TILE_X);
    if (x >= p.f.W || r >= p.f.R) return;
    const size_t i = (size_t)r * p.f.W + x;
    const float C[3] = {p.accum[3 * i + 0], p.accum[3 * i + 1], p.accum[3 * i + 2]};
    const float2 m = reinterpret_cast<const float2*>(p.moments)[i];
    const float M[2] = {m.x, m.y};
    const uint32_t idx = p.index[i];
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (p.f.normals) {
        n[0] = p.normal[3 * i + 0];
        n[1] = p.normal[3 * i + 1];
        n[2] = p.normal[3 * i + 2];
    }
    float oC[3], oM[2], oN, oZ;
    rthm::accumulate_pixel(p.f, x, r, C, M, p.depth[i], p.hits[i], idx, n, PrevState{p.prev}, rthm::NoCount{}, oC, oM, oN, oZ);
    p.next.accum[3 * i + 0] = oC[0];
    p.next.accum[3 * i + 1] = oC[1];
    p.next.accum[3 * i + 2] = oC[2];
    reinterpret_cast<float2*>(p.next.moments)[i] = make_float2(oM[0], oM[1]);
    p.next.length[i] = oN;
    p.next.depth[i] = oZ;
    p.next.index[i] = idx;
    if (p.f.normals) {
        p.next.normal[3 * i + 0] = n[0];
        p.next.normal[3 * i + 1] = n[1];
        p.next.normal[3 * i + 2] = n[2];
    }
}

}  // namespace rthk
