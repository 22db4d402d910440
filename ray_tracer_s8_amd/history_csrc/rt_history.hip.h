// rt_history.hip.h — the gfx950 kernel of the film-history library (rt_history.h), wave64, every per-pixel operation
// taken from rt_history_math.h (the lines the CPU harness runs too).
//
// One lane a pixel, 64 x 4 tiles of 256 lanes as the film's resolve: a wave is 64 neighbouring pixels of a row, so the current
// frame's planes are read and the next state's planes written in whole runs (768, 512 and 256 contiguous bytes a wave), and under a
// coherent camera motion the four taps of neighbouring lanes are neighbouring pixels of the previous state.  Out-of-image lanes do
// nothing.  A tap reads the three guard planes first (length, index, z: one dword each) and the colour sums and moments (a 12-byte
// and an 8-byte load) only once it is admitted.  State is film-shaped planes, so next.accum and next.moments ARE the resolve's
// inputs: nothing is written twice (the packed-record form that was measured against this one is in DESIGN.md 4.24 "Measured").
// No atomics, no inline assembly, and no LDS but the clip's window (below).  A tap outside the film is skipped before any address is
// formed.
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
    rthm::Clip clip;              // a clipping call only
    float* clip_amount;           // a clipping call only, or NULL
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

// The next state's record of pixel i.
__device__ __forceinline__ void store_pixel(const Params& p, size_t i, const float oC[3], const float oM[2], float oN, float oZ,
                                            uint32_t idx, const float n[3]) {
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

// The staged window of a clipping call: three planes of ROWS rows at a pitch of PITCH dwords, record wy * PITCH + wx.
template <int RHO>
struct Window {
    static constexpr uint32_t PITCH = TILE_X + 2u * RHO, ROWS = TILE_Y + 2u * RHO, RECORDS = PITCH * ROWS;
    const float* plane;           // [3][RECORDS]
    __device__ __forceinline__ void colour(size_t i, bool, float C[3]) const {      // (a record outside the film holds +0)
        C[0] = plane[i];
        C[1] = plane[RECORDS + i];
        C[2] = plane[2u * RECORDS + i];
    }
};

// The window of the direct form: the film's accum itself, record y W + x.  A tap that is not inside loads the centre's record in
// its place (no address outside the film is formed) and yields +0.
struct GlobalWindow {
    const float* accum;
    size_t centre;
    __device__ __forceinline__ void colour(size_t i, bool inside, float C[3]) const {
        const size_t j = inside ? i : centre;
        const float c0 = accum[3 * j + 0], c1 = accum[3 * j + 1], c2 = accum[3 * j + 2];
        C[0] = inside ? c0 : 0.0f;
        C[1] = inside ? c1 : 0.0f;
        C[2] = inside ? c2 : 0.0f;
    }
};

// One pixel of a clipping call, its window given: everything but the colour C of the pixel itself is loaded here.
template <int RHO, class Win>
__device__ __forceinline__ void clip_pixel(const Params& p, uint32_t x, uint32_t r, size_t i, const float C[3], const Win& win,
                                           size_t centre, size_t pitch) {
    const float2 m = reinterpret_cast<const float2*>(p.moments)[i];
    const float M[2] = {m.x, m.y};
    const uint32_t idx = p.index[i];
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (p.f.normals) {
        n[0] = p.normal[3 * i + 0];
        n[1] = p.normal[3 * i + 1];
        n[2] = p.normal[3 * i + 2];
    }
    float oC[3], oM[2], oN, oZ, amount;
    rthm::accumulate_pixel_clip<RHO>(p.f, p.clip, x, r, C, M, p.depth[i], p.hits[i], idx, n, PrevState{p.prev}, win, centre, pitch,
                                     rthm::NoCount{}, rthm::NoCount{}, oC, oM, oN, oZ, amount);
    store_pixel(p, i, oC, oM, oN, oZ, idx, n);
    if (p.clip_amount) p.clip_amount[i] = amount;
}

// RHO = 0: a call without the clip, no LDS and no barrier.  RHO = 1, 2: a clipping call (rt_history.h step 5a), in one of two forms
// that give the same bytes (DESIGN.md 4.26 has their times).
// Staged (DIRECT = false).  The workgroup first stages the (64 + 2 RHO) x (4 + 2 RHO) window of the current frame's accum around
// its tile into LDS, as three planes (one a channel) at a row pitch of 64 + 2 RHO dwords, so the 64 lanes of a wave, which are 64
// neighbouring pixels of a row, read 64 consecutive dwords, one a bank, at every tap.  All 256 lanes stage, those whose own pixel
// lies outside the image too, which is why they leave only behind the barrier.  A record outside the film is not loaded: it is
// staged as +0, which clip_history adds to its sums in the place of skipping the tap (rt_history_math.h says why the bits are the
// same), so a tap costs three LDS reads, two additions and a product a channel and no branch.  4752 and 6528 bytes of LDS a
// workgroup.
// Direct (DIRECT = true).  No LDS and no barrier: every lane reads its window from the film's accum, three dwords a tap at a stride
// of 12 bytes between neighbouring lanes, and leaves the sharing between neighbours to the caches.
template <int RHO, bool DIRECT>
__global__ __launch_bounds__(256) void rth_accumulate_kernel(const Params p) {
    const uint32_t tx = threadIdx.x & (TILE_X - 1u), ty = threadIdx.x / TILE_X;
    const uint32_t x = blockIdx.x * TILE_X + tx;
    const uint32_t r = blockIdx.y * TILE_Y + ty;
    if constexpr (RHO > 0 && !DIRECT) {
        using Win = Window<RHO>;
        __shared__ float window[3u * Win::RECORDS];
        const int bx = (int)(blockIdx.x * TILE_X) - RHO, by = (int)(blockIdx.y * TILE_Y) - RHO;
        for (uint32_t s = threadIdx.x; s < Win::RECORDS; s += BLOCK) {
            const uint32_t wy = s / Win::PITCH, wx = s - wy * Win::PITCH;
            const int gx = bx + (int)wx, gy = by + (int)wy;
            float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
            if (gx >= 0 && gx < (int)p.f.W && gy >= 0 && gy < (int)p.f.R) {
                const size_t j = (size_t)gy * p.f.W + (size_t)gx;
                c0 = p.accum[3 * j + 0];
                c1 = p.accum[3 * j + 1];
                c2 = p.accum[3 * j + 2];
            }
            window[s] = c0;
            window[Win::RECORDS + s] = c1;
            window[2u * Win::RECORDS + s] = c2;
        }
        __syncthreads();
        if (x >= p.f.W || r >= p.f.R) return;
        const Win win{window};
        const size_t centre = (size_t)(ty + RHO) * Win::PITCH + (tx + RHO);
        float C[3];
        win.colour(centre, true, C);
        clip_pixel<RHO>(p, x, r, (size_t)r * p.f.W + x, C, win, centre, (size_t)Win::PITCH);
    } else if constexpr (RHO > 0) {
        if (x >= p.f.W || r >= p.f.R) return;
        const size_t i = (size_t)r * p.f.W + x;
        const float C[3] = {p.accum[3 * i + 0], p.accum[3 * i + 1], p.accum[3 * i + 2]};
        clip_pixel<RHO>(p, x, r, i, C, GlobalWindow{p.accum, i}, i, (size_t)p.f.W);
    } else {
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
        store_pixel(p, i, oC, oM, oN, oZ, idx, n);
    }
}

}  // namespace rthk
