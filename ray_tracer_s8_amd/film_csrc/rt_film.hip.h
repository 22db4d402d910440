// rt_film.hip.h — the gfx950 kernels of the film library (rt_film.h), wave64, every per-pixel operation taken from
// rt_film_math.h (the lines the CPU harness runs too).
//
//   - fold: a lane per pixel of a strip walks its own 12 n contiguous bytes of records in order and adds them to the pixel's running
//     sums.  A wave's 64 rows are one contiguous 768 n bytes, so every cache line fetched is used whole; a form that staged a
//     workgroup's records in LDS with coalesced loads first was written, measured and dropped (DESIGN.md 4.23 "Measured");
//   - entry: r0 and v0 of each pixel as one float4 record, and the packed guide, into the caller's scratch;
//   - step<LDS, FINAL>: one iteration on the pattern of csrc/rt_denoise.hip.h, 64 x 4 tiles, the (64 + 4s) x (4 + 4s) window of
//     records (and guides) staged in LDS or each tap a float4 load; the prefilter's distance-1 taps lie inside the window for every
//     s >= 1.  FINAL writes the outputs itself;
//   - output: iterations == 0 — r0, v0 to the outputs.
// The film's planes are whole-frame contiguous: one pointer per plane.  Taps outside P are skipped before any load, so no lane reads
// outside the image; out-of-image lanes of a tile only help stage.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_consts.h"
#include "rt_denoise_math.h"
#include "rt_film_math.h"

namespace rtfk {

constexpr uint32_t BLOCK = 256;

__global__ __launch_bounds__(256) void rtf_fold_kernel(const float* __restrict__ rec, uint64_t P, uint32_t n, float* __restrict__ accum,
                                                       float* __restrict__ mom) {
    const uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    float acc[3] = {accum[p * 3 + 0], accum[p * 3 + 1], accum[p * 3 + 2]};
    float mo[2] = {mom[p * 2 + 0], mom[p * 2 + 1]};
    rtfm::fold_pixel(rec + p * n * 3u, n, acc, mo);
    accum[p * 3 + 0] = acc[0];
    accum[p * 3 + 1] = acc[1];
    accum[p * 3 + 2] = acc[2];
    mom[p * 2 + 0] = mo[0];
    mom[p * 2 + 1] = mo[1];
}

struct ResolveParams {
    uint32_t W, R;               // the image P
    uint32_t planes;             // rtdn::P_NORMAL | P_DEPTH | P_HITS of the call
    uint32_t s;                  // step kernel: the step 2^i
    float e_f;                   // samples as a float
    float sigma_l, var_eps, kn, kd;
    const float* accum;          // [R*W*3]
    const float* moments;        // [R*W*2]
    const float* normal;         // [R*W*3] or nullptr
    const float* depth;          // [R*W]
    const uint32_t* hits;        // [R*W]
    float4* guide;               // [W*R] scratch
    const float4* src;           // [W*R] the records read
    float4* dst;                 // [W*R] the records written (entry, non-final steps)
    uint8_t* rgb;                // outputs or nullptr
    float* f32;
    float* lin;
    float* var;
};

__global__ __launch_bounds__(256) void rtf_entry_kernel(const ResolveParams p) {
    const uint64_t total = (uint64_t)p.R * p.W;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (uint64_t)gridDim.x * blockDim.x) {
        const float C[3] = {p.accum[g * 3 + 0], p.accum[g * 3 + 1], p.accum[g * 3 + 2]};
        float r[3];
        rtdn::entry_color(C, p.e_f, nullptr, r);
        const float v = rtfm::entry_variance(p.moments[g * 2 + 0], p.moments[g * 2 + 1], p.e_f);
        p.dst[g] = make_float4(r[0], r[1], r[2], v);
        if (p.planes & (rtdn::P_NORMAL | rtdn::P_DEPTH | rtdn::P_HITS)) {
            float N[3] = {0.0f, 0.0f, 0.0f};
            if (p.planes & rtdn::P_NORMAL) {
                N[0] = p.normal[g * 3 + 0];
                N[1] = p.normal[g * 3 + 1];
                N[2] = p.normal[g * 3 + 2];
            }
            float D = 0.0f;
            uint32_t hits = 0;
            if (p.planes & rtdn::P_DEPTH) D = p.depth[g];
            if (p.planes & rtdn::P_HITS) hits = p.hits[g];
            const rtdn::Guide gd = rtdn::entry_guide((p.planes & rtdn::P_NORMAL) ? N : nullptr, (p.planes & rtdn::P_DEPTH) ? &D : nullptr,
                                                     (p.planes & rtdn::P_HITS) ? &hits : nullptr);
            p.guide[g] = make_float4(gd.nx, gd.ny, gd.nz, gd.zg);
        }
    }
}

// the outputs of pixel g from its final record
__device__ __forceinline__ void rtf_write(const ResolveParams& p, size_t g, const float r[4]) {
    rtdn::output_pixel(r, nullptr, p.lin ? p.lin + g * 3 : nullptr, p.f32 ? p.f32 + g * 3 : nullptr, p.rgb ? p.rgb + g * 3 : nullptr);
    if (p.var) p.var[g] = r[3];
}

// One iteration: a workgroup per 64 x 4 tile of the image, in a 1-D grid (tiles_x per row of tiles).
template <bool LDS, bool FINAL>
__global__ __launch_bounds__(256) void rtf_step_kernel(const ResolveParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 rtf_win[];       // LDS: [WW * WH] records, then [WW * WH] guides (a guided call)
    const uint32_t tiles_x = (p.W + 63u) / 64u;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t lx = threadIdx.x & 63u, ly = threadIdx.x >> 6;
    const uint32_t x = tx * 64u + lx, y = ty * 4u + ly;
    const bool guided = (p.planes & (rtdn::P_NORMAL | rtdn::P_DEPTH | rtdn::P_HITS)) != 0;
    const int s = (int)p.s;
    rtfm::Step st;
    st.sigma_l = p.sigma_l;
    st.var_eps = p.var_eps;
    st.kn = p.kn;
    st.kd = p.kd;
    st.s = s;
    st.planes = p.planes;
    const bool live = x < p.W && y < p.R;
    float out[4];
    if (LDS) {
        const int WW = 64 + 4 * s, WH = 4 + 4 * s;
        const int wx0 = (int)(tx * 64u) - 2 * s, wy0 = (int)(ty * 4u) - 2 * s;
        float4* wg = rtf_win + WW * WH;
        for (int i = (int)threadIdx.x; i < WW * WH; i += 256) {
            const int wy = i / WW, wx = i - wy * WW;
            const int gx = wx0 + wx, gy = wy0 + wy;
            if (gx >= 0 && gx < (int)p.W && gy >= 0 && gy < (int)p.R) {      // (cells outside P are never read: their taps are skipped)
                const size_t g = (size_t)gy * p.W + gx;
                rtf_win[i] = p.src[g];
                if (guided) wg[i] = p.guide[g];
            }
        }
        __syncthreads();
        if (!live) return;
        auto load = [&](int qx, int qy, float r[4], rtdn::Guide& gd) {
            const int i = (qy - wy0) * WW + (qx - wx0);
            const float4 c = rtf_win[i];
            r[0] = c.x;
            r[1] = c.y;
            r[2] = c.z;
            r[3] = c.w;
            if (guided) {
                const float4 v = wg[i];
                gd = {v.x, v.y, v.z, v.w};
            }
        };
        rtfm::step_pixel(st, (int)x, (int)y, (int)p.W, (int)p.R, load, out);
    } else {
        if (!live) return;
        auto load = [&](int qx, int qy, float r[4], rtdn::Guide& gd) {
            const size_t g = (size_t)qy * p.W + qx;
            const float4 c = p.src[g];
            r[0] = c.x;
            r[1] = c.y;
            r[2] = c.z;
            r[3] = c.w;
            if (guided) {
                const float4 v = p.guide[g];
                gd = {v.x, v.y, v.z, v.w};
            }
        };
        rtfm::step_pixel(st, (int)x, (int)y, (int)p.W, (int)p.R, load, out);
    }
    const size_t g = (size_t)y * p.W + x;
    if (FINAL)
        rtf_write(p, g, out);
    else
        p.dst[g] = make_float4(out[0], out[1], out[2], out[3]);
}

// iterations == 0: the outputs of (r0, v0)
__global__ __launch_bounds__(256) void rtf_output_kernel(const ResolveParams p) {
    const uint64_t total = (uint64_t)p.R * p.W;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (uint64_t)gridDim.x * blockDim.x) {
        const float4 c = p.src[g];
        const float r[4] = {c.x, c.y, c.z, c.w};
        rtf_write(p, g, r);
    }
}

}  // namespace rtfk
