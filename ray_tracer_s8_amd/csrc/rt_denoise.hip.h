// rt_denoise.hip.h — gfx950 edge-avoiding a-trous denoiser (rt_scene_denoise*, rt_tile.h "denoiser").
//
// Three kernels over the W x R image P that the strips of a call stack into, one lane per pixel, every per-pixel operation taken from
// rt_denoise_math.h (the lines the CPU harness runs too):
//   - entry: reads a band of up to DN_BAND strips (accum and planes through per-strip pointers), writes r0 and the packed guide
//     (unit normal, zg) of each pixel to the caller's scratch as float4 records;
//   - step<LDS, FINAL>: one iteration over the whole image from one colour buffer into the other.  LDS: the workgroup first stages
//     the (64 + 4s) x (4 + 4s) window of colour (and guide) records its 64 x 4 tile reads, then every tap reads LDS; otherwise each
//     tap is a float4 load through L1 / L2.  FINAL: the last iteration, launched per band of up to DN_BAND strips, remodulates
//     by d (recomputed from the albedo plane with the entry's lines), and writes the per-strip outputs itself;
//   - output: iterations == 0 — r0 to the outputs.
// Taps outside P are skipped before any load, so no lane reads outside the image; out-of-image lanes of a tile only help stage.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_consts.h"
#include "rt_denoise_math.h"

namespace rtk {

constexpr uint32_t DN_BAND = 32;     // strips per band: the entry, final and output launches carry 8 pointers of each in their arguments

struct DnStrip {
    const float* accum;          // [Hs*W*3]
    const float* albedo;         // [Hs*W*3] or nullptr (the same set of planes for every strip of a call)
    const float* normal;         // [Hs*W*3]
    const float* depth;          // [Hs*W]
    const uint32_t* hits;        // [Hs*W]
    uint8_t* rgb;                // outputs [Hs*W*3] or nullptr (the same set for every strip of a call)
    float* f32;
    float* lin;
};

struct DnParams {
    uint32_t W, R;               // the image P
    uint32_t Hs;                 // rows of a strip
    uint32_t row0, rows;         // the band of rows this launch writes: [row0, row0 + rows) (entry, final, output: whole strips)
    uint32_t planes;             // rtdn::P_* of the call
    uint32_t s;                  // step kernel: the step 2^i
    float e_f, k_f;              // color_samples, aov_samples as floats
    float eps;                   // albedo_eps
    float kc, kn, kd;            // this iteration's k_color, k_normal, k_depth
    uint32_t n_strips;           // strips in the band (entry, final, output)
    uint32_t pad;
    float4* guide;               // [W*R] scratch
    const float4* src;           // [W*R] the colour records read
    float4* dst;                 // [W*R] the colour records written (entry, non-final steps)
    DnStrip strips[DN_BAND];     // the band's strips, strip 0 at row row0
};
static_assert(sizeof(DnParams) <= 4096, "DnParams must fit the kernel argument segment");

// The kernels are defined in rt_kernels_denoise.hip only (which defines RT_DENOISE_KERNELS); rt_api.hip sees the parameters and the
// getters.
#ifdef RT_DENOISE_KERNELS
// the strip of the band and the offset of pixel (x, y) in it
__device__ __forceinline__ const DnStrip& dn_strip(const DnParams& p, uint32_t x, uint32_t y, size_t& off) {
    const uint32_t b = y - p.row0;
    const uint32_t si = b / p.Hs;
    off = (size_t)(b - si * p.Hs) * p.W + x;
    return p.strips[si];
}

__global__ __launch_bounds__(256) void rt_dn_entry_kernel(const DnParams p) {
    const uint64_t total = (uint64_t)p.rows * p.W;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t y = p.row0 + (uint32_t)(i / p.W), x = (uint32_t)(i % p.W);
        size_t off;
        const DnStrip& sd = dn_strip(p, x, y, off);
        const size_t g = (size_t)y * p.W + x;
        float C[3] = {sd.accum[off * 3 + 0], sd.accum[off * 3 + 1], sd.accum[off * 3 + 2]};
        float d[3], r[3];
        if (p.planes & rtdn::P_ALBEDO) {
            const float A[3] = {sd.albedo[off * 3 + 0], sd.albedo[off * 3 + 1], sd.albedo[off * 3 + 2]};
            rtdn::albedo_d(A, p.k_f, p.eps, d);
        }
        rtdn::entry_color(C, p.e_f, (p.planes & rtdn::P_ALBEDO) ? d : nullptr, r);
        p.dst[g] = make_float4(r[0], r[1], r[2], 0.0f);
        if (p.planes & (rtdn::P_NORMAL | rtdn::P_DEPTH | rtdn::P_HITS)) {
            float N[3];
            if (p.planes & rtdn::P_NORMAL) {
                N[0] = sd.normal[off * 3 + 0];
                N[1] = sd.normal[off * 3 + 1];
                N[2] = sd.normal[off * 3 + 2];
            }
            float D = 0.0f;
            uint32_t hits = 0;
            if (p.planes & rtdn::P_DEPTH) D = sd.depth[off];
            if (p.planes & rtdn::P_HITS) hits = sd.hits[off];
            const rtdn::Guide gd = rtdn::entry_guide((p.planes & rtdn::P_NORMAL) ? N : nullptr, (p.planes & rtdn::P_DEPTH) ? &D : nullptr,
                                                     (p.planes & rtdn::P_HITS) ? &hits : nullptr);
            p.guide[g] = make_float4(gd.nx, gd.ny, gd.nz, gd.zg);
        }
    }
}

// the outputs of pixel (x, y) of the band from its final colour r
__device__ __forceinline__ void dn_write(const DnParams& p, uint32_t x, uint32_t y, const float r[3]) {
    size_t off;
    const DnStrip& sd = dn_strip(p, x, y, off);
    float d[3];
    if (p.planes & rtdn::P_ALBEDO) {
        const float A[3] = {sd.albedo[off * 3 + 0], sd.albedo[off * 3 + 1], sd.albedo[off * 3 + 2]};
        rtdn::albedo_d(A, p.k_f, p.eps, d);
    }
    rtdn::output_pixel(r, (p.planes & rtdn::P_ALBEDO) ? d : nullptr, sd.lin ? sd.lin + off * 3 : nullptr,
                       sd.f32 ? sd.f32 + off * 3 : nullptr, sd.rgb ? sd.rgb + off * 3 : nullptr);
}

// One iteration: a workgroup per 64 x 4 tile of the band [row0, row0 + rows), in a 1-D grid (tiles_x per row of tiles).
template <bool LDS, bool FINAL>
__global__ __launch_bounds__(256) void rt_dn_step_kernel(const DnParams p) {
    extern __shared__ float4 dn_win[];       // LDS: [WW * WH] colours, then [WW * WH] guides (a guided call)
    const uint32_t tiles_x = (p.W + 63u) / 64u;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t lx = threadIdx.x & 63u, ly = threadIdx.x >> 6;
    const uint32_t x = tx * 64u + lx, y = p.row0 + ty * 4u + ly;
    const bool guided = (p.planes & (rtdn::P_NORMAL | rtdn::P_DEPTH | rtdn::P_HITS)) != 0;
    const int s = (int)p.s;
    rtdn::Step st;
    st.kc = p.kc;
    st.kn = p.kn;
    st.kd = p.kd;
    st.s = s;
    st.planes = p.planes;
    const bool live = x < p.W && y < p.row0 + p.rows;
    float out[3];
    if (LDS) {
        const int WW = 64 + 4 * s, WH = 4 + 4 * s;
        const int wx0 = (int)(tx * 64u) - 2 * s, wy0 = (int)(p.row0 + ty * 4u) - 2 * s;
        float4* wg = dn_win + WW * WH;
        for (int i = (int)threadIdx.x; i < WW * WH; i += 256) {
            const int wy = i / WW, wx = i - wy * WW;
            const int gx = wx0 + wx, gy = wy0 + wy;
            if (gx >= 0 && gx < (int)p.W && gy >= 0 && gy < (int)p.R) {      // (cells outside P are never read: their taps are skipped)
                const size_t g = (size_t)gy * p.W + gx;
                dn_win[i] = p.src[g];
                if (guided) wg[i] = p.guide[g];
            }
        }
        __syncthreads();
        if (!live) return;
        auto load = [&](int qx, int qy, float r[3], rtdn::Guide& gd) {
            const int i = (qy - wy0) * WW + (qx - wx0);
            const float4 c = dn_win[i];
            r[0] = c.x;
            r[1] = c.y;
            r[2] = c.z;
            if (guided) {
                const float4 v = wg[i];
                gd = {v.x, v.y, v.z, v.w};
            }
        };
        rtdn::step_pixel(st, (int)x, (int)y, (int)p.W, (int)p.R, load, out);
    } else {
        if (!live) return;
        auto load = [&](int qx, int qy, float r[3], rtdn::Guide& gd) {
            const size_t g = (size_t)qy * p.W + qx;
            const float4 c = p.src[g];
            r[0] = c.x;
            r[1] = c.y;
            r[2] = c.z;
            if (guided) {
                const float4 v = p.guide[g];
                gd = {v.x, v.y, v.z, v.w};
            }
        };
        rtdn::step_pixel(st, (int)x, (int)y, (int)p.W, (int)p.R, load, out);
    }
    if (FINAL)
        dn_write(p, x, y, out);
    else
        p.dst[(size_t)y * p.W + x] = make_float4(out[0], out[1], out[2], 0.0f);
}

// iterations == 0: the outputs of r0
__global__ __launch_bounds__(256) void rt_dn_output_kernel(const DnParams p) {
    const uint64_t total = (uint64_t)p.rows * p.W;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t y = p.row0 + (uint32_t)(i / p.W), x = (uint32_t)(i % p.W);
        const float4 c = p.src[(size_t)y * p.W + x];
        const float r[3] = {c.x, c.y, c.z};
        dn_write(p, x, y, r);
    }
}

#endif  // RT_DENOISE_KERNELS

using DnFn = void (*)(const DnParams);
DnFn dn_entry_kernel();                           // rt_kernels_denoise.hip
DnFn dn_step_kernel(bool lds, bool final_step);
DnFn dn_output_kernel();

}  // namespace rtk
