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
//   - output: iterations == 0 — r0, v0 to the outputs;
//   - regress fit: a workgroup of 1024 lanes per node, a lane per pixel of its 32 x 32 window (lane l = 32 wy + wx, so a wave is two
//     window rows and the group k of rt_film.h's window sum).  The count, zlo and zhi first, then the 60 window sums: each the xor
//     butterfly of a wave, the sixteen wave totals through LDS, added in order by one lane.  The sums, the Cholesky factor and the
//     record stay in LDS; lane 0 factors, lanes 0 ... 2 solve a channel each, 32 lanes store the record;
//   - regress apply: a lane per pixel; it reads its four nodes' records, which the cache holds (128 B a node).
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

// ---- the regression resolve ---------------------------------------------------------------------------------------
struct RegressParams {
    uint32_t W, R, NX, NY;
    float ridge;
    rtfm::RgPlanes pl;
    float* model;                // [NY*NX*32]
    uint8_t* rgb;                // outputs or nullptr
    float* f32;
    float* lin;
};

constexpr uint32_t RG_BLOCK = 1024, RG_WAVES = 16;

// the adjacent-pair tree over a wave's 64 values, in every lane: level 0 adds lanes 2m and 2m + 1, f32 addition commutes
__device__ __forceinline__ float rtf_wave_tree(float v) {
    RT_DN_UNROLL
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(1024) void rtf_regress_fit_kernel(const RegressParams p) {
    __shared__ float part[rtfm::RG_NS][RG_WAVES];
    __shared__ float S[rtfm::RG_NS];
    __shared__ float L[rtfm::RG_M * rtfm::RG_M];
    __shared__ __attribute__((aligned(16))) float rec[rtfm::RG_RECORD];
    __shared__ float wlo[RG_WAVES], whi[RG_WAVES];
    __shared__ uint32_t wn[RG_WAVES];
    __shared__ uint32_t fit_ok;
    const uint32_t node = blockIdx.x;
    const int j = (int)(node / p.NX), i = (int)(node - (uint32_t)j * p.NX);
    const uint32_t l = threadIdx.x, wave = l >> 6, lane = l & 63u;
    const int x = rtfm::RG_T * i - rtfm::RG_T + (int)(l & 31u), y = rtfm::RG_T * j - rtfm::RG_T + (int)(l >> 5);
    const bool inside = x >= 0 && x < (int)p.W && y >= 0 && y < (int)p.R;
    rtfm::RgPixel px;
    px.r[0] = px.r[1] = px.r[2] = 0.0f;
    px.g = {0.0f, 0.0f, 0.0f, -1.0f};
    px.z = 0.0f;
    px.valid = false;
    if (inside) px = rtfm::rg_entry(p.pl, (size_t)y * p.W + (size_t)x);
    const bool valid = inside && px.valid;
    // the window's count, zlo and zhi: z is never a NaN and never -0, so min and max by comparison are those of the text
    float lo = valid ? px.z : __builtin_inff(), hi = valid ? px.z : 0.0f;
    RT_DN_UNROLL
    for (int m = 1; m < 64; m <<= 1) {
        const float ol = __shfl_xor(lo, m, 64), oh = __shfl_xor(hi, m, 64);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(valid));
    if (lane == 0) {
        wlo[wave] = lo;
        whi[wave] = hi;
        wn[wave] = cnt;
    }
    __syncthreads();
    uint32_t n = 0;
    float zlo = __builtin_inff(), zhi = 0.0f;
    for (uint32_t k = 0; k < RG_WAVES; k++) {
        n += wn[k];
        zlo = wlo[k] < zlo ? wlo[k] : zlo;
        zhi = whi[k] > zhi ? whi[k] : zhi;
    }
    if (n == 0u || !p.pl.depth) zlo = zhi = 0.0f;
    const float s = zhi - zlo;
    float phi[rtfm::RG_M];
    rtfm::rg_features(px, x, y, i, j, zlo, s, phi);
    // the window sums: A_ab, a <= b, then B_ac
    RT_DN_UNROLL
    for (int a = 0; a < rtfm::RG_M; a++) {
        RT_DN_UNROLL
        for (int b = a; b < rtfm::RG_M; b++) {
            const float t = rtf_wave_tree(valid ? phi[a] * phi[b] : 0.0f);
            if (lane == 0) part[rtfm::rg_ai(a, b)][wave] = t;
        }
        RT_DN_UNROLL
        for (int c = 0; c < 3; c++) {
            const float t = rtf_wave_tree(valid ? phi[a] * px.r[c] : 0.0f);
            if (lane == 0) part[rtfm::RG_NA + 3 * a + c][wave] = t;
        }
    }
    __syncthreads();
    if (l < (uint32_t)rtfm::RG_NS) {
        float t = 0.0f;
        for (uint32_t k = 0; k < RG_WAVES; k++) t = t + part[l][k];
        S[l] = t;
    }
    __syncthreads();
    if (l == 0) fit_ok = rtfm::rg_cholesky(S, n, p.ridge, L) ? 1u : 0u;
    __syncthreads();
    const bool ok = fit_ok != 0u;
    if (l < 3u) rtfm::rg_solve(S, n, ok, L, (int)l, rec);
    if (l == 3u) rtfm::rg_record_tail(n, zlo, s, ok, rec);
    __syncthreads();
    if (l < (uint32_t)rtfm::RG_RECORD) p.model[(size_t)node * rtfm::RG_RECORD + l] = rec[l];
}

__global__ __launch_bounds__(256) void rtf_regress_apply_kernel(const RegressParams p) {
    const uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= (uint64_t)p.R * p.W) return;
    const int y = (int)(g / p.W), x = (int)(g - (uint64_t)y * p.W);
    const rtfm::RgPixel px = rtfm::rg_entry(p.pl, (size_t)g);
    float r[3] = {px.r[0], px.r[1], px.r[2]};
    if (px.valid) rtfm::rg_apply(px, x, y, p.model, p.NX, r);
    rtdn::output_pixel(r, p.pl.albedo ? px.d : nullptr, p.lin ? p.lin + g * 3 : nullptr, p.f32 ? p.f32 + g * 3 : nullptr,
                       p.rgb ? p.rgb + g * 3 : nullptr);
}

}  // namespace rtfk
