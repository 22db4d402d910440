// rt_sampler.hip.h — the gfx950 kernels of the film-sampler library (rt_sampler.h), wave64, every per-pixel operation
// taken from rt_sampler_math.h (the lines the CPU harness runs too).
//
// The select is four launches.  (1) metric: one lane a pixel over the whole image, the err plane and a noisy byte.  (2) count: one
// lane a strip index, workgroups of 256 consecutive indices of ONE strip; the lane reads the noisy bytes of its window (they cross
// strips), writes its active byte, and the workgroup's number of active lanes is the sum of its four waves' ballot popcounts.
// (3) scan: one workgroup a strip walks the strip's workgroup numbers 256 at a time, in order, carrying the running total: a wave
// scan by shuffles, the four wave totals through LDS.  (4) write: the count's geometry again; a lane's position in the strip's list
// is the scanned offset of its workgroup plus the active lanes below it (the lower waves' popcounts and the prefix popcount of its
// own wave's ballot), so the list is ascending by construction.  No atomics and no inline assembly; no workgroup reads what another
// of the same launch writes, so none waits on another, and every loop has a bound known at launch.
// The gather moves 16 bytes a lane (half a record), so a wave writes 1 KiB runs; the fold and the normalisation are one lane a pixel.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_sampler_math.h"

namespace rtsk {

constexpr uint32_t BLOCK = 256, WAVE = 64, WAVES = BLOCK / WAVE;

struct SelectParams {
    uint32_t W, R, Hs, dilate;
    uint32_t P;                   // Hs W
    uint32_t bps;                 // workgroups per strip: ceil(P / BLOCK)
    float threshold, eps;
    const float* moments;
    const int32_t* counts;
    float* err;
    uint32_t* active;
    uint32_t* strip_counts;
    uint8_t* noisy;               // [R W]
    uint8_t* act;                 // [R W]
    uint32_t* offsets;            // [R / Hs][bps]: the count writes numbers, the scan turns them into exclusive offsets
};

struct NoisyPlane {
    const uint8_t* b;
    __device__ __forceinline__ uint8_t operator()(size_t i) const { return b[i]; }
};

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ __launch_bounds__(256) void rts_metric_kernel(const SelectParams p) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (size_t)p.R * p.W) return;
    const float2 m = reinterpret_cast<const float2*>(p.moments)[i];
    const float err = rtsm::pixel_error(m.x, m.y, p.counts[i], p.eps);
    p.err[i] = err;
    p.noisy[i] = rtsm::noisy(err, p.threshold) ? 1 : 0;
}

// the active lanes of the workgroup below this wave, and (total) in the whole workgroup; every lane of the workgroup calls it
__device__ __forceinline__ uint32_t waves_below(unsigned long long mask, uint32_t* lds, uint32_t& total) {
    const uint32_t w = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1u)) == 0u) lds[w] = (uint32_t)__builtin_popcountll(mask);
    __syncthreads();
    uint32_t below = 0;
    total = 0;
    for (uint32_t k = 0; k < WAVES; k++) {
        const uint32_t c = lds[k];
        below += k < w ? c : 0u;
        total += c;
    }
    return below;
}

__global__ __launch_bounds__(256) void rts_count_kernel(const SelectParams p) {
    __shared__ uint32_t lds[WAVES];
    const uint32_t strip = blockIdx.y;
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    bool a = false;
    if (q < p.P) {
        const uint32_t y = strip * p.Hs + q / p.W, x = q % p.W;
        a = rtsm::active_pixel(x, y, p.W, p.R, p.dilate, NoisyPlane{p.noisy});
        p.act[(size_t)strip * p.P + q] = a ? 1 : 0;
    }
    uint32_t total;
    waves_below(__ballot(a), lds, total);
    if (threadIdx.x == 0) p.offsets[(size_t)strip * p.bps + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void rts_scan_kernel(const SelectParams p) {
    __shared__ uint32_t lds[WAVES];
    uint32_t* off = p.offsets + (size_t)blockIdx.x * p.bps;
    const uint32_t lane = threadIdx.x & (WAVE - 1u), w = threadIdx.x / WAVE;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < p.bps; base += BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < p.bps ? off[i] : 0u;
        uint32_t s = v;                                           // inclusive scan of the wave
        for (uint32_t d = 1; d < WAVE; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)s, d, WAVE);
            s += lane >= d ? t : 0u;
        }
        if (lane == WAVE - 1u) lds[w] = s;
        __syncthreads();
        uint32_t below = 0, total = 0;
        for (uint32_t k = 0; k < WAVES; k++) {
            const uint32_t c = lds[k];
            below += k < w ? c : 0u;
            total += c;
        }
        if (i < p.bps) off[i] = carry + below + (s - v);
        carry += total;
        __syncthreads();                                          // lds is written again by the next round
    }
    if (threadIdx.x == 0) p.strip_counts[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void rts_write_kernel(const SelectParams p) {
    __shared__ uint32_t lds[WAVES];
    const uint32_t strip = blockIdx.y;
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    const bool a = q < p.P && p.act[(size_t)strip * p.P + q] != 0;
    const unsigned long long mask = __ballot(a);
    uint32_t total;
    const uint32_t below = waves_below(mask, lds, total);
    if (a) p.active[(size_t)strip * p.P + p.offsets[(size_t)strip * p.bps + blockIdx.x] + below + lanes_below(mask)] = q;
}

struct GatherParams {
    uint32_t n_active, k, pixels;
    const uint32_t* active;
    const uint4* rays;
    const uint4* states;
    uint4* out_rays;
    uint4* out_states;
};

__global__ __launch_bounds__(256) void rts_gather_kernel(const GatherParams p) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;          // half a record
    const uint64_t rec = t >> 1;
    if (rec >= (uint64_t)p.n_active * p.k) return;
    const uint32_t a = (uint32_t)(rec / p.k), j = (uint32_t)(rec % p.k);
    const uint32_t q = p.active[a];
    if (q >= p.pixels) return;
    const uint64_t src = (rtsm::record_index(q, p.k, j) << 1) | (t & 1u);
    p.out_rays[t] = p.rays[src];
    p.out_states[t] = p.states[src];
}

struct FoldParams {
    uint32_t n_active, k, pixels;
    const uint32_t* active;
    const float* rgb;
    float* accum;
    float* moments;
    int32_t* counts;
};

__global__ __launch_bounds__(256) void rts_fold_kernel(const FoldParams p) {
    const uint32_t a = blockIdx.x * BLOCK + threadIdx.x;
    if (a >= p.n_active) return;
    const size_t q = p.active[a];
    if (q >= p.pixels) return;
    float acc[3] = {p.accum[3 * q + 0], p.accum[3 * q + 1], p.accum[3 * q + 2]};
    const float2 m = reinterpret_cast<const float2*>(p.moments)[q];
    float mom[2] = {m.x, m.y};
    rtsm::fold_pixel(p.rgb + 3 * (size_t)a * p.k, p.k, acc, mom);
    p.accum[3 * q + 0] = acc[0];
    p.accum[3 * q + 1] = acc[1];
    p.accum[3 * q + 2] = acc[2];
    reinterpret_cast<float2*>(p.moments)[q] = make_float2(mom[0], mom[1]);
    p.counts[q] = p.counts[q] + (int32_t)p.k;
}

struct NormaliseParams {
    uint64_t pixels;
    int32_t e0;
    float e0_f;
    const float* accum;
    const float* moments;
    const int32_t* counts;
    float* out_accum;
    float* out_moments;
};

__global__ __launch_bounds__(256) void rts_normalise_kernel(const NormaliseParams p) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= p.pixels) return;
    const float A[3] = {p.accum[3 * i + 0], p.accum[3 * i + 1], p.accum[3 * i + 2]};
    const float2 m = reinterpret_cast<const float2*>(p.moments)[i];
    const float M[2] = {m.x, m.y};
    const int32_t n = p.counts[i];
    float oA[3] = {A[0], A[1], A[2]}, oM[2] = {M[0], M[1]};
    if (n != p.e0) rtsm::normalise_pixel(A, M, n, p.e0_f, oA, oM);         // n == e0: the bytes as they are
    p.out_accum[3 * i + 0] = oA[0];
    p.out_accum[3 * i + 1] = oA[1];
    p.out_accum[3 * i + 2] = oA[2];
    reinterpret_cast<float2*>(p.out_moments)[i] = make_float2(oM[0], oM[1]);
}

}  // namespace rtsk
