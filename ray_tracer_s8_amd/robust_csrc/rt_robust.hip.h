// rt_robust.hip.h — the gfx950 kernels of the robust-film library (rt_robust.h), wave64, every per-pixel operation
// taken from rt_robust_math.h (the lines the CPU harness runs too).
//
// Both kernels: one lane a pixel, blocks of 256 lanes over the pixels in order, so a wave reads and writes 64 neighbouring pixels of
// a bucket (768 contiguous bytes a wave for a three-float plane).  No LDS, no barrier, no atomics, no cross-lane work, no inline
// assembly; every address comes from the sizes alone.  Lanes past the last pixel do nothing.
//
// rtr_fold_kernel: per bucket a sample of the call falls into, the lane loads its three sums once, adds the bucket's records of the
// call in ascending order and stores once; K and n are kernel arguments, and nothing is kept in a per-lane array.
// rtr_resolve_kernel<K>: K is the template argument and every loop over buckets is unrolled, so the means, keys and ranks of a pixel
// are registers: no scratch memory (DESIGN.md 4.29 holds the code objects' metadata).  The six outputs are tested, once a lane, on
// kernel arguments, which are uniform.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_robust_math.h"

namespace rtrk {

constexpr uint32_t BLOCK = 256;

struct FoldParams {
    uint32_t pixels, n, first_mod_K, K;
    size_t bucket_stride;
    const float* records;
    float* buckets;
};

__global__ __launch_bounds__(256) void rtr_fold_kernel(const FoldParams p) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= p.pixels) return;
    rtrm::fold_pixel(p.records + (size_t)i * p.n * 3u, p.n, p.first_mod_K, p.K, p.buckets + (size_t)i * 3u, p.bucket_stride);
}

struct ResolveParams {
    rtrm::Call call;
    uint32_t pixels;
    const float* buckets;
    float* out_linear;
    float* out_gini;
    int32_t* out_kept;
    float* out_variance;
    float* out_accum;
    float* out_moments;
};

// the pixel's sums: bucket k at k pixels 3
struct PixelBuckets {
    const float* at;
    size_t stride;
    __device__ __forceinline__ float operator()(int k, int c) const { return at[(size_t)k * stride + (size_t)c]; }
};

template <int K>
__global__ __launch_bounds__(256) void rtr_resolve_kernel(const ResolveParams p) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= p.pixels) return;
    rtrm::Pixel o;
    rtrm::resolve_pixel<K>(p.call, PixelBuckets{p.buckets + (size_t)i * 3u, (size_t)p.pixels * 3u}, o);
    if (p.out_linear) {
        p.out_linear[3 * (size_t)i + 0] = o.r[0];
        p.out_linear[3 * (size_t)i + 1] = o.r[1];
        p.out_linear[3 * (size_t)i + 2] = o.r[2];
    }
    if (p.out_gini) p.out_gini[i] = o.G;
    if (p.out_kept) p.out_kept[i] = o.kept;
    if (p.out_variance) p.out_variance[i] = o.v;
    if (p.out_accum) {
        p.out_accum[3 * (size_t)i + 0] = o.accum[0];
        p.out_accum[3 * (size_t)i + 1] = o.accum[1];
        p.out_accum[3 * (size_t)i + 2] = o.accum[2];
    }
    if (p.out_moments) {
        p.out_moments[2 * (size_t)i + 0] = o.S1;
        p.out_moments[2 * (size_t)i + 1] = o.S2;
    }
}

}  // namespace rtrk
