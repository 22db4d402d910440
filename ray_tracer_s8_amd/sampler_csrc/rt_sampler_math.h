// rt_sampler_math.h — the per-pixel arithmetic of the film-sampler library (rt_sampler.h): the error metric and the
// noisy rule of a pixel, the dilation of the noisy plane, the fold of an active pixel's records and the normalisation of its sums to
// the film's count.  Plain C++ that compiles as HIP device code (rt_sampler.hip.h) and under g++ -ffp-contract=off
// (tests/host/sampler_host.cpp), so the kernels and the CPU harness run the same lines.  Every operation is one IEEE f32 rounding in
// the order rt_sampler.h writes it: no fused multiply-add, correctly rounded division and sqrt, no transcendental function.  The fold's
// lines restate the film library's fold (film_csrc/rt_film_math.h, which is not this library's to include); tests/test_sampler_host.py
// holds the two to the same bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RTS_HOST_DEVICE __host__ __device__ inline
#else
#define RTS_HOST_DEVICE inline
#endif

namespace rtsm {

// the one NaN the library writes: the quiet NaN 0x7FC00000
RTS_HOST_DEVICE float canonical(float x) { return x != x ? __builtin_nanf("") : x; }

// d of a pixel at its true count: the clamped spread of y, S2 / n - (S1 / n)^2
RTS_HOST_DEVICE float spread(float S1, float S2, float n_f) {
    const float m = S1 / n_f;
    const float a = S2 / n_f;
    const float d = a - m * m;
    return d > 0.0f ? d : 0.0f;
}

// ---- the metric ---------------------------------------------------------------------------------------------------------------------
// err of a pixel from its sums over n samples: the standard error of the mean of y relative to |mean| + eps.  n < 2: the quiet NaN.
RTS_HOST_DEVICE float pixel_error(float S1, float S2, int32_t n, float eps) {
    if (n < 2) return __builtin_nanf("");
    const float n_f = (float)n;
    const float m = S1 / n_f;
    const float d = spread(S1, S2, n_f);
    const float v = d / (n_f - 1.0f);
    const float err = __builtin_sqrtf(v) / (__builtin_fabsf(m) + eps);
    return canonical(err);
}

// noisy: err > threshold (false for a NaN err)
RTS_HOST_DEVICE bool noisy(float err, float threshold) { return err > threshold; }

// ---- the dilation -------------------------------------------------------------------------------------------------------------------
// active: any pixel of the (2 dilate + 1)^2 window around (x, y), clipped to the W x R image, is noisy.  flag(i): the noisy byte of
// pixel i = y W + x.
template <class Flag>
RTS_HOST_DEVICE bool active_pixel(uint32_t x, uint32_t y, uint32_t W, uint32_t R, uint32_t dilate, const Flag& flag) {
    const uint32_t x0 = x >= dilate ? x - dilate : 0u, y0 = y >= dilate ? y - dilate : 0u;
    const uint32_t x1 = x + dilate < W ? x + dilate : W - 1u, y1 = y + dilate < R ? y + dilate : R - 1u;
    bool any = false;
    for (uint32_t qy = y0; qy <= y1; qy++)
        for (uint32_t qx = x0; qx <= x1; qx++) any = any || flag((size_t)qy * W + qx) != 0;
    return any;
}

// ---- the gather ---------------------------------------------------------------------------------------------------------------------
// the record of (pixel q, sample j) in a strip buffer of k samples a pixel: the layout rt_scene_camera_rays_device writes
RTS_HOST_DEVICE uint64_t record_index(uint32_t q, uint32_t k, uint32_t j) { return (uint64_t)q * k + j; }

// ---- the fold -----------------------------------------------------------------------------------------------------------------------
// k records (3 floats each, in sample order) into the pixel's running sums: acc += c per channel, y = (c0 + c1) + c2, mom[0] += y,
// mom[1] += y y
RTS_HOST_DEVICE void fold_pixel(const float* rec, uint32_t k, float acc[3], float mom[2]) {
    for (uint32_t j = 0; j < k; j++) {
        const float* c = rec + 3 * (size_t)j;
        acc[0] = acc[0] + c[0];
        acc[1] = acc[1] + c[1];
        acc[2] = acc[2] + c[2];
        const float y = (c[0] + c[1]) + c[2];
        mom[0] = mom[0] + y;
        mom[1] = mom[1] + y * y;
    }
}

// ---- the normalisation --------------------------------------------------------------------------------------------------------------
// The sums of a pixel with n samples restated at the film's count e0 (rt_sampler.h "rts_normalise").  n == e0: the caller copies the
// bytes and does not come here.
RTS_HOST_DEVICE void normalise_pixel(const float A[3], const float M[2], int32_t n, float e0_f, float oA[3], float oM[2]) {
    const float n_f = (float)n;
    const float r = e0_f / n_f;
    oA[0] = canonical(A[0] * r);
    oA[1] = canonical(A[1] * r);
    oA[2] = canonical(A[2] * r);
    const float S1p = M[0] * r;
    const float d = spread(M[0], M[1], n_f);
    const float g = (e0_f - 1.0f) / (n_f - 1.0f);
    const float mm = S1p / e0_f;
    const float S2p = (mm * mm + d * g) * e0_f;
    oM[0] = canonical(S1p);
    oM[1] = canonical(S2p);
}

}  // namespace rtsm
