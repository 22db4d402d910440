/* rt_film.h — the private C declarations of librt_film.so, the film library: the moments fold and the
 * variance-guided a-trous resolve of ray_tracer_s8_amd/film.py.  Private: this header is not installed under include/, the library is
 * loaded by ray_tracer_s8_amd/_film_lib.py only, and nothing here is part of the tile ABI (include/rt_tile.h).
 *
 * Every function returns an int status (RTF_OK or an RTF_ERR_*), catches everything inside its body, launches on the stream the
 * caller gives and checks hipGetLastError after each launch.  There is no global state, no scene and no allocation: every buffer is
 * the caller's device memory, and a call returns once its launches are enqueued.
 *
 * NORMATIVE ARITHMETIC.  Every operation is one IEEE f32 rounding in the order written: no FMA, division and sqrt correctly
 * rounded, no transcendental function (the discipline of rt_tile.h's denoiser section).
 *
 * Moments.  For the colour c that the integrator returned for the camera ray of (p, s), let y = (c0 + c1) + c2.  After passes
 * covering [0, e):
 *   - S1[p] is the f32 sum from +0, in the order s = 0 ... e-1, of y;
 *   - S2[p] is the same sum of y*y;
 *   - accum[p] is the film's running colour sum, the same f32 sum per channel.
 * All three are bit for bit independent of how the samples were cut into passes or sub-ranges (each call continues the running
 * sums in sample order).
 *
 * Guided resolve over the image P (W columns, R rows), e = samples >= 2, e_f = (float)e.
 *   Entry:
 *     r0 = C / e_f per channel.
 *     m = S1 / e_f;  a = S2 / e_f;  d = a - m*m;  d = d > 0 ? d : +0.
 *     v0 = d / (e_f - 1): the variance of the mean of y.
 *     The guide (n, zg) is rtdn::entry_guide (csrc/rt_denoise_math.h), unchanged.
 *   Iteration i = 0 ... I-1, step s = 2^i, from the records (r_i, v_i):
 *     Prefilter, not dilated: taps (dy, dx) in {-1, 0, 1}^2, dy outer, dx inner, both ascending, q = p + (dx, dy).  A tap is
 *       skipped if q lies outside P or, in a guided call, g_q != g_p.  G = (1/4, 1/2, 1/4);  Gw += G[dy]*G[dx];
 *       Gv += (G[dy]*G[dx]) * v_q, both from +0.  gv_p = Gv / Gw.
 *     a_p = 1 / (sigma_l * sqrt(gv_p) + var_eps), and y(r) = (r0 + r1) + r2.
 *     The main taps are rt_tile.h's denoiser's: the same set, order, skip rule, H and centre tap t = 1.
 *     Any other tap: x = |y(r_q) - y(r_p)| * a_p; the normal and depth terms of rtdn::tap_t are then added exactly as they stand;
 *       t = 1 - x if that is > 0, else +0.
 *     w = H[dy]*H[dx]*(t*t).  Sw += w;  Sc += w * r_q;  Sv += (w*w) * v_q.
 *     r_{i+1} = Sc / Sw;  v_{i+1} = Sv / (Sw*Sw).
 *   Outputs (each optional, at least one): linear, f32 and rgb as rtdn::output_pixel without albedo; variance: v_I as an (R, W) f32
 *     plane.
 * With I = 0, f32 and rgb are the film's preview, bit for bit.  There is no albedo demodulation.
 *
 * Subnormal, infinite and NaN inputs.  The film writes finite, non-negative sums, but no value of a plane is refused, and nothing
 * faults or reads outside a buffer whatever the planes hold: no address depends on a plane's value.  The arithmetic above proceeds
 * as IEEE 754 defines it for every operand, with subnormal operands and results kept (nothing is flushed to zero), signed zeros
 * and infinities as the operations make them, and each `x > 0 ? x : +0` as written: false for a NaN and for -0, so both give +0.
 * Where the text yields a NaN the output is a NaN, of unspecified payload and sign; `as u8` of a NaN is 0.  Every other output
 * value, the signs of zeros included, is the one the text defines (tests/test_gpu_film_extremes.py holds the
 * kernels to it). */
#ifndef RT_FILM_H
#define RT_FILM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTF_VERSION 1u

#define RTF_OK 0
#define RTF_ERR_BAD_ARG 1        /* a null pointer, a zero size, a value out of range */
#define RTF_ERR_LIMIT 2          /* an image or a strip beyond what the kernels index */
#define RTF_ERR_SCRATCH 3        /* scratch_bytes < rtf_resolve_scratch_bytes(W, R) */
#define RTF_ERR_HIP 4            /* a HIP call or a launch failed */
#define RTF_ERR_INTERNAL 5       /* an exception was caught at the boundary */

#define RTF_MAX_ITERATIONS 8u
/* lds_max_step: the largest step whose window is staged in LDS; 0: every step loads directly; RTF_LDS_PLAN (or anything above
 * 2^30): the plan's own choice, rtplan::DN_LDS_MAX_STEP.  A window that does not fit a CU's LDS loads directly whatever it says. */
#define RTF_LDS_PLAN 0xFFFFFFFFu

/* The planes a resolve call reads: rtdn::P_NORMAL, P_DEPTH, P_HITS by which pointers are set (depth needs hits). */
typedef struct rtf_resolve_args {
    uint32_t W, R;                /* the image P */
    uint32_t samples;             /* e >= 2 */
    uint32_t iterations;          /* I <= RTF_MAX_ITERATIONS */
    uint32_t lds_max_step;
    uint32_t reserved;            /* 0 */
    float sigma_l, var_eps;       /* finite, sigma_l >= 0, var_eps > 0 */
    float k_normal, k_depth;      /* finite, >= 0 */
    const float* accum;           /* [R*W*3] */
    const float* moments;         /* [R*W*2]: S1, S2 */
    const float* normal;          /* [R*W*3] or NULL */
    const float* depth;           /* [R*W] or NULL */
    const uint32_t* hits;         /* [R*W] or NULL */
    void* scratch;                /* rtf_resolve_scratch_bytes(W, R) bytes, 16-byte aligned */
    uint64_t scratch_bytes;
    uint8_t* out_rgb;             /* [R*W*3] or NULL */
    float* out_f32;               /* [R*W*3] or NULL */
    float* out_linear;            /* [R*W*3] or NULL */
    float* out_variance;          /* [R*W] or NULL */
} rtf_resolve_args;

int rtf_version(uint32_t* version);

/* accum [P*3] and moments [P*2] += the records [P*n*3] (pixel major, then sample, then channel), sample by sample in record order.
 * Reads the records once; reads and writes accum and moments once each.  stream: a hipStream_t. */
int rtf_fold_moments(const float* records, uint64_t P, uint32_t n, float* accum, float* moments, void* stream);

int rtf_resolve_scratch_bytes(uint32_t W, uint32_t R, uint64_t* bytes);

int rtf_resolve(const rtf_resolve_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
