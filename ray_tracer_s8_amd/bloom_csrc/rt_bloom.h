/* rt_bloom.h — the private C declarations of librt_bloom.so, the bloom library: a pyramid bloom of a linear HDR
 * image, for ray_tracer_s8_amd/film_bloom.py.  The image is sanitised, optionally thresholded, filtered down through up to eight levels
 * of half the size each, the levels are summed back up with a weight that falls from level to level, and the sum is mixed into the
 * image.  Private: this header is not installed under include/, the library is loaded by ray_tracer_s8_amd/_bloom_lib.py only, it
 * includes no csrc/ header, and nothing here is part of the tile ABI (include/rt_tile.h) or of the film, history, sampler, upsample,
 * robust, display and JPEG libraries.
 *
 * Every function returns an int status (RTB_OK or an RTB_ERR_*), catches everything inside its body, enqueues on the stream the caller
 * gives and checks hipGetLastError after each launch.  There is no global state, no scene and no allocation: every buffer is the
 * caller's device memory, a call returns once its work is enqueued, and nothing comes back to the host.
 *
 * NORMATIVE ARITHMETIC.  Every operation is one IEEE f32 rounding in the order written: no FMA, division correctly rounded, no
 * transcendental function.  Subnormal operands and results are kept.  Every comparison is as written: each is false for a NaN.
 * Images are [rows][cols][3] of f32.  "3 x" is the product 3.0f * x.
 *
 * Levels.  R_0 = R, W_0 = W; R_k = (R_{k-1} + 1) >> 1 and W_k likewise, for k = 1 ... L, L in 1 ... RTB_MAX_LEVELS = 8.  A side that has
 *   reached 1 stays 1.
 *
 * Sanitised input, per channel c of the input:
 *   1. q = c > 0 ? c : +0      (a NaN, both zeros and every negative give +0);
 *   2. p = q < cap ? q : cap   (cap is finite and positive, so +inf becomes cap).
 *
 * Threshold (T > 0 only; with T = 0 the pixel p is used as it is), per pixel:
 *   m = max(max(p0, p1), p2), with max(a, b) = a > b ? a : b;
 *   s = m - (T - K);  s = s > 0 ? s : 0;  s = s < K + K ? s : K + K;
 *   g = (s s) / ((K + K) + (K + K) + 1e-5f);
 *   e = m - T;  g = g > e ? g : e;  g = g > 0 ? g : 0;
 *   f = g / (m > 1e-5f ? m : 1e-5f);  p_i = p_i f.
 *   T is the caller's threshold and K = T knee its knee, computed by the caller as an f32, 0 <= K <= T.
 *   (s <= m and s <= 2 K give g <= m, so f is at most about 1; with cap <= RTB_MAX_CAP = 2^62 the square s s is finite.)
 *
 * Down.  S is the thresholded p for k = 0 and D_k otherwise.  For the pixel (i, j) of level k + 1:
 *   rows r_a = clamp(2 i - 1 + a, 0, R_k - 1) and columns c_b = clamp(2 j - 1 + b, 0, W_k - 1), a, b = 0 ... 3;
 *   h_a = (S[r_a][c_0] + 3 S[r_a][c_1]) + (3 S[r_a][c_2] + S[r_a][c_3]);
 *   v = (h_0 + 3 h_1) + (3 h_2 + h_3);
 *   D_{k+1}[i][j] = v 0.015625f.
 *   (h_a depends on the source row and on j only: a kernel computes it once and shares it.)
 *
 * Up.  up(X) of a level-(k + 1) image X at the level-k pixel (y, x):
 *   ya = (y + 1) / 2 - 1 (integer division), yb = ya + 1;  wya = (y & 1) ? 3 : 1, wyb = 4 - wya;
 *   both rows are clamped to [0, R_{k+1} - 1] after the weights are chosen;  xa, xb, wxa, wxb likewise from x;
 *   g_r = wxa X[r][xa] + wxb X[r][xb] for r = ya, yb;
 *   u = (wya g_ya + wyb g_yb) 0.0625f.
 *
 * Accumulate.  U_L = D_L; for k = L - 1 ... 1: U_k = D_k + spread up(U_{k+1}), in place in D_k.  For L = 1 only U_1 = D_1 exists.
 *
 * Combine, per channel of the level-0 pixel: b = up(U_1) norm.
 *   RTB_MIX: out = (1 - strength) q + strength b, the factor 1 - strength being one f32 subtraction;
 *   RTB_ADD: out = q + strength b;
 *   out_bloom, where asked for, is b.
 *   norm is the caller's: ray_tracer_s8_amd/_bloom_lib.py passes the f32 nearest to 1 / (spread^0 + ... + spread^(L-1)), in double.
 *
 * No NaN leaves the library, and a +inf of the input stays +inf: q is never a NaN, every p is in [0, cap], every pyramid value is a
 * sum of non-negative products and at most 64 cap a step before its factor (a product that overflows gives +inf, never a NaN, and
 * nothing is ever subtracted from it), f is finite, and both mixes add two non-negative terms.  tests/test_bloom_host.py sweeps it.
 *
 * rtb_apply refuses (RTB_ERR_BAD_ARG, or RTB_ERR_LIMIT for sizes): null pointers (out_bloom may be NULL), zero sizes, more than
 * 2^31 - 1 pixels, levels outside 1 ... 8, a mode or a form it does not know, a reserved word that is not 0, spread not in (0, 1],
 * strength not in (0, 1) under RTB_MIX or not finite and positive under RTB_ADD, norm not finite and positive, cap, T or K not finite,
 * cap <= 0 or cap > RTB_MAX_CAP, T < 0 or T > cap, K < 0 or K > T, a buffer that is not 16-byte aligned, a scratch smaller than
 * rtb_scratch_bytes, and any overlap among the input, the outputs and the scratch.
 *
 * Scratch.  Levels 1 ... L one after the other, level k being R_k W_k 12 bytes rounded up to 16, so that each starts on a 16-byte
 * boundary.  What it holds after a call is U_1 ... U_L under RTB_FORM_LEVELS; under RTB_FORM_TAIL the levels above the tail's first are
 * not written.
 *
 * The two forms give the same bytes.  RTB_FORM_LEVELS is a launch a level each way (2 L launches).  RTB_FORM_TAIL gives every level from
 * tail_from on to one workgroup, which keeps them in LDS: tail_from is the least k >= 1 with R_k W_k 12 + ... + R_L W_L 12 bytes within
 * 160 KiB, the LDS of a compute unit (at 1920 x 1080 with eight levels that is level 4, 120 x 68, and 8 launches); where not even the
 * last level fits there is no tail and the form is RTB_FORM_LEVELS'.
 *
 * Whatever the image holds, nothing faults or reads outside a buffer: every address comes from the sizes alone. */
#ifndef RT_BLOOM_H
#define RT_BLOOM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTB_VERSION 1u

#define RTB_MAX_LEVELS 8u

#define RTB_MIX 0u               /* out = (1 - strength) q + strength b */
#define RTB_ADD 1u               /* out = q + strength b */

#define RTB_FORM_LEVELS 0u       /* a launch a level */
#define RTB_FORM_TAIL 1u         /* the small levels in one workgroup's LDS */

#define RTB_OK 0
#define RTB_ERR_BAD_ARG 1        /* a null pointer, a zero size, a value out of range, a misaligned buffer, buffers that alias */
#define RTB_ERR_LIMIT 2          /* sizes beyond what the kernels index: more than 2^31 - 1 pixels */
#define RTB_ERR_HIP 3            /* a launch failed */
#define RTB_ERR_INTERNAL 4       /* an exception was caught at the boundary */

typedef struct rtb_apply_args {
    uint32_t W, R;                /* the image: its columns and rows */
    uint32_t levels;              /* L, 1 ... RTB_MAX_LEVELS */
    uint32_t mode;                /* RTB_MIX or RTB_ADD */
    uint32_t form;                /* RTB_FORM_LEVELS or RTB_FORM_TAIL: the same bytes either way */
    uint32_t reserved;            /* 0 */
    float spread;                 /* in (0, 1] */
    float strength;               /* RTB_MIX: in (0, 1); RTB_ADD: finite and positive */
    float norm;                   /* finite and positive */
    float cap;                    /* in (0, 2^62] */
    float T, K;                   /* 0 <= K <= T <= cap; T = 0: no threshold */
    const float* in;              /* [R*W*3], 16-byte aligned; never written */
    float* out;                   /* [R*W*3], 16-byte aligned */
    float* out_bloom;             /* [R*W*3], 16-byte aligned, or NULL */
    void* scratch;                /* 16-byte aligned */
    uint64_t scratch_bytes;       /* at least rtb_scratch_bytes(W, R, levels) */
} rtb_apply_args;

int rtb_version(uint32_t* version);

/* The size of the scratch of an image of W columns and R rows with `levels` levels. */
int rtb_scratch_bytes(uint32_t W, uint32_t R, uint32_t levels, uint64_t* bytes);

/* The image with its bloom.  stream: a hipStream_t. */
int rtb_apply(const rtb_apply_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
