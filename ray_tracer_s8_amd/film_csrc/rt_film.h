/* rt_film.h — the private C declarations of librt_film.so, the film library: the moments fold, the
 * variance-guided a-trous resolve and the feature-regression resolve of ray_tracer_s8_amd/film.py.  Private: this header is not installed under include/, the library is
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
 * Regression resolve (kind RTF_RESOLVE_REGRESS) over the image P, e = samples >= 1, e_f = (float)e,
 * k_f = (float)aov_samples, T = 16: the colour is fitted, window by window, as a linear function of eight features of the noise-free
 * planes, and every pixel takes the bilinear blend of the four fits around it.
 *   Per pixel p = (x, y):
 *     d_p = rtdn::albedo_d(A_p, k_f, albedo_eps) when the albedo is given;  r_p = rtdn::entry_color(C_p, e_f, d_p or nullptr);
 *     g_p = rtdn::entry_guide(N_p, D_p, hits_p), absent planes as nullptr.  p is VALID iff g_p.zg >= 0: without a hits plane every
 *     pixel is, with one a pixel no sample of which hit anything is not.  z_p = g_p.zg > 0 ? g_p.zg : +0.
 *   Nodes: NX = (W-1)/16 + 2, NY = (R-1)/16 + 2 (integer division).  Node (i, j) has the window of the pixels with
 *     16i-16 <= x < 16i+16 and 16j-16 <= y < 16j+16 that lie inside P, at most 32 x 32.  Window-local coordinates wx = x-(16i-16),
 *     wy = y-(16j-16); the window lane is l = 32*wy + wx.
 *   Window statistics: n = the number of valid pixels of the window, n_f = (float)n;  zlo = the fmin of z_p over them, zhi the fmax
 *     (a NaN operand is ignored, so both are independent of order); both +0 when n = 0 or no depth plane is given;  s = zhi - zlo.
 *   Features of a pixel in node (i, j), M = 8:  phi0 = 1;  phi1..3 = g_p.nx, ny, nz;  zeta = s > 0 ? (z_p - zlo)/s : +0,
 *     phi4 = zeta, phi5 = zeta*zeta;  phi6 = ((float)(x-16i) + 0.5f)/16,  phi7 = ((float)(y-16j) + 0.5f)/16 (both exact).
 *   The window sum S(v) of per-lane values v_l, +0 for a lane outside P or an invalid pixel: for each group k = 0 ... 15 of 64
 *     consecutive lanes, t_k is the adjacent-pair tree over the group's 64 values (six levels, level 0 adds v[2m] + v[2m+1], level 1
 *     those sums in adjacent pairs, and so on);  S = ((+0 + t_0) + t_1) + ... + t_15.  Every sum below is this one sum, whatever the
 *     launch shape; there are no atomics.  (On the device: the xor butterfly of a wave, then the sixteen wave totals in order.)
 *   The normal equations: A_ab = S(phi_a*phi_b) for a <= b;  B_ac = S(phi_a*r_c), c = 0, 1, 2;  then
 *     A_aa = A_aa + ridge*n_f for a >= 1.
 *   Cholesky, a = 0 ... 7:  p = A_aa, then p = p - L_at*L_at for t = 0 ... a-1 in order; if !(p > 0) the fit FAILS (and stops);
 *     L_aa = sqrt(p);  for b > a: q = A_ab, then q = q - L_bt*L_at for t = 0 ... a-1 in order, L_ba = q/L_aa.
 *   Solving, per channel c:  forward, a = 0 ... 7: y_a = B_ac, then y_a = y_a - L_at*y_t for t = 0 ... a-1 in order, y_a = y_a/L_aa;
 *     back, a = 7 ... 0: w_ac = y_a, then w_ac = w_ac - L_ta*w_tc for t = a+1 ... 7 in order, w_ac = w_ac/L_aa.
 *     On a failed fit or n = 0:  w_0c = n > 0 ? B_0c/n_f : +0, every other w is +0.
 *   The node's record in `model`: 32 floats at ((j*NX + i)*32): w_ac at 3a+c;  zlo at 24, s at 25, n_f at 26;  word 27 the fit flag,
 *     1.0f solved, 0.0f the constant fallback;  words 28 ... 31 +0.
 *   Apply, per pixel p: an invalid pixel keeps r' = r_p, bit for bit.  Otherwise ci = x>>4, cj = y>>4,
 *     fx = ((float)(x&15)+0.5f)/16, fy likewise; the four nodes in the order (ci,cj), (ci+1,cj), (ci,cj+1), (ci+1,cj+1) have the
 *     weights (1-fx)*(1-fy), fx*(1-fy), (1-fx)*fy, fx*fy (all exact).  m_c = the sum over a ascending, from +0, of w_ac*phi_a, phi
 *     formed with that node's zlo, s, i, j;  r'_c = the sum over the four nodes in that order, from +0, of weight*m_c;  then
 *     r'_c = r'_c > 0 ? r'_c : +0 (the valid pixels only).
 *   Outputs (each optional, at least one): rtdn::output_pixel(r', d_p or nullptr, lin, f32, rgb).
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

#define RTF_VERSION 2u

#define RTF_OK 0
#define RTF_ERR_BAD_ARG 1        /* a null pointer, a zero size, a value out of range */
#define RTF_ERR_LIMIT 2          /* an image or a strip beyond what the kernels index */
#define RTF_ERR_SCRATCH 3        /* scratch_bytes < rtf_resolve_scratch_bytes(W, R), or model_bytes < NX*NY*128 */
#define RTF_ERR_HIP 4            /* a HIP call or a launch failed */
#define RTF_ERR_INTERNAL 5       /* an exception was caught at the boundary */

#define RTF_MAX_ITERATIONS 8u
/* lds_max_step: the largest step whose window is staged in LDS; 0: every step loads directly; RTF_LDS_PLAN (or anything above
 * 2^30): the plan's own choice, rtplan::DN_LDS_MAX_STEP.  A window that does not fit a CU's LDS loads directly whatever it says. */
#define RTF_LDS_PLAN 0xFFFFFFFFu

/* The kinds of a resolve call. */
#define RTF_RESOLVE_ATROUS 0u     /* the variance-guided a-trous */
#define RTF_RESOLVE_REGRESS 1u    /* the local feature regression */
#define RTF_REGRESS_RECORD 32u    /* the floats of a node's record in `model` */

/* The planes a resolve call reads: rtdn::P_NORMAL, P_DEPTH, P_HITS (and P_ALBEDO, kind 1) by which pointers are set (depth needs
 * hits).
 * Kind 0 needs samples >= 2, accum, moments and scratch, and every field after out_variance 0 or NULL.
 * Kind 1 needs samples >= 1, iterations == 0, out_variance == NULL, one of out_rgb, out_f32, out_linear, accum, a 16-byte aligned
 * model of model_bytes >= NX*NY*128 (RTF_ERR_SCRATCH otherwise), a finite ridge > 0, aov_samples >= 1 whenever a plane is given and,
 * with albedo, a finite albedo_eps > 0; moments and scratch may be NULL, and lds_max_step, sigma_l, var_eps, k_normal and k_depth are
 * not read. */
typedef struct rtf_resolve_args {
    uint32_t W, R;                /* the image P */
    uint32_t samples;             /* e >= 2 (kind 1: e >= 1) */
    uint32_t iterations;          /* I <= RTF_MAX_ITERATIONS */
    uint32_t lds_max_step;
    uint32_t kind;                /* RTF_RESOLVE_* */
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
    const float* albedo;          /* [R*W*3] or NULL (kind 1) */
    uint32_t aov_samples;         /* k: the samples of the planes (kind 1) */
    float albedo_eps;
    float ridge;
    uint32_t reserved;            /* 0 */
    float* model;                 /* [NY*NX*32]: the records of the fit (kind 1) */
    uint64_t model_bytes;
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
