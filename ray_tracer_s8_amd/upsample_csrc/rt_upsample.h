/* rt_upsample.h — the private C declarations of librt_upsample.so, the film-upsampler library: joint-bilateral
 * upsampling for ray_tracer_s8_amd/film_upsampler.py.  A linear image of a low-resolution film is reconstructed at s times the
 * resolution, s in 2 ... 4, with the edges taken from feature buffers rendered at both resolutions; with the albedo divided out of the
 * low-resolution colour and the full-resolution albedo multiplied back in.  Private: this header is not installed under include/, the
 * library is loaded by ray_tracer_s8_amd/_upsample_lib.py only, and nothing here is part of the tile ABI (include/rt_tile.h) or of
 * the film, history and sampler libraries.
 *
 * Every function returns an int status (RTU_OK or an RTU_ERR_*), catches everything inside its body, launches on the stream the
 * caller gives and checks hipGetLastError after the launch.  There is no global state, no scene and no allocation: every buffer is
 * the caller's device memory, and a call returns once its launch is enqueued.
 *
 * NORMATIVE ARITHMETIC.  Every operation is one IEEE f32 rounding in the order written: no FMA, division and sqrt correctly
 * rounded, no transcendental function on the device.  dot(a, b) = (a0 b0 + a1 b1) + a2 b2.  A vector expression is evaluated per
 * component, left to right.
 *
 * The two frames.  One scene under one camera, rendered twice: the low frame of Wl x Hl pixels and the high frame of Wh x Hh, with
 * Wh = s Wl, Hh = s Hl and an integer s in 2 ... 4.  Their f32 aspect ratios (float)W / (float)H are therefore the same bits, so
 * rtplan::fill_camera (csrc/rt_plan.h) gives both the same frustum; they agree on fov, focal_length, aperture and focus_distance,
 * which this library never reads.  The low film holds rows [y0l, y0l + Rl) of its frame and the output rows [y0h, y0h + Rh) of the
 * high one, y0 = division_no (H / divisions) of the first strip on each side.  Per frame, on the host and exactly as fill_camera
 * forms them:  aspect = (float)W / (float)H;  u_den = aspect (float)H - 1;  v_den = (float)H - 1.
 *
 * Inputs.  L: the low-resolution linear mean colour, [Rl Wl 3].  Per side the feature SUMS as rt_scene_render_aovs_device writes them,
 * with their sample counts kl and kh: albedo A[3], normal n[3], depth D, hits h, index i.  Each plane is optional, on both sides
 * together; depth needs hits.  The albedo planes switch the demodulation on, with eps (finite, > 0).  A call without the hits planes
 * takes every pixel as hit where a test below says "where both hit".
 *
 * Per output pixel (x, r), with the high side's values Ah, nh, Dh, hh, ih at (x, r):
 *   1. zh = hh > 0 ? Dh / (float)hh : +0.  For a tap, zl is formed the same way from Dl and hl.
 *   2. The position in the low film (the inverse of camera_ray's u and v, as rt_history.h step 4):
 *        u = ((float)x + 0.5) / u_den_h;                         fx = u u_den_l - 0.5;
 *        v = ((float)(Hh - (y0h + r) - 1) + 0.5) / v_den_h;      cv = v v_den_l - 0.5;
 *        fy = ((float)(Hl - 1) - cv) - (float)y0l;
 *        x0 = floor(fx), y0t = floor(fy), ax = fx - (float)x0, ay = fy - (float)y0t.
 *   3. Taps.  For dy in (0, 1) outer and dx in (0, 1) inner the tap q is (clamp(x0 + dx, 0, Wl - 1), clamp(y0t + dy, 0, Rl - 1)) with
 *      the weight b = (dx ? ax : 1 - ax) (dy ? ay : 1 - ay).  Clamp to the edge: every address formed is inside the film.  A tap is
 *      ADMITTED if every test whose planes the call has passes, in this order:
 *        index:   il == ih  (RT_HIT_NONE equals itself: sky matches sky);
 *        hits:    (hl == 0) == (hh == 0);
 *        depth    (only where both hit):  |zh - zl| <= k_depth zh;
 *        normal   (only where both hit):  c = dot(nh, nl) > 0 and c c >= k_normal^2 (dot(nh, nh) dot(nl, nl)), with
 *                 k_normal^2 = k_normal k_normal rounded once on the host.
 *   4. The tap's value.  V_q[k] = L_q[k], or with albedo V_q[k] = L_q[k] / (Al_q[k] / (float)kl + eps): the divisor is albedo_d of
 *      csrc/rt_denoise_math.h.
 *   5. The weighted sum.  From +0, in tap order over the admitted taps:  Sw += b;  Sv[k] += b V_q[k].  If Sw > 0:  V = Sv / Sw, class 0.
 *      Otherwise (nothing admitted, or only zero weights) the same sums run over all four taps unconditionally: V = Sv / Sw, class 1.
 *      That is the plain bilinear value, which always has Sw > 0.
 *   6. out[k] = V[k], or with albedo V[k] (Ah[k] / (float)kh + eps).
 *   7. Outputs, each optional and at least one given.  out_linear is out.  out_f32 and out_rgb apply the exit transform of the
 *      denoiser and of rtf_resolve, rtdn::output_pixel of csrc/rt_denoise_math.h: f = sqrt(out), and the byte is f 255.999 under the
 *      tile's `as u8` rule.  out_class is [Rh Wh] uint8, the class of step 5.
 *
 * What class 0 keeps: the roundings.  With u = 2^-24: each of Sv and Sw takes at most four product roundings and three sum
 * roundings (the first sum, from +0, is exact), and V one quotient.  Where every admitted V_q is one value c, Sv = c Sw up to those
 * roundings, so V is within 15 u < 2^-20 of c, relatively, to first order, the slack to 2^-20 taking every higher-order term.
 * (tests/test_upsample_host.py holds the restatement to that.)
 *
 * Subnormal, infinite and NaN inputs.  The film writes finite sums, but no value of a plane is refused, and nothing faults or reads
 * outside a buffer whatever the planes hold: every tap address comes from the two frames' sizes alone and is clamped into the low
 * film.  The arithmetic above proceeds as IEEE 754 defines it for every operand, with subnormal operands and results kept (nothing
 * is flushed to zero), signed zeros and infinities as the operations make them, and every comparison as written: each is false for
 * a NaN, so a tap whose depth or normal test meets a NaN is rejected, and `!(Sw > 0)` sends a pixel whose weights sum to a NaN to
 * class 1.  (float)hits is the correctly rounded conversion, above 2^24 too; eps + A / k = 0 divides by zero as IEEE does.  Where
 * the text yields a NaN the output is a NaN, of unspecified payload and sign; `as u8` of a NaN is 0.  Every other output value, the
 * signs of zeros included, is the one the text defines (tests/test_gpu_film_extremes.py holds the kernel to it). */
#ifndef RT_UPSAMPLE_H
#define RT_UPSAMPLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTU_VERSION 1u

#define RTU_MIN_SCALE 2u
#define RTU_MAX_SCALE 4u

#define RTU_OK 0
#define RTU_ERR_BAD_ARG 1        /* a null pointer, a zero size, a value out of range, frames that do not fit, buffers that alias */
#define RTU_ERR_LIMIT 2          /* a frame beyond what the kernel indexes: more than 2^31 - 1 output pixels, a side of 2^24 or more */
#define RTU_ERR_HIP 3            /* the launch failed */
#define RTU_ERR_INTERNAL 4       /* an exception was caught at the boundary */

/* The feature sums of one side, each [R*W] records, and their sample count.  A plane that is NULL on one side is NULL on the other. */
typedef struct rtu_planes {
    const float* albedo;          /* [R*W*3] or NULL; given: the call demodulates */
    const float* normal;          /* [R*W*3] or NULL */
    const float* depth;           /* [R*W] or NULL; needs hits */
    const uint32_t* hits;         /* [R*W] or NULL */
    const uint32_t* index;        /* [R*W] or NULL */
    uint32_t samples;             /* k >= 1: the samples the sums hold; read only with albedo */
    uint32_t reserved;            /* 0 */
} rtu_planes;

typedef struct rtu_upsample_args {
    uint32_t Wl, Rl, Hl, y0l;     /* the low film: its columns and rows, its frame's rows, its first global row */
    uint32_t Wh, Rh, Hh, y0h;     /* the output, likewise: Wh = scale Wl, Hh = scale Hl */
    uint32_t scale;               /* RTU_MIN_SCALE ... RTU_MAX_SCALE */
    uint32_t form;                /* 0: the library's choice.  One form exists (every lane reads its taps from memory): another value is refused */
    float k_depth, k_normal;      /* finite, >= 0; read only with the planes they test */
    float eps;                    /* finite, > 0; read only with albedo */
    uint32_t reserved;            /* 0 */
    const float* linear;          /* [Rl*Wl*3] L */
    rtu_planes lo, hi;
    float* out_linear;            /* [Rh*Wh*3] or NULL */
    float* out_f32;               /* [Rh*Wh*3] or NULL */
    uint8_t* out_rgb;             /* [Rh*Wh*3] or NULL */
    uint8_t* out_class;           /* [Rh*Wh] or NULL; no output may overlap an input or another output */
} rtu_upsample_args;

int rtu_version(uint32_t* version);

/* One upsampling.  stream: a hipStream_t. */
int rtu_upsample(const rtu_upsample_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
