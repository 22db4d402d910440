/* rt_history.h — the private C declarations of librt_history.so, the film-history library: temporal accumulation
 * for ray_tracer_s8_amd/film_history.py.  The last frame's colour sums, moments and history length are reprojected into the current
 * frame by the current frame's depth and the two camera poses, optionally clipped to the current frame's colour box (step 5a), and
 * blended with the current frame's.  Private: this header is not
 * installed under include/, the library is loaded by ray_tracer_s8_amd/_history_lib.py only, and nothing here is part of the tile ABI
 * (include/rt_tile.h) or of the film library (film_csrc/rt_film.h).
 *
 * Every function returns an int status (RTH_OK or an RTH_ERR_*), catches everything inside its body, launches on the stream the
 * caller gives and checks hipGetLastError after each launch.  There is no global state, no scene and no allocation: every buffer is
 * the caller's device memory, and a call returns once its launch is enqueued.
 *
 * NORMATIVE ARITHMETIC.  Every operation is one IEEE f32 rounding in the order written: no FMA, division and sqrt correctly
 * rounded, no transcendental function on the device.  dot(a, b) = (a0 b0 + a1 b1) + a2 b2.  A vector expression is evaluated per
 * component, left to right.
 *
 * The film.  W columns and R rows; film row r is global row y0 + r of an H-row frame, y0 = division_no Hs, Hs = H / divisions, with
 * the division_no of the film's first strip.  Both frames of a call agree on W, H, divisions and division_no.
 *
 * Cameras, on the host.  For each frame the call gives the request fields rtplan::fill_camera reads and an rt_camera or none.
 *   - The current frame's org, llc, hor, ver, u_den, v_den are fill_camera's (csrc/rt_plan.h), with the pose of make_pose, or the
 *     reference camera's code path when no camera is given: the vectors the frame's passes and features were rendered with.
 *   - The previous frame's basis (org', u', v', w') is make_pose of its rt_camera, or of rt_camera_defaults' pose when none is given;
 *     vh' = 2 tan(fov / 2), vw' = ((float)width / (float)height) vh', f' = focal_length, u_den' and v_den' as fill_camera takes them.
 *
 * Current pixel p = (x, r), with the film's accum C[3], moments (S1, S2), and the feature sums depth, hits, index and (optionally)
 * normal n[3], as rt_scene_render_aovs_device writes them.
 *   1. hits == 0: no history, and the stored z is +0.  Otherwise z = depth / (float)hits.
 *   2. No previous frame (the first frame of a history), or index == RT_HIT_NONE: no history.
 *   3. The pixel's centre ray, camera_ray (csrc/rt_path_steps.hip.h) with both jitter draws 0.5 and no lens offset:
 *        u = ((float)x + 0.5) / u_den;  v = ((float)(H - (y0 + r) - 1) + 0.5) / v_den;
 *        e = ((llc + u hor) + v ver) - org;  k = 1 / sqrt(dot(e, e));  e1 = k > 0 and k < inf ? e k : 0   (normalize_or_zero)
 *        d = e1 / sqrt(dot(e1, e1))                                                                      (Ray::new's normalize)
 *      X = org + z d.
 *   4. Into the previous camera: q = X - org';  cx = dot(q, u');  cy = dot(q, v');  cz = -dot(q, w').  cz not > 0: no history.
 *        t = f' / cz;  sx = cx t;  sy = cy t;
 *        fx = (sx / vw' + 0.5) u_den' - 0.5;  cv = (sy / vh' + 0.5) v_den' - 0.5;  fy = ((float)(H - 1) - cv) - (float)y0.
 *      (fx, fy) is the continuous position in the film whose integer values are pixel centres: the inverse of camera_ray's u and v.
 *      Unless fx > -1 and fx < (float)W and fy > -1 and fy < (float)R (a NaN fails it): no history; no tap could lie inside.
 *      z' = sqrt(dot(q, q)).
 *   5. Taps.  x0 = floor(fx), y0t = floor(fy), ax = fx - (float)x0, ay = fy - (float)y0t.  For dy in (0, 1) outer and dx in (0, 1)
 *      inner: the tap is (x0 + dx, y0t + dy) with weight w = (dx ? ax : 1 - ax) (dy ? ay : 1 - ay).  It is admitted only if, tested
 *      in this order, it lies inside the film; its stored length is >= 1; its stored index is not RT_HIT_NONE and equals the current
 *      index; |z' - z_stored| <= k_depth z'; and, in a call with normals, c = dot(n, n_stored) > 0 and
 *      c c >= k_normal^2 (dot(n, n) dot(n_stored, n_stored)), with k_normal^2 = k_normal k_normal rounded once on the host.  No
 *      address is formed for a tap that is not inside.
 *      From +0, in tap order: Sw += w;  Sc += w C_q per channel;  S1w += w S1_q;  S2w += w S2_q;  Sn += w N_q.
 *      No admitted tap, or Sw not > 0: no history.  Otherwise Ch = Sc / Sw, S1h = S1w / Sw, S2h = S2w / Sw, Nh = Sn / Sw.
 *   5a. Clip, only in a call with clip_gamma > 0: g = clip_gamma, rho = clip_radius in {1, 2}, e_f = (float)samples.
 *      The history that reached the blend is rectified to the colour statistics of the current frame around the pixel.
 *      Window.  For dy = -rho ... rho outer and dx = -rho ... rho inner, q = (x + dx, r + dy).  A tap outside the film is skipped and
 *      no address is formed for it; the centre is always inside.  From +0, in tap order: n += 1 (an integer), and per channel k
 *      A_k += C_q[k];  B_k += C_q[k] C_q[k].  C is the current frame's accum.
 *      Box.  n_f = (float)n;  mu_k = A_k / n_f;  d_k = B_k / n_f - mu_k mu_k;  d_k = d_k > 0 ? d_k : +0;  s_k = g sqrt(d_k);
 *        lo_k = mu_k - s_k;  hi_k = mu_k + s_k.
 *      Clip.  Ch'_k = Ch_k < lo_k ? lo_k : (Ch_k > hi_k ? hi_k : Ch_k).  A NaN bound never clips.
 *      Moments.  If neither comparison was taken for any channel, Ch, S1h and S2h go on unchanged, bit for bit, and amount = +0.
 *      Otherwise y = (Ch_0 + Ch_1) + Ch_2 and y' = (Ch'_0 + Ch'_1) + Ch'_2;
 *        S1h' = S1h + (y' - y), then S1h' = S1h' > 0 ? S1h' : +0;
 *        S2h' = S2h + (S1h' S1h' - S1h S1h) / e_f, then S2h' = S2h' > 0 ? S2h' : +0;
 *        amount = (|Ch_0 - Ch'_0| + |Ch_1 - Ch'_1|) + |Ch_2 - Ch'_2|.
 *      Step 6 then blends Ch', S1h' and S2h'; Nh is not touched.  A pixel with "no history" has amount = +0.
 *      What the shift keeps.  v = S2h - S1h^2 / e is the history's own spread (e times the resolve's variance of the mean, before its
 *      normalisation); the clip moves the history's mean and leaves v, so the guided resolve's variance stays that of the history.
 *      To the roundings: with u = 2^-24, a = S1h'^2, b = S1h^2 and no clamp of S2h' taken, the products round to a (1 + d1) and
 *      b (1 + d2), their difference once more, the quotient by e_f once more and the sum with S2h once more, every |d| <= u.  The
 *      first three leave (a - b) / e off by at most (u (a + b) + 2 u |a - b|) / e <= 3 u (a + b) / e to first order, and the last
 *      rounding adds at most u S2h' / (1 - u).  So  |(S2h' - S1h'^2 / e) - v| <= 2^-23 S2h' + 2^-22 (S1h^2 + S1h'^2) / e,  where the
 *      factors 2 and 4/3 over the first-order terms take every higher-order term.  (tests/test_history_clip_host.py holds it to that.)
 *   6. Blend.  N = Nh + 1, and N = n_max if N > n_max.  a = 1 / N, and a = alpha if alpha > a.  b = 1 - a.  Each of the five values
 *      C[0..2], S1, S2 becomes b h + a c (two products, one sum).
 *   "No history": the five outputs are the current values bit for bit and N = 1.
 *
 * Stored for the next frame, per pixel: the blended C, S1, S2 and N, the frame's z and index, and the normal sum if the call has one.
 * State is held in two sets of planes that the caller alternates: a call reads `prev` and writes `next`, never the same memory.
 *
 * Why sums may be blended.  C, S1 and S2 are sums over the film's sample count e, on both sides of the blend; blending two sums at
 * equal e is e times blending the means.  So next.accum and next.moments have exactly the layout and meaning rtf_resolve and
 * rt_scene_denoise_device take with samples = e, which is why every frame of a history has the same e.  The variance the guided
 * resolve derives from blended moments is SVGF's: the variance of the integrated signal at e samples per frame, NOT divided by the
 * history length.  It steers the edge-stop; it is not the variance of the blended mean.
 *
 * Subnormal, infinite and NaN inputs.  The film writes finite sums, but no value of a plane or of the previous state is refused, and
 * nothing faults or reads outside a buffer whatever they hold: the one index that depends on a plane's value is the reprojected
 * position (fx, fy), which step 4 tests against the film's bounds before it is converted to an integer (a NaN or an infinity fails
 * that test: "no history"), and every tap is tested against the bounds again.  The arithmetic above proceeds as IEEE 754 defines it
 * for every operand, with subnormal operands and results kept (nothing is flushed to zero), signed zeros and infinities as the
 * operations make them, and every comparison as written: each is false for a NaN, so `!(x <= lim)` rejects a tap whose distance is
 * a NaN, `N > n_max` and `alpha > a` keep a NaN, the clip leaves a channel alone whose bound or value is a NaN, and
 * `d > 0 ? d : +0` gives +0 for a NaN and for -0.  (float)hits is the correctly rounded conversion, above 2^24 too.  Where the text
 * yields a NaN the output is a NaN, of unspecified payload and sign, and it stays in the state for the frames that read it.  Every
 * other output value, the signs of zeros included, is the one the text defines (DESIGN.md 4.28:
 * tests/test_gpu_film_extremes.py holds the kernels to it, both forms of the clip among them). */
#ifndef RT_HISTORY_H
#define RT_HISTORY_H

#include <stdint.h>

#include "rt_tile.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTH_VERSION 2u

/* The two forms of a clipping call's kernel, which give the same bytes: the window staged in LDS by the workgroup, or read by
 * every lane from memory.  clip_form = 0 takes the faster one as measured: direct at radius 1, staged at radius 2. */
#define RTH_CLIP_FORM_STAGED 1u
#define RTH_CLIP_FORM_DIRECT 2u

#define RTH_OK 0
#define RTH_ERR_BAD_ARG 1        /* a null pointer, a zero size, a value out of range, a pose make_pose refuses, frames that differ */
#define RTH_ERR_LIMIT 2          /* a film beyond what the kernel indexes */
#define RTH_ERR_HIP 3            /* the launch failed */
#define RTH_ERR_INTERNAL 4       /* an exception was caught at the boundary */

/* One set of state planes, each [R*W] records.  normal: NULL in a call without normals. */
typedef struct rth_state {
    float* accum;                 /* [R*W*3] blended colour sums: rtf_resolve's accum */
    float* moments;               /* [R*W*2] blended S1, S2: rtf_resolve's moments */
    float* length;                /* [R*W] N */
    float* depth;                 /* [R*W] z */
    uint32_t* index;              /* [R*W] */
    float* normal;                /* [R*W*3] or NULL */
} rth_state;

typedef struct rth_accumulate_args {
    uint32_t W, R;                /* the film */
    uint32_t have_prev;           /* 0: the first frame of a history; prev, prev_request and prev_camera are not read */
    uint32_t reserved;            /* 0 */
    float alpha;                  /* 0 < alpha <= 1 */
    float n_max;                  /* >= 1 */
    float k_depth, k_normal;      /* finite, >= 0; k_normal is read only in a call with normals */
    const rt_tile_request* request;        /* the film's first strip: width == W, height, divisions, division_no, and the camera fields */
    const rt_camera* camera;               /* the frame's camera, NULL: the reference camera */
    const rt_tile_request* prev_request;   /* the same of the previous frame */
    const rt_camera* prev_camera;
    const float* accum;           /* [R*W*3] the film's accum */
    const float* moments;         /* [R*W*2] the film's moments */
    const float* depth;           /* [R*W] feature sums */
    const uint32_t* hits;         /* [R*W] */
    const uint32_t* index;        /* [R*W] */
    const float* normal;          /* [R*W*3] or NULL: a call with normals has it and both states' normal planes */
    rth_state prev;               /* read */
    rth_state next;               /* written; no plane of it may be one of prev's or an input */
    float clip_gamma;             /* 0: no clip, and none of the fields below is read; otherwise finite and > 0 (step 5a) */
    uint32_t clip_radius;         /* 1 or 2 */
    uint32_t samples;             /* e, the film's sample count: >= 1 */
    uint32_t clip_form;           /* 0: the library's choice; RTH_CLIP_FORM_*: private, for tests and tools; another value is refused */
    float* clip_amount;           /* [R*W] the amount of every pixel, or NULL; 4-byte aligned, none of the call's other planes */
} rth_accumulate_args;

int rth_version(uint32_t* version);

/* One frame into the history.  stream: a hipStream_t. */
int rth_accumulate(const rth_accumulate_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
