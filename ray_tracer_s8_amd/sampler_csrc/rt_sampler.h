/* rt_sampler.h — the private C declarations of librt_sampler.so, the film-sampler library: adaptive sampling for
 * ray_tracer_s8_amd/film_sampler.py.  From the per-pixel sample moments it decides which pixels still need samples, lists them per
 * strip in ascending order, gathers their camera rays and RNG states out of a strip's ray buffer, folds the traced colours back by
 * pixel and restates the sums at the film's count for the film's resolves.  Private: this header is not installed under include/,
 * the library is loaded by ray_tracer_s8_amd/_sampler_lib.py only, and nothing here is part of the tile ABI (include/rt_tile.h), of
 * the film library (film_csrc/rt_film.h) or of the history library (history_csrc/rt_history.h).
 *
 * Every function returns an int status (RTS_OK or an RTS_ERR_*) and catches everything inside its body.  rts_version and
 * rts_scratch_bytes are host arithmetic.  The others check their arguments before any launch, launch on the stream the caller gives
 * and check hipGetLastError after each launch.  There is no global state, no scene and no allocation: every buffer is the caller's
 * device memory, and a call returns once its launches are enqueued.
 *
 * NORMATIVE ARITHMETIC.  Every operation is one IEEE f32 rounding in the order written: no FMA, division and sqrt correctly rounded.
 * (float)n of an int32 rounds to nearest even.  A NaN that rts_select or rts_normalise computes is stored as the quiet NaN 0x7FC00000
 * (rts_fold's lines are the film fold's, and rts_gather copies bytes).
 *
 * The image.  W columns and R rows in strips of Hs rows, R a multiple of Hs; strip i is rows [i Hs, (i + 1) Hs), and pixel (x, y) of
 * it has the strip index p = (y - i Hs) W + x.  moments holds (S1, S2) per pixel, the sums of the samples' y = (c0 + c1) + c2 and of
 * y y; counts holds n, the samples folded into the pixel.
 *
 * rts_select.  Per pixel, with n_f = (float)n:
 *     m = S1 / n_f;  a = S2 / n_f;  d = a - m m;  d = d > 0 ? d : +0;  v = d / (n_f - 1);  err = sqrt(v) / (|m| + eps).
 *   A pixel with n < 2 is refused: it has no variance, its err is the quiet NaN and it is not noisy.  A pixel is NOISY iff
 *   err > threshold (false for a NaN).  A pixel is ACTIVE iff a pixel (x + dx, y + dy) with |dx|, |dy| <= dilate that lies in the
 *   image is noisy: the window crosses strip boundaries.  Written: the err plane; for strip i the strip indices of its active
 *   pixels, strictly ascending, from element i Hs W of `active` (the elements behind a strip's list are not written); the number
 *   of them in strip_counts[i].
 *   Four kernels: the metric and the noisy byte of every pixel; the active byte and the number of active pixels of every workgroup
 *   of 256 consecutive strip indices, by wave ballots; one workgroup per strip that scans those numbers in order; the write, where
 *   a pixel's position is the workgroup's scanned offset plus the active lanes below it in the workgroup (ballot and prefix
 *   popcount).  No atomic decides a position and no workgroup waits on another.
 *
 * rts_gather.  A strip chunk of k sample indices: record a k + j of out_rays and of out_states is record active[a] k + j of rays
 *   and of states, for a < n_active and j < k.  A record is 32 bytes.  Never in place: the outputs may not overlap the inputs.
 *   n_active == 0 returns RTS_OK without a launch.  An active[a] >= pixels copies nothing.
 *
 * rts_fold.  One lane per a < n_active, p = active[a]; in order j = 0 ... k - 1, with c = rgb[a k + j]:
 *     accum[p] += c per channel;  y = (c0 + c1) + c2;  S1 += y;  S2 += y y
 *   (the film fold's lines), then counts[p] += k.  The entries of active are distinct.  n_active == 0 returns RTS_OK without a launch.
 *
 * rts_normalise.  The sums "at the film's count" e0, so that the film's resolves, which divide by e0, read them.  Per pixel with
 *   n != e0, n_f = (float)n, e0_f = (float)e0:
 *     r = e0_f / n_f;  A' = A r per channel;  S1' = S1 r;
 *     m = S1 / n_f;  a = S2 / n_f;  d = a - m m;  d = d > 0 ? d : +0;            (d of the true count, as in rts_select)
 *     g = (e0_f - 1) / (n_f - 1);  mm = S1' / e0_f;  S2' = (mm mm + d g) e0_f.
 *   A pixel with n == e0 is copied byte for byte.  n >= 2; otherwise the values are unspecified.
 *   The film's entry variance on the primed sums is m' = S1' / e0_f = mm (the same operation on the same operands), a' = S2' / e0_f,
 *   d' = a' - mm mm clamped at +0, v0' = d' / (e0_f - 1).  The true-count variance is v = d / (n_f - 1).
 *   THE BOUND.  Let u = 2^-24, Q = fl(mm mm), t = fl(d g), and no operation overflow or underflow.  g carries one rounding and t one
 *   more: t = d (e0 - 1) / (n - 1) (1 + th2), |th2| <= 2u + u^2 (e0_f - 1 and n_f - 1 are exact up to 2^24).  The sum Q + t, the
 *   product by e0_f and the division by e0_f are three roundings: a' = (Q + t)(1 + th3), |th3| <= 3u + O(u^2), so a' - Q = t + eps
 *   with |eps| <= (3u + O(u^2)) (Q + t) <= (3u + O(u^2)) a' / (1 - 3u).  The subtraction and the division by e0_f - 1 are two more
 *   roundings, and v itself is one rounding from d / (n - 1).  The clamp only moves d' towards t >= 0.  So
 *       |v0' - v| <= 6u v + 4u a' / (e0_f - 1),
 *   five relative roundings on v's side and one on v, and three on a', the constants rounded up to cover the second-order terms.
 *
 * Values are finite as the film writes them; otherwise the results follow the arithmetic above, and nothing faults or reads outside
 * a buffer. */
#ifndef RT_SAMPLER_H
#define RT_SAMPLER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTS_VERSION 1u

#define RTS_OK 0
#define RTS_ERR_BAD_ARG 1        /* a null or misaligned pointer, a zero size, a value out of range, buffers that overlap */
#define RTS_ERR_LIMIT 2          /* an image beyond what the kernels index */
#define RTS_ERR_HIP 3            /* a launch failed */
#define RTS_ERR_INTERNAL 4       /* an exception was caught at the boundary */
#define RTS_ERR_SCRATCH 5        /* scratch_bytes below rts_scratch_bytes */

#define RTS_RECORD_BYTES 32u     /* a camera ray, and an RNG state */

typedef struct rts_select_args {
    uint32_t W, R, Hs;            /* the image and the rows of a strip: all non-zero, R a multiple of Hs */
    uint32_t dilate;              /* 0 or 1 */
    uint32_t reserved;            /* 0 */
    float threshold;              /* not a NaN, >= 0; +inf: no pixel is noisy */
    float eps;                    /* finite, > 0 */
    uint32_t reserved2;           /* 0 */
    const float* moments;         /* [R*W*2], 8-byte aligned */
    const int32_t* counts;        /* [R*W] */
    float* err;                   /* [R*W] written */
    uint32_t* active;             /* [R*W] written: strip i's list from element i*Hs*W */
    uint32_t* strip_counts;       /* [R/Hs] written */
    void* scratch;                /* rts_scratch_bytes(W, R, Hs), 8-byte aligned */
    uint64_t scratch_bytes;
} rts_select_args;

typedef struct rts_gather_args {
    uint32_t n_active;            /* <= pixels */
    uint32_t k;                   /* the chunk's sample indices, non-zero */
    uint32_t pixels;              /* Hs*W of the strip, non-zero */
    uint32_t reserved;            /* 0 */
    const uint32_t* active;       /* [n_active] */
    const void* rays;             /* [pixels*k] records, 16-byte aligned */
    const void* states;           /* [pixels*k] records, 16-byte aligned */
    void* out_rays;               /* [n_active*k] records, 16-byte aligned */
    void* out_states;             /* [n_active*k] records, 16-byte aligned */
} rts_gather_args;

typedef struct rts_fold_args {
    uint32_t n_active;            /* <= pixels */
    uint32_t k;                   /* non-zero */
    uint32_t pixels;              /* non-zero */
    uint32_t reserved;            /* 0 */
    const uint32_t* active;       /* [n_active], distinct */
    const float* rgb;             /* [n_active*k*3] */
    float* accum;                 /* [pixels*3] the strip's */
    float* moments;               /* [pixels*2] the strip's, 8-byte aligned */
    int32_t* counts;              /* [pixels] the strip's */
} rts_fold_args;

typedef struct rts_normalise_args {
    uint32_t W, R;                /* non-zero */
    uint32_t e0;                  /* the film's count, >= 2 and <= 2^24 */
    uint32_t reserved;            /* 0 */
    const float* accum;           /* [R*W*3] */
    const float* moments;         /* [R*W*2], 8-byte aligned */
    const int32_t* counts;        /* [R*W] */
    float* out_accum;             /* [R*W*3]; not an input */
    float* out_moments;           /* [R*W*2], 8-byte aligned; not an input */
} rts_normalise_args;

int rts_version(uint32_t* version);

/* The bytes of rts_select's scratch for a W x R image in strips of Hs rows. */
int rts_scratch_bytes(uint32_t W, uint32_t R, uint32_t Hs, uint64_t* bytes);

/* stream: a hipStream_t. */
int rts_select(const rts_select_args* args, void* stream);
int rts_gather(const rts_gather_args* args, void* stream);
int rts_fold(const rts_fold_args* args, void* stream);
int rts_normalise(const rts_normalise_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
