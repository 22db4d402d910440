/* rt_display.h — the private C declarations of librt_display.so, the display library: the last stage of a film that
 * yields a linear HDR image, for ray_tracer_s8_amd/film_display.py.  A frame is metered into a luminance histogram, the histogram is
 * turned into an exposure record that stays in device memory, and the frame is scaled, tone-mapped and quantised under that record.
 * Private: this header is not installed under include/, the library is loaded by ray_tracer_s8_amd/_display_lib.py only, it includes no
 * csrc/ header, and nothing here is part of the tile ABI (include/rt_tile.h) or of the film, history, sampler, upsample and robust
 * libraries.
 *
 * Every function returns an int status (RTD_OK or an RTD_ERR_*), catches everything inside its body, enqueues on the stream the caller
 * gives and checks hipGetLastError after the launch.  There is no global state, no scene and no allocation: every buffer is the
 * caller's device memory, a call returns once its work is enqueued, and nothing comes back to the host.
 *
 * NORMATIVE ARITHMETIC.  Every operation is one IEEE f32 rounding in the order written: no FMA, division and sqrt correctly rounded,
 * no transcendental function.  Subnormal operands and results are kept.  Every comparison is as written: each is false for a NaN.
 *
 * rtd_meter.  The input is a linear image [R][W][3] of f32.  Per pixel y = (c0 + c1) + c2, the luminance the film's moments use.
 *   A pixel with y != y or !(y > 0) is excluded: NaN, both zeros and every negative y.  Otherwise u is y's bit pattern, q = u >> 20 (the
 *   exponent and three mantissa bits) and bin = clamp(q - 888, 0, 255): eight bins an octave over 2^-16 ... 2^16.  Every y below 2^-16,
 *   subnormals included, is in bin 0; every y from 2^15 1.875 up, +inf included, is in bin 255.
 *   The output is RTD_HIST_WORDS = 257 u32 counts: H[0 ... 255], and H[256], the excluded.  rtd_meter clears them and counts the image.
 *   The counts are exact integers: they do not depend on the order of anything or on the form (RTD_HIST_*) that counted them, and
 *   the sum of the 257 is R W.
 *
 * rtd_expose.  It turns the histogram into the exposure record, eight 32-bit words in device memory:
 *   word 0 scale, 1 white, 2 target (f32); 3 bin_key, 4 bin_white, 5 counted, 6 excluded, 7 frames (u32).
 *   The record is the memory of the adaptation: rtd_expose reads it and writes it, and the host never does.
 *   rep(b) is the float whose bits are ((b + 888) << 20) | 0x80000, the middle of bin b.
 *   RTD_AUTO.  N = H[0] + ... + H[255].  For a percentile q16 in 0 ... 65535: t = (uint32)(((uint64)N q16) >> 16), and bin(q16) is the
 *     least b with H[0] + ... + H[b] > t; it exists whenever N > 0, since t < N.
 *     If N > 0:
 *       bin_key = bin(key_q16);  bin_white = bin(white_q16);
 *       target = key / rep(bin_key);  target = target < scale_min ? scale_min : target;  target = target < scale_max ? target : scale_max;
 *       scale = target if the record's frames == 0 or rate >= 1; otherwise d = target - prev, scale = prev + rate d, prev the record's
 *       scale;
 *       white = (rep(bin_white) scale) / 3;  white = white > 1 ? white : 1.
 *     If N == 0: bin_key = bin_white = 0; a record with frames == 0 gets scale = 1, white = +inf, target = 1; any other record keeps
 *       its scale, white and target.
 *     Either way counted = N, excluded = H[256] and frames is incremented (it stays at 0xFFFFFFFF once there).
 *   RTD_MANUAL.  scale and white are the caller's, written as they are: each finite or +inf, scale > 0, white >= 1.  target = scale,
 *     bin_key = bin_white = 0, frames is incremented likewise; counted and excluded keep their values, and no histogram is read.
 *   The host refuses key, rate, scale_min and scale_max that are not finite and positive, scale_min > scale_max, rate > 1, a q16 above
 *   65535 and white_q16 < key_q16.
 *
 * rtd_apply.  It reads scale and white from the record, on the device.  Per channel value c of the image:
 *   1. x = c scale;  x = x > 0 ? x : +0  (a NaN and every negative give +0).
 *   2. RTD_NONE      t = x.
 *      RTD_REINHARD  w2 = white white;  t = (x (1 + x / w2)) / (1 + x);  t = t < 1 ? t : 1.
 *      RTD_FILMIC    n = x (2.51f x + 0.03f);  d = x (2.43f x + 0.59f) + 0.14f;  t = n / d;  t = t < 1 ? t : 1.
 *      (The last clamp also maps the NaN of inf / inf to 1: no NaN leaves step 2.)
 *   3. f = sqrt(t).  out_f32 = f.
 *   4. out_rgb = as_u8(f 255.999f) without dither; with dither as_u8(f 255 + ((float)B[row & 3][col & 3] + 0.5f) / 16), with B the
 *      4 x 4 Bayer matrix {0, 8, 2, 10; 12, 4, 14, 6; 3, 11, 1, 9; 15, 7, 13, 5} and (row, col) the pixel's.  as_u8 is the tile's:
 *      NaN and v <= 0 give 0, v >= 255 gives 255, every other v is truncated.
 *   Under RTD_NONE with scale = 1 and no dither out_rgb is sqrt(c) 255.999f through as_u8, the "rgb" of the film's resolves.
 *   Over the positive floats in ascending order t, and with it f and both quantisations, never decreases, for RTD_FILMIC and for
 *   RTD_REINHARD at every white (tests/test_display_host.py sweeps them).
 *
 * Whatever the image holds, nothing faults or reads outside a buffer: every address comes from the sizes alone, and a bin index is
 * clamped before it is used. */
#ifndef RT_DISPLAY_H
#define RT_DISPLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTD_VERSION 1u

#define RTD_HIST_WORDS 257u      /* H[0 ... 255] and the excluded */
#define RTD_RECORD_WORDS 8u

#define RTD_AUTO 0u              /* the exposure from the histogram */
#define RTD_MANUAL 1u            /* the caller's scale and white */

#define RTD_NONE 0u              /* the curves */
#define RTD_REINHARD 1u
#define RTD_FILMIC 2u

#define RTD_HIST_WAVE 0u         /* the histogram forms: an LDS histogram a wave, one LDS atomic a pixel */
#define RTD_HIST_MATCH 1u        /* equal bins of a wave aggregated first: one LDS add per distinct bin of a wave */

#define RTD_OK 0
#define RTD_ERR_BAD_ARG 1        /* a null pointer, a zero size, a value out of range, a misaligned buffer, buffers that alias */
#define RTD_ERR_LIMIT 2          /* sizes beyond what the kernels index: more than 2^31 - 1 pixels */
#define RTD_ERR_HIP 3            /* the launch failed */
#define RTD_ERR_INTERNAL 4       /* an exception was caught at the boundary */

typedef struct rtd_meter_args {
    uint32_t W, R;                /* the image: its columns and rows */
    uint32_t form;                /* RTD_HIST_WAVE or RTD_HIST_MATCH: the same counts either way */
    uint32_t reserved;            /* 0 */
    const float* linear;          /* [R*W*3] */
    uint32_t* hist;               /* [RTD_HIST_WORDS]; it may not overlap the image */
} rtd_meter_args;

typedef struct rtd_expose_args {
    uint32_t mode;                /* RTD_AUTO or RTD_MANUAL */
    float key;                    /* RTD_AUTO: what the key percentile's luminance is scaled to */
    uint32_t key_q16, white_q16;  /* RTD_AUTO: the percentiles, 0 ... 65535, key_q16 <= white_q16 */
    float rate;                   /* RTD_AUTO: in (0, 1]; 1 takes every frame's target as it is */
    float scale_min, scale_max;   /* RTD_AUTO: the clamps of the target */
    float scale, white;           /* RTD_MANUAL */
    uint32_t reserved;            /* 0 */
    const uint32_t* hist;         /* [RTD_HIST_WORDS]; RTD_MANUAL: not read, and may be NULL */
    uint32_t* record;             /* [RTD_RECORD_WORDS], read and written; it may not overlap the histogram */
} rtd_expose_args;

typedef struct rtd_apply_args {
    uint32_t W, R;                /* the image */
    uint32_t curve;               /* RTD_NONE, RTD_REINHARD or RTD_FILMIC */
    uint32_t dither;              /* 0 or 1 */
    const float* linear;          /* [R*W*3], 16-byte aligned */
    const uint32_t* record;       /* [RTD_RECORD_WORDS] */
    float* out_f32;               /* [R*W*3], 16-byte aligned, or NULL */
    uint8_t* out_rgb;             /* [R*W*3], 4-byte aligned, or NULL; at least one output, and none may overlap another buffer */
} rtd_apply_args;

int rtd_version(uint32_t* version);

/* The histogram of an image: the 257 counts cleared and counted.  stream: a hipStream_t. */
int rtd_meter(const rtd_meter_args* args, void* stream);

/* The exposure record from the histogram, or from the caller's values.  stream: a hipStream_t. */
int rtd_expose(const rtd_expose_args* args, void* stream);

/* The displayed image under the record.  stream: a hipStream_t. */
int rtd_apply(const rtd_apply_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
