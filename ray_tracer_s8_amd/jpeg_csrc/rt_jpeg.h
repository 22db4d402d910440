/* rt_jpeg.h — the private C declarations of librt_jpeg.so, the JPEG library: a baseline JPEG encoder whose input is
 * an (R, W, 3) uint8 frame in device memory and whose output is a complete JFIF file in device memory, for
 * ray_tracer_s8_amd/frame_encoder.py.  Private: this header is not installed under include/, the library is loaded by
 * ray_tracer_s8_amd/_jpeg_lib.py only, it includes no csrc/ header, and nothing here is part of the tile ABI (include/rt_tile.h) or of
 * the film, history, sampler, upsample, robust and display libraries.
 *
 * Every function returns an int status (RTJ_OK or an RTJ_ERR_*) and catches everything inside its body.  rtj_encode enqueues on the
 * stream the caller gives and checks hipGetLastError after each launch.  There is no global state and no allocation: every buffer
 * is the caller's, a call returns once its work is enqueued, and nothing comes back to the host.
 *
 * THE FORMAT (normative; ITU-T T.81).  All arithmetic is in 32-bit two's-complement integers, >> is arithmetic, / truncates.
 *
 * File.  Baseline sequential DCT (SOF0), 8 bits, three components Y (id 1), Cb (2), Cr (3), each sampled 1 x 1, one interleaved scan;
 *   an MCU is one 8 x 8 block of Y, of Cb and of Cr, and MCUs go in raster order.  The segments: SOI; APP0 "JFIF\0" 1.01, units 0,
 *   density 1:1, no thumbnail; DQT table 0; DQT table 1 (8-bit entries in zigzag order); SOF0 (Y with table 0, Cb and Cr with table 1);
 *   DHT DC 0, AC 0, DC 1, AC 1, the tables of Annex K.3 (Y codes with DC 0 / AC 0, Cb and Cr with DC 1 / AC 1); DRI; SOS (Ss 0, Se 63,
 *   Ah Al 0); the entropy data; EOI.  SOI ... SOS are RTJ_HEADER_LEN = 629 bytes whatever the arguments.
 * Quantisation tables.  The caller's two tables of 64 entries 1 ... 255 in natural (row) order, or, from a quality 1 ... 100, the IJG
 *   rule over Annex K.1 (table 0) and K.2 (table 1): scale = quality < 50 ? 5000 / quality : 200 - 2 quality;
 *   entry = clamp((base scale + 50) / 100, 1, 255).
 * Colour, per pixel, from r, g, b in 0 ... 255:
 *   Y  = ( 19595 r + 38470 g +  7471 b + 32768) >> 16
 *   Cb = (-11059 r - 21709 g + 32768 b + (128 << 16) + 32767) >> 16
 *   Cr = ( 32768 r - 27439 g -  5329 b + (128 << 16) + 32767) >> 16,  each in 0 ... 255; every sum is below 2^24.
 * Padding.  Sample (x, y) of a block outside the frame is the frame's sample at (min(x, W - 1), min(y, R - 1)).
 * Transform.  d = sample - 128.  One 8-point pass over d[0 ... 7] (Loeffler, Ligtenberg and Moschytz; constants of 13 bits):
 *     t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4
 *     t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
 *     e1 = (t12 + t13) 4433;  o2 = e1 + t13 6270;  o6 = e1 + t12 (-15137)
 *     z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;  z5 = (z3 + z4) 9633
 *     p4 = t4 2446, p5 = t5 16819, p6 = t6 25172, p7 = t7 12299
 *     z1 = z1 (-7373), z2 = z2 (-20995), z3 = z3 (-16069) + z5, z4 = z4 (-3196) + z5
 *     o7 = p4 + z1 + z3, o5 = p5 + z2 + z4, o3 = p6 + z2 + z3, o1 = p7 + z1 + z4
 *   with D(x, n) = (x + (1 << (n - 1))) >> n.  The first pass runs over each row of the block and keeps 2 more bits:
 *     d0 = (t10 + t11) 4, d4 = (t10 - t11) 4, dk = D(ok, 11) for the other k.
 *   The second runs over each column of the result and takes them off: d0 = D(t10 + t11, 2), d4 = D(t10 - t11, 2), dk = D(ok, 15).
 *   The block is then the DCT times 8.  Bounds: the first pass yields |d| <= 4096 with every sum below 2^26; the second has sums of two
 *   inputs <= 2^13, of four <= 2^14 and z3 + z4 <= 2^15, so a line's three products and z5 stay below
 *   2^13 25172 + 2^14 20995 + 2^14 16069 + 2^15 9633 < 1.2e9 < 2^31, and yields |d| <= 8192.
 * Quantisation.  For coefficient c and table entry q: q8 = 8 q, v = (|c| + (q8 >> 1)) / q8, negated if c < 0: c / (8 q) rounded half
 *   away from zero.  |v| <= 1024, so a DC difference has category <= 11 and an AC coefficient category <= 10 (|AC| <= 1023 for 8-bit
 *   samples).  The coefficients are kept as int16 in zigzag order.
 * Entropy coding (T.81 F.1.2).  The category of v is the number of bits of |v|.  DC: diff = DC - predictor, the predictor the DC of
 *   the same component's last block and 0 at the start of a restart interval; the code of the category, then, if it is not 0, the low
 *   category bits of diff, or of diff - 1 if diff < 0.  AC, in zigzag order with run the zeros since the last non-zero coefficient:
 *   for a non-zero v, ZRL (0xF0) while run >= 16 (run -= 16), then the code of (run << 4) | category and the low category bits of v
 *   or v - 1; after the last coefficient EOB (0x00) if run > 0.  Bits go into bytes from the most significant end.
 * Restart intervals.  `interval` MCUs (1 ... 65535) form a restart interval; the last may be shorter; with interval >= the number
 *   of MCUs there is one.  Each interval's bits are padded with 1-bits to a byte; every 0xFF byte of entropy data, a padded last byte
 *   included, is followed by 0x00; interval k is followed by RST(k mod 8) (0xFF 0xD0 + k mod 8), the last by EOI (0xFF 0xD9).  DRI
 *   carries `interval` always.
 * Sizes.  A block takes at most 22 + 63 * 26 = 1660 bits: a DC code of at most 11 bits and 11 of amplitude, and per AC coefficient a
 *   code of at most 16 bits and 10 of amplitude (ZRL and EOB stand in for coefficients and are shorter).  With M MCUs in N intervals,
 *   raw_bound = ceil(M * 4980 / 8) + N covers the padding, and rtj_bound = 629 + 2 raw_bound + 2 N the stuffing and the markers.
 *   RTJ_ERR_LIMIT if 8 raw_bound or rtj_bound does not fit 32 bits (more than about 860 000 MCUs).
 *
 * THE DEVICE RECORD, eight 32-bit words written by rtj_encode's last kernel: 0 total, the bytes of the file; 1 raw, the entropy bytes
 *   before stuffing (every interval padded); 2 stuffed, the 0x00 bytes added; 3 intervals; 4 overflow, 1 if total > capacity;
 *   5 ... 7 zero.  On overflow nothing is written at or past out + capacity, the bytes below it are the file's, and total is still
 *   the true size.
 *
 * Whatever the frame holds, nothing faults or reads outside a buffer: every address comes from the sizes alone, or from bit counts
 * that are bounded by them. */
#ifndef RT_JPEG_H
#define RT_JPEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTJ_VERSION 1u

#define RTJ_HEADER_LEN 629u
#define RTJ_RECORD_WORDS 8u
#define RTJ_MAX_INTERVAL 65535u
#define RTJ_MAX_SIDE 65535u

#define RTJ_OK 0
#define RTJ_ERR_BAD_ARG 1        /* a null pointer, a zero size, a value out of range, a misaligned buffer, buffers that alias */
#define RTJ_ERR_LIMIT 2          /* sizes beyond what the kernels index */
#define RTJ_ERR_HIP 3            /* a launch or the clear of the scratch failed */
#define RTJ_ERR_INTERNAL 4       /* an exception was caught at the boundary */

typedef struct rtj_encode_args {
    uint32_t W, R;                /* the frame: its columns and rows, 1 ... 65535 */
    uint32_t quality;             /* 1 ... 100, or 0: the tables are `tables` */
    uint32_t interval;            /* MCUs a restart interval, 1 ... 65535 */
    const uint8_t* tables;        /* HOST memory, [2][64] in natural order, each 1 ... 255; NULL unless quality == 0 */
    const uint8_t* rgb;           /* device, [R][W][3], 4-byte aligned */
    void* scratch;                /* device, 256-byte aligned */
    uint64_t scratch_bytes;       /* at least rtj_scratch_bytes */
    uint8_t* out;                 /* device; its first header_len bytes are rtj_header's, written by the caller */
    uint64_t capacity;            /* the bytes of out, more than header_len */
    uint32_t header_len;          /* RTJ_HEADER_LEN */
    uint32_t reserved;            /* 0 */
    uint32_t* record;             /* device, [RTJ_RECORD_WORDS] */
} rtj_encode_args;

int rtj_version(uint32_t* version);

/* Host only: the bytes SOI ... SOS for args' W, R, quality or tables, and interval (nothing else of args is read) into out, HOST
 * memory of `capacity` bytes, and their number into *out_len.  RTJ_ERR_LIMIT if capacity is below RTJ_HEADER_LEN. */
int rtj_header(const rtj_encode_args* args, uint8_t* out, uint64_t capacity, uint64_t* out_len);

/* Host only: the most bytes a file of this frame can have. */
int rtj_bound(uint32_t W, uint32_t R, uint32_t interval, uint64_t* out_bytes);

/* Host only: the scratch rtj_encode needs. */
int rtj_scratch_bytes(uint32_t W, uint32_t R, uint32_t interval, uint64_t* out_bytes);

/* The entropy data and EOI after the header, and the record.  No buffer may overlap another.  stream: a hipStream_t. */
int rtj_encode(const rtj_encode_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
