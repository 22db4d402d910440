// rt_jpeg_math.h — the per-pixel, per-block and per-symbol arithmetic of the JPEG library (rt_jpeg.h): the colour
// transform, the two passes of the 8-point integer DCT, the quantisation, the tables of T.81 Annex K, the header's bytes, the bit count
// of a block and its symbols.  Plain C++ that compiles as HIP device code (rt_jpeg.hip.h) and under g++ (tests/host/jpeg_host.cpp), so
// the kernels and the CPU harness run the same lines.  Every operation is a 32-bit integer one in the order rt_jpeg.h writes it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HOST_DEVICE __host__ __device__ inline
#else
#define RT_HOST_DEVICE inline
#endif
// a table the device code indexes: device memory in the device pass, host memory otherwise
#if defined(__HIP_DEVICE_COMPILE__)
#define RTJM_TABLE static __device__ constexpr
#else
#define RTJM_TABLE static constexpr
#endif

namespace rtjm {

constexpr uint32_t RECORD_WORDS = 8u, HEADER_LEN = 629u, MAX_INTERVAL = 65535u, MAX_SIDE = 65535u;
// the most bits a block can take: a DC code of 11 bits with 11 bits of amplitude (category 11), and 63 coefficients each under the
// longest AC code, 16 bits, with 10 bits of amplitude (category 10).  ZRL and EOB stand for coefficients and are shorter.
constexpr uint32_t BLOCK_BITS_MAX = 22u + 63u * 26u, MCU_BITS_MAX = 3u * BLOCK_BITS_MAX;

// ---- tables -------------------------------------------------------------------------------------------------------------------------
// zigzag position k holds the coefficient at natural (row-major) index ZIGZAG[k]; NATURAL_TO_ZIGZAG is the inverse
RTJM_TABLE uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
RTJM_TABLE uint8_t NATURAL_TO_ZIGZAG[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                            41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                            46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// T.81 K.1 and K.2 in natural order (host only)
static constexpr uint8_t BASE_QUANT[2][64] = {
    {16, 11, 10, 16, 24, 40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68, 109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// T.81 K.3: for each table the number of codes of each length 1 ... 16, then the symbols in code order (a DHT payload without its
// first byte)
struct HuffSpec {
    uint8_t bits[16];
    uint8_t vals[162];
    uint32_t count;
};
static constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
static constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
static constexpr HuffSpec AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};
static constexpr HuffSpec AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};

// the code of each symbol: (length << 16) | code, 0 for a symbol the table does not hold (T.81 C.2: codes of a length are consecutive,
// and the first code of a length is twice the one after the last of the length before)
struct HuffCodes {
    uint32_t e[256];
};
constexpr HuffCodes make_codes(const HuffSpec& s) {
    HuffCodes t{};
    uint32_t code = 0, k = 0;
    for (uint32_t len = 1; len <= 16; len++) {
        for (uint32_t i = 0; i < s.bits[len - 1]; i++) t.e[s.vals[k++]] = (len << 16) | code++;
        code <<= 1;
    }
    return t;
}
// [0] luma, [1] chroma
RTJM_TABLE HuffCodes DC_CODES[2] = {make_codes(DC_LUMA), make_codes(DC_CHROMA)};
RTJM_TABLE HuffCodes AC_CODES[2] = {make_codes(AC_LUMA), make_codes(AC_CHROMA)};

// ---- colour -------------------------------------------------------------------------------------------------------------------------
// 16-bit fixed point, every sum within 2^24
RT_HOST_DEVICE int32_t luma(int32_t r, int32_t g, int32_t b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
RT_HOST_DEVICE int32_t chroma_b(int32_t r, int32_t g, int32_t b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
RT_HOST_DEVICE int32_t chroma_r(int32_t r, int32_t g, int32_t b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// ---- the transform ------------------------------------------------------------------------------------------------------------------
// (x + 2^(n-1)) >> n, the shift arithmetic
RT_HOST_DEVICE int32_t descale(int32_t x, int32_t n) { return (x + (1 << (n - 1))) >> n; }

// One 8-point pass of Loeffler, Ligtenberg and Moschytz's DCT with 13-bit constants.  ROWS: the first pass, whose outputs carry 2 more
// bits (d[0] and d[4] times 4, the others descaled by 11); otherwise the second, which takes those bits off again (d[0] and d[4]
// descaled by 2, the others by 15).  After both the block is the DCT times 8.
// Bounds for samples in -128 ... 127: a first pass yields |d| <= 4096 (products <= 1024 * 9633 + 2 * 512 * 25172 < 2^26); a second
// pass of such inputs has the sums of two <= 2^13, of four <= 2^14, z3 + z4 <= 2^15, so a line's three products and z5 are at most
// 2^13 * 25172 + 2^14 * 20995 + 2^14 * 16069 + 2^15 * 9633 < 1.2e9 < 2^31, and yields |d| <= 8192, a quantised value within +-1024.
template <bool ROWS>
RT_HOST_DEVICE void fdct_pass(int32_t d[8]) {
    const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int32_t odd = ROWS ? 11 : 15;
    d[0] = ROWS ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d[4] = ROWS ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    const int32_t e1 = (t12 + t13) * 4433;
    d[2] = descale(e1 + t13 * 6270, odd);
    d[6] = descale(e1 + t12 * -15137, odd);
    int32_t z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * 9633;
    const int32_t p4 = t4 * 2446, p5 = t5 * 16819, p6 = t6 * 25172, p7 = t7 * 12299;
    z1 = z1 * -7373;
    z2 = z2 * -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = descale(p4 + z1 + z3, odd);
    d[5] = descale(p5 + z2 + z4, odd);
    d[3] = descale(p6 + z2 + z3, odd);
    d[1] = descale(p7 + z1 + z4, odd);
}

// the coefficient (the DCT times 8) over 8 q, rounded half away from zero
RT_HOST_DEVICE int32_t quantise(int32_t c, int32_t q) {
    const int32_t q8 = q * 8, a = c < 0 ? -c : c;
    const int32_t v = (a + (q8 >> 1)) / q8;
    return c < 0 ? -v : v;
}

// ---- quantisation tables (host) -----------------------------------------------------------------------------------------------------
// the IJG rule; natural order
inline void quant_tables(uint32_t quality, uint8_t out[2][64]) {
    const uint32_t scale = quality < 50u ? 5000u / quality : 200u - 2u * quality;
    for (int t = 0; t < 2; t++)
        for (int i = 0; i < 64; i++) {
            const uint32_t v = (BASE_QUANT[t][i] * scale + 50u) / 100u;
            out[t][i] = (uint8_t)(v < 1u ? 1u : v > 255u ? 255u : v);
        }
}

// ---- entropy coding (T.81 F.1.2) ----------------------------------------------------------------------------------------------------
// the category of a magnitude: the number of bits of a
RT_HOST_DEVICE uint32_t category(uint32_t a) { return a == 0u ? 0u : 32u - (uint32_t)__builtin_clz(a); }

// The symbols of one block in zigzag order, given the DC predictor: put(code, length) is called for every Huffman code and for every
// amplitude (length 1 ... 16 each).  The amplitude of a negative v is the low bits of v - 1.
template <class Put>
RT_HOST_DEVICE void code_block(const int16_t* zz, int32_t pred, const HuffCodes& dc, const HuffCodes& ac, Put&& put) {
    int32_t v = (int32_t)zz[0] - pred;
    uint32_t cat = category((uint32_t)(v < 0 ? -v : v));
    uint32_t e = dc.e[cat];
    put(e & 0xffffu, e >> 16);
    if (cat) put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u), cat);
    uint32_t run = 0;
    for (int k = 1; k < 64; k++) {
        v = zz[k];
        if (v == 0) {
            run++;
            continue;
        }
        for (; run >= 16u; run -= 16u) {
            e = ac.e[0xf0];
            put(e & 0xffffu, e >> 16);
        }
        cat = category((uint32_t)(v < 0 ? -v : v));
        e = ac.e[(run << 4) | cat];
        put(e & 0xffffu, e >> 16);
        put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u), cat);
        run = 0;
    }
    if (run) {
        e = ac.e[0];
        put(e & 0xffffu, e >> 16);
    }
}

// the bits code_block emits
RT_HOST_DEVICE uint32_t block_bits(const int16_t* zz, int32_t pred, const HuffCodes& dc, const HuffCodes& ac) {
    uint32_t bits = 0;
    code_block(zz, pred, dc, ac, [&](uint32_t, uint32_t len) { bits += len; });
    return bits;
}

// ---- sizes --------------------------------------------------------------------------------------------------------------------------
struct Sizes {
    uint32_t mw, mh;           // MCUs a row, rows of MCUs
    uint32_t mcus, intervals;
    uint64_t raw_bound;        // the most entropy bytes before stuffing, every interval padded
    uint64_t bound;            // the most bytes of a file
};
RT_HOST_DEVICE Sizes sizes_of(uint32_t W, uint32_t R, uint32_t interval) {
    Sizes s;
    s.mw = (W + 7u) / 8u, s.mh = (R + 7u) / 8u;
    s.mcus = s.mw * s.mh;
    s.intervals = (s.mcus + interval - 1u) / interval;
    // an interval's bits are at most MCU_BITS_MAX a MCU and are padded by less than a byte; every byte may be 0xFF and is then
    // followed by a zero; every interval ends with a marker of two bytes
    s.raw_bound = ((uint64_t)s.mcus * MCU_BITS_MAX + 7u) / 8u + s.intervals;
    s.bound = HEADER_LEN + 2u * s.raw_bound + 2u * (uint64_t)s.intervals;
    return s;
}

// ---- the header (host) --------------------------------------------------------------------------------------------------------------
// SOI ... SOS, HEADER_LEN bytes, for tables in natural order
inline void write_header(uint32_t W, uint32_t R, uint32_t interval, const uint8_t q[2][64], uint8_t* out) {
    uint8_t* p = out;
    auto b = [&](uint32_t v) { *p++ = (uint8_t)v; };
    auto marker = [&](uint32_t m, uint32_t payload) { b(0xff), b(m), b((payload + 2u) >> 8), b((payload + 2u) & 0xffu); };
    b(0xff), b(0xd8);
    marker(0xe0, 14);                                                   // APP0: JFIF 1.01, no units, 1:1, no thumbnail
    for (uint8_t c : {0x4a, 0x46, 0x49, 0x46, 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00}) b(c);
    for (uint32_t t = 0; t < 2; t++) {                                  // DQT: 8-bit entries in zigzag order
        marker(0xdb, 65);
        b(t);
        for (int k = 0; k < 64; k++) b(q[t][ZIGZAG[k]]);
    }
    marker(0xc0, 15);                                                   // SOF0
    b(8), b(R >> 8), b(R & 0xffu), b(W >> 8), b(W & 0xffu), b(3);
    b(1), b(0x11), b(0), b(2), b(0x11), b(1), b(3), b(0x11), b(1);
    const HuffSpec* specs[4] = {&DC_LUMA, &AC_LUMA, &DC_CHROMA, &AC_CHROMA};
    const uint32_t ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; t++) {                                       // DHT
        marker(0xc4, 17 + specs[t]->count);
        b(ids[t]);
        for (int i = 0; i < 16; i++) b(specs[t]->bits[i]);
        for (uint32_t i = 0; i < specs[t]->count; i++) b(specs[t]->vals[i]);
    }
    marker(0xdd, 2);                                                    // DRI
    b(interval >> 8), b(interval & 0xffu);
    marker(0xda, 10);                                                   // SOS: one interleaved scan of all of the spectrum
    b(3), b(1), b(0x00), b(2), b(0x11), b(3), b(0x11), b(0), b(63), b(0);
}

}  // namespace rtjm
