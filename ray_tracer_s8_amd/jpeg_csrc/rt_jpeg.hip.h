// rt_jpeg.hip.h — the gfx950 kernels of the JPEG library (rt_jpeg.h), wave64, every per-pixel, per-block and
// per-symbol operation taken from rt_jpeg_math.h (the lines the CPU harness runs too).  No inline assembly, no workgroup waits for
// another, and every address comes from the sizes alone or from bit counts the sizes bound (Layout::raw covers rtjm::Sizes::raw_bound).
//
// rtj_transform_kernel: a block of 256 lanes takes 32 MCUs, a lane one row of one MCU: it loads the row's eight pixels (clamped to
//   the frame: the padding), converts them, runs the first DCT pass on the three components and leaves the rows in LDS, a row 9 words
//   apart so that neither pass meets a bank twice.  After the barrier the lane takes a column of the same MCU: second pass,
//   quantisation, and the int16 result to its zigzag place in LDS; then the block's 12 288 bytes go out as consecutive words.
// rtj_size_kernel: a lane a MCU: the bits of its three blocks, the DC predictors taken from the MCU before unless it starts an interval.
// rtj_scan_blocks_kernel / rtj_scan_sums_kernel: an exclusive scan of n words in place as chunks of 1 024 (a block of 256 lanes, four
//   words a lane) and a single block of 1 024 lanes over the chunks' totals, whose word n gets the grand total.  A consumer adds the
//   two (prefix()).  Used three times: bits a MCU, bytes an interval, 0xFF bytes an interval.
// rtj_interval_kernel: a lane an interval: its bytes, the difference of two bit prefixes rounded up.
// rtj_pack_kernel: a lane a MCU: its symbols again, now shifted into a 64-bit register and written a 32-bit word at a time at its exact
//   bit offset in the raw stream (cleared before): the first and the last word of a MCU, which neighbours share, by a global OR, the
//   words between by plain stores.  The last MCU of an interval adds the 1-bits.
// rtj_count_kernel: a wave an interval: its 0xFF bytes.
// rtj_scatter_kernel: a wave an interval: 64 bytes a trip, a ballot of the 0xFF lanes gives every byte its place after the header, the
//   stuffed zeros and the markers before it; then the interval's marker, and from the first wave the record.  Nothing is stored at or
//   past the capacity.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_jpeg_math.h"

namespace rtjk {

constexpr uint32_t BLOCK = 256, WAVES = BLOCK / 64;
constexpr uint32_t MCUS_PER_BLOCK = BLOCK / 8;                  // the transform's
constexpr uint32_t ROW_WORDS = 9, PLANE_WORDS = 8 * ROW_WORDS;  // a block's rows in LDS
constexpr uint32_t CHUNK = 1024, CHUNK_SHIFT = 10;              // the scan's
constexpr uint32_t SUMS_BLOCK = 1024;

constexpr uint64_t align256(uint64_t v) { return (v + 255u) & ~(uint64_t)255u; }
constexpr uint32_t chunks(uint32_t n) { return (n + CHUNK - 1u) / CHUNK; }

// the scratch, in bytes from its start
struct Layout {
    uint64_t coef;       // int16 [mcus][3][64], zigzag order
    uint64_t mbits;      // u32 [mcus]: bits a MCU, scanned in place
    uint64_t msums;      // u32 [chunks(mcus) + 1]
    uint64_t ibytes;     // u32 [intervals]: raw bytes an interval, scanned in place
    uint64_t isums;      // u32 [chunks(intervals) + 1]
    uint64_t iff;        // u32 [intervals]: 0xFF bytes an interval, scanned in place
    uint64_t fsums;      // u32 [chunks(intervals) + 1]
    uint64_t raw;        // the entropy bytes before stuffing, as whole words
    uint64_t raw_bytes;
    uint64_t total;
};
inline Layout layout_of(const rtjm::Sizes& s) {
    Layout l;
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t here = at;
        at = align256(at + bytes);
        return here;
    };
    l.coef = take((uint64_t)s.mcus * 384u);
    l.mbits = take(4ull * s.mcus);
    l.msums = take(4ull * (chunks(s.mcus) + 1u));
    l.ibytes = take(4ull * s.intervals);
    l.isums = take(4ull * (chunks(s.intervals) + 1u));
    l.iff = take(4ull * s.intervals);
    l.fsums = take(4ull * (chunks(s.intervals) + 1u));
    l.raw_bytes = ((s.raw_bound + 3u) & ~(uint64_t)3u) + 4u;
    l.raw = take(l.raw_bytes);
    l.total = at;
    return l;
}

// element i of a scanned array of n (i <= n): the chunk-local prefix plus the chunk's, or the grand total
__device__ inline uint32_t prefix(const uint32_t* a, const uint32_t* sums, uint32_t i, uint32_t n) {
    return i < n ? a[i] + sums[i >> CHUNK_SHIFT] : sums[chunks(n)];
}

__device__ inline uint32_t wave_inclusive(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// the exclusive prefix of v over the block's lanes and the block's total; wsum: LDS of blockDim.x / 64 words
__device__ inline uint32_t block_exclusive(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const uint32_t inc = wave_inclusive(v), wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    if ((threadIdx.x & 63u) == 63u) wsum[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t w = 0; w < waves; w++) {
        const uint32_t s = wsum[w];
        base += w < wave ? s : 0u;
        tot += s;
    }
    __syncthreads();                                                  // wsum is free again
    total = tot;
    return base + inc - v;
}

// ---- the transform --------------------------------------------------------------------------------------------------------------------
struct TransformParams {
    uint32_t W, R, mw, mcus;
    const uint8_t* rgb;
    uint32_t* coef;                  // the int16 coefficients as words
    uint16_t q[2][64];               // natural order
};

__global__ __launch_bounds__(256) void rtj_transform_kernel(const TransformParams p) {
    __shared__ int32_t rows[MCUS_PER_BLOCK * 3 * PLANE_WORDS];
    __shared__ int16_t zz[MCUS_PER_BLOCK * 192];
    __shared__ uint16_t q[128];
    const uint32_t tid = threadIdx.x, ml = tid >> 3, r = tid & 7u;
    if (tid < 128u) q[tid] = p.q[tid >> 6][tid & 63u];
    const uint32_t m0 = blockIdx.x * MCUS_PER_BLOCK + ml;
    const uint32_t m = m0 < p.mcus ? m0 : p.mcus - 1u;               // a lane past the end repeats the last MCU and stores nothing
    const uint32_t mx = m % p.mw, my = m / p.mw;
    {
        const uint32_t y0 = my * 8u + r, y = y0 < p.R ? y0 : p.R - 1u;
        const uint8_t* line = p.rgb + (size_t)y * p.W * 3u;
        int32_t d[3][8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) {
            const uint32_t x0 = mx * 8u + j, x = x0 < p.W ? x0 : p.W - 1u;
            const int32_t cr = line[3u * x], cg = line[3u * x + 1u], cb = line[3u * x + 2u];
            d[0][j] = rtjm::luma(cr, cg, cb) - 128;
            d[1][j] = rtjm::chroma_b(cr, cg, cb) - 128;
            d[2][j] = rtjm::chroma_r(cr, cg, cb) - 128;
        }
#pragma unroll
        for (uint32_t c = 0; c < 3u; c++) {
            rtjm::fdct_pass<true>(d[c]);
            int32_t* row = rows + (ml * 3u + c) * PLANE_WORDS + r * ROW_WORDS;
#pragma unroll
            for (uint32_t j = 0; j < 8u; j++) row[j] = d[c][j];
        }
    }
    __syncthreads();
    {
        const uint32_t col = r;
#pragma unroll
        for (uint32_t c = 0; c < 3u; c++) {
            const int32_t* plane = rows + (ml * 3u + c) * PLANE_WORDS;
            int32_t d[8];
#pragma unroll
            for (uint32_t i = 0; i < 8u; i++) d[i] = plane[i * ROW_WORDS + col];
            rtjm::fdct_pass<false>(d);
#pragma unroll
            for (uint32_t i = 0; i < 8u; i++) {
                const uint32_t n = i * 8u + col;
                zz[ml * 192u + c * 64u + rtjm::NATURAL_TO_ZIGZAG[n]] = (int16_t)rtjm::quantise(d[i], (int32_t)q[(c ? 64u : 0u) + n]);
            }
        }
    }
    __syncthreads();
    const uint32_t* words = reinterpret_cast<const uint32_t*>(zz);
    const uint64_t first = (uint64_t)blockIdx.x * (MCUS_PER_BLOCK * 96u), end = (uint64_t)p.mcus * 96u;
#pragma unroll
    for (uint32_t k = 0; k < MCUS_PER_BLOCK * 96u / BLOCK; k++) {
        const uint32_t w = k * BLOCK + tid;
        if (first + w < end) p.coef[first + w] = words[w];
    }
}

// ---- sizes ----------------------------------------------------------------------------------------------------------------------------
struct StreamParams {
    uint32_t mcus, interval, intervals, header_len;
    uint64_t capacity;
    const int16_t* coef;
    uint32_t *mbits, *msums, *ibytes, *isums, *iff, *fsums;
    uint32_t* raw;
    uint8_t* out;
    uint32_t* record;
};

__global__ __launch_bounds__(256) void rtj_size_kernel(const StreamParams p) {
    const uint32_t m = blockIdx.x * BLOCK + threadIdx.x;
    if (m >= p.mcus) return;
    const int16_t* zz = p.coef + (size_t)m * 192u;
    const bool first = m % p.interval == 0u;
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t c = 0; c < 3u; c++) {
        const int32_t pred = first ? 0 : (int32_t)zz[(int)(c * 64u) - 192];
        bits += rtjm::block_bits(zz + c * 64u, pred, rtjm::DC_CODES[c ? 1 : 0], rtjm::AC_CODES[c ? 1 : 0]);
    }
    p.mbits[m] = bits;
}

struct ScanParams {
    uint32_t n;
    uint32_t* a;
    uint32_t* sums;
};

__global__ __launch_bounds__(256) void rtj_scan_blocks_kernel(const ScanParams p) {
    __shared__ uint32_t wsum[WAVES];
    const uint32_t base = blockIdx.x * CHUNK + threadIdx.x * 4u;
    uint32_t v[4], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        v[j] = base + j < p.n ? p.a[base + j] : 0u;
        mine += v[j];
    }
    uint32_t total;
    uint32_t at = block_exclusive(mine, wsum, total);
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        if (base + j < p.n) p.a[base + j] = at;
        at += v[j];
    }
    if (threadIdx.x == 0u) p.sums[blockIdx.x] = total;
}

// one block: the chunk totals sums[0 ... n) scanned in place, the grand total to sums[n]
__global__ __launch_bounds__(1024) void rtj_scan_sums_kernel(const ScanParams p) {
    __shared__ uint32_t wsum[SUMS_BLOCK / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < p.n; base += SUMS_BLOCK) {         // uniform over the block
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < p.n ? p.sums[i] : 0u;
        uint32_t total;
        const uint32_t at = block_exclusive(v, wsum, total);
        if (i < p.n) p.sums[i] = carry + at;
        carry += total;
    }
    if (threadIdx.x == 0u) p.sums[p.n] = carry;
}

__global__ __launch_bounds__(256) void rtj_interval_kernel(const StreamParams p) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= p.intervals) return;
    const uint32_t m0 = k * p.interval, m1 = p.mcus - m0 > p.interval ? m0 + p.interval : p.mcus;
    const uint32_t bits = prefix(p.mbits, p.msums, m1, p.mcus) - prefix(p.mbits, p.msums, m0, p.mcus);
    p.ibytes[k] = (bits + 7u) >> 3;
}

// ---- packing --------------------------------------------------------------------------------------------------------------------------
struct BitSink {
    uint32_t* words;
    uint64_t acc;
    uint32_t n, w;
    bool first;
    __device__ void store(uint32_t word) {
        const uint32_t v = __builtin_bswap32(word);                    // the first bit of the stream is a byte's most significant
        if (first)
            atomicOr(words + w, v);
        else
            words[w] = v;
        first = false;
        w++;
    }
    __device__ void put(uint32_t code, uint32_t len) {                 // len <= 16, n < 32
        acc = (acc << len) | code;
        n += len;
        if (n >= 32u) {
            n -= 32u;
            store((uint32_t)(acc >> n));
            acc &= (1ull << n) - 1ull;
        }
    }
    __device__ void finish() {
        if (n) atomicOr(words + w, __builtin_bswap32((uint32_t)(acc << (32u - n))));
    }
};

__global__ __launch_bounds__(256) void rtj_pack_kernel(const StreamParams p) {
    const uint32_t m = blockIdx.x * BLOCK + threadIdx.x;
    if (m >= p.mcus) return;
    const uint32_t k = m / p.interval, m0 = k * p.interval;
    const bool first = m == m0, last = m + 1u == p.mcus || m + 1u == m0 + p.interval;
    const uint32_t in_interval = prefix(p.mbits, p.msums, m, p.mcus) - prefix(p.mbits, p.msums, m0, p.mcus);
    const uint32_t at = prefix(p.ibytes, p.isums, k, p.intervals) * 8u + in_interval;        // (8 raw_bound fits 32 bits)
    BitSink s{p.raw, 0ull, at & 31u, at >> 5, true};
    const int16_t* zz = p.coef + (size_t)m * 192u;
#pragma unroll
    for (uint32_t c = 0; c < 3u; c++) {
        const int32_t pred = first ? 0 : (int32_t)zz[(int)(c * 64u) - 192];
        rtjm::code_block(zz + c * 64u, pred, rtjm::DC_CODES[c ? 1 : 0], rtjm::AC_CODES[c ? 1 : 0],
                         [&](uint32_t code, uint32_t len) { s.put(code, len); });
    }
    if (last) {
        const uint32_t pad = (0u - s.n) & 7u;
        if (pad) s.put((1u << pad) - 1u, pad);
    }
    s.finish();
}

// ---- stuffing -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rtj_count_kernel(const StreamParams p) {
    const uint32_t k = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (k >= p.intervals) return;                                       // uniform over the wave
    const uint32_t b0 = prefix(p.ibytes, p.isums, k, p.intervals), b1 = prefix(p.ibytes, p.isums, k + 1u, p.intervals);
    const uint8_t* raw = reinterpret_cast<const uint8_t*>(p.raw);
    uint32_t count = 0;
    for (uint32_t i = b0 + lane; i < b1; i += 64u) count += raw[i] == 0xffu ? 1u : 0u;
    count = wave_inclusive(count);
    if (lane == 63u) p.iff[k] = count;
}

__global__ __launch_bounds__(256) void rtj_scatter_kernel(const StreamParams p) {
    const uint32_t k = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (k >= p.intervals) return;                                       // uniform over the wave
    const uint32_t b0 = prefix(p.ibytes, p.isums, k, p.intervals), b1 = prefix(p.ibytes, p.isums, k + 1u, p.intervals);
    const uint32_t f0 = prefix(p.iff, p.fsums, k, p.intervals);
    const uint8_t* raw = reinterpret_cast<const uint8_t*>(p.raw);
    uint64_t at = (uint64_t)p.header_len + b0 + f0 + 2ull * k;          // where the interval's first byte goes
    for (uint32_t base = b0; base < b1; base += 64u) {                  // uniform over the wave
        const uint32_t i = base + lane;
        const bool valid = i < b1;
        const uint32_t byte = valid ? raw[i] : 0u;
        const unsigned long long ff = __ballot(byte == 0xffu);
        const uint64_t mine = at + lane + (uint32_t)__popcll(ff & ((1ull << lane) - 1ull));
        if (valid && mine < p.capacity) p.out[mine] = (uint8_t)byte;
        if (valid && byte == 0xffu && mine + 1u < p.capacity) p.out[mine + 1u] = 0u;
        at += 64u + (uint32_t)__popcll(ff);
    }
    if (lane == 0u) {
        const uint64_t end = (uint64_t)p.header_len + b1 + prefix(p.iff, p.fsums, k + 1u, p.intervals) + 2ull * k;
        if (end < p.capacity) p.out[end] = 0xffu;
        if (end + 1u < p.capacity) p.out[end + 1u] = (uint8_t)(k + 1u == p.intervals ? 0xd9u : 0xd0u + (k & 7u));
        if (k == 0u) {
            const uint32_t raw_total = prefix(p.ibytes, p.isums, p.intervals, p.intervals);
            const uint32_t ff_total = prefix(p.iff, p.fsums, p.intervals, p.intervals);
            const uint64_t total = (uint64_t)p.header_len + raw_total + ff_total + 2ull * p.intervals;
            p.record[0] = (uint32_t)total;                              // (rtj_bound fits 32 bits)
            p.record[1] = raw_total;
            p.record[2] = ff_total;
            p.record[3] = p.intervals;
            p.record[4] = total > p.capacity ? 1u : 0u;
            p.record[5] = p.record[6] = p.record[7] = 0u;
        }
    }
}

}  // namespace rtjk
