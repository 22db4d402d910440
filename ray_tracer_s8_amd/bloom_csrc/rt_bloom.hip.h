// rt_bloom.hip.h — the gfx950 kernels of the bloom library (rt_bloom.h), wave64, every arithmetic line taken from
// rt_bloom_math.h (the lines the CPU harness runs too).  No inline assembly, no atomics, and no kernel waits for another workgroup:
// the order between launches is the stream's.  Every address comes from the sizes alone.
//
// rtb_down_kernel<FIRST, THRESH>: a workgroup of 256 lanes owns a tile of 32 x 8 pixels of level k + 1.  Its source window is the
//   66 x 18 pixels of level k around them, what lies outside the level left out (the taps clamp when they read).  (1) The window's
//   rows are copied to LDS with 16-byte loads: a row's floats are covered by the aligned groups of four they lie in, a group that
//   would pass the end of the level is read float by float, and only the floats inside the window are kept.  (2) FIRST: every pixel
//   of the window is sanitised and, with THRESH, thresholded in place, once.  (3) The horizontal sums h of the 18 rows at the 32
//   columns go to LDS.  (4) A lane a pixel sums four h and puts the pixel in an LDS tile.  (5) The tile's rows are stored as the
//   aligned 16-byte groups that lie wholly inside them, and float by float at their ends, which belong to the neighbouring tiles.
// rtb_upadd_kernel: U_k = D_k + spread up(U_{k+1}) in place.  A lane takes the 2 x 2 pixels (2 by - 1 ... 2 by, 2 bx - 1 ... 2 bx) of
//   level k, which share their four taps (by - 1 ... by, bx - 1 ... bx) of level k + 1: twelve loads for up to four pixels.
// rtb_tail_kernel<FIRST, THRESH>: one workgroup of 1 024 lanes and every level from `first` to `last` in dynamic LDS.  It filters
//   level first - 1 (FIRST: the image, sanitised and thresholded as it is read) down into LDS, then level by level inside LDS, then
//   accumulates back up in place, a barrier between two levels, and writes U_first, the only level that leaves the chip.
// rtb_combine_kernel<MODE, BLOOM>: the image is a flat float array and a lane takes a group of four floats, which lie in at most two
//   neighbouring pixels: one 16-byte load of the input, four taps of U_1 a float, one 16-byte store an output.  The lane of the
//   last, partial group works float by float.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_bloom_math.h"

namespace rtbk {

constexpr uint32_t BLOCK = 256;
constexpr uint32_t TW = 32, TH = 8;                          // a tile of the destination level
constexpr uint32_t SW = 2 * TW + 2, SH = 2 * TH + 2;        // its source window
constexpr uint32_t SROW = 3 * SW;                            // floats of a window row
constexpr uint32_t LOAD_GROUPS = (SROW + 3) / 4 + 1;         // the aligned groups of four that cover a window row, at most
constexpr uint32_t STORE_GROUPS = (3 * TW + 3) / 4 + 1;      // ... a tile row
constexpr uint32_t TAIL_BLOCK = 1024;
static_assert(TW * TH == BLOCK, "a lane a pixel of the tile");

struct DownParams {
    uint32_t Ws, Rs;              // the source level
    uint32_t Wd, Rd;              // the destination level: each side half the source's, rounded up
    const float* src;
    float* dst;
    float cap, T, K;              // FIRST
};

template <bool FIRST, bool THRESH>
__global__ __launch_bounds__(256) void rtb_down_kernel(const DownParams p) {
    __shared__ float raw[SH * SROW];
    __shared__ float hs[SH * TW * 3];
    __shared__ float tile[TH * TW * 3];
    const uint32_t tid = threadIdx.x;
    const uint32_t i0 = blockIdx.y * TH, j0 = blockIdx.x * TW;                       // the tile's first pixel
    const int32_t r0 = 2 * (int32_t)i0 - 1, c0 = 2 * (int32_t)j0 - 1;                // the window's first pixel (-1 at an edge)
    // the part of the window inside the level: rows ra ... rb and columns ca ... cb (i0 < Rd gives 2 i0 - 1 <= Rs - 1)
    const uint32_t ra = r0 < 0 ? 0u : (uint32_t)r0, ca = c0 < 0 ? 0u : (uint32_t)c0;
    const uint32_t rb = (uint32_t)(r0 + (int32_t)SH - 1) < p.Rs - 1u ? (uint32_t)(r0 + (int32_t)SH - 1) : p.Rs - 1u;
    const uint32_t cb = (uint32_t)(c0 + (int32_t)SW - 1) < p.Ws - 1u ? (uint32_t)(c0 + (int32_t)SW - 1) : p.Ws - 1u;
    const uint32_t rows = rb - ra + 1u, cols = cb - ca + 1u, nf = 3u * cols;
    const uint64_t floats = 3ull * p.Ws * p.Rs;

    // (1) the window's rows
    for (uint32_t idx = tid; idx < rows * LOAD_GROUPS; idx += BLOCK) {
        const uint32_t row = idx / LOAD_GROUPS, gi = idx - row * LOAD_GROUPS;
        const uint64_t gs = 3ull * ((uint64_t)(ra + row) * p.Ws + ca);                 // the row's first float
        const uint64_t g = (gs >> 2) + gi;
        if (4ull * g >= gs + nf) continue;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (4ull * g + 4ull <= floats) {
            const float4 q = reinterpret_cast<const float4*>(p.src)[g];
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
            for (uint32_t e = 0; e < 4u; e++)
                if (4ull * g + e < floats) v[e] = p.src[4ull * g + e];
        }
        float* to = raw + (ra + row - (uint32_t)r0) * SROW + 3u * (ca - (uint32_t)c0);  // (unsigned wrap-around: ra >= r0)
#pragma unroll
        for (uint32_t e = 0; e < 4u; e++) {
            const uint64_t f = 4ull * g + e;
            if (f >= gs && f < gs + nf) to[(uint32_t)(f - gs)] = v[e];
        }
    }
    __syncthreads();

    // (2) the pixels a pyramid starts from
    if (FIRST) {
        for (uint32_t idx = tid; idx < rows * cols; idx += BLOCK) {
            const uint32_t row = idx / cols, col = idx - row * cols;
            float* c = raw + (ra + row - (uint32_t)r0) * SROW + 3u * (ca + col - (uint32_t)c0);
            float q[3];
            rtbm::source_pixel<THRESH>(c, p.cap, p.T, p.K, q);
            c[0] = q[0], c[1] = q[1], c[2] = q[2];
        }
        __syncthreads();
    }

    // (3) h of every window row at every column of the tile
    for (uint32_t idx = tid; idx < SH * TW; idx += BLOCK) {
        const uint32_t wr = idx / TW, j = idx - wr * TW;
        if (j0 + j >= p.Wd) continue;
        const int32_t r = r0 + (int32_t)wr;
        const uint32_t rc = r < 0 ? 0u : ((uint32_t)r > p.Rs - 1u ? p.Rs - 1u : (uint32_t)r);        // in ra ... rb
        const float* line = raw + (rc - (uint32_t)r0) * SROW;
        const float* s[4];
#pragma unroll
        for (uint32_t b = 0; b < 4u; b++) s[b] = line + 3u * (rtbm::down_tap(j0 + j, b, p.Ws) - (uint32_t)c0);
#pragma unroll
        for (uint32_t c = 0; c < 3u; c++) hs[3u * idx + c] = rtbm::sum_1331(s[0][c], s[1][c], s[2][c], s[3][c]);
    }
    __syncthreads();

    // (4) a lane a pixel: window rows 2 i ... 2 i + 3 are the taps of tile row i
    {
        const uint32_t i = tid / TW, j = tid - i * TW;
        if (i0 + i < p.Rd && j0 + j < p.Wd) {
            const float* h = hs + 3u * (2u * i * TW + j);
#pragma unroll
            for (uint32_t c = 0; c < 3u; c++)
                tile[3u * tid + c] = rtbm::down_value(h[c], h[3u * TW + c], h[6u * TW + c], h[9u * TW + c]);
        }
    }
    __syncthreads();

    // (5) the tile's rows
    const uint32_t trows = p.Rd - i0 < TH ? p.Rd - i0 : TH, tcols = p.Wd - j0 < TW ? p.Wd - j0 : TW, tf = 3u * tcols;
    for (uint32_t idx = tid; idx < trows * STORE_GROUPS; idx += BLOCK) {
        const uint32_t row = idx / STORE_GROUPS, gi = idx - row * STORE_GROUPS;
        const uint64_t gs = 3ull * ((uint64_t)(i0 + row) * p.Wd + j0);
        const uint64_t g = (gs >> 2) + gi;
        if (4ull * g >= gs + tf) continue;
        const float* from = tile + 3u * row * TW;
        if (4ull * g >= gs && 4ull * g + 4ull <= gs + tf) {
            const uint32_t at = (uint32_t)(4ull * g - gs);
            reinterpret_cast<float4*>(p.dst)[g] = make_float4(from[at], from[at + 1u], from[at + 2u], from[at + 3u]);
        } else {
            for (uint32_t e = 0; e < 4u; e++) {
                const uint64_t f = 4ull * g + e;
                if (f >= gs && f < gs + tf) p.dst[f] = from[(uint32_t)(f - gs)];
            }
        }
    }
}

struct UpAddParams {
    uint32_t Wf, Rf;              // level k, read and written
    uint32_t Wc, Rc;              // level k + 1, read
    float* fine;
    const float* coarse;
    float spread;
};

__global__ __launch_bounds__(256) void rtb_upadd_kernel(const UpAddParams p) {
    const uint32_t bx = blockIdx.x * TW + (threadIdx.x & (TW - 1u)), by = blockIdx.y * TH + threadIdx.x / TW;
    if (bx > p.Wf / 2u || by > p.Rf / 2u) return;
    // the four taps: rows by - 1 and by, columns bx - 1 and bx, clamped
    const uint32_t ya = by == 0u ? 0u : (by - 1u < p.Rc - 1u ? by - 1u : p.Rc - 1u), yb = by < p.Rc - 1u ? by : p.Rc - 1u;
    const uint32_t xa = bx == 0u ? 0u : (bx - 1u < p.Wc - 1u ? bx - 1u : p.Wc - 1u), xb = bx < p.Wc - 1u ? bx : p.Wc - 1u;
    const float* aa = p.coarse + 3u * ((size_t)ya * p.Wc + xa);
    const float* ab = p.coarse + 3u * ((size_t)ya * p.Wc + xb);
    const float* ba = p.coarse + 3u * ((size_t)yb * p.Wc + xa);
    const float* bb = p.coarse + 3u * ((size_t)yb * p.Wc + xb);
    float X[4][3];
#pragma unroll
    for (uint32_t c = 0; c < 3u; c++) X[0][c] = aa[c], X[1][c] = ab[c], X[2][c] = ba[c], X[3][c] = bb[c];
#pragma unroll
    for (uint32_t dy = 0; dy < 2u; dy++) {
        const uint32_t y = 2u * by + dy - 1u;                                          // (by = 0, dy = 0 wraps round and fails y < Rf)
        if (y >= p.Rf) continue;
        const float wya = dy == 0u ? 3.0f : 1.0f, wyb = 4.0f - wya;                      // y odd: 3 and 1
#pragma unroll
        for (uint32_t dx = 0; dx < 2u; dx++) {
            const uint32_t x = 2u * bx + dx - 1u;
            if (x >= p.Wf) continue;
            const float wxa = dx == 0u ? 3.0f : 1.0f, wxb = 4.0f - wxa;
            float* d = p.fine + 3u * ((size_t)y * p.Wf + x);
#pragma unroll
            for (uint32_t c = 0; c < 3u; c++)
                d[c] = rtbm::accumulate(d[c], p.spread, rtbm::up_value(X[0][c], X[1][c], X[2][c], X[3][c], wxa, wxb, wya, wyb));
        }
    }
}

struct TailParams {
    uint32_t Ws, Rs;              // level first - 1 (FIRST: the image)
    uint32_t first, last;         // the levels held in LDS
    uint32_t W[rtbm::MAX_LEVELS], R[rtbm::MAX_LEVELS];      // of level first + n
    uint32_t at[rtbm::MAX_LEVELS];                           // where level first + n begins in LDS, in floats
    const float* src;
    float* dst;                   // U_first
    float cap, T, K, spread;
};

template <bool FIRST, bool THRESH>
__global__ __launch_bounds__(1024) void rtb_tail_kernel(const TailParams p) {
    extern __shared__ float lds[];
    const uint32_t tid = threadIdx.x, count = p.last - p.first + 1u;
    // level first, from memory
    {
        const uint32_t W = p.W[0], R = p.R[0];
        const auto fetch = [&](uint32_t r, uint32_t c, float* s) {
            const float* q = p.src + 3u * ((size_t)r * p.Ws + c);
            if (FIRST)
                rtbm::source_pixel<THRESH>(q, p.cap, p.T, p.K, s);
            else
                s[0] = q[0], s[1] = q[1], s[2] = q[2];
        };
        for (uint32_t idx = tid; idx < W * R; idx += TAIL_BLOCK) {
            const uint32_t i = idx / W, j = idx - i * W;
            float v[3];
            rtbm::down_pixel(fetch, i, j, p.Rs, p.Ws, v);
            lds[3u * idx] = v[0], lds[3u * idx + 1u] = v[1], lds[3u * idx + 2u] = v[2];
        }
    }
    __syncthreads();
    // the levels below it, each from the one above
    for (uint32_t n = 1; n < count; n++) {
        const uint32_t W = p.W[n], R = p.R[n], Wp = p.W[n - 1u], Rp = p.R[n - 1u];
        const float* above = lds + p.at[n - 1u];
        float* here = lds + p.at[n];
        const auto fetch = [&](uint32_t r, uint32_t c, float* s) {
            const float* q = above + 3u * (r * Wp + c);
            s[0] = q[0], s[1] = q[1], s[2] = q[2];
        };
        for (uint32_t idx = tid; idx < W * R; idx += TAIL_BLOCK) {
            const uint32_t i = idx / W, j = idx - i * W;
            float v[3];
            rtbm::down_pixel(fetch, i, j, Rp, Wp, v);
            here[3u * idx] = v[0], here[3u * idx + 1u] = v[1], here[3u * idx + 2u] = v[2];
        }
        __syncthreads();
    }
    // back up, in place
    for (uint32_t n = count - 1u; n > 0u; n--) {
        const uint32_t W = p.W[n - 1u], R = p.R[n - 1u];
        const float* below = lds + p.at[n];
        float* here = lds + p.at[n - 1u];
        for (uint32_t idx = tid; idx < W * R; idx += TAIL_BLOCK) {
            const uint32_t y = idx / W, x = idx - y * W;
            float u[3];
            rtbm::up_pixel(below, p.R[n], p.W[n], y, x, u);
#pragma unroll
            for (uint32_t c = 0; c < 3u; c++) here[3u * idx + c] = rtbm::accumulate(here[3u * idx + c], p.spread, u[c]);
        }
        __syncthreads();
    }
    // U_first leaves: level first begins the LDS and its destination is 16-byte aligned
    const uint32_t nf = 3u * p.W[0] * p.R[0];
    for (uint32_t g = tid; 4u * g < nf; g += TAIL_BLOCK) {
        if (4u * g + 4u <= nf) {
            reinterpret_cast<float4*>(p.dst)[g] = make_float4(lds[4u * g], lds[4u * g + 1u], lds[4u * g + 2u], lds[4u * g + 3u]);
        } else {
            for (uint32_t f = 4u * g; f < nf; f++) p.dst[f] = lds[f];
        }
    }
}

struct CombineParams {
    uint32_t W;
    uint32_t W1, R1;              // level 1
    uint32_t groups;              // ceil(floats / 4)
    uint64_t floats;              // 3 R W
    const float* in;
    const float* U1;
    float* out;
    float* out_bloom;
    float strength, keep, norm;   // keep: 1 - strength
};

template <uint32_t MODE, bool BLOOM>
__global__ __launch_bounds__(256) void rtb_combine_kernel(const CombineParams p) {
    const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= p.groups) return;
    // float 4 g is channel g mod 3 of pixel g + g div 3, and float 4 g + j lies in the next pixel once g mod 3 + j reaches 3
    const uint32_t third = g / 3u, ch = g - 3u * third, pixel = g + third;
    const uint32_t y0 = pixel / p.W, x0 = pixel - y0 * p.W;
    const bool wraps = x0 + 1u == p.W;
    const uint32_t y1 = wraps ? y0 + 1u : y0, x1 = wraps ? 0u : x0 + 1u;
    const uint64_t at = 4ull * g;
    const uint32_t left = at + 4ull <= p.floats ? 4u : (uint32_t)(p.floats - at);
    float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (left == 4u) {
        const float4 v = reinterpret_cast<const float4*>(p.in)[g];
        c[0] = v.x, c[1] = v.y, c[2] = v.z, c[3] = v.w;
    } else {
        for (uint32_t j = 0; j < left; j++) c[j] = p.in[at + j];
    }
    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f}, b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        if (j >= left) continue;
        const bool next = ch + j >= 3u;
        const uint32_t y = next ? y1 : y0, x = next ? x1 : x0, k = next ? ch + j - 3u : ch + j;
        const rtbm::UpTap ty = rtbm::up_tap(y, p.R1), tx = rtbm::up_tap(x, p.W1);
        const float* rowa = p.U1 + 3u * (size_t)ty.a * p.W1 + k;
        const float* rowb = p.U1 + 3u * (size_t)ty.b * p.W1 + k;
        const float u = rtbm::up_value(rowa[3u * tx.a], rowa[3u * tx.b], rowb[3u * tx.a], rowb[3u * tx.b], tx.wa, tx.wb, ty.wa, ty.wb);
        b[j] = rtbm::bloom_value(u, p.norm);
        o[j] = rtbm::mix<MODE>(rtbm::positive(c[j]), b[j], p.strength, p.keep);
    }
    if (left == 4u) {
        reinterpret_cast<float4*>(p.out)[g] = make_float4(o[0], o[1], o[2], o[3]);
        if (BLOOM) reinterpret_cast<float4*>(p.out_bloom)[g] = make_float4(b[0], b[1], b[2], b[3]);
    } else {
        for (uint32_t j = 0; j < left; j++) {
            p.out[at + j] = o[j];
            if (BLOOM) p.out_bloom[at + j] = b[j];
        }
    }
}

}  // namespace rtbk
