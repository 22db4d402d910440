// Test harness (CPU only, built by tests/test_jpeg_host.py with g++): the JPEG library's encoder (jpeg_csrc/rt_jpeg.h) run serially
// with the product's own per-pixel, per-block and per-symbol lines (jpeg_csrc/rt_jpeg_math.h) over plain arrays.  With
// -DJPEG_HOST_MAIN it is a stand-alone program (its own main) that reads a corpus file (frames and settings), encodes every frame into
// exactly sized buffers and writes the coefficients and the files to a result file, for a sanitizer build.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_jpeg_math.h"

namespace {

// the quantised coefficients of a frame: int16 [mcus][3][64] in zigzag order
void transform(const uint8_t* rgb, uint32_t W, uint32_t R, const uint8_t q[2][64], int16_t* coef) {
    const rtjm::Sizes s = rtjm::sizes_of(W, R, 1);
    for (uint32_t m = 0; m < s.mcus; m++) {
        const uint32_t mx = m % s.mw, my = m / s.mw;
        int32_t d[3][8][8];
        for (uint32_t r = 0; r < 8; r++) {
            const uint32_t y0 = my * 8 + r, y = y0 < R ? y0 : R - 1;
            int32_t row[3][8];
            for (uint32_t j = 0; j < 8; j++) {
                const uint32_t x0 = mx * 8 + j, x = x0 < W ? x0 : W - 1;
                const uint8_t* px = rgb + 3 * ((size_t)y * W + x);
                row[0][j] = rtjm::luma(px[0], px[1], px[2]) - 128;
                row[1][j] = rtjm::chroma_b(px[0], px[1], px[2]) - 128;
                row[2][j] = rtjm::chroma_r(px[0], px[1], px[2]) - 128;
            }
            for (uint32_t c = 0; c < 3; c++) {
                rtjm::fdct_pass<true>(row[c]);
                for (uint32_t j = 0; j < 8; j++) d[c][r][j] = row[c][j];
            }
        }
        for (uint32_t c = 0; c < 3; c++)
            for (uint32_t col = 0; col < 8; col++) {
                int32_t v[8];
                for (uint32_t i = 0; i < 8; i++) v[i] = d[c][i][col];
                rtjm::fdct_pass<false>(v);
                for (uint32_t i = 0; i < 8; i++) {
                    const uint32_t n = i * 8 + col;
                    coef[(size_t)m * 192 + c * 64 + rtjm::NATURAL_TO_ZIGZAG[n]] = (int16_t)rtjm::quantise(v[i], q[c ? 1 : 0][n]);
                }
            }
    }
}

struct Writer {
    std::vector<uint8_t>& out;
    uint64_t acc = 0;
    uint32_t n = 0, raw = 0, stuffed = 0;
    void byte(uint32_t b) {
        out.push_back((uint8_t)b);
        raw++;
        if (b == 0xffu) out.push_back(0), stuffed++;
    }
    void put(uint32_t code, uint32_t len) {
        acc = (acc << len) | code;
        n += len;
        while (n >= 8) {
            n -= 8;
            byte((uint32_t)(acc >> n) & 0xffu);
        }
        acc &= (1ull << n) - 1ull;
    }
    void pad() {
        if (n) put((1u << (8 - n)) - 1u, 8 - n);
    }
};

// the whole file; record[5]: total, raw, stuffed, intervals, 0
void encode(const uint8_t* rgb, uint32_t W, uint32_t R, uint32_t quality, uint32_t interval, std::vector<int16_t>& coef,
            std::vector<uint8_t>& out, uint32_t record[5]) {
    const rtjm::Sizes s = rtjm::sizes_of(W, R, interval);
    uint8_t q[2][64];
    rtjm::quant_tables(quality, q);
    coef.assign((size_t)s.mcus * 192, 0);
    transform(rgb, W, R, q, coef.data());
    out.assign(rtjm::HEADER_LEN, 0);
    rtjm::write_header(W, R, interval, q, out.data());
    Writer w{out};
    for (uint32_t k = 0; k < s.intervals; k++) {
        for (uint32_t m = k * interval; m < s.mcus && m < (k + 1) * interval; m++)
            for (uint32_t c = 0; c < 3; c++) {
                const int16_t* zz = coef.data() + (size_t)m * 192 + c * 64;
                const int32_t pred = m == k * interval ? 0 : zz[-192];
                const uint32_t before = 8 * w.raw + w.n;
                rtjm::code_block(zz, pred, rtjm::DC_CODES[c ? 1 : 0], rtjm::AC_CODES[c ? 1 : 0],
                                 [&](uint32_t code, uint32_t len) { w.put(code, len); });
                if (8 * w.raw + w.n - before != rtjm::block_bits(zz, pred, rtjm::DC_CODES[c ? 1 : 0], rtjm::AC_CODES[c ? 1 : 0]) ||
                    8 * w.raw + w.n - before > rtjm::BLOCK_BITS_MAX)
                    std::abort();                                       // the sizing pass and the packing pass disagree
            }
        w.pad();
        out.push_back(0xff);
        out.push_back((uint8_t)(k + 1 == s.intervals ? 0xd9 : 0xd0 + (k & 7)));
    }
    record[0] = (uint32_t)out.size(), record[1] = w.raw, record[2] = w.stuffed, record[3] = s.intervals, record[4] = 0;
}

}  // namespace

extern "C" {

// The file of a frame into out (capacity bytes; nothing is written if it does not fit), its size into record[0], the coefficients
// into coef[mcus * 192].  0, or 1 if the file does not fit.
int jpeg_encode_host(const uint8_t* rgb, uint32_t W, uint32_t R, uint32_t quality, uint32_t interval, int16_t* coef, uint8_t* out,
                     uint64_t capacity, uint32_t* record) {
    std::vector<int16_t> c;
    std::vector<uint8_t> o;
    encode(rgb, W, R, quality, interval, c, o, record);
    std::memcpy(coef, c.data(), c.size() * sizeof(int16_t));
    if (o.size() > capacity) return 1;
    std::memcpy(out, o.data(), o.size());
    return 0;
}

uint64_t jpeg_bound_host(uint32_t W, uint32_t R, uint32_t interval) { return rtjm::sizes_of(W, R, interval).bound; }

void jpeg_tables_host(uint32_t quality, uint8_t* out) { rtjm::quant_tables(quality, reinterpret_cast<uint8_t(*)[64]>(out)); }

}  // extern "C"

#ifdef JPEG_HOST_MAIN
// jpeg_host CORPUS RESULT.  CORPUS: u32 count, then per frame u32 W, R, quality, interval and R W 3 bytes.  RESULT: per frame the five
// record words, u32 mcus, the coefficients and the file.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* res = std::fopen(argv[2], "wb");
    if (!in || !res) return 2;
    uint32_t count = 0, frames = 0;
    if (std::fread(&count, 4, 1, in) != 1) return 2;
    uint64_t bytes = 0;
    for (uint32_t f = 0; f < count; f++) {
        uint32_t head[4];
        if (std::fread(head, 4, 4, in) != 4) return 2;
        std::vector<uint8_t> rgb((size_t)head[0] * head[1] * 3);          // exactly sized: a read past the frame is caught
        if (std::fread(rgb.data(), 1, rgb.size(), in) != rgb.size()) return 2;
        std::vector<int16_t> coef;
        std::vector<uint8_t> out;
        uint32_t record[5];
        encode(rgb.data(), head[0], head[1], head[2], head[3], coef, out, record);
        if (out.size() > rtjm::sizes_of(head[0], head[1], head[3]).bound) return 3;
        const uint32_t mcus = (uint32_t)(coef.size() / 192);
        std::fwrite(record, 4, 5, res);
        std::fwrite(&mcus, 4, 1, res);
        std::fwrite(coef.data(), 2, coef.size(), res);
        std::fwrite(out.data(), 1, out.size(), res);
        bytes += out.size(), frames++;
    }
    std::fclose(in);
    if (std::fclose(res) != 0) return 2;
    std::printf("%u frames encoded, %llu bytes\n", frames, (unsigned long long)bytes);
    return 0;
}
#endif
