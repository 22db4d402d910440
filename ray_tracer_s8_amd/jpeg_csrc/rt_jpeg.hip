// rt_jpeg.hip — the host side of librt_jpeg.so (rt_jpeg.h): argument checks, the header's bytes, the sizes, the
// launches.  No global state, no allocation; every function catches everything inside its body.
#include <cstring>

#include "rt_jpeg.h"
#include "rt_jpeg.hip.h"
#include "rt_private_host.h"

using namespace rtpriv;

static_assert(RTJ_HEADER_LEN == rtjm::HEADER_LEN && RTJ_RECORD_WORDS == rtjm::RECORD_WORDS, "the header's sizes");
static_assert(RTJ_MAX_INTERVAL == rtjm::MAX_INTERVAL && RTJ_MAX_SIDE == rtjm::MAX_SIDE, "the header's limits");

namespace {

bool frame_ok(uint32_t W, uint32_t R, uint32_t interval) {
    return W >= 1u && W <= RTJ_MAX_SIDE && R >= 1u && R <= RTJ_MAX_SIDE && interval >= 1u && interval <= RTJ_MAX_INTERVAL;
}

// what the kernels index in 32 bits: the raw stream's bits and the file's bytes
bool fits(const rtjm::Sizes& s) { return 8u * s.raw_bound <= 0xffffffffull && s.bound <= 0xffffffffull; }

// the two tables of the arguments in natural order: RTJ_OK, or RTJ_ERR_BAD_ARG for a quality out of range, tables with a quality,
// no tables without one, or an entry of 0
int tables_of(const rtj_encode_args* a, uint8_t q[2][64]) {
    if (a->quality > 100u || (a->quality == 0u) != (a->tables != nullptr)) return RTJ_ERR_BAD_ARG;
    if (a->quality) {
        rtjm::quant_tables(a->quality, q);
        return RTJ_OK;
    }
    std::memcpy(q, a->tables, 128);
    for (int i = 0; i < 128; i++)
        if (q[i >> 6][i & 63] == 0u) return RTJ_ERR_BAD_ARG;
    return RTJ_OK;
}

}  // namespace

RT_PRIVATE_EXPORT int rtj_version(uint32_t* version) {
    return guarded<RTJ_ERR_INTERNAL>([&] {
        if (!version) return RTJ_ERR_BAD_ARG;
        *version = RTJ_VERSION;
        return RTJ_OK;
    });
}

RT_PRIVATE_EXPORT int rtj_header(const rtj_encode_args* a, uint8_t* out, uint64_t capacity, uint64_t* out_len) {
    return guarded<RTJ_ERR_INTERNAL>([&] {
        if (!a || !out || !out_len || !frame_ok(a->W, a->R, a->interval)) return RTJ_ERR_BAD_ARG;
        uint8_t q[2][64];
        if (const int status = tables_of(a, q)) return status;
        if (capacity < RTJ_HEADER_LEN) return RTJ_ERR_LIMIT;
        rtjm::write_header(a->W, a->R, a->interval, q, out);
        *out_len = RTJ_HEADER_LEN;
        return RTJ_OK;
    });
}

RT_PRIVATE_EXPORT int rtj_bound(uint32_t W, uint32_t R, uint32_t interval, uint64_t* out_bytes) {
    return guarded<RTJ_ERR_INTERNAL>([&] {
        if (!out_bytes || !frame_ok(W, R, interval)) return RTJ_ERR_BAD_ARG;
        const rtjm::Sizes s = rtjm::sizes_of(W, R, interval);
        if (!fits(s)) return RTJ_ERR_LIMIT;
        *out_bytes = s.bound;
        return RTJ_OK;
    });
}

RT_PRIVATE_EXPORT int rtj_scratch_bytes(uint32_t W, uint32_t R, uint32_t interval, uint64_t* out_bytes) {
    return guarded<RTJ_ERR_INTERNAL>([&] {
        if (!out_bytes || !frame_ok(W, R, interval)) return RTJ_ERR_BAD_ARG;
        const rtjm::Sizes s = rtjm::sizes_of(W, R, interval);
        if (!fits(s)) return RTJ_ERR_LIMIT;
        *out_bytes = rtjk::layout_of(s).total;
        return RTJ_OK;
    });
}

RT_PRIVATE_EXPORT int rtj_encode(const rtj_encode_args* a, void* stream) {
    return guarded<RTJ_ERR_INTERNAL>([&] {
        if (!a || !frame_ok(a->W, a->R, a->interval) || a->reserved != 0u) return RTJ_ERR_BAD_ARG;
        uint8_t q[2][64];
        if (const int status = tables_of(a, q)) return status;
        if (!a->rgb || !a->scratch || !a->out || !a->record) return RTJ_ERR_BAD_ARG;
        if (misaligned(a->rgb) || misaligned(a->scratch, 256) || misaligned(a->record)) return RTJ_ERR_BAD_ARG;
        if (a->header_len != RTJ_HEADER_LEN || a->capacity <= a->header_len) return RTJ_ERR_BAD_ARG;
        const rtjm::Sizes s = rtjm::sizes_of(a->W, a->R, a->interval);
        if (!fits(s)) return RTJ_ERR_LIMIT;
        const rtjk::Layout l = rtjk::layout_of(s);
        if (a->scratch_bytes < l.total) return RTJ_ERR_BAD_ARG;
        // no buffer overlaps another
        const Range all[] = {range(a->rgb, (uint64_t)a->W * a->R * 3u), range(a->scratch, a->scratch_bytes), range(a->out, a->capacity),
                             range(a->record, 4u * RTJ_RECORD_WORDS)};
        if (any_overlap(all)) return RTJ_ERR_BAD_ARG;

        const hipStream_t st = (hipStream_t)stream;
        uint8_t* base = static_cast<uint8_t*>(a->scratch);
        auto words = [&](uint64_t at) { return reinterpret_cast<uint32_t*>(base + at); };

        rtjk::TransformParams t;
        std::memset(&t, 0, sizeof t);
        t.W = a->W, t.R = a->R, t.mw = s.mw, t.mcus = s.mcus;
        t.rgb = a->rgb;
        t.coef = words(l.coef);
        for (int i = 0; i < 128; i++) t.q[i >> 6][i & 63] = q[i >> 6][i & 63];

        rtjk::StreamParams p;
        std::memset(&p, 0, sizeof p);
        p.mcus = s.mcus, p.interval = a->interval, p.intervals = s.intervals, p.header_len = a->header_len;
        p.capacity = a->capacity;
        p.coef = reinterpret_cast<const int16_t*>(base + l.coef);
        p.mbits = words(l.mbits), p.msums = words(l.msums), p.ibytes = words(l.ibytes), p.isums = words(l.isums);
        p.iff = words(l.iff), p.fsums = words(l.fsums), p.raw = words(l.raw);
        p.out = a->out;
        p.record = a->record;

        const dim3 block(rtjk::BLOCK);
        const dim3 per_mcu((s.mcus + rtjk::BLOCK - 1u) / rtjk::BLOCK), per_interval((s.intervals + rtjk::BLOCK - 1u) / rtjk::BLOCK);
        const dim3 per_wave((s.intervals + rtjk::WAVES - 1u) / rtjk::WAVES);
        // an exclusive scan of n words in place: two launches
        auto scan = [&](uint32_t* v, uint32_t* sums, uint32_t n) {
            const rtjk::ScanParams sp{n, v, sums};
            hipLaunchKernelGGL(rtjk::rtj_scan_blocks_kernel, dim3(rtjk::chunks(n)), block, 0, st, sp);
            if (hipGetLastError() != hipSuccess) return false;
            const rtjk::ScanParams tp{rtjk::chunks(n), v, sums};
            hipLaunchKernelGGL(rtjk::rtj_scan_sums_kernel, dim3(1), dim3(rtjk::SUMS_BLOCK), 0, st, tp);
            return hipGetLastError() == hipSuccess;
        };
#define RTJ_LAUNCHED() \
    if (hipGetLastError() != hipSuccess) return RTJ_ERR_HIP

        if (hipMemsetAsync(base + l.raw, 0, l.raw_bytes, st) != hipSuccess) return RTJ_ERR_HIP;
        hipLaunchKernelGGL(rtjk::rtj_transform_kernel, dim3((s.mcus + rtjk::MCUS_PER_BLOCK - 1u) / rtjk::MCUS_PER_BLOCK), block, 0, st, t);
        RTJ_LAUNCHED();
        hipLaunchKernelGGL(rtjk::rtj_size_kernel, per_mcu, block, 0, st, p);
        RTJ_LAUNCHED();
        if (!scan(p.mbits, p.msums, s.mcus)) return RTJ_ERR_HIP;
        hipLaunchKernelGGL(rtjk::rtj_interval_kernel, per_interval, block, 0, st, p);
        RTJ_LAUNCHED();
        if (!scan(p.ibytes, p.isums, s.intervals)) return RTJ_ERR_HIP;
        hipLaunchKernelGGL(rtjk::rtj_pack_kernel, per_mcu, block, 0, st, p);
        RTJ_LAUNCHED();
        hipLaunchKernelGGL(rtjk::rtj_count_kernel, per_wave, block, 0, st, p);
        RTJ_LAUNCHED();
        if (!scan(p.iff, p.fsums, s.intervals)) return RTJ_ERR_HIP;
        hipLaunchKernelGGL(rtjk::rtj_scatter_kernel, per_wave, block, 0, st, p);
#undef RTJ_LAUNCHED
        return after_launch(RTJ_OK, RTJ_ERR_HIP);
    });
}
