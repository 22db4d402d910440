// rt_display.hip — the host side of librt_display.so (rt_display.h): argument checks, the choice of the kernels'
// instances, the launches.  No global state, no allocation; every function catches everything inside its body.
#include <cstring>

#include "rt_display.h"
#include "rt_display.hip.h"
#include "rt_private_host.h"

using namespace rtpriv;

static_assert(RTD_HIST_WORDS == rtdm::HIST_WORDS && RTD_RECORD_WORDS == rtdm::RECORD_WORDS, "the header's sizes");
static_assert(RTD_AUTO == rtdm::MODE_AUTO && RTD_MANUAL == rtdm::MODE_MANUAL, "the header's modes");
static_assert(RTD_NONE == rtdm::CURVE_NONE && RTD_REINHARD == rtdm::CURVE_REINHARD && RTD_FILMIC == rtdm::CURVE_FILMIC, "the header's curves");
static_assert(RTD_HIST_WAVE == rtdk::FORM_WAVE && RTD_HIST_MATCH == rtdk::FORM_MATCH, "the header's forms");

namespace {

using ApplyKernel = void (*)(const rtdk::ApplyParams);

// the instance for a curve and the dither flag: six of them
ApplyKernel apply_instance(uint32_t curve, bool dither) {
    switch (curve) {
        case RTD_NONE: return dither ? rtdk::rtd_apply_kernel<RTD_NONE, true> : rtdk::rtd_apply_kernel<RTD_NONE, false>;
        case RTD_REINHARD: return dither ? rtdk::rtd_apply_kernel<RTD_REINHARD, true> : rtdk::rtd_apply_kernel<RTD_REINHARD, false>;
        case RTD_FILMIC: return dither ? rtdk::rtd_apply_kernel<RTD_FILMIC, true> : rtdk::rtd_apply_kernel<RTD_FILMIC, false>;
        default: return nullptr;
    }
}

constexpr uint64_t MAX_PIXELS = 0x7fffffffull;
constexpr uint64_t HIST_BYTES = 4 * RTD_HIST_WORDS, RECORD_BYTES = 4 * RTD_RECORD_WORDS;

}  // namespace

RT_PRIVATE_EXPORT int rtd_version(uint32_t* version) {
    return guarded<RTD_ERR_INTERNAL>([&] {
        if (!version) return RTD_ERR_BAD_ARG;
        *version = RTD_VERSION;
        return RTD_OK;
    });
}

RT_PRIVATE_EXPORT int rtd_meter(const rtd_meter_args* a, void* stream) {
    return guarded<RTD_ERR_INTERNAL>([&] {
        if (!a || a->W == 0 || a->R == 0 || a->reserved != 0) return RTD_ERR_BAD_ARG;
        if (a->form != RTD_HIST_WAVE && a->form != RTD_HIST_MATCH) return RTD_ERR_BAD_ARG;
        if (!a->linear || !a->hist || misaligned(a->linear) || misaligned(a->hist)) return RTD_ERR_BAD_ARG;
        const uint64_t n = (uint64_t)a->W * a->R;
        if (n > MAX_PIXELS) return RTD_ERR_LIMIT;
        if (overlap(range(a->linear, n * 12), range(a->hist, HIST_BYTES))) return RTD_ERR_BAD_ARG;

        if (hipMemsetAsync(a->hist, 0, HIST_BYTES, (hipStream_t)stream) != hipSuccess) return RTD_ERR_HIP;
        rtdk::MeterParams p;
        std::memset(&p, 0, sizeof p);
        p.pixels = (uint32_t)n;
        p.linear = a->linear;
        p.hist = a->hist;
        const uint64_t blocks = (n + rtdk::CHUNK - 1) / rtdk::CHUNK;
        const dim3 grid((uint32_t)(blocks < rtdk::MAX_GRID ? blocks : rtdk::MAX_GRID));
        if (a->form == RTD_HIST_WAVE)
            hipLaunchKernelGGL(rtdk::rtd_meter_kernel<rtdk::FORM_WAVE>, grid, dim3(rtdk::METER_BLOCK), 0, (hipStream_t)stream, p);
        else
            hipLaunchKernelGGL(rtdk::rtd_meter_kernel<rtdk::FORM_MATCH>, grid, dim3(rtdk::METER_BLOCK), 0, (hipStream_t)stream, p);
        return after_launch(RTD_OK, RTD_ERR_HIP);
    });
}

RT_PRIVATE_EXPORT int rtd_expose(const rtd_expose_args* a, void* stream) {
    return guarded<RTD_ERR_INTERNAL>([&] {
        if (!a || a->reserved != 0) return RTD_ERR_BAD_ARG;
        rtdk::ExposeParams p;
        std::memset(&p, 0, sizeof p);
        p.e.mode = a->mode;
        p.e.key = a->key, p.e.key_q16 = a->key_q16, p.e.white_q16 = a->white_q16;
        p.e.rate = a->rate, p.e.scale_min = a->scale_min, p.e.scale_max = a->scale_max;
        p.e.scale = a->scale, p.e.white = a->white;
        if (!rtdm::exposure_ok(p.e)) return RTD_ERR_BAD_ARG;
        if (!a->record || misaligned(a->record) || misaligned(a->hist)) return RTD_ERR_BAD_ARG;
        if (a->mode == RTD_AUTO) {
            if (!a->hist || overlap(range(a->hist, HIST_BYTES), range(a->record, RECORD_BYTES))) return RTD_ERR_BAD_ARG;
            p.hist = a->hist;
        }
        p.record = a->record;
        hipLaunchKernelGGL(rtdk::rtd_expose_kernel, dim3(1), dim3(rtdk::BLOCK), 0, (hipStream_t)stream, p);
        return after_launch(RTD_OK, RTD_ERR_HIP);
    });
}

RT_PRIVATE_EXPORT int rtd_apply(const rtd_apply_args* a, void* stream) {
    return guarded<RTD_ERR_INTERNAL>([&] {
        if (!a || a->W == 0 || a->R == 0 || a->dither > 1u) return RTD_ERR_BAD_ARG;
        const ApplyKernel k = apply_instance(a->curve, a->dither != 0u);
        if (!k) return RTD_ERR_BAD_ARG;
        if (!a->linear || !a->record || (!a->out_f32 && !a->out_rgb)) return RTD_ERR_BAD_ARG;
        if (misaligned(a->linear, 16) || misaligned(a->out_f32, 16) || misaligned(a->out_rgb) || misaligned(a->record)) return RTD_ERR_BAD_ARG;
        const uint64_t n = (uint64_t)a->W * a->R;
        if (n > MAX_PIXELS) return RTD_ERR_LIMIT;
        // no buffer overlaps another
        const Range all[] = {range(a->linear, n * 12), range(a->record, RECORD_BYTES), range(a->out_f32, n * 12), range(a->out_rgb, n * 3)};
        if (any_overlap(all)) return RTD_ERR_BAD_ARG;

        rtdk::ApplyParams p;
        std::memset(&p, 0, sizeof p);
        p.W = a->W;
        p.floats = 3 * n;
        p.groups = (uint32_t)((p.floats + 3) / 4);
        p.linear = a->linear;
        p.record = a->record;
        p.out_f32 = a->out_f32;
        p.out_rgb = a->out_rgb;
        const dim3 grid((p.groups + rtdk::BLOCK - 1) / rtdk::BLOCK);
        hipLaunchKernelGGL(k, grid, dim3(rtdk::BLOCK), 0, (hipStream_t)stream, p);
        return after_launch(RTD_OK, RTD_ERR_HIP);
    });
}
