// rt_bloom.hip — the host side of librt_bloom.so (rt_bloom.h): argument checks, the plan of a call's launches under
// its form, the choice of the kernels' instances, the launches.  No global state, no allocation; every function catches everything
// inside its body.
#include <cstring>

#include "rt_bloom.h"
#include "rt_bloom.hip.h"
#include "rt_private_host.h"

using namespace rtpriv;

static_assert(RTB_MAX_LEVELS == rtbm::MAX_LEVELS, "the header's limit");
static_assert(RTB_MIX == rtbm::MODE_MIX && RTB_ADD == rtbm::MODE_ADD, "the header's modes");
static_assert(RTB_FORM_LEVELS == rtbm::FORM_LEVELS && RTB_FORM_TAIL == rtbm::FORM_TAIL, "the header's forms");

namespace {

using DownKernel = void (*)(const rtbk::DownParams);
using TailKernel = void (*)(const rtbk::TailParams);
using CombineKernel = void (*)(const rtbk::CombineParams);

DownKernel down_instance(bool first, bool thresh) {
    if (!first) return rtbk::rtb_down_kernel<false, false>;
    return thresh ? rtbk::rtb_down_kernel<true, true> : rtbk::rtb_down_kernel<true, false>;
}

TailKernel tail_instance(bool first, bool thresh) {
    if (!first) return rtbk::rtb_tail_kernel<false, false>;
    return thresh ? rtbk::rtb_tail_kernel<true, true> : rtbk::rtb_tail_kernel<true, false>;
}

CombineKernel combine_instance(uint32_t mode, bool bloom) {
    if (mode == RTB_MIX) return bloom ? rtbk::rtb_combine_kernel<RTB_MIX, true> : rtbk::rtb_combine_kernel<RTB_MIX, false>;
    return bloom ? rtbk::rtb_combine_kernel<RTB_ADD, true> : rtbk::rtb_combine_kernel<RTB_ADD, false>;
}

dim3 tiles(uint32_t W, uint32_t R) { return dim3((W + rtbk::TW - 1) / rtbk::TW, (R + rtbk::TH - 1) / rtbk::TH); }

// the sizes both exports check: BAD_ARG, LIMIT or OK
int check_sizes(uint32_t W, uint32_t R, uint32_t levels) {
    if (W == 0 || R == 0 || levels < 1u || levels > RTB_MAX_LEVELS) return RTB_ERR_BAD_ARG;
    if ((uint64_t)W * R > rtbm::MAX_PIXELS) return RTB_ERR_LIMIT;
    return RTB_OK;
}

}  // namespace

RT_PRIVATE_EXPORT int rtb_version(uint32_t* version) {
    return guarded<RTB_ERR_INTERNAL>([&] {
        if (!version) return RTB_ERR_BAD_ARG;
        *version = RTB_VERSION;
        return RTB_OK;
    });
}

RT_PRIVATE_EXPORT int rtb_scratch_bytes(uint32_t W, uint32_t R, uint32_t levels, uint64_t* bytes) {
    return guarded<RTB_ERR_INTERNAL>([&] {
        if (!bytes) return RTB_ERR_BAD_ARG;
        const int sizes = check_sizes(W, R, levels);
        if (sizes != RTB_OK) return sizes;
        *bytes = rtbm::level_offset(W, R, levels + 1u);
        return RTB_OK;
    });
}

RT_PRIVATE_EXPORT int rtb_apply(const rtb_apply_args* a, void* stream_) {
    return guarded<RTB_ERR_INTERNAL>([&] {
        if (!a || a->reserved != 0) return RTB_ERR_BAD_ARG;
        const int sizes = check_sizes(a->W, a->R, a->levels);
        if (sizes != RTB_OK) return sizes;
        if (a->form != RTB_FORM_LEVELS && a->form != RTB_FORM_TAIL) return RTB_ERR_BAD_ARG;
        const rtbm::Settings s = {a->levels, a->mode, a->spread, a->strength, a->norm, a->cap, a->T, a->K};
        if (!rtbm::settings_ok(s)) return RTB_ERR_BAD_ARG;
        if (!a->in || !a->out || !a->scratch) return RTB_ERR_BAD_ARG;
        if (misaligned(a->in, 16) || misaligned(a->out, 16) || misaligned(a->out_bloom, 16) || misaligned(a->scratch, 16)) return RTB_ERR_BAD_ARG;
        const uint32_t W = a->W, R = a->R, L = a->levels;
        const uint64_t n = (uint64_t)W * R, need = rtbm::level_offset(W, R, L + 1u);
        if (a->scratch_bytes < need) return RTB_ERR_BAD_ARG;
        const Range all[] = {range(a->in, n * 12), range(a->out, n * 12), range(a->out_bloom, n * 12), range(a->scratch, need)};
        if (any_overlap(all)) return RTB_ERR_BAD_ARG;

        const hipStream_t stream = (hipStream_t)stream_;
        const bool thresh = a->T > 0.0f;
        const auto side_w = [&](uint32_t k) { return rtbm::level_side(W, k); };
        const auto side_r = [&](uint32_t k) { return rtbm::level_side(R, k); };
        // level k: the image for k = 0 (read only), otherwise its place in the scratch
        const auto level = [&](uint32_t k) { return (float*)((char*)a->scratch + rtbm::level_offset(W, R, k)); };

        // the tail takes the levels tf ... L; L + 1: there is none
        const uint32_t tf = a->form == RTB_FORM_TAIL ? rtbm::tail_from(W, R, L, rtbm::LDS_BUDGET) : L + 1u;
        const uint32_t downs = tf <= L ? tf - 1u : L;                                   // the levels 1 ... downs come from down launches

        for (uint32_t k = 1; k <= downs; k++) {
            rtbk::DownParams p;
            std::memset(&p, 0, sizeof p);
            p.Ws = side_w(k - 1u), p.Rs = side_r(k - 1u), p.Wd = side_w(k), p.Rd = side_r(k);
            p.src = k == 1u ? a->in : level(k - 1u);
            p.dst = level(k);
            p.cap = a->cap, p.T = a->T, p.K = a->K;
            hipLaunchKernelGGL(down_instance(k == 1u, thresh), tiles(p.Wd, p.Rd), dim3(rtbk::BLOCK), 0, stream, p);
            if (hipGetLastError() != hipSuccess) return RTB_ERR_HIP;
        }
        if (tf <= L) {
            rtbk::TailParams p;
            std::memset(&p, 0, sizeof p);
            p.Ws = side_w(tf - 1u), p.Rs = side_r(tf - 1u);
            p.first = tf, p.last = L;
            uint32_t at = 0;
            for (uint32_t k = tf; k <= L; k++) {
                p.W[k - tf] = side_w(k), p.R[k - tf] = side_r(k), p.at[k - tf] = at;
                at += 3u * p.W[k - tf] * p.R[k - tf];
            }
            if (4ull * at > rtbm::LDS_BUDGET) return RTB_ERR_INTERNAL;                  // (tail_from's rule)
            p.src = tf == 1u ? a->in : level(tf - 1u);
            p.dst = level(tf);
            p.cap = a->cap, p.T = a->T, p.K = a->K, p.spread = a->spread;
            const TailKernel k = tail_instance(tf == 1u, thresh);
            if (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rtbm::LDS_BUDGET) != hipSuccess)
                return RTB_ERR_HIP;
            hipLaunchKernelGGL(k, dim3(1), dim3(rtbk::TAIL_BLOCK), 4u * at, stream, p);
            if (hipGetLastError() != hipSuccess) return RTB_ERR_HIP;
        }
        // U_k = D_k + spread up(U_{k+1}) for the levels above the tail's first (or above the last)
        for (uint32_t k = (tf <= L ? tf : L) - 1u; k >= 1u; k--) {
            rtbk::UpAddParams p;
            std::memset(&p, 0, sizeof p);
            p.Wf = side_w(k), p.Rf = side_r(k), p.Wc = side_w(k + 1u), p.Rc = side_r(k + 1u);
            p.fine = level(k);
            p.coarse = level(k + 1u);
            p.spread = a->spread;
            hipLaunchKernelGGL(rtbk::rtb_upadd_kernel, tiles(p.Wf / 2u + 1u, p.Rf / 2u + 1u), dim3(rtbk::BLOCK), 0, stream, p);
            if (hipGetLastError() != hipSuccess) return RTB_ERR_HIP;
        }
        rtbk::CombineParams p;
        std::memset(&p, 0, sizeof p);
        p.W = W, p.W1 = side_w(1), p.R1 = side_r(1);
        p.floats = 3 * n;
        p.groups = (uint32_t)((p.floats + 3) / 4);
        p.in = a->in, p.U1 = level(1), p.out = a->out, p.out_bloom = a->out_bloom;
        p.strength = a->strength, p.keep = 1.0f - a->strength, p.norm = a->norm;
        hipLaunchKernelGGL(combine_instance(a->mode, a->out_bloom != nullptr), dim3((p.groups + rtbk::BLOCK - 1) / rtbk::BLOCK),
                           dim3(rtbk::BLOCK), 0, stream, p);
        return after_launch(RTB_OK, RTB_ERR_HIP);
    });
}
