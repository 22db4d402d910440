// rt_film.hip — the host side of librt_film.so (rt_film.h): argument checks, the plan, the launches.  No global
// state, no allocation; every function catches everything inside its body.
#include <cmath>
#include <cstring>

#include "rt_film.h"
#include "rt_film.hip.h"
#include "rt_private_host.h"
#include "rt_plan.h"

using namespace rtpriv;

namespace {

bool finite_nonneg(float v) { return std::isfinite(v) && v >= 0.0f; }

using StepFn = void (*)(const rtfk::ResolveParams);

StepFn step_kernel(bool lds, bool final_step) {
    if (lds) return final_step ? rtfk::rtf_step_kernel<true, true> : rtfk::rtf_step_kernel<true, false>;
    return final_step ? rtfk::rtf_step_kernel<false, true> : rtfk::rtf_step_kernel<false, false>;
}

// grid cap of the grid-stride kernels: 256 CUs of 8 workgroups of 256
constexpr uint64_t GRID_CAP = 2048;
// dynamic LDS above this needs the kernel's limit raised first
constexpr size_t LDS_DEFAULT_MAX = 64 * 1024;

int check_image(uint32_t W, uint32_t R) {
    if (W == 0 || R == 0) return RTF_ERR_BAD_ARG;
    if (W >= (1u << 30) || R >= (1u << 30)) return RTF_ERR_LIMIT;                 // (taps in int)
    if ((uint64_t)W * R > 0x7FFFFFFFull) return RTF_ERR_LIMIT;                    // plan_denoise's largest frame
    return RTF_OK;
}

// the appended fields of rtf_resolve_args, which kind 0 leaves at 0
bool regress_fields_unset(const rtf_resolve_args* a) {
    return !a->albedo && a->aov_samples == 0 && a->albedo_eps == 0.0f && a->ridge == 0.0f && a->reserved == 0 && !a->model &&
           a->model_bytes == 0;
}

// kind RTF_RESOLVE_REGRESS: the fit, a workgroup per node, then the apply, a lane per pixel
int resolve_regress(const rtf_resolve_args* a, void* stream) {
    if (a->samples < 1 || a->iterations != 0 || a->out_variance || a->reserved != 0) return RTF_ERR_BAD_ARG;
    if (!a->out_rgb && !a->out_f32 && !a->out_linear) return RTF_ERR_BAD_ARG;
    if (!a->accum || !a->model || misaligned(a->model, 16)) return RTF_ERR_BAD_ARG;
    if (!std::isfinite(a->ridge) || !(a->ridge > 0.0f)) return RTF_ERR_BAD_ARG;
    if (a->depth && !a->hits) return RTF_ERR_BAD_ARG;
    if (a->albedo && (!std::isfinite(a->albedo_eps) || !(a->albedo_eps > 0.0f))) return RTF_ERR_BAD_ARG;
    if ((a->albedo || a->normal || a->depth || a->hits) && a->aov_samples < 1) return RTF_ERR_BAD_ARG;
    const uint32_t NX = rtfm::rg_nodes(a->W), NY = rtfm::rg_nodes(a->R);
    const uint64_t nodes = (uint64_t)NX * NY;
    if (nodes > 0x7FFFFFFFull) return RTF_ERR_LIMIT;
    if (a->model_bytes < nodes * rtfm::RG_RECORD * sizeof(float)) return RTF_ERR_SCRATCH;
    hipStream_t st = (hipStream_t)stream;

    rtfk::RegressParams p;
    std::memset(&p, 0, sizeof p);
    p.W = a->W;
    p.R = a->R;
    p.NX = NX;
    p.NY = NY;
    p.ridge = a->ridge;
    p.pl.accum = a->accum;
    p.pl.albedo = a->albedo;
    p.pl.normal = a->normal;
    p.pl.depth = a->depth;
    p.pl.hits = a->hits;
    p.pl.e_f = (float)a->samples;
    p.pl.k_f = (float)a->aov_samples;
    p.pl.albedo_eps = a->albedo_eps;
    p.model = a->model;
    p.rgb = a->out_rgb;
    p.f32 = a->out_f32;
    p.lin = a->out_linear;
    hipLaunchKernelGGL(rtfk::rtf_regress_fit_kernel, dim3((uint32_t)nodes), dim3(rtfk::RG_BLOCK), 0, st, p);
    if (int rc = after_launch(RTF_OK, RTF_ERR_HIP)) return rc;
    const uint64_t npix = (uint64_t)a->W * a->R;
    hipLaunchKernelGGL(rtfk::rtf_regress_apply_kernel, dim3((uint32_t)((npix + rtfk::BLOCK - 1) / rtfk::BLOCK)), dim3(rtfk::BLOCK), 0, st, p);
    return after_launch(RTF_OK, RTF_ERR_HIP);
}

}  // namespace

RT_PRIVATE_EXPORT int rtf_version(uint32_t* version) {
    return guarded<RTF_ERR_INTERNAL>([&] {
        if (!version) return RTF_ERR_BAD_ARG;
        *version = RTF_VERSION;
        return RTF_OK;
    });
}

RT_PRIVATE_EXPORT int rtf_fold_moments(const float* records, uint64_t P, uint32_t n, float* accum, float* moments, void* stream) {
    return guarded<RTF_ERR_INTERNAL>([&] {
        if (!records || !accum || !moments || P == 0 || n == 0) return RTF_ERR_BAD_ARG;
        if (P > 0x7FFFFFFFull) return RTF_ERR_LIMIT;                              // a strip of the tile ABI's largest frame
        const uint32_t blocks = (uint32_t)((P + rtfk::BLOCK - 1) / rtfk::BLOCK);
        hipLaunchKernelGGL(rtfk::rtf_fold_kernel, dim3(blocks), dim3(rtfk::BLOCK), 0, (hipStream_t)stream, records, P, n, accum, moments);
        return after_launch(RTF_OK, RTF_ERR_HIP);
    });
}

RT_PRIVATE_EXPORT int rtf_resolve_scratch_bytes(uint32_t W, uint32_t R, uint64_t* bytes) {
    return guarded<RTF_ERR_INTERNAL>([&] {
        if (!bytes) return RTF_ERR_BAD_ARG;
        if (int rc = check_image(W, R)) return rc;
        *bytes = rtplan::plan_denoise(W, R, 0, false).scratch_bytes;
        return RTF_OK;
    });
}

RT_PRIVATE_EXPORT int rtf_resolve(const rtf_resolve_args* a, void* stream) {
    return guarded<RTF_ERR_INTERNAL>([&] {
        if (!a) return RTF_ERR_BAD_ARG;
        if (int rc = check_image(a->W, a->R)) return rc;
        if (a->kind == RTF_RESOLVE_REGRESS) return resolve_regress(a, stream);
        if (a->kind != RTF_RESOLVE_ATROUS || !regress_fields_unset(a)) return RTF_ERR_BAD_ARG;
        if (a->samples < 2 || a->iterations > RTF_MAX_ITERATIONS) return RTF_ERR_BAD_ARG;
        if (!finite_nonneg(a->sigma_l) || !finite_nonneg(a->k_normal) || !finite_nonneg(a->k_depth)) return RTF_ERR_BAD_ARG;
        if (!std::isfinite(a->var_eps) || !(a->var_eps > 0.0f)) return RTF_ERR_BAD_ARG;
        if (!a->accum || !a->moments || !a->scratch) return RTF_ERR_BAD_ARG;
        if (a->depth && !a->hits) return RTF_ERR_BAD_ARG;
        if (!a->out_rgb && !a->out_f32 && !a->out_linear && !a->out_variance) return RTF_ERR_BAD_ARG;
        if (misaligned(a->scratch, 16)) return RTF_ERR_BAD_ARG;
        const uint32_t W = a->W, R = a->R;
        const uint32_t mask = (a->normal ? rtdn::P_NORMAL : 0u) | (a->depth ? rtdn::P_DEPTH : 0u) | (a->hits ? rtdn::P_HITS : 0u);
        const bool guided = mask != 0;
        const uint32_t lstep = a->lds_max_step > (1u << 30) ? rtplan::DN_LDS_MAX_STEP : a->lds_max_step;
        const rtplan::DenoisePlan pl = rtplan::plan_denoise(W, R, a->iterations, guided, lstep);
        if (a->scratch_bytes < pl.scratch_bytes) return RTF_ERR_SCRATCH;
        char* scratch = (char*)a->scratch;
        hipStream_t st = (hipStream_t)stream;

        rtfk::ResolveParams p;
        std::memset(&p, 0, sizeof p);
        p.W = W;
        p.R = R;
        p.planes = mask;
        p.e_f = (float)a->samples;
        p.sigma_l = a->sigma_l;
        p.var_eps = a->var_eps;
        p.kn = a->k_normal;
        p.kd = a->k_depth;
        p.accum = a->accum;
        p.moments = a->moments;
        p.normal = a->normal;
        p.depth = a->depth;
        p.hits = a->hits;
        p.rgb = a->out_rgb;
        p.f32 = a->out_f32;
        p.lin = a->out_linear;
        p.var = a->out_variance;
        p.guide = (float4*)(scratch + pl.off_guide);
        float4* buf[2] = {(float4*)(scratch + pl.off_color[0]), (float4*)(scratch + pl.off_color[1])};
        const uint32_t stride_blocks = (uint32_t)std::min<uint64_t>((pl.npix + rtfk::BLOCK - 1) / rtfk::BLOCK, GRID_CAP);
        const uint32_t tiles = pl.tiles_x * ((R + rtplan::DN_TILE_Y - 1) / rtplan::DN_TILE_Y);

        p.dst = buf[0];
        hipLaunchKernelGGL(rtfk::rtf_entry_kernel, dim3(stride_blocks), dim3(rtfk::BLOCK), 0, st, p);
        if (int rc = after_launch(RTF_OK, RTF_ERR_HIP)) return rc;
        uint32_t cur = 0;
        for (uint32_t i = 0; i < a->iterations; i++) {
            p.s = pl.step[i];
            p.src = buf[cur];
            p.dst = buf[cur ^ 1u];
            const StepFn kern = step_kernel(pl.lds[i] != 0, i + 1 == a->iterations);
            if (pl.lds[i] > LDS_DEFAULT_MAX &&
                hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rtplan::DN_LDS_CU) != hipSuccess)
                return RTF_ERR_HIP;
            hipLaunchKernelGGL(kern, dim3(tiles), dim3(rtplan::DN_BLOCK), pl.lds[i], st, p);
            if (int rc = after_launch(RTF_OK, RTF_ERR_HIP)) return rc;
            cur ^= 1u;
        }
        if (a->iterations == 0) {
            p.src = buf[0];
            hipLaunchKernelGGL(rtfk::rtf_output_kernel, dim3(stride_blocks), dim3(rtfk::BLOCK), 0, st, p);
            if (int rc = after_launch(RTF_OK, RTF_ERR_HIP)) return rc;
        }
        return RTF_OK;
    });
}
