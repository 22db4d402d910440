// rt_robust.hip — the host side of librt_robust.so (rt_robust.h): argument checks, the choice of the resolve kernel's
// instance by K, the launches.  No global state, no allocation; every function catches everything inside its body.
#include <cstring>

#include "rt_robust.h"
#include "rt_robust.hip.h"
#include "rt_private_host.h"

using namespace rtpriv;

namespace {

using ResolveKernel = void (*)(const rtrk::ResolveParams);

// the instance for a bucket count: seven of them, odd 3 ... 15
ResolveKernel resolve_instance(uint32_t K) {
    switch (K) {
        case 3: return rtrk::rtr_resolve_kernel<3>;
        case 5: return rtrk::rtr_resolve_kernel<5>;
        case 7: return rtrk::rtr_resolve_kernel<7>;
        case 9: return rtrk::rtr_resolve_kernel<9>;
        case 11: return rtrk::rtr_resolve_kernel<11>;
        case 13: return rtrk::rtr_resolve_kernel<13>;
        case 15: return rtrk::rtr_resolve_kernel<15>;
        default: return nullptr;
    }
}

constexpr uint64_t MAX_COUNT = 0x7fffffffull;     // pixels, and records, of a call

}  // namespace

RT_PRIVATE_EXPORT int rtr_version(uint32_t* version) {
    return guarded<RTR_ERR_INTERNAL>([&] {
        if (!version) return RTR_ERR_BAD_ARG;
        *version = RTR_VERSION;
        return RTR_OK;
    });
}

RT_PRIVATE_EXPORT int rtr_fold(const rtr_fold_args* a, void* stream) {
    return guarded<RTR_ERR_INTERNAL>([&] {
        if (!a || a->pixels == 0 || a->n == 0 || !rtrm::buckets_ok(a->K)) return RTR_ERR_BAD_ARG;
        if (!a->records || !a->buckets || misaligned(a->records) || misaligned(a->buckets)) return RTR_ERR_BAD_ARG;
        const uint64_t P = a->pixels;
        if (a->bucket_stride < 3 * P) return RTR_ERR_BAD_ARG;          // the parts of two buckets would overlap
        if (P > MAX_COUNT || P * a->n > MAX_COUNT || a->bucket_stride > (1ull << 40)) return RTR_ERR_LIMIT;
        const Range rec = range(a->records, P * a->n * 12);
        for (uint32_t k = 0; k < a->K; k++)
            if (overlap(rec, range((const void*)((uintptr_t)a->buckets + (uintptr_t)(k * a->bucket_stride * 4)), P * 12)))
                return RTR_ERR_BAD_ARG;

        rtrk::FoldParams p;
        std::memset(&p, 0, sizeof p);
        p.pixels = a->pixels, p.n = a->n, p.first_mod_K = a->first % a->K, p.K = a->K;
        p.bucket_stride = (size_t)a->bucket_stride;
        p.records = a->records;
        p.buckets = a->buckets;
        const dim3 grid((a->pixels + rtrk::BLOCK - 1) / rtrk::BLOCK);
        hipLaunchKernelGGL(rtrk::rtr_fold_kernel, grid, dim3(rtrk::BLOCK), 0, (hipStream_t)stream, p);
        return after_launch(RTR_OK, RTR_ERR_HIP);
    });
}

RT_PRIVATE_EXPORT int rtr_resolve(const rtr_resolve_args* a, void* stream) {
    return guarded<RTR_ERR_INTERNAL>([&] {
        if (!a || a->W == 0 || a->R == 0 || !rtrm::buckets_ok(a->K) || a->samples < a->K) return RTR_ERR_BAD_ARG;
        if (a->mode != RTR_GINI && a->mode != RTR_TRIM) return RTR_ERR_BAD_ARG;
        if (a->mode == RTR_TRIM ? a->c > (a->K - 1) / 2 : a->c != 0) return RTR_ERR_BAD_ARG;
        if (!a->buckets) return RTR_ERR_BAD_ARG;
        if (!a->out_linear && !a->out_gini && !a->out_kept && !a->out_variance && !a->out_accum && !a->out_moments) return RTR_ERR_BAD_ARG;
        const void* dwords[] = {a->buckets, a->out_linear, a->out_gini, a->out_kept, a->out_variance, a->out_accum, a->out_moments};
        for (const void* q : dwords)
            if (misaligned(q)) return RTR_ERR_BAD_ARG;
        const uint64_t n = (uint64_t)a->W * a->R;
        if (n > MAX_COUNT) return RTR_ERR_LIMIT;
        // an output overlaps neither the buckets nor another output
        const Range all[] = {range(a->buckets, n * a->K * 12), range(a->out_linear, n * 12), range(a->out_gini, n * 4),
                             range(a->out_kept, n * 4),        range(a->out_variance, n * 4), range(a->out_accum, n * 12),
                             range(a->out_moments, n * 8)};
        if (any_overlap(all)) return RTR_ERR_BAD_ARG;

        rtrk::ResolveParams p;
        std::memset(&p, 0, sizeof p);
        p.call = rtrm::make_call(a->K, a->samples, a->mode, a->c);
        p.pixels = (uint32_t)n;
        p.buckets = a->buckets;
        p.out_linear = a->out_linear;
        p.out_gini = a->out_gini;
        p.out_kept = a->out_kept;
        p.out_variance = a->out_variance;
        p.out_accum = a->out_accum;
        p.out_moments = a->out_moments;
        const ResolveKernel k = resolve_instance(a->K);
        if (!k) return RTR_ERR_INTERNAL;
        const dim3 grid(((uint32_t)n + rtrk::BLOCK - 1) / rtrk::BLOCK);
        hipLaunchKernelGGL(k, grid, dim3(rtrk::BLOCK), 0, (hipStream_t)stream, p);
        return after_launch(RTR_OK, RTR_ERR_HIP);
    });
}
