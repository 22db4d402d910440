// rt_sampler.hip — the host side of librt_sampler.so (rt_sampler.h): argument checks, the scratch layout, the launches.
// No global state, no allocation; every function catches everything inside its body, and every refusal comes before any launch.
#include <cmath>
#include <cstring>

#include "rt_sampler.h"
#include "rt_sampler.hip.h"
#include "rt_private_host.h"

using namespace rtpriv;

namespace {

// the select's scratch: the noisy bytes, the active bytes, then (8-byte aligned) the workgroup offsets of every strip
struct Layout {
    uint32_t P, strips, bps;
    uint64_t offsets_at, bytes;
};

int check_image(uint32_t W, uint32_t R) {
    if (W == 0 || R == 0) return RTS_ERR_BAD_ARG;
    if ((uint64_t)W * R > 0x7FFFFFFFull) return RTS_ERR_LIMIT;                    // strip indices and list positions in uint32
    return RTS_OK;
}

int layout(uint32_t W, uint32_t R, uint32_t Hs, Layout& l) {
    if (int rc = check_image(W, R)) return rc;
    if (Hs == 0 || R % Hs != 0) return RTS_ERR_BAD_ARG;
    l.P = Hs * W;
    l.strips = R / Hs;
    if (l.strips > 65535u) return RTS_ERR_LIMIT;                                  // a strip is a grid row
    l.bps = (l.P + rtsk::BLOCK - 1u) / rtsk::BLOCK;
    const uint64_t pixels = (uint64_t)W * R;
    l.offsets_at = (2u * pixels + 7u) & ~7ull;
    l.bytes = l.offsets_at + 4ull * l.strips * l.bps;
    return RTS_OK;
}

// what gather and fold agree on
int check_chunk(uint32_t n_active, uint32_t k, uint32_t pixels, uint32_t reserved, const uint32_t* active) {
    if (k == 0 || pixels == 0 || reserved != 0 || n_active > pixels) return RTS_ERR_BAD_ARG;
    if (n_active != 0 && (!active || misaligned(active))) return RTS_ERR_BAD_ARG;
    if ((uint64_t)pixels * k > (1ull << 30)) return RTS_ERR_LIMIT;                // half-records and floats in a grid of uint32 blocks
    return RTS_OK;
}

}  // namespace

RT_PRIVATE_EXPORT int rts_version(uint32_t* version) {
    return guarded<RTS_ERR_INTERNAL>([&] {
        if (!version) return RTS_ERR_BAD_ARG;
        *version = RTS_VERSION;
        return RTS_OK;
    });
}

RT_PRIVATE_EXPORT int rts_scratch_bytes(uint32_t W, uint32_t R, uint32_t Hs, uint64_t* bytes) {
    return guarded<RTS_ERR_INTERNAL>([&] {
        if (!bytes) return RTS_ERR_BAD_ARG;
        Layout l;
        if (int rc = layout(W, R, Hs, l)) return rc;
        *bytes = l.bytes;
        return RTS_OK;
    });
}

RT_PRIVATE_EXPORT int rts_select(const rts_select_args* a, void* stream) {
    return guarded<RTS_ERR_INTERNAL>([&] {
        if (!a || a->reserved != 0 || a->reserved2 != 0 || a->dilate > 1u) return RTS_ERR_BAD_ARG;
        Layout l;
        if (int rc = layout(a->W, a->R, a->Hs, l)) return rc;
        if (!(a->threshold >= 0.0f) || !std::isfinite(a->eps) || !(a->eps > 0.0f)) return RTS_ERR_BAD_ARG;
        if (!a->moments || !a->counts || !a->err || !a->active || !a->strip_counts || !a->scratch) return RTS_ERR_BAD_ARG;
        if (misaligned(a->moments, 8) || misaligned(a->counts) || misaligned(a->err) || misaligned(a->active) ||
            misaligned(a->strip_counts) || misaligned(a->scratch, 8))
            return RTS_ERR_BAD_ARG;
        if (a->scratch_bytes < l.bytes) return RTS_ERR_SCRATCH;

        rtsk::SelectParams p;
        std::memset(&p, 0, sizeof p);
        p.W = a->W;
        p.R = a->R;
        p.Hs = a->Hs;
        p.dilate = a->dilate;
        p.P = l.P;
        p.bps = l.bps;
        p.threshold = a->threshold;
        p.eps = a->eps;
        p.moments = a->moments;
        p.counts = a->counts;
        p.err = a->err;
        p.active = a->active;
        p.strip_counts = a->strip_counts;
        const uint64_t pixels = (uint64_t)a->W * a->R;
        p.noisy = static_cast<uint8_t*>(a->scratch);
        p.act = p.noisy + pixels;
        p.offsets = reinterpret_cast<uint32_t*>(p.noisy + l.offsets_at);
        const hipStream_t s = (hipStream_t)stream;
        const dim3 block(rtsk::BLOCK), per_strip(l.bps, l.strips);
        hipLaunchKernelGGL(rtsk::rts_metric_kernel, dim3((uint32_t)((pixels + rtsk::BLOCK - 1) / rtsk::BLOCK)), block, 0, s, p);
        if (int rc = after_launch(RTS_OK, RTS_ERR_HIP)) return rc;
        hipLaunchKernelGGL(rtsk::rts_count_kernel, per_strip, block, 0, s, p);
        if (int rc = after_launch(RTS_OK, RTS_ERR_HIP)) return rc;
        hipLaunchKernelGGL(rtsk::rts_scan_kernel, dim3(l.strips), block, 0, s, p);
        if (int rc = after_launch(RTS_OK, RTS_ERR_HIP)) return rc;
        hipLaunchKernelGGL(rtsk::rts_write_kernel, per_strip, block, 0, s, p);
        return after_launch(RTS_OK, RTS_ERR_HIP);
    });
}

RT_PRIVATE_EXPORT int rts_gather(const rts_gather_args* a, void* stream) {
    return guarded<RTS_ERR_INTERNAL>([&] {
        if (!a) return RTS_ERR_BAD_ARG;
        if (int rc = check_chunk(a->n_active, a->k, a->pixels, a->reserved, a->active)) return rc;
        if (!a->rays || !a->states || !a->out_rays || !a->out_states) return RTS_ERR_BAD_ARG;
        if (misaligned(a->rays, 16) || misaligned(a->states, 16) || misaligned(a->out_rays, 16) || misaligned(a->out_states, 16))
            return RTS_ERR_BAD_ARG;
        // never in place; an output that takes nothing is still a place (one byte of it)
        const uint64_t in_bytes = (uint64_t)a->pixels * a->k * RTS_RECORD_BYTES, taken = (uint64_t)a->n_active * a->k * RTS_RECORD_BYTES;
        const uint64_t out_bytes = taken ? taken : 1;
        const Range in[] = {range(a->rays, in_bytes), range(a->states, in_bytes)};
        const Range out[] = {range(a->out_rays, out_bytes), range(a->out_states, out_bytes)};
        if (any_overlap(in, out) || any_overlap(out)) return RTS_ERR_BAD_ARG;
        if (a->n_active == 0) return RTS_OK;
        rtsk::GatherParams p = {a->n_active, a->k, a->pixels, a->active, static_cast<const uint4*>(a->rays),
                                static_cast<const uint4*>(a->states), static_cast<uint4*>(a->out_rays), static_cast<uint4*>(a->out_states)};
        const uint64_t halves = 2ull * a->n_active * a->k;
        hipLaunchKernelGGL(rtsk::rts_gather_kernel, dim3((uint32_t)((halves + rtsk::BLOCK - 1) / rtsk::BLOCK)), dim3(rtsk::BLOCK), 0,
                           (hipStream_t)stream, p);
        return after_launch(RTS_OK, RTS_ERR_HIP);
    });
}

RT_PRIVATE_EXPORT int rts_fold(const rts_fold_args* a, void* stream) {
    return guarded<RTS_ERR_INTERNAL>([&] {
        if (!a) return RTS_ERR_BAD_ARG;
        if (int rc = check_chunk(a->n_active, a->k, a->pixels, a->reserved, a->active)) return rc;
        if (!a->rgb || !a->accum || !a->moments || !a->counts) return RTS_ERR_BAD_ARG;
        if (misaligned(a->rgb) || misaligned(a->accum) || misaligned(a->moments, 8) || misaligned(a->counts)) return RTS_ERR_BAD_ARG;
        if (a->n_active == 0) return RTS_OK;
        rtsk::FoldParams p = {a->n_active, a->k, a->pixels, a->active, a->rgb, a->accum, a->moments, a->counts};
        hipLaunchKernelGGL(rtsk::rts_fold_kernel, dim3((a->n_active + rtsk::BLOCK - 1u) / rtsk::BLOCK), dim3(rtsk::BLOCK), 0,
                           (hipStream_t)stream, p);
        return after_launch(RTS_OK, RTS_ERR_HIP);
    });
}

RT_PRIVATE_EXPORT int rts_normalise(const rts_normalise_args* a, void* stream) {
    return guarded<RTS_ERR_INTERNAL>([&] {
        if (!a || a->reserved != 0) return RTS_ERR_BAD_ARG;
        if (int rc = check_image(a->W, a->R)) return rc;
        if (a->e0 < 2u) return RTS_ERR_BAD_ARG;
        if (a->e0 > (1u << 24)) return RTS_ERR_LIMIT;                             // (float)e0 and e0 - 1 exact
        if (!a->accum || !a->moments || !a->counts || !a->out_accum || !a->out_moments) return RTS_ERR_BAD_ARG;
        if (misaligned(a->accum) || misaligned(a->moments, 8) || misaligned(a->counts) || misaligned(a->out_accum) ||
            misaligned(a->out_moments, 8))
            return RTS_ERR_BAD_ARG;
        if (a->out_accum == a->accum || a->out_moments == a->moments) return RTS_ERR_BAD_ARG;
        const uint64_t pixels = (uint64_t)a->W * a->R;
        rtsk::NormaliseParams p = {pixels, (int32_t)a->e0, (float)a->e0, a->accum, a->moments, a->counts, a->out_accum, a->out_moments};
        hipLaunchKernelGGL(rtsk::rts_normalise_kernel, dim3((uint32_t)((pixels + rtsk::BLOCK - 1) / rtsk::BLOCK)), dim3(rtsk::BLOCK), 0,
                           (hipStream_t)stream, p);
        return after_launch(RTS_OK, RTS_ERR_HIP);
    });
}
