// rt_history.hip — the host side of librt_history.so (rt_history.h): argument checks, the two cameras, the launch.
// No global state, no allocation; every function catches everything inside its body.
#include <cmath>
#include <cstring>

#include "rt_history.h"
#include "rt_history.hip.h"
#include "rt_private_host.h"
#include "rt_plan.h"

using namespace rtpriv;

namespace {

bool finite_nonneg(float v) { return std::isfinite(v) && v >= 0.0f; }

bool request_ok(const rt_tile_request* rq, uint32_t W, uint32_t R) {
    if (!rq || rq->width != W || rq->height == 0 || rq->divisions == 0 || rq->division_no >= rq->divisions) return false;
    const uint32_t Hs = rq->height / rq->divisions;
    if (Hs == 0 || R % Hs != 0) return false;
    return (uint64_t)rq->division_no * Hs + R <= rq->height;
}

bool planes_ok(const rth_state& s, bool normals) {
    return s.accum && s.moments && s.length && s.depth && s.index && (!normals || s.normal) && !misaligned(s.moments, 8);
}

// whether q is one of the call's planes: an input, or a plane of next or (in a call that reads it) of prev
bool is_a_plane(const rth_accumulate_args& a, const void* q) {
    const void* in[] = {a.accum, a.moments, a.depth, a.hits, a.index, a.normal};
    for (const void* v : in)
        if (v == q) return true;
    const rth_state* states[2] = {&a.next, &a.prev};
    for (int k = 0; k < (a.have_prev ? 2 : 1); k++) {
        const rth_state& s = *states[k];
        const void* planes[] = {s.accum, s.moments, s.length, s.depth, s.index, s.normal};
        for (const void* v : planes)
            if (v == q) return true;
    }
    return false;
}

}  // namespace

RT_PRIVATE_EXPORT int rth_version(uint32_t* version) {
    return guarded<RTH_ERR_INTERNAL>([&] {
        if (!version) return RTH_ERR_BAD_ARG;
        *version = RTH_VERSION;
        return RTH_OK;
    });
}

RT_PRIVATE_EXPORT int rth_accumulate(const rth_accumulate_args* a, void* stream) {
    return guarded<RTH_ERR_INTERNAL>([&] {
        if (!a || a->W == 0 || a->R == 0 || a->reserved != 0) return RTH_ERR_BAD_ARG;
        if (a->W >= (1u << 24) || a->R >= (1u << 24)) return RTH_ERR_LIMIT;                   // (float)W, (float)R and the taps exact
        if (!request_ok(a->request, a->W, a->R)) return RTH_ERR_BAD_ARG;
        if (a->request->height >= (1u << 24)) return RTH_ERR_LIMIT;
        if (!(a->alpha > 0.0f && a->alpha <= 1.0f) || !(a->n_max >= 1.0f) || !std::isfinite(a->n_max)) return RTH_ERR_BAD_ARG;
        if (!finite_nonneg(a->k_depth) || !finite_nonneg(a->k_normal)) return RTH_ERR_BAD_ARG;
        if (!a->accum || !a->moments || !a->depth || !a->hits || !a->index || misaligned(a->moments, 8)) return RTH_ERR_BAD_ARG;
        const bool normals = a->normal != nullptr;
        if (!planes_ok(a->next, normals)) return RTH_ERR_BAD_ARG;
        const bool clip = a->clip_gamma != 0.0f;                  // (a NaN is not 0, and is refused below)
        if (clip) {
            if (!(a->clip_gamma > 0.0f) || !std::isfinite(a->clip_gamma)) return RTH_ERR_BAD_ARG;
            if ((a->clip_radius != 1u && a->clip_radius != 2u) || a->samples == 0 || a->clip_form > RTH_CLIP_FORM_DIRECT)
                return RTH_ERR_BAD_ARG;
            if (a->clip_amount && (misaligned(a->clip_amount) || is_a_plane(*a, a->clip_amount))) return RTH_ERR_BAD_ARG;
        }
        const rt_tile_request& rq = *a->request;

        rthk::Params p;
        std::memset(&p, 0, sizeof p);
        rthm::Frame& f = p.f;
        f.W = a->W;
        f.R = a->R;
        f.normals = normals ? 1u : 0u;
        f.alpha = a->alpha;
        f.n_max = a->n_max;
        f.kd = a->k_depth;
        f.kn2 = a->k_normal * a->k_normal;
        if (a->have_prev) {
            if (!planes_ok(a->prev, normals) || !request_ok(a->prev_request, a->W, a->R)) return RTH_ERR_BAD_ARG;
            if (a->prev.accum == a->next.accum || a->prev.moments == a->next.moments || a->prev.length == a->next.length ||
                a->prev.depth == a->next.depth || a->prev.index == a->next.index || (normals && a->prev.normal == a->next.normal))
                return RTH_ERR_BAD_ARG;                           // a frame never reads what it writes
            const rt_tile_request& pq = *a->prev_request;
            if (pq.height != rq.height || pq.divisions != rq.divisions || pq.division_no != rq.division_no) return RTH_ERR_BAD_ARG;
        }
        if (!rthm::set_cameras(f, rq, a->camera, a->have_prev ? a->prev_request : nullptr, a->prev_camera)) return RTH_ERR_BAD_ARG;
        p.accum = a->accum;
        p.moments = a->moments;
        p.depth = a->depth;
        p.hits = a->hits;
        p.index = a->index;
        p.normal = a->normal;
        const rth_state* src[2] = {&a->prev, &a->next};
        rthk::State* dst[2] = {&p.prev, &p.next};
        for (int k = f.have_prev ? 0 : 1; k < 2; k++) {
            dst[k]->accum = src[k]->accum;
            dst[k]->moments = src[k]->moments;
            dst[k]->length = src[k]->length;
            dst[k]->depth = src[k]->depth;
            dst[k]->index = src[k]->index;
            dst[k]->normal = src[k]->normal;
        }
        const dim3 grid((a->W + rthk::TILE_X - 1) / rthk::TILE_X, (a->R + rthk::TILE_Y - 1) / rthk::TILE_Y);
        if (grid.y > 65535u) return RTH_ERR_LIMIT;
        const dim3 block(rthk::BLOCK);
        const hipStream_t st = (hipStream_t)stream;
        if (!clip) {
            hipLaunchKernelGGL((rthk::rth_accumulate_kernel<0, false>), grid, block, 0, st, p);
        } else {
            p.clip.gamma = a->clip_gamma;
            p.clip.e = (float)a->samples;
            p.clip_amount = a->clip_amount;
            // the library's choice, as measured: direct at radius 1 (2 to 4 % ahead), staged at radius 2 (11 %)
            const uint32_t choice = a->clip_radius == 1u ? RTH_CLIP_FORM_DIRECT : RTH_CLIP_FORM_STAGED;
            const bool direct = (a->clip_form ? a->clip_form : choice) == RTH_CLIP_FORM_DIRECT;
            if (a->clip_radius == 1u && !direct)
                hipLaunchKernelGGL((rthk::rth_accumulate_kernel<1, false>), grid, block, 0, st, p);
            else if (a->clip_radius == 1u)
                hipLaunchKernelGGL((rthk::rth_accumulate_kernel<1, true>), grid, block, 0, st, p);
            else if (!direct)
                hipLaunchKernelGGL((rthk::rth_accumulate_kernel<2, false>), grid, block, 0, st, p);
            else
                hipLaunchKernelGGL((rthk::rth_accumulate_kernel<2, true>), grid, block, 0, st, p);
        }
        return after_launch(RTH_OK, RTH_ERR_HIP);
    });
}
