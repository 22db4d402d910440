// rt_upsample.hip — the host side of librt_upsample.so (rt_upsample.h): argument checks, the two frames, the choice of
// the kernel instance by the call's planes, the launch.  No global state, no allocation; every function catches everything inside its
// body.
#include <cmath>
#include <cstring>
#include <utility>

#include "rt_upsample.h"
#include "rt_upsample.hip.h"
#include "rt_private_host.h"

using namespace rtpriv;

namespace {

bool finite_nonneg(float v) { return std::isfinite(v) && v >= 0.0f; }

// the planes a side has, as rtum::P_*
uint32_t planes_of(const rtu_planes& s) {
    return (s.albedo ? rtum::P_ALBEDO : 0u) | (s.normal ? rtum::P_NORMAL : 0u) | (s.depth ? rtum::P_DEPTH : 0u) |
           (s.hits ? rtum::P_HITS : 0u) | (s.index ? rtum::P_INDEX : 0u);
}

using Kernel = void (*)(const rtuk::Params);

// the instance for a plane set: a table over every set, the ones a call cannot have left empty
template <uint32_t P>
constexpr Kernel instance() {
    if constexpr (rtum::planes_ok(P))
        return rtuk::rtu_upsample_kernel<P>;
    else
        return nullptr;
}
template <uint32_t... P>
Kernel pick(uint32_t planes, std::integer_sequence<uint32_t, P...>) {
    static const Kernel table[] = {instance<P>()...};
    return table[planes];
}

}  // namespace

RT_PRIVATE_EXPORT int rtu_version(uint32_t* version) {
    return guarded<RTU_ERR_INTERNAL>([&] {
        if (!version) return RTU_ERR_BAD_ARG;
        *version = RTU_VERSION;
        return RTU_OK;
    });
}

RT_PRIVATE_EXPORT int rtu_upsample(const rtu_upsample_args* a, void* stream) {
    return guarded<RTU_ERR_INTERNAL>([&] {
        if (!a || a->reserved != 0 || a->lo.reserved != 0 || a->hi.reserved != 0 || a->form != 0) return RTU_ERR_BAD_ARG;
        if (a->Wl == 0 || a->Rl == 0 || a->Hl == 0 || a->Wh == 0 || a->Rh == 0 || a->Hh == 0) return RTU_ERR_BAD_ARG;
        if (a->scale < RTU_MIN_SCALE || a->scale > RTU_MAX_SCALE) return RTU_ERR_BAD_ARG;
        const uint32_t lim = 1u << 24;                            // (float) of every size, row and tap exact
        if (a->Wl >= lim || a->Hl >= lim || a->Wh >= lim || a->Hh >= lim) return RTU_ERR_LIMIT;
        if ((uint64_t)a->Wl * a->scale != a->Wh || (uint64_t)a->Hl * a->scale != a->Hh) return RTU_ERR_BAD_ARG;
        if ((uint64_t)a->y0l + a->Rl > a->Hl || (uint64_t)a->y0h + a->Rh > a->Hh) return RTU_ERR_BAD_ARG;
        const uint64_t nh = (uint64_t)a->Wh * a->Rh, nl = (uint64_t)a->Wl * a->Rl;
        if (nh > 0x7fffffffull) return RTU_ERR_LIMIT;
        if (!a->linear || (!a->out_linear && !a->out_f32 && !a->out_rgb && !a->out_class)) return RTU_ERR_BAD_ARG;
        const uint32_t planes = planes_of(a->lo);
        if (planes != planes_of(a->hi) || !rtum::planes_ok(planes)) return RTU_ERR_BAD_ARG;
        if ((planes & rtum::P_DEPTH) && !finite_nonneg(a->k_depth)) return RTU_ERR_BAD_ARG;
        if ((planes & rtum::P_NORMAL) && !finite_nonneg(a->k_normal)) return RTU_ERR_BAD_ARG;
        if (planes & rtum::P_ALBEDO) {
            if (!(a->eps > 0.0f) || !std::isfinite(a->eps) || a->lo.samples == 0 || a->hi.samples == 0) return RTU_ERR_BAD_ARG;
        }
        const void* dwords[] = {a->linear,   a->lo.albedo, a->lo.normal, a->lo.depth, a->lo.hits, a->lo.index, a->hi.albedo,
                                a->hi.normal, a->hi.depth,  a->hi.hits,   a->hi.index, a->out_linear, a->out_f32};
        for (const void* q : dwords)
            if (misaligned(q)) return RTU_ERR_BAD_ARG;
        // an output overlaps neither an input nor another output
        const Range in[] = {range(a->linear, nl * 12),      range(a->lo.albedo, nl * 12), range(a->lo.normal, nl * 12),
                            range(a->lo.depth, nl * 4),     range(a->lo.hits, nl * 4),    range(a->lo.index, nl * 4),
                            range(a->hi.albedo, nh * 12),   range(a->hi.normal, nh * 12), range(a->hi.depth, nh * 4),
                            range(a->hi.hits, nh * 4),      range(a->hi.index, nh * 4)};
        const Range out[] = {range(a->out_linear, nh * 12), range(a->out_f32, nh * 12), range(a->out_rgb, nh * 3),
                             range(a->out_class, nh)};
        if (any_overlap(out, in) || any_overlap(out)) return RTU_ERR_BAD_ARG;

        rtuk::Params p;
        std::memset(&p, 0, sizeof p);
        rtum::Frame& f = p.f;
        f.Wl = a->Wl, f.Rl = a->Rl, f.Hl = a->Hl, f.y0l = a->y0l;
        f.Wh = a->Wh, f.Rh = a->Rh, f.Hh = a->Hh, f.y0h = a->y0h;
        rtum::frame_dens(a->Wl, a->Hl, f.u_den_l, f.v_den_l);
        rtum::frame_dens(a->Wh, a->Hh, f.u_den_h, f.v_den_h);
        if (!(f.u_den_h >= 1.0f) || !(f.v_den_h >= 1.0f)) return RTU_ERR_BAD_ARG;       // (Wh, Hh >= 2: never)
        f.kd = a->k_depth;
        f.kn2 = a->k_normal * a->k_normal;
        f.eps = a->eps;
        f.kl_f = (float)a->lo.samples;
        f.kh_f = (float)a->hi.samples;
        p.linear = a->linear;
        p.lo = {a->lo.albedo, a->lo.normal, a->lo.depth, a->lo.hits, a->lo.index};
        p.hi = {a->hi.albedo, a->hi.normal, a->hi.depth, a->hi.hits, a->hi.index};
        p.out_linear = a->out_linear;
        p.out_f32 = a->out_f32;
        p.out_rgb = a->out_rgb;
        p.out_class = a->out_class;
        const dim3 grid((a->Wh + rtuk::TILE_X - 1) / rtuk::TILE_X, (a->Rh + rtuk::TILE_Y - 1) / rtuk::TILE_Y);
        if (grid.y > 65535u) return RTU_ERR_LIMIT;
        const Kernel k = pick(planes, std::make_integer_sequence<uint32_t, rtum::P_ALL + 1u>{});
        if (!k) return RTU_ERR_INTERNAL;
        hipLaunchKernelGGL(k, grid, dim3(rtuk::BLOCK), 0, (hipStream_t)stream, p);
        return after_launch(RTU_OK, RTU_ERR_HIP);
    });
}
