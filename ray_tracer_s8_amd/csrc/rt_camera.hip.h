// rt_camera.hip.h — gfx950 camera rays of a strip (rt_scene_camera_rays*, rt_tile.h "placed camera").
//
// One lane per (pixel, sample) of the strip: the lane seeds the sample's stream, makes Camera::get_ray's draws and stores the ray the
// tile kernel would trace first for that sample — the lens point, and the direction as it is handed to ray_color — and, when asked,
// the xoshiro256++ state after the draws.  The camera ray restates the tile kernel's camera arm (rt_kernel.hip.h, the !bounce
// branch) with the same operations in the same order, as rt_aov.hip.h does.
//
// Records are numbered pixel-major, sample-minor: record (row W + x) n + (s - s_begin), n the samples of the call.  Neighbouring
// lanes hold neighbouring records, so a wave's 64 ray records are 2 KiB of consecutive bytes (as are its 64 states), stored as two
// 16-byte halves per lane.  Persistent waves stride over the records with 64-bit offsets.  No LDS, no scene data, no atomics.
#pragma once
#include "rt_kernel.hip.h"

namespace rtk {

struct CParams {
    float org[3], llc[3], hor[3], ver[3];   // Camera::new (camera.rs:19-47), host-computed by rtplan::fill_camera
    float lens_radius, focus_distance;
    float lens_u[3], lens_v[3];  // the lens disc's axes (as KParams)
    float u_den, v_den;          // aspect*H_f - 1, H_f - 1 (camera.rs:115-117)
    float t_min, t_max;
    uint32_t W, H;               // image size
    uint32_t y0;                 // first global row of the strip = Hs * division_no
    uint32_t spp_all;            // S: samples of the job (the stream stride)
    uint32_t s_begin, n_smp;     // the samples of this launch: [s_begin, s_begin + n_smp)
    uint64_t total;              // records: Hs * W * n_smp
    uint64_t seed;
    float4* rays;                // [2 total]: rt_ray (o, t_min) (d, t_max)
    ulonglong2* state;           // [2 total]: (s0, s1) (s2, s3), or nullptr
};

// STATES: the RNG states are stored as well (p.state is not NULL)
template <bool STATES>
__global__ __launch_bounds__(256) void rt_camera_rays_kernel(const CParams p) {
    const V3 corg = mk(p.org[0], p.org[1], p.org[2]);
    const V3 llc = mk(p.llc[0], p.llc[1], p.llc[2]);
    const V3 hor = mk(p.hor[0], p.hor[1], p.hor[2]);
    const V3 ver = mk(p.ver[0], p.ver[1], p.ver[2]);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.total; i += (uint64_t)gridDim.x * blockDim.x) {
        // the pixel of the strip and the sample in it: a 32-bit division while the record number fits
        uint32_t pix, k;
        if (i <= 0xffffffffull) {
            pix = (uint32_t)i / p.n_smp;
            k = (uint32_t)i - pix * p.n_smp;
        } else {
            pix = (uint32_t)(i / p.n_smp);
            k = (uint32_t)(i - (uint64_t)pix * p.n_smp);
        }
        const uint32_t row = pix / p.W, px = pix - row * p.W;
        const uint32_t pyg = p.y0 + row;
        // the sample's stream: seed + 4 PHI ((y W + x) S + s)
        Rng rng = seed_state(p.seed + (((uint64_t)pyg * p.W + px) * p.spp_all + p.s_begin + k) * (4ull * PHI));
        // ---- Camera::get_ray (camera.rs:109-129), as the tile kernel's camera arm
        float x1, x2, sm;
        for (;;) {
            x1 = uniform_m1_1(rng);
            x2 = uniform_m1_1(rng);
            sm = x1 * x1 + x2 * x2;
            if (sm <= 1.0f) break;                                             // UnitDisc
        }
        const V3 offset = lens_offset(p, x1, x2);
        const float u = ((float)px + gen_range_01(rng)) / p.u_den;
        const float v = ((float)(p.H - pyg - 1) + gen_range_01(rng)) / p.v_den;       // camera row, main.rs:71
        const V3 dir0 = normalize_or_zero(llc + u * hor + v * ver - corg);
        const V3 d1 = normalize(dir0);                                         // Ray::new re-normalises (ray.rs:134)
        const V3 focal_point = corg + p.focus_distance * d1;
        const V3 o = corg + offset;
        const V3 pre = focal_point - o;
        V3 xdir;
        if (!try_normalize(pre, xdir)) xdir = mk(0.f, 0.f, 0.f);                // normalize_or_zero
        const V3 d = normalize(xdir);                                          // Ray::new (ray.rs:134)
        p.rays[2 * i + 0] = make_float4(o.x, o.y, o.z, p.t_min);
        p.rays[2 * i + 1] = make_float4(d.x, d.y, d.z, p.t_max);
        if (STATES) {
            p.state[2 * i + 0] = make_ulonglong2(rng.s0, rng.s1);
            p.state[2 * i + 1] = make_ulonglong2(rng.s2, rng.s3);
        }
    }
}

using CameraFn = void (*)(const CParams);
CameraFn camera_rays_kernel(bool states);      // rt_kernels_camera.hip

}  // namespace rtk
