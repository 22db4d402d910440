// rt_camera.hip.h — gfx950 camera rays of a strip (rt_scene_camera_rays*, rt_tile.h "placed camera").
//
// One lane per (pixel, sample) of the strip: the lane seeds the sample's stream, makes Camera::get_ray's draws and stores the ray the
// tile kernel would trace first for that sample — the lens point, and the direction as it is handed to ray_color — and, when asked,
// the xoshiro256++ state after the draws.  The camera ray is the shared step camera_ray of rt_path_steps.hip.h, as in rt_aov.hip.h.
//
// Records are numbered pixel-major, sample-minor: record (row W + x) n + (s - s_begin), n the samples of the call.  Neighbouring
// lanes hold neighbouring records, so a wave's 64 ray records are 2 KiB of consecutive bytes (as are its 64 states), stored as two
// 16-byte halves per lane.  Persistent waves stride over the records with 64-bit offsets.  No LDS, no scene data, no atomics.
#pragma once
#include "rt_path_steps.hip.h"

namespace rtk {

struct CParams : CameraRefs {
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
    const CameraBasis basis = camera_basis(p);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.total; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t pix, k;                                                       // the pixel of the strip and the sample in it
        split_index(i, p.n_smp, pix, k);
        const uint32_t row = pix / p.W, px = pix - row * p.W;
        const uint32_t pyg = p.y0 + row;
        // the sample's stream: seed + 4 PHI ((y W + x) S + s)
        Rng rng = seed_state(p.seed + (((uint64_t)pyg * p.W + px) * p.spp_all + p.s_begin + k) * (4ull * PHI));
        V3 o, d;
        camera_ray(p, basis, px, pyg, rng, o, d);                              // Camera::get_ray (camera.rs:109-129)
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
