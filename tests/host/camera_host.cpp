// Test harness (CPU only, built by tests/test_camera_plan.py with g++ -ffp-contract=off): the placed camera of csrc/rt_plan.h — the
// product's make_pose and fill_camera — on hand-built poses and requests.  Params has the camera fields of rtk::KParams, lens vectors
// included; the values go back to Python as float32 bits.
#include <cstdint>
#include <cstring>

#include "rt_plan.h"

namespace {
struct Params {
    float org[3], llc[3], hor[3], ver[3];
    float lens_radius, focus_distance;
    float lens_u[3], lens_v[3];
    float u_den, v_den;
};
}  // namespace

extern "C" {

// rqv: width, height, aperture, focus_distance, fov, focal_length (the camera's knobs).  cam: an rt_camera (44 bytes), or NULL for the
// reference camera.  out: org, llc, hor, ver, lens_u, lens_v (3 each), lens_radius, focus_distance, u_den, v_den: 22 floats.
// Returns 0, or -1 where make_pose refuses the pose (out untouched).
int camera_vectors(const uint32_t* size, const float* knobs, const void* cam, float* out) {
    rt_tile_request rq;
    std::memset(&rq, 0, sizeof rq);
    rq.width = size[0];
    rq.height = size[1];
    rq.aperture = knobs[0];
    rq.focus_distance = knobs[1];
    rq.fov = knobs[2];
    rq.focal_length = knobs[3];
    Params p;
    std::memset(&p, 0, sizeof p);
    rtplan::Pose ps;
    if (cam) {
        rt_camera c;
        std::memcpy(&c, cam, sizeof c);
        if (!rtplan::make_pose(c, ps)) return -1;
    }
    rtplan::fill_camera(rq, cam ? &ps : nullptr, p);
    int k = 0;
    for (const float* v : {p.org, p.llc, p.hor, p.ver, p.lens_u, p.lens_v})
        for (int i = 0; i < 3; i++) out[k++] = v[i];
    out[k++] = p.lens_radius;
    out[k++] = p.focus_distance;
    out[k++] = p.u_den;
    out[k++] = p.v_den;
    return 0;
}

// u, v, w of a pose (9 floats); -1 where it is refused.
int camera_basis(const void* cam, float* out) {
    rt_camera c;
    std::memcpy(&c, cam, sizeof c);
    rtplan::Pose ps;
    if (!rtplan::make_pose(c, ps)) return -1;
    for (int i = 0; i < 3; i++) {
        out[i] = ps.u[i];
        out[3 + i] = ps.v[i];
        out[6 + i] = ps.w[i];
    }
    return 0;
}

uint32_t camera_sizeof(void) { return (uint32_t)sizeof(rt_camera); }

}  // extern "C"
