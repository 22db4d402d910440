// Test harness (CPU only, built by tests/test_launch_plan_variants.py with g++ -ffp-contract=off): the two choices of csrc/rt_plan.h
// that pick a variant of the LDS-tree kernels — Plan::tris (the sphere-only instantiation) and plain_frame (the commit without the
// launch-uniform tests) — on hand-built scene shapes, requests and knobs.  tests/host/plan_host.cpp's Params, cut down to what these
// two read.
#include <cstdint>
#include <cstring>

#include "rt_plan.h"

namespace {
struct Params {
    uint32_t W, H, Hs, upp, depth, spp_all, s_begin, gap, acc_out, n_sph, n_sph_pad, n_tri, chunk, n_chunks, flags, path32, lds_cand_off,
        lds_path_off, lds_rr_off, lds_stack_off, lds_cmp_off, lds_stage_off, n_strips, tiles_x, tiles_per_strip, tiles_total, tiles_big,
        sub_shift, n_tiles, n_slots, grp, grp_magic, slot_stride, commit_slots, spp_magic, slotu_magic, root_ref, maxl, list16, stack_lds,
        ovf_stride, refill_eighths, n_internal, lds_node_off;
    float lens_radius, focus_distance, u_den, v_den, t_min, t_max, spp_f, spp_rcp;
    float org[3], llc[3], hor[3], ver[3];
};
}  // namespace

extern "C" {

// n_sph spheres and n_tri triangles in a balanced tree of the given depth; a width x height frame in one strip at spp samples per
// pixel, samples [s_begin, s_end) of them (pass != 0: a progressive pass).  out: engine, tris, plain_shape, and plain_frame for
// (no f32 plane, no strip cost), (an f32 plane), (a strip cost).
void plan_variants(uint32_t n_sph, uint32_t n_tri, uint32_t bvh_depth, uint32_t flags, uint32_t width, uint32_t height, uint32_t spp,
                   uint32_t s_begin, uint32_t s_end, int pass, int ltree_general, int plain_knob, int lds_tree, int32_t* out) {
    rtplan::SceneShape sh;
    sh.n_sph = n_sph;
    sh.n_sph_pad = (n_sph + 7u) / 8u * 8u;
    sh.n_tri = n_tri;
    sh.bvh_depth = bvh_depth;
    sh.n_internal = n_sph + n_tri ? n_sph + n_tri - 1u : 0u;
    sh.root_ref = n_sph + n_tri > 1u ? 0u : rtk::LEAF_BIT;
    sh.cull_density = 1.0f;
    sh.quant_ok = true;
    sh.tri_ok = n_tri != 0;
    sh.r_slack = 0.5f;
    sh.expanded = true;
    sh.leaf_density = 1.0f;
    rt_tile_request rq;
    std::memset(&rq, 0, sizeof rq);
    rq.width = width;
    rq.height = height;
    rq.divisions = 1;
    rq.spp = spp;
    rq.max_bounces = 8;
    rq.flags = flags;
    rq.aperture = 0.1f;
    rq.focus_distance = 1.0f;
    rq.fov = 1.5707964f;
    rq.focal_length = 1.0f;
    rq.t_min = 0.001f;
    rq.t_max = 1000.0f;
    rtplan::Knobs kn;
    kn.ltree_general = ltree_general;
    kn.plain_frame = plain_knob;
    kn.lds_tree = lds_tree;
    Params p;
    std::memset(&p, 0, sizeof p);
    const rtplan::Plan pl = rtplan::plan_launch(sh, rq, 1, rtplan::SampleRange{s_begin, s_end, pass != 0}, kn, p);
    out[0] = pl.status == RT_OK ? pl.engine : -1;
    out[1] = pl.tris;
    out[2] = pl.plain_shape;
    out[3] = rtplan::plain_frame(pl, false, false);
    out[4] = rtplan::plain_frame(pl, true, false);
    out[5] = rtplan::plain_frame(pl, false, true);
}

uint32_t sphere_only_max_tris() { return rtplan::LT_SPHERE_ONLY_MAX_TRIS; }

}  // extern "C"
