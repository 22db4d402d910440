// Test harness (CPU only, built by tests/test_launch_plan.py with g++ -ffp-contract=off): the launch plan of csrc/rt_plan.h — the
// product's plan_launch / plan_queue — on hand-built scene shapes, requests and knobs.  The planner writes the kernel parameters
// into any struct with rtk::KParams's scalar field names; Params below is that struct, and every value goes back to Python as
// a double (exact for the u32 and f32 fields), named by plan_field_names().
#include <cstdint>
#include <cstring>
#include <string>

#include "rt_plan.h"

namespace {

#define U32_FIELDS(X)                                                                                                              \
    X(W) X(H) X(Hs) X(upp) X(depth) X(spp_all) X(s_begin) X(gap) X(acc_out) X(n_sph) X(n_sph_pad) X(n_tri) X(chunk) X(n_chunks)     \
    X(flags) X(path32) X(lds_cand_off) X(lds_path_off) X(lds_rr_off) X(lds_stack_off) X(lds_cmp_off) X(lds_stage_off) X(n_strips)  \
    X(tiles_x) X(tiles_per_strip) X(tiles_total) X(tiles_big) X(sub_shift) X(n_tiles) X(n_slots) X(grp) X(grp_magic)               \
    X(slot_stride) X(commit_slots) X(spp_magic) X(slotu_magic) X(root_ref) X(maxl) X(list16) X(stack_lds) X(ovf_stride)            \
    X(refill_eighths) X(n_internal) X(lds_node_off)
#define F32_FIELDS(X) X(lens_radius) X(focus_distance) X(u_den) X(v_den) X(t_min) X(t_max) X(spp_f) X(spp_rcp)
#define PLAN_FIELDS(X) X(status) X(engine) X(capped) X(isect) X(block) X(expanded) X(count_steps) X(lds) X(maxl_l2) X(ovf_entries) \
    X(blocks) X(ring_bytes) X(ovf_words)

struct Params {
#define DECL_U32(f) uint32_t f;
#define DECL_F32(f) float f;
    U32_FIELDS(DECL_U32)
    F32_FIELDS(DECL_F32)
    float org[3], llc[3], hor[3], ver[3];
};

std::string names() {
    std::string s;
#define NAME(f) s += #f ",";
    PLAN_FIELDS(NAME)
    U32_FIELDS(NAME)
    F32_FIELDS(NAME)
    for (const char* v : {"org", "llc", "hor", "ver"})
        for (int i = 0; i < 3; i++) s += std::string(v) + std::to_string(i) + ",";
    s.pop_back();
    return s;
}

}  // namespace

extern "C" {

const char* plan_field_names() {
    static const std::string s = names();
    return s.c_str();
}

// shape: the SceneShape fields in declaration order.  rq: width, height, divisions, spp, max_bounces, flags, aperture,
// focus_distance, fov, focal_length, t_min, t_max.  knobs: the Knobs fields in declaration order.  grid: the workgroups the chip
// holds (n_cu x per_cu); 0 skips plan_queue.  out: the values plan_field_names() names.
void plan(const double* shape, const double* rqv, uint32_t n_strips, uint32_t s_begin, uint32_t s_end, int pass, const int32_t* knobs,
          uint32_t grid, double* out) {
    rtplan::SceneShape sh;
    sh.n_sph = (uint32_t)shape[0];
    sh.n_sph_pad = (uint32_t)shape[1];
    sh.n_tri = (uint32_t)shape[2];
    sh.bvh_depth = (uint32_t)shape[3];
    sh.n_internal = (uint32_t)shape[4];
    sh.root_ref = (uint32_t)shape[5];
    sh.cull_density = (float)shape[6];
    sh.cull_pays = shape[7] != 0;
    sh.xcull_pays = shape[8] != 0;
    sh.quant_ok = shape[9] != 0;
    sh.tri_ok = shape[10] != 0;
    sh.r_slack = (float)shape[11];
    sh.inverted_boxes = shape[12] != 0;
    sh.expanded = shape[13] != 0;
    sh.leaf_density = (float)shape[14];
    rt_tile_request rq;
    std::memset(&rq, 0, sizeof rq);
    rq.width = (uint32_t)rqv[0];
    rq.height = (uint32_t)rqv[1];
    rq.divisions = (uint32_t)rqv[2];
    rq.spp = (uint32_t)rqv[3];
    rq.max_bounces = (uint32_t)rqv[4];
    rq.flags = (uint32_t)rqv[5];
    rq.aperture = (float)rqv[6];
    rq.focus_distance = (float)rqv[7];
    rq.fov = (float)rqv[8];
    rq.focal_length = (float)rqv[9];
    rq.t_min = (float)rqv[10];
    rq.t_max = (float)rqv[11];
    rtplan::Knobs kn;
    kn.lds_tree = knobs[0];
    kn.cull_walk = knobs[1];
    kn.no_stage = knobs[2];
    kn.slots = knobs[3];
    kn.commit_slots = knobs[4];
    kn.force_capped = knobs[5];
    kn.stack_lds = knobs[6];
    kn.compact = knobs[7];
    kn.refill_eighths = knobs[8];
    kn.tail_tiles = knobs[9];
    Params p;
    std::memset(&p, 0, sizeof p);
    rtplan::Plan pl = rtplan::plan_launch(sh, rq, n_strips, rtplan::SampleRange{s_begin, s_end, pass != 0}, kn, p);
    if (pl.status == RT_OK && grid) rtplan::plan_queue(pl, grid, kn, p);
    int k = 0;
#define OUT_PLAN(f) out[k++] = (double)pl.f;
#define OUT_P(f) out[k++] = (double)p.f;
    PLAN_FIELDS(OUT_PLAN)
    U32_FIELDS(OUT_P)
    F32_FIELDS(OUT_P)
    for (const float* v : {p.org, p.llc, p.hor, p.ver})
        for (int i = 0; i < 3; i++) out[k++] = v[i];
}

// The engine table: ISECT, capped-stack ISECT (-1: none) and workgroup size of engine e.
void plan_engine(int e, int32_t* out) {
    out[0] = rtplan::ENGINES[e].isect;
    out[1] = rtplan::ENGINES[e].isect_capped;
    out[2] = rtplan::ENGINES[e].block;
}

// The constants the rules are written in, by name (NaN: unknown).
double plan_const(const char* name) {
    const std::string n = name;
#define CONST(c) if (n == #c) return (double)c;
    using namespace rtplan;
    using namespace rtk;
    CONST(LDS_LIMIT) CONST(RESIDENT_MAX) CONST(STREAM_CHUNK) CONST(STACK_LDS_MAX) CONST(RT_QNODES_MIN_PRIMS)
    CONST(DENSE_SCAN_MAX_PRIMS) CONST(DENSE_SCAN_MIN_DENSITY) CONST(DENSE_MID_MIN_DENSITY) CONST(DENSE_MID_MIN_PRIMS)
    CONST(FIELD_MID_MIN_DENSITY) CONST(LT_CULL_MIN_DENSITY) CONST(TRAVERSE_MIN_PRIMS) CONST(N_ISECT)
    CONST(BLOCK) CONST(LTREE_BLOCK) CONST(TRAV_STACK) CONST(MAXL) CONST(MINL) CONST(MAXL_EXACT) CONST(MAXL_LTREE)
    CONST(MAXL_LTREE_MAX) CONST(LNODE_DW) CONST(SLOTS_MAX) CONST(STAGE_TILES) CONST(STAGE_TILE_BYTES) CONST(MAXC)
    return __builtin_nan("");
}

}  // extern "C"
