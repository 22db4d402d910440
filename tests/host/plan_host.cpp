// Test harness (CPU only, built by tests/test_launch_plan.py with g++ -ffp-contract=off): the launch plan of csrc/rt_plan.h — the
// product's plan_launch / plan_queue — on hand-built scene shapes, requests and knobs.  The planner writes the kernel parameters
// into any struct with rtk::KParams's scalar field names; Params below is that struct, and every value goes back to Python as
// a double (exact for the u32 and f32 fields), named by plan_field_names().  Also the staging layout of the host forms (stage_layout,
// dn_stage_list), and with -DPLAN_HOST_MAIN a program that runs those (for the sanitizers).
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

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
    CONST(DN_ALIGN)
    return __builtin_nan("");
}

// The staging layout (rtplan::stage_layout) of n entries of bytes[k]; host[k] != 0: the entry has a host side, device_only[k] != 0: it
// is STAGE_DEVICE.  off[k], present[k]: what the layout says of entry k; returns the total.
uint64_t stage_layout(const uint64_t* bytes, const uint8_t* host, const uint8_t* device_only, uint32_t n, uint64_t* off, uint8_t* present) {
    static const char side = 0;
    std::vector<rtplan::StageEntry> e(n);
    for (uint32_t k = 0; k < n; k++)
        e[k] = {host[k] ? &side : nullptr, (size_t)bytes[k], device_only[k] ? rtplan::STAGE_DEVICE : rtplan::STAGE_UP, ~(size_t)0};
    const size_t total = rtplan::stage_layout(e.data(), n);
    for (uint32_t k = 0; k < n; k++) {
        off[k] = e[k].off;
        present[k] = e[k].present();
    }
    return total;
}

// The denoiser's list (rtplan::dn_stage_list) for n strips of a width x height frame in `divisions`, laid out.  planes: bit k set: the
// strips have guide plane k (albedo, normal, depth, hits); outs: bit k set: output k is asked for (rgb, f32, linear).  bytes, off,
// present: 1 + DN_STAGE_STRIP * n values each; returns the total.
uint64_t stage_denoise(uint32_t width, uint32_t height, uint32_t divisions, uint32_t n, uint32_t planes, uint32_t outs, uint64_t* bytes,
                       uint64_t* off, uint8_t* present) {
    static float side = 0.f;
    rt_tile_request rq;
    std::memset(&rq, 0, sizeof rq);
    rq.width = width;
    rq.height = height;
    rq.divisions = divisions;
    const rt_aov_planes pl = {planes & 1 ? &side : nullptr, planes & 2 ? &side : nullptr, planes & 4 ? &side : nullptr,
                              planes & 8 ? (uint32_t*)&side : nullptr, nullptr};
    const std::vector<const float*> acc(n, &side);
    const std::vector<rt_aov_planes> pls(n, pl);
    const std::vector<uint8_t*> rgb(n, (uint8_t*)&side);
    const std::vector<float*> f32(n, &side);
    std::vector<rtplan::StageEntry> e = rtplan::dn_stage_list(rq, n, acc.data(), pls.data(), outs & 1 ? rgb.data() : nullptr,
                                                              outs & 2 ? f32.data() : nullptr, outs & 4 ? f32.data() : nullptr);
    const size_t total = rtplan::stage_layout(e.data(), e.size());
    for (size_t k = 0; k < e.size(); k++) {
        bytes[k] = e[k].bytes;
        off[k] = e[k].off;
        present[k] = e[k].present();
    }
    return total;
}

int stage_per_strip() { return rtplan::DN_STAGE_STRIP; }
double stage_scratch_bytes(uint32_t width, uint32_t rows) { return (double)rtplan::plan_denoise(width, rows, 0, false).scratch_bytes; }

}  // extern "C"

#ifdef PLAN_HOST_MAIN
// The same exports as a program (built with the sanitizers by tests/test_launch_plan.py): seeded lists through stage_layout, the
// denoiser's lists of 1, 3 and 66 strips with every set of planes and outputs; every present entry aligned, in order, inside the total.
#include <cstdio>
namespace {
bool laid_out(const std::vector<uint64_t>& bytes, const std::vector<uint64_t>& off, const std::vector<uint8_t>& present, uint64_t total) {
    uint64_t top = 0;
    for (size_t k = 0; k < bytes.size(); k++) {
        if (!present[k]) continue;
        if (off[k] % rtplan::DN_ALIGN || off[k] < top) return false;
        top = off[k] + bytes[k];
    }
    return top <= total;
}
}  // namespace
int main() {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&] { return (x = x * 6364136223846793005ull + 1442695040888963407ull) >> 33; };
    for (int round = 0; round < 2000; round++) {
        const uint32_t n = (uint32_t)(rnd() % 40);
        std::vector<uint64_t> bytes(n), off(n);
        std::vector<uint8_t> host(n), dev(n), present(n);
        for (uint32_t k = 0; k < n; k++) {
            bytes[k] = rnd() % 3 ? rnd() % 5000 : 0;
            host[k] = rnd() % 3 != 0;
            dev[k] = rnd() % 4 == 0;
        }
        const uint64_t total = stage_layout(bytes.data(), host.data(), dev.data(), n, off.data(), present.data());
        for (uint32_t k = 0; k < n; k++)
            if (present[k] != (host[k] || dev[k])) return std::puts("stage_layout: present"), 1;
        if (!laid_out(bytes, off, present, total)) return std::puts("stage_layout: layout"), 1;
    }
    for (uint32_t n : {1u, 3u, 66u})
        for (uint32_t planes = 0; planes < 16; planes++)
            for (uint32_t outs = 1; outs < 8; outs++) {
                const size_t m = 1 + (size_t)stage_per_strip() * n;
                std::vector<uint64_t> bytes(m), off(m);
                std::vector<uint8_t> present(m);
                const uint64_t total = stage_denoise(40, 132, 66, n, planes, outs, bytes.data(), off.data(), present.data());
                if (!present[0] || off[0] != 0 || !laid_out(bytes, off, present, total)) return std::puts("stage_denoise: layout"), 1;
            }
    std::puts("staging ok");
    return 0;
}
#endif
