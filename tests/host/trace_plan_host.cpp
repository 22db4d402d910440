// Test harness (CPU only, built by tests/test_trace_plan.py with g++): the plan of path tracing of caller rays in csrc/rt_plan.h — the
// product's plan_trace — on hand-built scene shapes, request flags and bounce counts.
#include <cstdint>

#include "rt_plan.h"

extern "C" {

// shape: n_sph, n_tri, bvh_depth, inverted_boxes; out: engine, scan_mode, full_chain, block, path32, lds_path_off, lds bytes
void trace_plan(const uint32_t* shape, uint32_t flags, uint32_t max_bounces, uint64_t* out) {
    rtplan::SceneShape sh;
    sh.n_sph = shape[0];
    sh.n_tri = shape[1];
    sh.bvh_depth = shape[2];
    sh.inverted_boxes = shape[3] != 0;
    const rtplan::TracePlan t = rtplan::plan_trace(sh, flags, max_bounces);
    out[0] = (uint64_t)t.engine;
    out[1] = (uint64_t)t.scan_mode;
    out[2] = t.full_chain ? 1u : 0u;
    out[3] = (uint64_t)t.block;
    out[4] = t.path32 ? 1u : 0u;
    out[5] = (uint64_t)t.lds_path_off;
    out[6] = (uint64_t)t.lds;
}

uint32_t trace_trav_stack(void) { return (uint32_t)rtk::TRAV_STACK; }
uint32_t trace_max_bounces(void) { return (uint32_t)RT_MAX_BOUNCES; }
}
