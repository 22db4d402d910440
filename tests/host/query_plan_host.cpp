// Test harness (CPU only, built by tests/test_query_plan.py with g++): the ray-query engine choice of csrc/rt_plan.h — the
// product's plan_query — on hand-built scene shapes and request flags.
#include <cstdint>

#include "rt_plan.h"

extern "C" {

// shape: n_sph, n_tri, bvh_depth, inverted_boxes; out: engine, scan_mode, full_chain, lds bytes
void query_plan(const uint32_t* shape, uint32_t flags, uint64_t* out) {
    rtplan::SceneShape sh;
    sh.n_sph = shape[0];
    sh.n_tri = shape[1];
    sh.bvh_depth = shape[2];
    sh.inverted_boxes = shape[3] != 0;
    const rtplan::QueryPlan q = rtplan::plan_query(sh, flags);
    out[0] = (uint64_t)q.engine;
    out[1] = (uint64_t)q.scan_mode;
    out[2] = q.full_chain ? 1u : 0u;
    out[3] = (uint64_t)q.lds;
}

uint32_t query_trav_stack(void) { return (uint32_t)rtk::TRAV_STACK; }
uint32_t query_block(void) { return (uint32_t)rtplan::QUERY_BLOCK; }
}
