// CPU harness around the PRODUCT's frame plan (ray_tracer_s8_amd/csrc/rt_frame_plan.h), for tests/test_frame_plan.py.
#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_frame_plan.h"

namespace {
// pose: NULL (the reference camera) or the 12 floats of rtplan::Pose
rtframe::Pose pose_of(const float* pose) {
    rtframe::Pose ps = {};
    if (pose) std::memcpy(&ps, pose, sizeof ps);
    return ps;
}
}  // namespace

extern "C" {

uint32_t fp_max_batch() { return (uint32_t)rtk::MAX_BATCH; }
uint32_t fp_cost_copies() { return rtk::COST_COPIES; }

uint32_t fp_strips(uint32_t height, uint32_t divisions, uint32_t n_entries, int queue, int static_) {
    return rtframe::strips_of_frame(height, divisions, n_entries, queue != 0, static_ != 0);
}

// ---- the cost memory behind a handle
void* fp_mem_new() { return new rtframe::CostMemory; }
void fp_mem_free(void* m) { delete (rtframe::CostMemory*)m; }
void fp_mem_forget(void* m) { ((rtframe::CostMemory*)m)->forget(); }
int fp_mem_usable(const void* m, const rt_tile_request* rq, const float* pose) {
    return ((const rtframe::CostMemory*)m)->usable(*rq, pose_of(pose), pose != nullptr) ? 1 : 0;
}
void fp_mem_remember(void* m, const rt_tile_request* rq, const float* pose, const unsigned long long* cost, uint32_t n, int counting_on) {
    ((rtframe::CostMemory*)m)->remember(*rq, pose_of(pose), pose != nullptr, std::vector<unsigned long long>(cost, cost + n), counting_on != 0);
}

// plan_frame: returns the strips of the cut; rq_out = the kernels' request, owner_out: room for 4 * max(divisions, 6 n) + 1 entries
uint32_t fp_plan(const void* m, const rt_tile_request* rq_in, uint32_t n_entries, const float* pose, rt_tile_request* rq_out,
                 uint64_t* strip_bytes_out, uint32_t* mode_out, uint32_t* owner_out) {
    const rtframe::FramePlan p = rtframe::plan_frame(*rq_in, n_entries, *(const rtframe::CostMemory*)m, pose_of(pose), pose != nullptr);
    *rq_out = p.rq;
    *strip_bytes_out = p.strip_bytes;
    *mode_out = (uint32_t)p.mode;
    for (size_t k = 0; k < p.owner.size(); k++) owner_out[k] = p.owner[k];
    return (uint32_t)p.owner.size();
}
// what rt_frame_ctx_render does after the frame of this request: plan it again (pure), then remember_frame with the costs "measured"
void fp_remember_frame(void* m, const rt_tile_request* rq_in, uint32_t n_entries, const float* pose, const unsigned long long* cost, uint32_t n,
                       int counting_on) {
    rtframe::CostMemory& mem = *(rtframe::CostMemory*)m;
    const rtframe::FramePlan p = rtframe::plan_frame(*rq_in, n_entries, mem, pose_of(pose), pose != nullptr);
    rtframe::remember_frame(mem, p, pose_of(pose), pose != nullptr, std::vector<unsigned long long>(cost, cost + n), counting_on != 0);
}

// bit 0: release, bit 1: acquire
uint32_t fp_pin_step(int want_pin, uintptr_t held_ptr, uint64_t held_len, uintptr_t out, uint64_t frame_bytes) {
    const rtframe::PinStep s = rtframe::pin_step(want_pin != 0, (const void*)held_ptr, (size_t)held_len, (const void*)out, (size_t)frame_bytes);
    return (s.release ? 1u : 0u) | (s.acquire ? 2u : 0u);
}

// groups_out: room for n / MAX_BATCH + 2 pairs (first, count); returns the number of groups
uint32_t fp_launch_groups(uint32_t n, uint64_t strip_bytes, uint32_t* groups_out) {
    const auto groups = rtframe::launch_groups(n, (size_t)strip_bytes);
    for (size_t g = 0; g < groups.size(); g++) {
        groups_out[2 * g] = groups[g].first;
        groups_out[2 * g + 1] = groups[g].second;
    }
    return (uint32_t)groups.size();
}

// raw: n_groups x COST_COPIES x MAX_BATCH counters; groups: n_groups pairs (first, count); out: one sum per strip
void fp_fold_strip_costs(const unsigned long long* raw, const uint32_t* groups, uint32_t n_groups, unsigned long long* out) {
    std::vector<std::pair<uint32_t, uint32_t>> g;
    for (uint32_t i = 0; i < n_groups; i++) g.emplace_back(groups[2 * i], groups[2 * i + 1]);
    rtframe::fold_strip_costs(raw, g, out);
}

void fp_fold_frame_stats(const rt_tile_stats* st, const float* busy_ms, uint32_t n, int queue, rt_frame_stats* out) {
    std::vector<rtframe::EntryResult> e;
    for (uint32_t i = 0; i < n; i++) e.push_back({st[i], busy_ms[i]});
    *out = rtframe::fold_frame_stats(e.data(), e.size(), queue != 0);
}
}
