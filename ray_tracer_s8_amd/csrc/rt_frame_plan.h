// rt_frame_plan.h — the decisions of one frame of a frame context (rt_api.hip rt_frame_ctx_render, rt_scene_render_tiles): how the
// frame is cut into strips, whether last frame's strip costs still hold, which entry renders which strip, what happens to the
// page-locked registration, how an entry's strips are grouped into launches, and how the entries' results fold into rt_frame_stats.
// Pure functions of their arguments: plain C++, no HIP, no threads, no globals (also built by g++ in the CPU harness
// tests/host/frame_plan_host.cpp, tests/test_frame_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "rt_assign.h"
#include "rt_consts.h"
#include "rt_plan.h"   // rtplan::Pose
#include "rt_tile.h"

namespace rtframe {

using rtplan::Pose;

constexpr uint32_t FRAME_FLAGS = RT_FLAG_FRAME_QUEUE | RT_FLAG_FRAME_NO_PIN | RT_FLAG_FRAME_STATIC;   // frame-level: not the kernels' business
constexpr uint32_t STRIPS_PER_ENTRY = 6;            // the balanced assignments' own cut: at least this many strips per entry
constexpr uint64_t SPLIT_BYTES = 64ull << 20;       // a call's strips above this many bytes: the last quarter is its own launch

// RGB8 bytes of one strip (rt_tile_bytes; controller main.rs:53-59)
inline size_t strip_bytes(const rt_tile_request& rq) {
    return rq.divisions ? (size_t)(rq.height / rq.divisions) * rq.width * 3 : 0;
}

// Two requests of the same frame: every field but division_no and seed (rt_scene_render_tiles' batches, the cost memory's key).  A
// knob that is NaN in both agrees — a request is of its own frame, so a single strip with a NaN knob is rendered (to NaN rays, as
// the reference's camera gives them) and not refused as a batch that disagrees.
inline bool same_knob(float a, float b) { return a == b || (a != a && b != b); }
inline bool same_frame(const rt_tile_request& a, const rt_tile_request& b) {
    return a.width == b.width && a.height == b.height && a.divisions == b.divisions && a.spp == b.spp &&
           a.max_bounces == b.max_bounces && same_knob(a.aperture, b.aperture) && same_knob(a.focus_distance, b.focus_distance) &&
           same_knob(a.fov, b.fov) && same_knob(a.focal_length, b.focal_length) && same_knob(a.t_min, b.t_min) &&
           same_knob(a.t_max, b.t_max) && a.flags == b.flags;
}

// The strips a frame is cut into (rt_tile.h "Strip assignment").  The balanced assignments cut the frame into their OWN strips: at
// least six per entry, so that longest-first has something to even out with (c5's 16 strips are two per entry at 8 devices: 3 % off the
// mean at best) — the first count from want = max(divisions, 6 n) up to min(height, 4 want) that divides the height, `divisions` if
// there is none.  `divisions` is the reference's wire format, not a property of the image: every sample's stream is keyed by its
// pixel's place in the FRAME (rt_tile.h `seed`), so any cut into whole rows gives the same bytes.  The strip queue, the static split
// and a single entry keep the request's strips.
inline uint32_t strips_of_frame(uint32_t height, uint32_t divisions, uint32_t n_entries, bool queue, bool static_) {
    if (queue || static_ || n_entries <= 1u) return divisions;
    const uint32_t want = std::max<uint32_t>(divisions, STRIPS_PER_ENTRY * n_entries);
    for (uint32_t dv = want; dv <= std::min<uint32_t>(height, 4u * want); dv++)
        if (height % dv == 0) return dv;
    return divisions;
}

// Ray segments per strip as the job's last frame measured them, and what they were measured on.  They hold for the same world
// (rt_frame_ctx_set_world forgets them) and the same frame geometry — size, strips, samples, depth, camera (its knobs and its pose), t
// window: the seed changes the paths, not where the expensive rows are.
struct CostMemory {
    std::vector<double> cost;      // one per strip of `rq`
    rt_tile_request rq = {};       // the frame they were measured on (as cut: divisions = the strips)
    Pose pose = {};                //   ... and the camera it was seen from (has_pose false: the reference camera)
    bool has_pose = false;
    bool valid = false;

    // The key: same_frame — which reads neither seed nor division_no — with the flags masked.  (All of them, not only the frame-level
    // ones: a frame that differs in a kernel-level flag still takes these costs.)
    bool usable(const rt_tile_request& now, const Pose& pose_now, bool has_pose_now) const {
        rt_tile_request a = now, b = rq;
        a.flags = b.flags = 0;
        const bool same_pose = has_pose_now == has_pose && (!has_pose_now || std::memcmp(&pose_now, &pose, sizeof pose) == 0);
        return valid && same_frame(a, b) && same_pose && cost.size() == now.divisions;
    }
    // Nothing counted — counting off (RT_STRIP_COST=0), or a frame without a ray — is no measurement: the next frame is a snake frame
    // again.
    void remember(const rt_tile_request& now, const Pose& pose_now, bool has_pose_now, const std::vector<unsigned long long>& cost_now,
                  bool counting_on) {
        cost.assign(cost_now.begin(), cost_now.end());
        rq = now;
        pose = pose_now;
        has_pose = has_pose_now;
        unsigned long long sum = 0ull;
        for (unsigned long long c : cost_now) sum += c;
        valid = counting_on && sum > 0ull;
    }
    void forget() { valid = false; }
};

// One frame as the dispatchers render it: the kernels' request (division_no 0, no frame-level flag, divisions = the strips of the
// cut), the bytes of one strip, and owner[k] = the entry of strip k.  A queue frame's entries pull strips and read no owner; it
// gets the STATIC_MOD owners all the same.
struct FramePlan {
    rt_tile_request rq = {};
    size_t strip_bytes = 0;
    rtassign::Mode mode = rtassign::STATIC_MOD;    // rt_frame_stats.assignment
    std::vector<uint32_t> owner;
};

inline FramePlan plan_frame(const rt_tile_request& rq_in, uint32_t n_entries, const CostMemory& mem, const Pose& pose, bool has_pose) {
    const bool queue = (rq_in.flags & RT_FLAG_FRAME_QUEUE) != 0, static_ = (rq_in.flags & RT_FLAG_FRAME_STATIC) != 0;
    FramePlan p;
    p.rq = rq_in;
    p.rq.division_no = 0;
    p.rq.flags &= ~FRAME_FLAGS;
    p.rq.divisions = strips_of_frame(rq_in.height, rq_in.divisions, n_entries, queue, static_);
    p.strip_bytes = strip_bytes(p.rq);
    const bool usable = mem.usable(p.rq, pose, has_pose);
    p.mode = queue ? rtassign::QUEUE : static_ ? rtassign::STATIC_MOD : usable ? rtassign::BY_COST : rtassign::SNAKE;
    rtassign::assign(p.rq.divisions, n_entries, usable ? mem.cost.data() : nullptr, p.mode == rtassign::QUEUE ? rtassign::STATIC_MOD : p.mode,
                     p.owner);
    return p;
}

// The strips' costs as the frame of `plan` measured them: the next frame of the job is assigned by them.  A queue frame measures
// nothing per strip and leaves the memory as it was.
inline void remember_frame(CostMemory& mem, const FramePlan& plan, const Pose& pose, bool has_pose,
                           const std::vector<unsigned long long>& cost_now, bool counting_on) {
    if (plan.mode != rtassign::QUEUE) mem.remember(plan.rq, pose, has_pose, cost_now, counting_on);
}

// What a frame does to the context's page-locked registration of the caller's buffer (held_ptr, held_len; nullptr: none) before it
// renders into `out`:
//
//     frame wants pinning | held                      | release | acquire
//     --------------------+---------------------------+---------+--------
//     no                  | nothing                   |   no    |   no
//     no                  | any buffer                |   yes   |   no       (a RT_FLAG_FRAME_NO_PIN frame drops what is held, even
//     yes                 | nothing                   |   no    |   yes       another buffer's registration)
//     yes                 | `out`, >= frame_bytes     |   no    |   no       (kept)
//     yes                 | `out`, <  frame_bytes     |   yes   |   yes
//     yes                 | another buffer            |   yes   |   yes
//
// acquire is best effort: a buffer that cannot be registered is used as it is, and nothing is held afterwards.
struct PinStep {
    bool release, acquire;
};
inline PinStep pin_step(bool want_pin, const void* held_ptr, size_t held_len, const void* out, size_t frame_bytes) {
    const bool kept = want_pin && held_ptr == out && held_len >= frame_bytes;
    return {!kept && held_ptr != nullptr, !kept && want_pin};
}

// Launch groups [first, count) of a call's n strips, none over MAX_BATCH: the last quarter of the strips goes out as its own launch,
// so that the D2H copies of the strips before it run under it and only the last group's copies are exposed — when the downloads are
// worth hiding: a second launch costs its own tail (half a millisecond at c3, one at c4), a frame's strips come down at about 50 GB/s,
// so up to 64 MiB per call one launch and an exposed download are faster (c3, 24.9 MB: 9.3 instead of 9.6 ms per frame; c4's 99.5 MB
// keeps the split).
inline std::vector<std::pair<uint32_t, uint32_t>> launch_groups(uint32_t n, size_t strip_bytes) {
    std::vector<std::pair<uint32_t, uint32_t>> groups;
    const uint32_t tail = (n >= 4 && (uint64_t)strip_bytes * n > SPLIT_BYTES) ? std::max<uint32_t>(1, n / 4) : 0;
    for (uint32_t i0 = 0; i0 < n - tail; i0 += rtk::MAX_BATCH) groups.emplace_back(i0, std::min<uint32_t>(rtk::MAX_BATCH, n - tail - i0));
    for (uint32_t i0 = n - tail; i0 < n; i0 += rtk::MAX_BATCH) groups.emplace_back(i0, std::min<uint32_t>(rtk::MAX_BATCH, n - i0));
    return groups;
}

// Per-strip costs: the kernels add the ray segments of strip i of launch group g to raw[g][copy][i], one block of COST_COPIES x
// MAX_BATCH counters per group (KParams::strip_cost).  out[first of g + i] = the sum over the copies.
constexpr size_t COST_BLOCK = (size_t)rtk::COST_COPIES * rtk::MAX_BATCH;
inline void fold_strip_costs(const unsigned long long* raw, const std::vector<std::pair<uint32_t, uint32_t>>& groups, unsigned long long* out) {
    for (size_t g = 0; g < groups.size(); g++)
        for (uint32_t i = 0; i < groups[g].second; i++) {
            unsigned long long sum = 0;
            for (uint32_t c = 0; c < rtk::COST_COPIES; c++) sum += raw[g * COST_BLOCK + (size_t)c * rtk::MAX_BATCH + i];
            out[groups[g].first + i] = sum;
        }
}

// What one entry's dispatcher brings back from a frame.
struct EntryResult {
    rt_tile_stats st;
    float busy_ms;      // dispatcher wall time of the render
};

// The reduction part of rt_frame_stats (the caller fills wall_ms, pin_ms, scene_ms, host_ms, n_devices, pinned, assignment): counters
// summed; the entries run concurrently, so totals' kernel_ms, h2d_ms and d2h_ms are the largest; engine and broad_form of the last
// entry that launched; kernel_ms and d2h_exposed_ms of the entry that finished last (the first of equals).  Strip-queue mode keeps
// two launches in flight per entry, so their event times overlap and do not add up to a duration: there kernel_ms is that
// dispatcher's wall time and nothing is booked as exposed download.  The balance is taken over all n entries, entry_segments holds
// the first RT_FRAME_STATS_ENTRIES.
inline rt_frame_stats fold_frame_stats(const EntryResult* entries, size_t n, bool queue) {
    rt_frame_stats fs;
    std::memset(&fs, 0, sizeof fs);
    rt_tile_stats& tot = fs.totals;
    float last = -1.f;
    unsigned long long seg_max = 0, seg_sum = 0;
    for (size_t e = 0; e < n; e++) {
        const rt_tile_stats& st = entries[e].st;
        tot.ray_segments += st.ray_segments;
        tot.primary_rays += st.primary_rays;
        tot.broad_candidates += st.broad_candidates;
        tot.exact_fallbacks += st.exact_fallbacks;
        tot.node_steps += st.node_steps;
        tot.kernel_ms = std::max(tot.kernel_ms, st.kernel_ms);
        tot.h2d_ms = std::max(tot.h2d_ms, st.h2d_ms);
        tot.d2h_ms = std::max(tot.d2h_ms, st.d2h_ms);
        tot.n_launches += st.n_launches;
        if (st.n_launches) {
            tot.engine = st.engine;
            tot.broad_form = st.broad_form;
        }
        if (entries[e].busy_ms > last) {
            last = entries[e].busy_ms;
            fs.kernel_ms = queue ? entries[e].busy_ms : st.kernel_ms;
            fs.d2h_exposed_ms = queue ? 0.f : st.d2h_ms;
        }
        if (e < RT_FRAME_STATS_ENTRIES) fs.entry_segments[e] = st.ray_segments;
        seg_max = std::max<unsigned long long>(seg_max, st.ray_segments);
        seg_sum += st.ray_segments;
    }
    fs.balance_max_over_mean = seg_sum ? (float)((double)seg_max * (double)n / (double)seg_sum) : 0.f;
    return fs;
}

}  // namespace rtframe
