// rt_api.hip — host side of the C-ABI declared in include/rt_tile.h.
//
// Plays the roles the reference gives to the slave's worker (ray-tracer-slave/src/main.rs:32-106:
// take a RenderInfo, produce the strip's RGB8 bytes) and, in rt_render_frame, to the
// controller's dispatch + assembly (ray-tracer-controller/src/main.rs:47-75, 109-115).
// No torch types, no CPU fallback: without a HIP device every entry point fails loudly.
// Device memory, events and streams are held by the owners of rt_device.h: nothing here frees or destroys one by hand.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <climits>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "rt_assign.h"
#include "rt_bvh.h"
#include "rt_device.h"
#include "rt_frame_plan.h"
#include "rt_kernel.hip.h"
#include "rt_plan.h"
#include "rt_query.hip.h"
#include "rt_scene_host.h"
#include "rt_trace.hip.h"
#include "rt_bounce.hip.h"
#include "rt_direct.hip.h"
#include "rt_nee.hip.h"
#include "rt_aov.hip.h"
#include "rt_camera.hip.h"
#include "rt_denoise.hip.h"
#include "rt_tile.h"
#ifdef RT_DEBUG_HOOKS
#include "rt_unit.hip.h"      // record sizes and launchers of the unit kernels, rt_unit_sampling.hip.h's too (rt_debug_unit)
#endif

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// Nothing may unwind across the C boundary (rt_tile.h: "never throws or aborts"): every extern "C" entry point runs its
// body through this.  The bodies allocate (std::vector, std::string, std::thread); a failed allocation becomes
// RT_ERR_OOM, anything else RT_ERR_HIP with the exception's text.  Setting the message must not throw either.
void set_err_noexcept(const char* what) noexcept {
    try {
        g_err = what;
    } catch (...) {
    }
}
template <class F>
int guarded(F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        set_err_noexcept("host allocation failed");
        return RT_ERR_OOM;
    } catch (const std::exception& e) {
        set_err_noexcept(e.what());
        return RT_ERR_HIP;
    } catch (...) {
        set_err_noexcept("internal error");
        return RT_ERR_HIP;
    }
}

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return fail(RT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ \
                                                                                        ":" +         \
                                        std::to_string(__LINE__) + ")");                              \
    } while (0)

using rtdev::DevArray;
using rtdev::Event;
using rtdev::EventPool;
using rtdev::GrowBuf;
using rtdev::Stream;

// A staging buffer grown to at least `bytes`.  Its owner has the device current and no work in flight on the old area.
int reserve(GrowBuf& buf, size_t bytes, const char* what) {
    if (buf.grow(bytes) == hipSuccess) return RT_OK;
    (void)hipGetLastError();   // (the failure is reported here: it must not stick to the next HIP call)
    return fail(RT_ERR_OOM, std::string("hipMalloc(") + what + ") failed");
}

struct DeviceCtx {
    int dev = -1;
    Stream stream;
    Stream copy_stream;   // D2H of finished strips while the next launch of the batch runs
    int n_cu = 0;
    std::mutex mu;   // serialises synchronous calls on one device
};

// Test / A-B knobs of the launch path.  They used to be getenv() calls inside launch_batch and rt_render_frame — read per
// launch from several worker threads while tests flipped them with setenv (undefined behaviour), and two of them overrode
// explicit request flags.  Now: one process-level table of atomics, filled from the environment ONCE by the first rt_init,
// changed afterwards only through rt_debug_set (exported, deliberately not in rt_tile.h: tests and tools only), and an
// explicit RT_FLAG_* in the request always wins over a knob.
enum DebugKnob {
    DBG_LDS_TREE = 0,      // RT_LDS_TREE        0: never the LDS-resident tree engine                      (default 1)
    DBG_CULL_WALK,         // RT_CULL_WALK       0 / 1: culled walk off / on wherever it is valid; -1: host rule (default -1)
    DBG_NO_STAGE,          // RT_NO_STAGE        1: no LDS output staging                                   (default 0)
    DBG_SLOTS,             // RT_SLOTS           sample units: pixel slots per wave, 1 ... 32 (more: 32); <= 0: host rule    (default 0)
    DBG_FORCE_CAPPED,      // RT_FORCE_CAPPED    1: quantised walks take the capped-stack kernel             (default 0)
    DBG_STACK_LDS,         // RT_STACK_LDS       capped-stack kernel: stack entries per lane in LDS; 0: STACK_LDS_MAX
    DBG_COMPACT,           // RT_COMPACT         0: per-lane root tests in the exact-node L2 kernel          (default 1)
    DBG_REFILL_EIGHTHS,    // RT_REFILL_EIGHTHS  refill threshold of the walks; 0: host rule
    DBG_COMMIT_SLOTS,      // RT_COMMIT_SLOTS    sample units: complete slots a commit waits for; 0: host rule             (default 0)
    DBG_VERBOSE,           // RT_VERBOSE         engine / LDS plan of every launch on stderr                 (default 0)
    DBG_REORDER,           // RT_REORDER         0: primitive records stay in the caller's order (A/B)          (default 1)
    DBG_TAIL_TILES,        // RT_TAIL_TILES      tiles at the end of a launch's queue handed out in quarters; -1: host rule (default -1)
    DBG_STRIP_COST,        // RT_STRIP_COST      0: the kernels do not count per-strip ray segments for the frame context (A/B)   (default 1)
    DBG_DENOISE_LDS_STEP,  // RT_DENOISE_LDS_STEP denoiser: largest step staged in LDS (0: none); -1: rtplan::DN_LDS_MAX_STEP    (default -1)
    DBG_LTREE_GENERAL,     // RT_LTREE_GENERAL   1: the LDS-tree engines take their general kernel for sphere-only worlds too (A/B, tests)  (default 0)
    DBG_PLAIN_FRAME,       // RT_PLAIN_FRAME     0: plain frames commit through the general path of the LDS-tree kernels (A/B, tests)       (default 1)
    DBG_N
};
std::atomic<int> g_dbg[DBG_N];
const struct { const char* env; int def; } g_dbg_spec[DBG_N] = {
    {"RT_LDS_TREE", 1}, {"RT_CULL_WALK", -1}, {"RT_NO_STAGE", 0}, {"RT_SLOTS", 0}, {"RT_FORCE_CAPPED", 0},
    {"RT_STACK_LDS", 0}, {"RT_COMPACT", 1}, {"RT_REFILL_EIGHTHS", 0}, {"RT_COMMIT_SLOTS", 0}, {"RT_VERBOSE", 0}, {"RT_REORDER", 1}, {"RT_TAIL_TILES", -1}, {"RT_STRIP_COST", 1},
    {"RT_DENOISE_LDS_STEP", -1}, {"RT_LTREE_GENERAL", 0}, {"RT_PLAIN_FRAME", 1}};
#ifdef RT_DEBUG_HOOKS
// An OUTPUT of the launch path, not a knob: which variant of an LDS-tree kernel the last tile launch of the process took — bit 0 the
// sphere-only instantiation, bit 1 the plain-frame commit.  Test library only (the product stores nothing); never read from the
// environment; tests exchange it through rt_debug_set under the name RT_LAST_VARIANT (tests/test_abi.py pins the set of
// rt_debug_* exports, so it has no entry point of its own and, for want of a scene argument there, is one word per process).
std::atomic<int> g_last_variant{0};
#endif
std::once_flag g_dbg_once;
void dbg_load_env() {
    std::call_once(g_dbg_once, [] {
        for (int k = 0; k < DBG_N; k++) {
            const char* e = getenv(g_dbg_spec[k].env);
            int v = g_dbg_spec[k].def;
            if (e) v = k == DBG_VERBOSE ? 1 : atoi(e);
            g_dbg[k].store(v, std::memory_order_relaxed);
        }
    });
}
inline int dbg(DebugKnob k) { return g_dbg[k].load(std::memory_order_relaxed); }

std::mutex g_mu;
bool g_init = false;
std::vector<DeviceCtx*> g_ctx;
std::atomic<int> g_live_scenes{0};   // rt_shutdown is refused while any scene is alive (scenes point at their DeviceCtx)

// The launch-path knobs the plan reads, read once per launch
rtplan::Knobs plan_knobs() {
    rtplan::Knobs k;
    k.lds_tree = dbg(DBG_LDS_TREE);
    k.cull_walk = dbg(DBG_CULL_WALK);
    k.no_stage = dbg(DBG_NO_STAGE);
    k.slots = dbg(DBG_SLOTS);
    k.commit_slots = dbg(DBG_COMMIT_SLOTS);
    k.force_capped = dbg(DBG_FORCE_CAPPED);
    k.stack_lds = dbg(DBG_STACK_LDS);
    k.compact = dbg(DBG_COMPACT);
    k.refill_eighths = dbg(DBG_REFILL_EIGHTHS);
    k.tail_tiles = dbg(DBG_TAIL_TILES);
    k.ltree_general = dbg(DBG_LTREE_GENERAL);
    k.plain_frame = dbg(DBG_PLAIN_FRAME);
    return k;
}

}  // namespace

// Its device resources are owners of rt_device.h, released by the (implicit) destructor: ctx->dev MUST be current on the thread that
// deletes a scene, a frame context's dispatcher included.  Only rt_scene_destroy_impl deletes one, and it sets the device first.
struct rt_scene {
    DeviceCtx* ctx = nullptr;
    rtplan::SceneShape shape;       // what the engine rules read (rt_plan.h)
    uint32_t n_lights = 0;          // direct lighting: the emitters of the scene (rt_scene_light_count)
    DevArray<uint32_t> d_lights;    //   their primitive numbers in ascending world position (rtscene::emitter_list)
    DevArray<float> d_light_c;      // RT_FLAG_LIGHTS_BY_POWER (rtscene::light_table): the running sums of the powers, per emitter
    DevArray<float> d_light_ip;     //   1 / p of an emitter, by primitive number
    float light_total = 0.f;        //   the last running sum
    std::vector<uint32_t> light_world;   // rt_scene_light_table: the world position and the mixture probability of every emitter
    std::vector<float> light_p;
    rtplan::Pose pose;              // the job's placed camera (rt_scene_set_camera); read when a call is enqueued
    bool has_pose = false;          //   false: the reference camera
    uint32_t light_sampling = RT_LIGHTS_AREA;   // how a sphere light is sampled (rt_scene_set_light_sampling); read when a direct-lighting
                                                //   or NEE call is enqueued, where it picks the kernel instance
    uint32_t glossy_sampling = RT_GLOSSY_BOUNCE;   // whether RT_NEE_MIS takes light samples at glossy hits (rt_scene_set_glossy_sampling);
                                                   //   read when an NEE call is enqueued, where it picks the kernel instance
    DevArray<float4> d_geom;
    DevArray<float4> d_geom_pk;
    DevArray<float4> d_geom_px;    // expanded-form broad phase records
    DevArray<float4> d_mat;
    DevArray<float> d_emis;
    DevArray<float> d_tri;
    DevArray<float4> d_tri_box;
    DevArray<float4> d_bvh;        // rtbvh::FlatNode[]
    DevArray<float4> d_trav;       // rtbvh::TravNode[]
    GrowBuf stack_ovf;             // quantised-node kernel: stack entries (uint32_t) beyond the LDS part, [entry][thread].  Its `done` is
                                   // the end of the last launch that used it: the area is one per scene, so such launches are
                                   // chained even when the caller spreads them over several streams
    DevArray<uint4> d_travq;       // rtbvh::QNode[] (quantised twin)
    DevArray<float4> d_geom_r;     // (cx,cy,cz,radius)
    DevArray<uint32_t> d_big;      // culled walk: spheres root-tested at query start (too large for its slack)
    uint32_t n_big = 0;
    float tri_k = 0.f, tri_diag = 0.f, tri_es = 0.f, tri_e = 0.f;   // culled walk over the exact nodes: maxima over the triangles not in `big`
    rtbvh::QGrid grid;
    DevArray<uint32_t> d_leaf_of;
    DevArray<uint32_t> d_world_rank;    // world_index of every primitive when the caller gave one (rt_tile.h "the world's order")
    bool has_order = false;
    float bvh_build_ms = 0.f;
    DevArray<unsigned long long> d_counters;    // [0..2] stats, [4 + slot] tile queues
    // Sample-unit rings (rt_kernel.hip.h "Sample units"): scratch of one launch, [waves][slots][16 B].  Launches on ONE stream
    // follow each other, so a ring belongs to the stream that used it last; a launch on another stream that has to share it
    // (more streams than rings) waits for that launch's end (the area's `done`) first.
    struct Ring {
        GrowBuf buf;
        hipStream_t last = nullptr;
        uint64_t stamp = 0;
    };
    Ring rings[4];
    uint64_t ring_clock = 0;
    // staging of the tile host form (grown on demand): the strips' bytes, their f32 twins, the running sums of
    // rt_scene_render_tile_pass and the per-strip ray segments of the batched call (frame context)
    GrowBuf d_out, d_outf, d_acc, d_cost;
    // ... and ONE buffer for the arrays of the eight other host forms (rt_scene_intersect, _trace, _bounce, _direct, _trace_nee,
    // _render_aov, _camera_rays, _denoise; Staging).  They can share it: every such call holds ctx->mu and sc->mu from start to end,
    // begins by collecting everything pending, and waits for its own downloads before it returns, so no two of them are ever in
    // flight; and GrowBuf::grow frees only when it grows, which is before the call has enqueued anything.
    GrowBuf d_stage;
    EventPool events;   // the pairs of events that time the launches; its pending list is the launches not yet collected
    uint64_t primary_rays = 0;
    float h2d_ms = 0.f;
    uint32_t last_engine = 0, last_form = 0;
    std::mutex mu;
};

namespace {

int check_request(const rt_tile_request* rq) {
    if (!rq) return fail(RT_ERR_BAD_ARG, "request is NULL");
    if (rq->width == 0 || rq->height == 0 || rq->divisions == 0 || rq->spp == 0)
        return fail(RT_ERR_BAD_ARG, "width, height, divisions and spp must be non-zero");
    if (rq->division_no >= rq->divisions) return fail(RT_ERR_BAD_ARG, "division_no >= divisions");
    if (rq->height / rq->divisions == 0) return fail(RT_ERR_BAD_ARG, "height / divisions == 0 rows");
    if (rq->max_bounces > RT_MAX_BOUNCES) return fail(RT_ERR_LIMIT, "max_bounces > RT_MAX_BOUNCES");
    if (rq->spp > RT_MAX_SPP) return fail(RT_ERR_LIMIT, "spp > RT_MAX_SPP");
    if (rq->reserved != 0) return fail(RT_ERR_BAD_ARG, "reserved must be 0");
    if ((uint64_t)rq->width * rq->height > 0x7fffffffull) return fail(RT_ERR_LIMIT, "image too large");
    return RT_OK;
}

constexpr uint32_t QUEUE_SLOTS = 16384;          // uncollected launches per scene (one 8-byte queue head each)
#ifdef RT_PROFILE_TIME
constexpr uint32_t COUNTER_WORDS = 4 + QUEUE_SLOTS + 16 * 8192;      // (+ one block per wave: the phase clock, tools/phase_time.py)
#else
constexpr uint32_t COUNTER_WORDS = 4 + QUEUE_SLOTS;
#endif

int check_slot(const rt_scene* sc) {
    if (sc->events.pending().size() >= QUEUE_SLOTS) return fail(RT_ERR_LIMIT, "too many uncollected launches: call rt_scene_collect()");
    return RT_OK;
}

// Enqueue one kernel launch on `stream`, between a pair of events that collect_locked times it by.  Every launch_* goes through
// here.  Caller holds sc->mu and has the device current.
template <class P>
int enqueue(rt_scene* sc, hipStream_t stream, void (*kern)(const P), uint32_t blocks, uint32_t block, size_t lds, const P& p) {
    EventPool::Lease ev;
    int rc = check_slot(sc);
    if (rc) return rc;
    HIPCHK(sc->events.lease(ev));
    HIPCHK(hipEventRecord(ev.a(), stream));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(block), lds, stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.b(), stream));
    ev.to_pending();
    return RT_OK;
}

// The grid of a persistent kernel: as many workgroups as the chip holds at this block size and dynamic LDS (per_cu of them a
// CU, at least one), and no more than it takes to give each of the `items` a lane.
struct Grid {
    uint32_t blocks = 0;
    int per_cu = 0;
};
template <class P>
int persistent_blocks(const rt_scene* sc, void (*kern)(const P), uint32_t block, size_t lds, uint64_t items, Grid& g) {
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&g.per_cu, kern, (int)block, lds));
    if (g.per_cu < 1) g.per_cu = 1;
    g.blocks = (uint32_t)std::min<uint64_t>((items + block - 1) / block, (uint64_t)sc->ctx->n_cu * (uint32_t)g.per_cu);
    return RT_OK;
}

// The scene as the first-hit kernels read it (rt_path_steps.hip.h SceneRefs), into their parameter block.
void scene_refs(const rt_scene* sc, bool full_chain, rtk::SceneRefs& r) {
    r.n_sph = sc->shape.n_sph;
    r.n_tri = sc->shape.n_tri;
    r.root_ref = sc->shape.root_ref;
    r.full_chain = full_chain ? 1u : 0u;
    r.trav = sc->d_trav.get();
    r.bvh_nodes = sc->d_bvh.get();
    r.leaf_of = sc->d_leaf_of.get();
    r.world_rank = sc->has_order ? sc->d_world_rank.get() : nullptr;
    r.geom_r = sc->d_geom_r.get();
    r.tri = sc->d_tri.get();
    r.counters = sc->d_counters.get();
}

// Enqueue a batch of strips of one frame (<= MAX_BATCH) as ONE launch of persistent waves.
// Caller holds sc->mu and has the device current.
// d_strip_cost: optional device array of COST_COPIES x MAX_BATCH counters (zeroed by the caller, on `stream`): the kernels add the ray
// segments of strip i of the batch to [copy][i] (KParams::strip_cost); the caller sums the copies.
// pass: a progressive pass (rt_scene_render_tile_pass) — samples [begin, end) of the request's spp, the strips' running sums in
// d_acc[i] (checked by the caller: begin < end <= spp, no NULL entry).  nullptr: all spp samples, no sum carried (one pass).
struct Pass {
    uint32_t begin, end;
    void* const* d_acc;
};
// The scene's stack-overflow area of the capped-stack kernels, grown to at least `words`.
int acquire_stack_ovf(rt_scene* sc, size_t words) {
    HIPCHK(sc->stack_ovf.grow(words * sizeof(uint32_t)));
    return RT_OK;
}

// The launch's sample-unit ring of at least `bytes`: the one this stream used last, else a free one, else the least recently used
// (after its last launch).
int acquire_ring(rt_scene* sc, hipStream_t stream, size_t bytes, rt_scene::Ring*& rg) {
    rg = nullptr;
    for (auto& r : sc->rings)
        if (r.buf.data() && r.last == stream) { rg = &r; break; }
    if (!rg)
        for (auto& r : sc->rings)
            if (!r.buf.data()) { rg = &r; break; }
    if (!rg) {
        rg = &sc->rings[0];
        for (auto& r : sc->rings)
            if (r.stamp < rg->stamp) rg = &r;
    }
    HIPCHK(rg->buf.grow(bytes));
    if (!rg->buf.done) HIPCHK(rg->buf.done.create(hipEventDisableTiming));
    else if (rg->last != stream) HIPCHK(hipStreamWaitEvent(stream, rg->buf.done.get(), 0));
    rg->last = stream;
    rg->stamp = ++sc->ring_clock;
    return RT_OK;
}

int launch_batch(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, void* const* d_rgb, void* const* d_f32,
                 hipStream_t stream, unsigned long long* d_strip_cost = nullptr, const Pass* pass = nullptr) {
    const rtplan::Knobs kn = plan_knobs();
    const rtplan::SceneShape& sh = sc->shape;
    rtk::KParams p;
    std::memset(&p, 0, sizeof p);
    const rtplan::SampleRange smp = pass ? rtplan::SampleRange{pass->begin, pass->end, true} : rtplan::SampleRange{0u, rqs[0].spp, false};
    rtplan::Plan pl = rtplan::plan_launch(sh, rqs[0], n, smp, kn, p, sc->has_pose ? &sc->pose : nullptr);
    if (pl.status != RT_OK) return fail(pl.status, pl.error);
    p.geom_pk = sc->d_geom_pk.get();
    p.geom_px = sc->d_geom_px.get();
    p.geom = sc->d_geom.get();
    p.mat = sc->d_mat.get();
    p.emis = sc->d_emis.get();
    p.tri = sc->d_tri.get();
    p.tri_box = sc->d_tri_box.get();
    p.bvh_nodes = sc->d_bvh.get();
    p.trav = sc->d_trav.get();
    p.travq = sc->d_travq.get();
    p.geom_r = sc->d_geom_r.get();
    for (int i = 0; i < 3; i++) {
        p.q_base[i] = sc->grid.base[i];
        p.q_step[i] = sc->grid.step[i];
        p.q_rstep[i] = 1.0f / sc->grid.step[i];
    }
    p.leaf_of = sc->d_leaf_of.get();
    p.world_rank = sc->has_order ? sc->d_world_rank.get() : nullptr;
    p.big = sc->d_big.get();
    p.n_big = sc->n_big;
    p.r_slack = sh.r_slack;
    p.tri_k = sc->tri_k;
    p.tri_diag = sc->tri_diag;
    p.tri_es = sc->tri_es;
    p.tri_e = sc->tri_e;
    for (uint32_t i = 0; i < n; i++) {
        p.strips[i].seed = rqs[i].seed;
        p.strips[i].rgb = (uint8_t*)d_rgb[i];
        p.strips[i].f32 = d_f32 ? (float*)d_f32[i] : nullptr;
        p.strips[i].acc = pass ? (float*)pass->d_acc[i] : nullptr;
        p.strips[i].y0 = p.Hs * rqs[i].division_no;
    }
    int rc = check_slot(sc);               // (here already: the slot is the launch's queue head)
    if (rc) return rc;
    p.counters = sc->d_counters.get();
    p.queue = sc->d_counters.get() + 4 + sc->events.pending().size();
    p.strip_cost = dbg(DBG_STRIP_COST) ? d_strip_cost : nullptr;
    bool any_f32 = false;
    for (uint32_t i = 0; i < n; i++) any_f32 = any_f32 || p.strips[i].f32 != nullptr;
    p.plain = rtplan::plain_frame(pl, any_f32, p.strip_cost != nullptr) ? 1u : 0u;

    // persistent grid: as many workgroups as the chip holds at this LDS/VGPR budget
    const rtk::KernelFn kern = pl.isect < 2 ? rtk::kernel_linear(pl.isect, pl.expanded) : rtk::kernel_traverse(pl.isect, pl.count_steps, pl.tris);
    int per_cu = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, pl.block, pl.lds));
    if (per_cu < 1) per_cu = 1;
    if (dbg(DBG_VERBOSE))
        fprintf(stderr, "[rt] engine %d%s  lds %zu B  workgroups/CU %d  leaf slots %u  bvh depth %u  leaf density %.3f  prims %u\n",
                pl.engine, pl.capped ? " (capped stack)" : "", pl.lds, per_cu, pl.maxl_l2, sh.bvh_depth, sh.leaf_density, sh.n_sph + sh.n_tri);
    rtplan::plan_queue(pl, (uint32_t)sc->ctx->n_cu * (uint32_t)per_cu, kn, p);
    p.stack_ovf = nullptr;
    if (pl.capped) {
        if ((rc = acquire_stack_ovf(sc, pl.ovf_words))) return rc;
        p.stack_ovf = (uint32_t*)sc->stack_ovf.data();
    }
    if (dbg(DBG_VERBOSE))
        fprintf(stderr, "[rt] sample-unit ring %zu B: %u units per pixel, %u slots of %u records per wave\n", pl.ring_bytes, p.upp, p.n_slots,
                p.slot_stride);
    rt_scene::Ring* rg = nullptr;
    if ((rc = acquire_ring(sc, stream, pl.ring_bytes, rg))) return rc;
    p.ring = (float*)rg->buf.data();
    if (p.stack_ovf) {
        if (sc->stack_ovf.done) HIPCHK(hipStreamWaitEvent(stream, sc->stack_ovf.done.get(), 0));
        else HIPCHK(sc->stack_ovf.done.create(hipEventDisableTiming));
    }
    HIPCHK(hipMemsetAsync(p.queue, 0, sizeof(unsigned long long), stream));
    sc->last_engine = (uint32_t)pl.engine;
    sc->last_form = pl.expanded ? 1u : 0u;
#ifdef RT_DEBUG_HOOKS
    g_last_variant.store((pl.tris ? 0 : 1) | (p.plain ? 2 : 0), std::memory_order_relaxed);
#endif
    if ((rc = enqueue(sc, stream, kern, pl.blocks, pl.block, pl.lds, p))) return rc;
    HIPCHK(hipEventRecord(rg->buf.done.get(), stream));
    if (p.stack_ovf) HIPCHK(hipEventRecord(sc->stack_ovf.done.get(), stream));
    sc->primary_rays += (uint64_t)p.Hs * p.W * p.upp * n;
    return RT_OK;
}

int collect_locked(rt_scene* sc, rt_tile_stats* st) {
    float ms = 0.f;
    uint32_t n = 0;
    for (const EventPool::Pair& pr : sc->events.pending()) {
        HIPCHK(hipEventSynchronize(pr.b));
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, pr.a, pr.b));
        ms += t;
        n++;
    }
    sc->events.collected();
    unsigned long long c[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(c, sc->d_counters.get(), sizeof c, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(sc->d_counters.get(), 0, sizeof c));
    if (st) {
        st->ray_segments = c[0];
        st->broad_candidates = c[1];
        st->exact_fallbacks = c[2];
        st->primary_rays = sc->primary_rays;
        st->kernel_ms = ms;
        st->n_launches = n;
        st->h2d_ms = sc->h2d_ms;
        st->d2h_ms = 0.f;
        st->engine = sc->last_engine;
        st->broad_form = sc->last_form;
        st->node_steps = c[3];
    }
    sc->primary_rays = 0;
    sc->h2d_ms = 0.f;
    return RT_OK;
}

// The skeleton of a synchronous host-buffer call on the scene's stream: uploads, the call's launches, downloads, each phase
// timed; the stats are the call's own.  Made under sc->ctx->mu and sc->mu with the device current.  The entry point checks its
// arguments and reserves its staging, then: begin(), upload, uploads_done(), launch_*, kernels_done(), download, finish().
// However it returns, the leased events go back to the scene's pool, the scene's upload time stays for the next tile call, and an error return
// waits for the stream: what is already enqueued writes into caller memory.
struct StagedCall {
    rt_scene* const sc;
    const hipStream_t st;
    const float scene_h2d_ms;
    EventPool::Lease up, down;
    bool finished = false;
    explicit StagedCall(rt_scene* s) : sc(s), st(s->ctx->stream.get()), scene_h2d_ms(s->h2d_ms) {}
    StagedCall(const StagedCall&) = delete;
    ~StagedCall() {
        if (!finished) (void)hipStreamSynchronize(st);
        sc->h2d_ms = scene_h2d_ms;
    }
    // settles anything enqueued earlier; the upload phase begins
    int begin() {
        int rc = collect_locked(sc, nullptr);
        if (rc) return rc;
        HIPCHK(sc->events.lease(up));
        HIPCHK(sc->events.lease(down));
        HIPCHK(hipEventRecord(up.a(), st));
        return RT_OK;
    }
    int uploads_done() {
        HIPCHK(hipEventRecord(up.b(), st));
        return RT_OK;
    }
    int kernels_done() {
        HIPCHK(hipEventRecord(down.a(), st));
        return RT_OK;
    }
    // waits for the downloads; *stats (optional): the call's launches, with its upload and download times
    int finish(rt_tile_stats* stats) {
        HIPCHK(hipEventRecord(down.b(), st));
        HIPCHK(hipEventSynchronize(down.b()));
        finished = true;
        rt_tile_stats s;
        float h2d = 0.f, d2h = 0.f;
        HIPCHK(hipEventElapsedTime(&h2d, up.a(), up.b()));
        HIPCHK(hipEventElapsedTime(&d2h, down.a(), down.b()));
        int rc = collect_locked(sc, &s);
        if (rc) return rc;
        s.h2d_ms = h2d;
        s.d2h_ms = d2h;
        if (stats) *stats = s;
        return RT_OK;
    }
};

// ---- what the caller-ray calls (ray queries, path tracing, path steps, direct lighting, next-event estimation) and the strip calls
// (feature buffers, camera rays, denoiser) share ------------------------------------------------------------------------------------
// A call's part of its launch's verbose line; empty, and nothing formatted, unless RT_VERBOSE is on.
__attribute__((format(printf, 1, 2))) std::string vtext(const char* fmt, ...) {
    if (!dbg(DBG_VERBOSE)) return {};
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

// The scene's materials, and its emitter list, into a parameter block that has the fields.
template <class P>
void material_refs(const rt_scene* sc, P& p) {
    p.mat = sc->d_mat.get();
    p.emis = sc->d_emis.get();
}
template <class P>
void light_refs(const rt_scene* sc, P& p) {
    p.lights = sc->d_lights.get();
    p.n_lights = sc->n_lights;
    p.table.light_c = sc->d_light_c.get();
    p.table.light_ip = sc->d_light_ip.get();
    p.table.light_total = sc->light_total;
}

// RT_FLAG_LIGHTS_BY_POWER picks the kernel instance; it is no business of the plan (rt_plan.h), which never sees an engine in it.
static bool lights_by_power(uint32_t flags) { return (flags & RT_FLAG_LIGHTS_BY_POWER) != 0; }
// ... and so does the scene's light sampling (rt_scene_set_light_sampling)
static bool lights_cone(const rt_scene* sc) { return sc->light_sampling == RT_LIGHTS_CONE; }
// ... and its glossy sampling (rt_scene_set_glossy_sampling), which only RT_NEE_MIS reads
static bool glossy_mis(const rt_scene* sc, const rt_nee_request* rq) { return sc->glossy_sampling == RT_GLOSSY_MIS && rq->mode == RT_NEE_MIS; }

// Enqueue one launch of persistent waves over `items` in workgroups of `block` on `stream` (caller holds sc->mu, device current),
// the block `p` complete.  The launches of the caller-ray calls, the feature buffers and the camera rays all end here.  what: the
// kernel's name in the error of a plan that has none; head, tail: the verbose line on either side of the occupancy (vtext; head up to
// and with its separator); primary: added to the scene's primary rays.  d_zero: a device word zeroed on the stream ahead of the
// launch (a step's *n_next), left alone when there is no slot for the launch.
template <class P>
int launch_persistent(rt_scene* sc, int engine, size_t lds, uint32_t block, void (*kern)(const P), const char* what, const P& p,
                      uint64_t items, const std::string& head, const std::string& tail, uint64_t primary, hipStream_t stream,
                      void* d_zero = nullptr) {
    if (!kern) return fail(RT_ERR_HIP, std::string("no ") + what + " kernel for this plan");
    Grid g;
    int rc = persistent_blocks(sc, kern, block, lds, items, g);
    if (rc || (d_zero && (rc = check_slot(sc)))) return rc;
    if (dbg(DBG_VERBOSE)) fprintf(stderr, "[rt] %sworkgroups/CU %d  %s\n", head.c_str(), g.per_cu, tail.c_str());
    if (d_zero) HIPCHK(hipMemsetAsync(d_zero, 0, sizeof(uint32_t), stream));
    if ((rc = enqueue(sc, stream, kern, g.blocks, block, lds, p))) return rc;
    sc->primary_rays += primary;
    sc->last_engine = (uint32_t)engine;
    sc->last_form = 0;
    return RT_OK;
}

// One caller-ray launch: the scene goes into the block (with the plan's slab test), then launch_persistent with the plan's engine
// and LDS.  Every launch_* of these calls ends here with its own fields filled in.
template <class P>
int launch_rays(rt_scene* sc, const rtplan::QueryPlan& qp, uint32_t block, void (*kern)(const P), const char* what, P& p, uint64_t items,
                const std::string& head, const std::string& tail, uint64_t primary, hipStream_t stream, void* d_zero = nullptr) {
    scene_refs(sc, qp.full_chain, p);
    return launch_persistent(sc, qp.engine, qp.lds, block, kern, what, p, items, head, tail, primary, stream, d_zero);
}

// The frame of a strip call into a parameter block that has the fields (AParams, CParams): the scene's camera, the request's ray
// interval and image size, the job's sample count and the call's first sample.
template <class P>
void frame_refs(const rt_scene* sc, const rt_tile_request& rq, uint32_t begin, P& p) {
    rtplan::fill_camera(rq, sc->has_pose ? &sc->pose : nullptr, p);
    p.t_min = rq.t_min;
    p.t_max = rq.t_max;
    p.W = rq.width;
    p.H = rq.height;
    p.spp_all = rq.spp;
    p.s_begin = begin;
}

// A device form: the scene's lock, the device, the caller's stream or the scene's own, then launch(stream).
template <class L>
int device_form(rt_scene* sc, void* hip_stream, L&& launch) {
    std::lock_guard<std::mutex> lk(sc->mu);
    HIPCHK(hipSetDevice(sc->ctx->dev));
    return launch(hip_stream ? (hipStream_t)hip_stream : sc->ctx->stream.get());
}

// The prologue of a host form: the device's lock and the scene's for the length of the call, and the device made current.
struct HostForm {
    rt_scene* const sc;
    std::lock_guard<std::mutex> dl, lk;
    explicit HostForm(rt_scene* s) : sc(s), dl(s->ctx->mu), lk(s->mu) {}
    int device() const {
        HIPCHK(hipSetDevice(sc->ctx->dev));
        return RT_OK;
    }
};

// The arrays of a host form, in the order they lie in the scene's one staging buffer (rt_scene::d_stage), laid out by
// rtplan::stage_layout.  An entry whose host pointer is NULL is an array the caller did not ask for: it is copied neither way and
// dev() gives nullptr — unless it is DEVICE, memory of the call's own on the device only.
struct Staging {
    enum : unsigned { UP = rtplan::STAGE_UP, DOWN = rtplan::STAGE_DOWN, DEVICE = rtplan::STAGE_DEVICE };
    using Entry = rtplan::StageEntry;     // {host, bytes, copy}
    GrowBuf& buf;
    std::vector<Entry> e;
    const size_t total;
    Staging(rt_scene* sc, std::vector<Entry> entries) : buf(sc->d_stage), e(std::move(entries)), total(rtplan::stage_layout(e.data(), e.size())) {}
    int reserve(const char* what) { return ::reserve(buf, total, what); }
    char* dev(size_t k) const { return e[k].present() ? buf.data() + e[k].off : nullptr; }    // (after reserve)
    // the upload phase of `call`, and its download phase up to finish()
    int upload(StagedCall& call) const {
        for (int k = 0; k < (int)e.size(); k++)
            if (e[k].host && e[k].bytes && (e[k].copy & UP)) HIPCHK(hipMemcpyAsync(dev(k), e[k].host, e[k].bytes, hipMemcpyHostToDevice, call.st));
        return call.uploads_done();
    }
    int download(StagedCall& call) const {
        int rc = call.kernels_done();
        if (rc) return rc;
        for (int k = 0; k < (int)e.size(); k++)
            if (e[k].host && e[k].bytes && (e[k].copy & DOWN))
                HIPCHK(hipMemcpyAsync(const_cast<void*>(e[k].host), dev(k), e[k].bytes, hipMemcpyDeviceToHost, call.st));
        return RT_OK;
    }
};

// The active list of a host form: at most n entries, each below n.
int check_active_list(const uint32_t* active, uint32_t n_active, uint32_t n) {
    if (!active) return RT_OK;
    if (n_active > n) return fail(RT_ERR_BAD_ARG, "n_active > n");
    for (uint32_t k = 0; k < n_active; k++)
        if (active[k] >= n) return fail(RT_ERR_BAD_ARG, "active[" + std::to_string(k) + "] >= n");
    return RT_OK;
}

}  // namespace

// =====================================================================================
extern "C" {

RT_API uint32_t rt_abi_version(void) { return RT_ABI_VERSION; }

RT_API const char* rt_strerror(int status) {
    switch (status) {
        case RT_OK: return "ok";
        case RT_ERR_BAD_ARG: return "bad argument";
        case RT_ERR_NOT_INITIALIZED: return "rt_init() has not succeeded";
        case RT_ERR_NO_DEVICE: return "no HIP device (this library has no CPU fallback)";
        case RT_ERR_BAD_DEVICE: return "device ordinal out of range";
        case RT_ERR_BUFFER_TOO_SMALL: return "output buffer smaller than (height/divisions)*width*3";
        case RT_ERR_FRAME_SIZE: return "height is not a multiple of divisions";
        case RT_ERR_HIP: return "HIP runtime error";
        case RT_ERR_LIMIT: return "limit exceeded";
        case RT_ERR_OOM: return "out of memory";
        default: return "unknown status";
    }
}

RT_API const char* rt_last_error(void) { return g_err.c_str(); }

RT_API void rt_tile_request_defaults(rt_tile_request* rq) {
    if (!rq) return;
    std::memset(rq, 0, sizeof *rq);
    rq->width = 1920;                 // controller main.rs:33-39
    rq->height = 1080;
    rq->divisions = 20;
    rq->division_no = 0;
    rq->spp = 100;                    // slave main.rs:51
    rq->max_bounces = 10;             // main.rs:39
    rq->aperture = 0.1f;              // main.rs:45
    rq->focus_distance = 1.0f;        // main.rs:46
    rq->fov = 3.14159265358979323846f / 2.0f;   // PI / 2f32, main.rs:47
    rq->focal_length = 1.0f;          // main.rs:48
    rq->t_min = 0.001f;               // shapes/mod.rs:12
    rq->t_max = 1000.0f;              // shapes/mod.rs:13
    rq->seed = 0;
    rq->flags = RT_FLAG_NONE;
}

RT_API size_t rt_tile_bytes(const rt_tile_request* rq) {
    return rq ? rtframe::strip_bytes(*rq) : 0;
}

static int rt_init_impl(int* n_devices) {
    dbg_load_env();
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_init) {
        if (n_devices) *n_devices = (int)g_ctx.size();
        return RT_OK;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        if (n_devices) *n_devices = 0;
        return fail(RT_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") +
                                          (e != hipSuccess ? hipGetErrorString(e) : "0 devices"));
    }
    // contexts are created lazily, on the first scene of a device: a rank of a multi-process job touches
    // only its own GPU
    for (int d = 0; d < n; d++) {
        DeviceCtx* c = new DeviceCtx;
        c->dev = d;
        g_ctx.push_back(c);
    }
    g_init = true;
    if (n_devices) *n_devices = n;
    return RT_OK;
}

// Create the device's stream and raise the kernels' dynamic-LDS limit (once per device).
static int ensure_ctx(DeviceCtx* c) {
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->stream) return RT_OK;
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, c->dev));
    for (int isect = 0; isect < rtplan::N_ISECT; isect++)
        for (int alt = 0; alt < 2; alt++)     // the expanded broad phase (ISECT 0, 1) / the node-visit counting twin (ISECT 2 ... 9)
            HIPCHK(hipFuncSetAttribute((const void*)(isect < 2 ? rtk::kernel_linear(isect, alt != 0) : rtk::kernel_traverse(isect, alt != 0)),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)rtplan::LDS_LIMIT));
    for (int isect : {5, 6})                  // ... and the sphere-only instantiations of the LDS-tree kernels
        for (int alt = 0; alt < 2; alt++)
            HIPCHK(hipFuncSetAttribute((const void*)rtk::kernel_traverse(isect, alt != 0, false), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)rtplan::LDS_LIMIT));
    Stream st, cs;                        // (both or neither: the context counts as made by its `stream`)
    HIPCHK(st.create(hipStreamNonBlocking));
    HIPCHK(cs.create(hipStreamNonBlocking));
    c->copy_stream = std::move(cs);
    c->stream = std::move(st);
    return RT_OK;
}

static int rt_shutdown_impl(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_live_scenes.load() > 0)
        return fail(RT_ERR_BAD_ARG, "rt_shutdown() refused: destroy every rt_scene first (their device contexts stay valid)");
    for (DeviceCtx* c : g_ctx) {
        (void)hipSetDevice(c->dev);      // (its streams go with it)
        delete c;
    }
    g_ctx.clear();
    g_init = false;
    return RT_OK;
}

static int rt_scene_destroy_impl(rt_scene* sc);

using rtscene::HostScene;
static_assert(sizeof(rtscene::F4) == sizeof(float4) && alignof(rtscene::F4) == alignof(float4), "HostScene's records are the device's float4");

static int check_world(const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt, const uint32_t* world_index) {
    if ((ns && !sp) || (nt && !tr)) return fail(RT_ERR_BAD_ARG, "primitive pointer is NULL");
    // the kernels address nodes (64 B), geometry (16 B), materials (16 B) and triangles (36 B) with 32-bit byte offsets
    if ((uint64_t)ns + nt > RT_MAX_PRIMITIVES) return fail(RT_ERR_LIMIT, "too many primitives (RT_MAX_PRIMITIVES)");
    if (world_index && !rtscene::world_is_permutation(world_index, ns + nt))
        return fail(RT_ERR_BAD_ARG, "world_index is not a permutation of 0 .. n_spheres + n_triangles - 1");
    return RT_OK;
}

// HostScene -> device: allocate, upload on the device's stream, hand back the handle
static int upload_scene(int device, const HostScene& hs, rt_scene** out) {
    const auto t_create0 = std::chrono::steady_clock::now();
    if (!g_init) return fail(RT_ERR_NOT_INITIALIZED, "call rt_init() first");
    if (device < 0 || device >= (int)g_ctx.size()) return fail(RT_ERR_BAD_DEVICE, "bad device ordinal");
    DeviceCtx* ctx = g_ctx[device];
    {
        int rc0 = ensure_ctx(ctx);
        if (rc0) return rc0;
    }
    HIPCHK(hipSetDevice(ctx->dev));
    struct Destroy {
        void operator()(rt_scene* s) const { rt_scene_destroy_impl(s); }
    };
    std::unique_ptr<rt_scene, Destroy> sc(new (std::nothrow) rt_scene);      // an error return or an exception below releases everything made so far
    if (!sc) return fail(RT_ERR_OOM, "host allocation failed");
    g_live_scenes.fetch_add(1);            // (rt_scene_destroy_impl takes it back)
    const rtbvh::FlatBVH& bvh = hs.bvh;
    sc->ctx = ctx;
    sc->shape = hs.shape;
    sc->bvh_build_ms = hs.bvh_build_ms;
    sc->grid = bvh.grid;
    sc->has_order = hs.has_order;
    sc->n_lights = hs.n_lights;
    sc->light_total = hs.light_total;
    sc->light_p.assign(hs.light_p.begin(), hs.light_p.begin() + hs.n_lights);
    sc->light_world.resize(hs.n_lights);
    for (uint32_t k = 0; k < hs.n_lights; k++) sc->light_world[k] = hs.has_order ? hs.world_rank[hs.lights[k]] : hs.lights[k];
    sc->n_big = hs.n_big;
    sc->tri_k = hs.tri_k;
    sc->tri_diag = hs.tri_diag;
    sc->tri_es = hs.tri_es;
    sc->tri_e = hs.tri_e;
    const hipStream_t st = ctx->stream.get();
    Event e0, e1;
    if (e0.create() != hipSuccess || e1.create() != hipSuccess) return fail(RT_ERR_HIP, "hipEventCreate failed");
    // The steps of the upload, in order; after the first that fails the rest are skipped.  Out of memory is its own status, and the
    // text names the array or the call.
    int rc = RT_OK;
    auto step = [&](hipError_t e, const char* what) {
        if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, std::string("scene upload, ") + what + ": " + hipGetErrorString(e));
    };
    auto up = [&](auto& dst, const auto& vec, const char* what) {
        if (!rc) step(dst.upload(vec, st), what);
    };
    step(hipEventRecord(e0.get(), st), "hipEventRecord");
    up(sc->d_geom, hs.geom, "geom");
    up(sc->d_geom_pk, hs.geom_pk, "geom_pk");
    up(sc->d_geom_px, hs.geom_px, "geom_px");
    up(sc->d_mat, hs.mat, "mat");
    up(sc->d_emis, hs.emis, "emis");
    up(sc->d_tri, hs.tri, "tri");
    up(sc->d_tri_box, hs.tri_box, "tri_box");
    up(sc->d_bvh, bvh.nodes, "bvh nodes");
    up(sc->d_leaf_of, bvh.leaf_of, "leaf_of");
    up(sc->d_world_rank, hs.world_rank, "world_rank");
    up(sc->d_trav, bvh.trav, "trav");
    up(sc->d_travq, bvh.travq, "travq");
    up(sc->d_geom_r, hs.geom_r, "geom_r");
    up(sc->d_big, hs.big, "big");
    up(sc->d_lights, hs.lights, "lights");
    up(sc->d_light_c, hs.light_c, "light_c");
    up(sc->d_light_ip, hs.light_ip_prim, "light_ip");
    if (!rc) step(sc->d_counters.alloc(COUNTER_WORDS), "counters");
    if (!rc) step(hipMemsetAsync(sc->d_counters.get(), 0, COUNTER_WORDS * sizeof(unsigned long long), st), "hipMemsetAsync(counters)");
    if (!rc) step(hipEventRecord(e1.get(), st), "hipEventRecord");
    if (!rc) step(hipEventSynchronize(e1.get()), "hipEventSynchronize");
    if (!rc) step(hipEventElapsedTime(&sc->h2d_ms, e0.get(), e1.get()), "hipEventElapsedTime");
    if (rc) return rc;
    if (dbg(DBG_VERBOSE))
        fprintf(stderr, "[rt] scene: %u prims  culled walk: %u big spheres, slack radius %g, box density %.3f -> %s  bvh build %.2f ms (host)  uploads %.2f ms  upload total %.2f ms\n",
                hs.shape.n_sph + hs.shape.n_tri, hs.n_big, hs.shape.r_slack, hs.shape.cull_density, hs.shape.cull_pays ? "default" : "off", sc->bvh_build_ms, sc->h2d_ms,
                std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_create0).count());
    *out = sc.release();
    return RT_OK;
}

static int rt_scene_create_impl(int device, const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt,
                                const uint32_t* world_index, rt_scene** out) {
    if (!out) return fail(RT_ERR_BAD_ARG, "out_scene is NULL");
    *out = nullptr;
    int rc = check_world(sp, ns, tr, nt, world_index);
    if (rc) return rc;
    if (!g_init) return fail(RT_ERR_NOT_INITIALIZED, "call rt_init() first");
    if (device < 0 || device >= (int)g_ctx.size()) return fail(RT_ERR_BAD_DEVICE, "bad device ordinal");
    HostScene hs;
    rtscene::build_host_scene(sp, ns, tr, nt, world_index, dbg(DBG_REORDER) != 0, hs);
    return upload_scene(device, hs, out);
}

// The scene's device is made current BEFORE `delete`: the members free their device memory and destroy their events in their
// destructors, on whichever thread this runs (a caller's, or a frame context's dispatcher).
static int rt_scene_destroy_impl(rt_scene* sc) {
    if (!sc) return RT_OK;
    if (sc->ctx) (void)hipSetDevice(sc->ctx->dev);
    for (const EventPool::Pair& pr : sc->events.pending()) (void)hipEventSynchronize(pr.b);
    delete sc;
    g_live_scenes.fetch_sub(1);
    return RT_OK;
}

static int check_batch(const rt_tile_request* rqs, uint32_t n) {
    if (!rqs || n == 0) return fail(RT_ERR_BAD_ARG, "empty request batch");
    for (uint32_t i = 0; i < n; i++) {
        int rc = check_request(&rqs[i]);
        if (rc) return rc;
        if (!rtframe::same_frame(rqs[0], rqs[i]))
            return fail(RT_ERR_BAD_ARG, "batched requests must agree on every field but division_no and seed");
    }
    return RT_OK;
}

// a sample range of a request: 0 <= begin < end <= spp
static int check_samples(uint32_t begin, uint32_t end, uint32_t spp) {
    if (begin >= end) return fail(RT_ERR_BAD_ARG, "sample_begin >= sample_end");
    if (end > spp) return fail(RT_ERR_BAD_ARG, "sample_end > spp");
    return RT_OK;
}

// a required array of n non-NULL entries
static int check_array(const void* const* a, uint32_t n, const char* what) {
    if (!a) return fail(RT_ERR_BAD_ARG, std::string(what) + " is NULL");
    for (uint32_t i = 0; i < n; i++)
        if (!a[i]) return fail(RT_ERR_BAD_ARG, std::string(what) + "[i] is NULL");
    return RT_OK;
}

// a progressive pass's own arguments (after check_batch): its sample range, a running sum per strip
static int check_pass(const rt_tile_request* rqs, uint32_t n, const Pass& pass) {
    int rc = check_samples(pass.begin, pass.end, rqs[0].spp);
    return rc ? rc : check_array(pass.d_acc, n, "accum");
}

// pass: nullptr, or a progressive pass whose d_acc holds one device sum per request (checked here)
static int rt_scene_render_tiles_device_impl(rt_scene* sc, const rt_tile_request* rqs, uint32_t n,
                                        void* const* d_out_rgb, size_t out_len_each, void* const* d_out_f32,
                                        void* hip_stream, const Pass* pass = nullptr) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    int rc = check_batch(rqs, n);
    if (rc) return rc;
    if ((rc = check_array(d_out_rgb, n, "d_out_rgb"))) return rc;
    if (out_len_each < rt_tile_bytes(&rqs[0])) return fail(RT_ERR_BUFFER_TOO_SMALL, "out_len < (H/div)*W*3");
    if (pass && (rc = check_pass(rqs, n, *pass))) return rc;
    return device_form(sc, hip_stream, [&](hipStream_t st) -> int {
        for (uint32_t i0 = 0; i0 < n; i0 += rtk::MAX_BATCH) {
            uint32_t m = std::min<uint32_t>(rtk::MAX_BATCH, n - i0);
            Pass part = {};
            if (pass) part = {pass->begin, pass->end, pass->d_acc + i0};
            int rc = launch_batch(sc, rqs + i0, m, d_out_rgb + i0, d_out_f32 ? d_out_f32 + i0 : nullptr, st, nullptr, pass ? &part : nullptr);
            if (rc) return rc;
        }
        return RT_OK;
    });
}

static int rt_scene_render_tile_device_impl(rt_scene* sc, const rt_tile_request* rq, void* d_out_rgb, size_t out_len,
                                       void* d_out_f32, void* hip_stream) {
    void* rgb[1] = {d_out_rgb};
    void* f32[1] = {d_out_f32};
    return rt_scene_render_tiles_device_impl(sc, rq, 1, rgb, out_len, d_out_f32 ? f32 : nullptr, hip_stream);
}

static int rt_scene_collect_impl(rt_scene* sc, rt_tile_stats* st) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    std::lock_guard<std::mutex> lk(sc->mu);
    HIPCHK(hipSetDevice(sc->ctx->dev));
    return collect_locked(sc, st);
}

// strip_cost_out: optional host array of n counters: the ray segments of every strip (frame context)
// pass: nullptr, or a progressive pass whose d_acc holds one HOST sum (float*) per request: uploaded before the launch when the pass
// continues one (begin > 0), downloaded with the strips
static int rt_scene_render_tiles_impl(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, uint8_t* const* out_rgb,
                                 size_t out_len_each, float* const* out_f32, rt_tile_stats* stats,
                                 unsigned long long* strip_cost_out = nullptr, const Pass* pass = nullptr) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    int rc = check_batch(rqs, n);
    if (rc) return rc;
    if ((rc = check_array((const void* const*)out_rgb, n, "out_rgb"))) return rc;
    const size_t need = rt_tile_bytes(&rqs[0]);
    if (out_len_each < need) return fail(RT_ERR_BUFFER_TOO_SMALL, "out_len < (H/div)*W*3");
    if (pass && (rc = check_pass(rqs, n, *pass))) return rc;
    bool want_f32 = false;
    if (out_f32)
        for (uint32_t i = 0; i < n; i++) want_f32 |= out_f32[i] != nullptr;
    HostForm hf(sc);
    hipStream_t st = sc->ctx->stream.get();
    if ((rc = hf.device()) || (rc = reserve(sc->d_out, need * n, "strips")) || (want_f32 && (rc = reserve(sc->d_outf, need * n * sizeof(float), "strips f32"))) ||
        (pass && (rc = reserve(sc->d_acc, need * n * sizeof(float), "running sums"))))
        return rc;
    // Launch groups [first, count): the last quarter of the strips as its own launch when the downloads are worth hiding, so that the
    // D2H copies of the strips before it (copy stream) run under it and only the last group's copies are exposed (d2h_ms = that part).
    const std::vector<std::pair<uint32_t, uint32_t>> groups = rtframe::launch_groups(n, need);
    // per-strip costs: one block of COST_COPIES x MAX_BATCH counters per launch group of the call
    constexpr size_t COST_BLOCK = rtframe::COST_BLOCK;
    unsigned long long* d_cost = nullptr;
    if (strip_cost_out) {
        const size_t cost_b = groups.size() * COST_BLOCK * sizeof(unsigned long long);
        if ((rc = reserve(sc->d_cost, cost_b, "strip costs"))) return rc;
        d_cost = (unsigned long long*)sc->d_cost.data();
        HIPCHK(hipMemsetAsync(d_cost, 0, cost_b, st));
    }
    // settle anything enqueued earlier so the stats of this call are its own
    rt_tile_stats prev;
    rc = collect_locked(sc, &prev);
    if (rc) return rc;
    sc->h2d_ms = prev.h2d_ms;
    std::vector<void*> drgb(n), df32(n), dacc(pass ? n : 0);
    for (uint32_t i = 0; i < n; i++) {
        drgb[i] = sc->d_out.data() + need * i;
        df32[i] = (want_f32 && out_f32[i]) ? sc->d_outf.data() + need * i * sizeof(float) : nullptr;
        if (pass) dacc[i] = sc->d_acc.data() + need * i * sizeof(float);
    }
    hipStream_t cs = sc->ctx->copy_stream.get();
    std::vector<EventPool::Lease> gev(groups.size());      // (back to the scene's pool however the call returns, after the wait below)
    // an error return waits for the work already enqueued: it writes into caller memory
    struct WaitOnError {
        hipStream_t a, b;
        bool ok = false;
        ~WaitOnError() {
            if (!ok) {
                (void)hipStreamSynchronize(a);
                (void)hipStreamSynchronize(b);
            }
        }
    } wait{st, cs};
    for (EventPool::Lease& e : gev) HIPCHK(sc->events.lease(e));
    if (pass && pass->begin > 0)            // (a pass from sample 0 reads no sum: the caller's buffer may be uninitialised)
        for (uint32_t i = 0; i < n; i++)
            HIPCHK(hipMemcpyAsync(dacc[i], pass->d_acc[i], need * sizeof(float), hipMemcpyHostToDevice, st));
    for (size_t g = 0; g < groups.size(); g++) {
        const uint32_t i0 = groups[g].first, m = groups[g].second;
        Pass part = {};
        if (pass) part = {pass->begin, pass->end, dacc.data() + i0};
        rc = launch_batch(sc, rqs + i0, m, drgb.data() + i0, want_f32 ? df32.data() + i0 : nullptr, st,
                          d_cost ? d_cost + g * COST_BLOCK : nullptr, pass ? &part : nullptr);
        if (rc) return rc;
        HIPCHK(hipEventRecord(gev[g].a(), st));
    }
    for (size_t g = 0; g < groups.size(); g++) {
        HIPCHK(hipStreamWaitEvent(cs, gev[g].a(), 0));
        for (uint32_t i = groups[g].first; i < groups[g].first + groups[g].second; i++) {
            HIPCHK(hipMemcpyAsync(out_rgb[i], drgb[i], need, hipMemcpyDeviceToHost, cs));
            if (df32[i]) HIPCHK(hipMemcpyAsync(out_f32[i], df32[i], need * sizeof(float), hipMemcpyDeviceToHost, cs));
            if (pass) HIPCHK(hipMemcpyAsync(pass->d_acc[i], dacc[i], need * sizeof(float), hipMemcpyDeviceToHost, cs));
        }
    }
    std::vector<unsigned long long> cost_raw;
    if (strip_cost_out) {
        cost_raw.resize(groups.size() * COST_BLOCK);
        HIPCHK(hipMemcpyAsync(cost_raw.data(), d_cost, cost_raw.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, cs));
    }
    HIPCHK(hipEventRecord(gev.back().b(), cs));
    HIPCHK(hipEventSynchronize(gev.back().b()));
    if (strip_cost_out) rtframe::fold_strip_costs(cost_raw.data(), groups, strip_cost_out);
    float d2h = 0.f;
    HIPCHK(hipEventElapsedTime(&d2h, gev.back().a(), gev.back().b()));   // last launch done -> last byte on the host
    wait.ok = true;
    rt_tile_stats s;
    rc = collect_locked(sc, &s);
    if (rc) return rc;
    s.d2h_ms = d2h;
    if (stats) *stats = s;
    return RT_OK;
}

static int rt_scene_render_tile_impl(rt_scene* sc, const rt_tile_request* rq, uint8_t* out_rgb, size_t out_len,
                                float* out_f32, rt_tile_stats* stats) {
    uint8_t* rgb[1] = {out_rgb};
    float* f32[1] = {out_f32};
    return rt_scene_render_tiles_impl(sc, rq, 1, rgb, out_len, out_f32 ? f32 : nullptr, stats);
}

static int rt_scene_render_tile_pass_impl(rt_scene* sc, const rt_tile_request* rq, uint32_t begin, uint32_t end, float* accum,
                                          uint8_t* out_rgb, size_t out_len, float* out_f32, rt_tile_stats* stats) {
    uint8_t* rgb[1] = {out_rgb};
    float* f32[1] = {out_f32};
    void* acc[1] = {accum};
    const Pass pass = {begin, end, acc};
    return rt_scene_render_tiles_impl(sc, rq, 1, rgb, out_len, out_f32 ? f32 : nullptr, stats, nullptr, &pass);
}

static int rt_scene_render_tiles_pass_device_impl(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, uint32_t begin, uint32_t end,
                                                  void* const* d_accum, void* const* d_out_rgb, size_t out_len_each,
                                                  void* const* d_out_f32, void* hip_stream) {
    const Pass pass = {begin, end, d_accum};
    return rt_scene_render_tiles_device_impl(sc, rqs, n, d_out_rgb, out_len_each, d_out_f32, hip_stream, &pass);
}

// ---- ray queries (rt_tile.h "ray queries", rt_query.hip.h) ---------------------------------------------------------------------
static int check_query(rt_scene* sc, const void* rays, uint32_t n, uint32_t mode, const void* hits) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    if (!rays || !hits) return fail(RT_ERR_BAD_ARG, "rays or hits is NULL");
    if (n == 0) return fail(RT_ERR_BAD_ARG, "n == 0");
    if (mode > RT_QUERY_ANY) return fail(RT_ERR_BAD_ARG, "mode is neither RT_QUERY_CLOSEST nor RT_QUERY_ANY");
    return RT_OK;
}

// Enqueue one query launch on `stream` (caller holds sc->mu, device current): persistent waves over the n rays.
static int launch_query(rt_scene* sc, const void* d_rays, uint32_t n, uint32_t mode, uint32_t flags, void* d_hits, hipStream_t stream) {
    const rtplan::QueryPlan qp = rtplan::plan_query(sc->shape, flags);
    rtk::QParams p;
    std::memset(&p, 0, sizeof p);
    p.rays = (const float4*)d_rays;
    p.hits = (uint4*)d_hits;
    p.n = n;
    return launch_rays(sc, qp, rtplan::QUERY_BLOCK, rtk::query_kernel(qp.engine, qp.scan_mode, mode == RT_QUERY_ANY), "query", p, n,
                       vtext("query: engine %d  scan mode %d  %s  lds %zu B  ", qp.engine, qp.scan_mode,
                             mode == RT_QUERY_ANY ? "any" : "closest", qp.lds),
                       vtext("rays %u", n), n, stream);
}

static int rt_scene_intersect_device_impl(rt_scene* sc, const void* d_rays, uint32_t n, uint32_t mode, uint32_t flags, void* d_hits,
                                          void* hip_stream) {
    int rc = check_query(sc, d_rays, n, mode, d_hits);
    if (rc) return rc;
    return device_form(sc, hip_stream, [&](hipStream_t st) { return launch_query(sc, d_rays, n, mode, flags, d_hits, st); });
}

static int rt_scene_intersect_impl(rt_scene* sc, const rt_ray* rays, uint32_t n, uint32_t mode, uint32_t flags, rt_hit* hits,
                                   rt_tile_stats* stats) {
    int rc = check_query(sc, rays, n, mode, hits);
    if (rc) return rc;
    HostForm hf(sc);
    Staging s(sc, {{rays, (size_t)n * sizeof(rt_ray), Staging::UP}, {hits, (size_t)n * sizeof(rt_hit), Staging::DOWN}});
    StagedCall call(sc);
    if ((rc = hf.device()) || (rc = s.reserve("rays / hits")) || (rc = call.begin()) || (rc = s.upload(call)) ||
        (rc = launch_query(sc, s.dev(0), n, mode, flags, s.dev(1), call.st)) || (rc = s.download(call)))
        return rc;
    return call.finish(stats);
}

// ---- path tracing of caller rays (rt_tile.h "path tracing of caller rays", rt_trace.hip.h) ---------------------------------------
static int check_trace(rt_scene* sc, const rt_trace_request* rq, const void* rays, uint32_t n, const void* rgb) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    if (!rq) return fail(RT_ERR_BAD_ARG, "request is NULL");
    if (!rays || !rgb) return fail(RT_ERR_BAD_ARG, "rays or out_rgb is NULL");
    if (n == 0) return fail(RT_ERR_BAD_ARG, "n == 0");
    if (rq->spp == 0) return fail(RT_ERR_BAD_ARG, "spp == 0");
    if (rq->ray_form > RT_TRACE_RAY_AS_GIVEN) return fail(RT_ERR_BAD_ARG, "ray_form is neither RT_TRACE_RAY_NEW nor RT_TRACE_RAY_AS_GIVEN");
    if (rq->spp > RT_MAX_SPP) return fail(RT_ERR_LIMIT, "spp > RT_MAX_SPP");
    if (rq->max_bounces > RT_MAX_BOUNCES) return fail(RT_ERR_LIMIT, "max_bounces > RT_MAX_BOUNCES");
    return RT_OK;
}

// Enqueue one trace launch on `stream` (caller holds sc->mu, device current): persistent waves over the n rays.
static int launch_trace(rt_scene* sc, const rt_trace_request* rq, const void* d_rays, uint32_t n, void* d_state, void* d_rgb,
                        void* d_segs, hipStream_t stream) {
    const rtplan::TracePlan tp = rtplan::plan_trace(sc->shape, rq->flags, rq->max_bounces);
    rtk::TParams p;
    std::memset(&p, 0, sizeof p);
    p.rays = (const float4*)d_rays;
    p.rgb = (float*)d_rgb;
    p.segments = (uint32_t*)d_segs;
    p.rng_state = (uint64_t*)d_state;
    p.n = n;
    p.seed = rq->seed;
    p.spp = rq->spp;
    p.depth = rq->max_bounces + 1;
    p.as_given = rq->ray_form == RT_TRACE_RAY_AS_GIVEN ? 1u : 0u;
    p.path32 = tp.path32 ? 1u : 0u;
    p.lds_path_off = (uint32_t)tp.lds_path_off;
    material_refs(sc, p);
    return launch_rays(sc, rtplan::QueryPlan{tp.engine, tp.scan_mode, tp.full_chain, tp.lds}, tp.block,
                       rtk::trace_kernel(tp.engine, tp.scan_mode), "trace", p, n,
                       vtext("trace: engine %d  scan mode %d  block %u  lds %zu B (path %s)  ", tp.engine, tp.scan_mode, tp.block, tp.lds,
                             tp.path32 ? "u32" : "u16"),
                       vtext("rays %u  spp %u  bounces %u", n, rq->spp, rq->max_bounces), (uint64_t)n * rq->spp, stream);
}

static int rt_scene_trace_device_impl(rt_scene* sc, const rt_trace_request* rq, const void* d_rays, uint32_t n, void* d_state,
                                      void* d_rgb, void* d_segs, void* hip_stream) {
    int rc = check_trace(sc, rq, d_rays, n, d_rgb);
    if (rc) return rc;
    return device_form(sc, hip_stream, [&](hipStream_t st) { return launch_trace(sc, rq, d_rays, n, d_state, d_rgb, d_segs, st); });
}

static int rt_scene_trace_impl(rt_scene* sc, const rt_trace_request* rq, const rt_ray* rays, uint32_t n, uint64_t* rng_state,
                               float* rgb, uint32_t* segs, rt_tile_stats* stats) {
    int rc = check_trace(sc, rq, rays, n, rgb);
    if (rc) return rc;
    HostForm hf(sc);
    Staging s(sc, {{rays, (size_t)n * sizeof(rt_ray), Staging::UP},
                   {rng_state, (size_t)n * 4 * sizeof(uint64_t), Staging::UP | Staging::DOWN},
                   {rgb, (size_t)n * 3 * sizeof(float), Staging::DOWN},
                   {segs, (size_t)n * sizeof(uint32_t), Staging::DOWN}});
    StagedCall call(sc);
    if ((rc = hf.device()) || (rc = s.reserve("trace buffers")) || (rc = call.begin()) || (rc = s.upload(call)) ||
        (rc = launch_trace(sc, rq, s.dev(0), n, s.dev(1), s.dev(2), s.dev(3), call.st)) || (rc = s.download(call)))
        return rc;
    return call.finish(stats);
}

// ---- path steps of caller rays (rt_tile.h "path steps", rt_bounce.hip.h) ----------------------------------------------------------
static int check_bounce(rt_scene* sc, const rt_bounce_request* rq, const void* rays, uint32_t n, const void* state, const void* active,
                        const void* n_active, const void* bounce, const void* next_active, const void* n_next) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    if (!rq) return fail(RT_ERR_BAD_ARG, "request is NULL");
    if (!rays || !state || !bounce) return fail(RT_ERR_BAD_ARG, "rays, rng_state or out_bounce is NULL");
    if (n == 0) return fail(RT_ERR_BAD_ARG, "n == 0");
    if (rq->ray_form > RT_TRACE_RAY_AS_GIVEN) return fail(RT_ERR_BAD_ARG, "ray_form is neither RT_TRACE_RAY_NEW nor RT_TRACE_RAY_AS_GIVEN");
    if (rq->seed_states > 1) return fail(RT_ERR_BAD_ARG, "seed_states is neither 0 nor 1");
    if (rq->reserved != 0) return fail(RT_ERR_BAD_ARG, "reserved must be 0");
    if (next_active && !n_next) return fail(RT_ERR_BAD_ARG, "next_active without n_next");
    if ((active != nullptr) != (n_active != nullptr)) return fail(RT_ERR_BAD_ARG, "active and n_active: both or neither");
    return RT_OK;
}

// Enqueue one step on `stream` (caller holds sc->mu, device current): *d_n_next zeroed, then persistent waves over the `count` entries
// of the active list (d_active == nullptr: rays 0 .. count - 1), of which the kernel takes the first *d_n_active when that is given.
static int launch_bounce(rt_scene* sc, const rt_bounce_request* rq, void* d_rays, uint32_t n, void* d_state, const void* d_active,
                         uint32_t count, const void* d_n_active, void* d_bounce, void* d_hits, void* d_next, void* d_n_next,
                         hipStream_t stream) {
    const rtplan::QueryPlan qp = rtplan::plan_query(sc->shape, rq->flags);
    rtk::BParams p;
    std::memset(&p, 0, sizeof p);
    p.rays = (float4*)d_rays;
    p.rng_state = (uint64_t*)d_state;
    p.active = (const uint32_t*)d_active;
    p.n_active = (const uint32_t*)d_n_active;
    p.bounce = (uint4*)d_bounce;
    p.hits = (uint4*)d_hits;
    p.next_active = (uint32_t*)d_next;
    p.n_next = (uint32_t*)d_n_next;
    p.n = n;
    p.count = count;
    p.seed = rq->seed;
    p.as_given = rq->ray_form == RT_TRACE_RAY_AS_GIVEN ? 1u : 0u;
    p.seed_states = rq->seed_states;
    material_refs(sc, p);
    return launch_rays(sc, qp, rtplan::QUERY_BLOCK, rtk::bounce_kernel(qp.engine, qp.scan_mode), "bounce", p, std::max<uint32_t>(count, 1u),
                       vtext("bounce: engine %d  scan mode %d  lds %zu B  ", qp.engine, qp.scan_mode, qp.lds),
                       vtext("rays %u  listed %s%u", n, d_n_active ? "<= " : "", count), 0, stream, d_n_next);
}

static int rt_scene_bounce_device_impl(rt_scene* sc, const rt_bounce_request* rq, void* d_rays, uint32_t n, void* d_state,
                                       const void* d_active, const void* d_n_active, void* d_bounce, void* d_hits, void* d_next,
                                       void* d_n_next, void* hip_stream) {
    int rc = check_bounce(sc, rq, d_rays, n, d_state, d_active, d_n_active, d_bounce, d_next, d_n_next);
    if (rc) return rc;
    return device_form(sc, hip_stream, [&](hipStream_t st) {
        return launch_bounce(sc, rq, d_rays, n, d_state, d_active, n, d_n_active, d_bounce, d_hits, d_next, d_n_next, st);
    });
}

static int rt_scene_bounce_impl(rt_scene* sc, const rt_bounce_request* rq, rt_ray* rays, uint32_t n, uint64_t* rng_state,
                                const uint32_t* active, uint32_t n_active, rt_bounce* bounce, rt_hit* hits, uint32_t* next_active,
                                uint32_t* n_next, rt_tile_stats* stats) {
    // (the host form's n_active is a value: the both-or-neither rule is the device form's)
    int rc = check_bounce(sc, rq, rays, n, rng_state, nullptr, nullptr, bounce, next_active, n_next);
    if (rc || (rc = check_active_list(active, n_active, n))) return rc;
    const uint32_t count = active ? n_active : n;
    HostForm hf(sc);
    // records of rays that are not listed come back as they went in: the caller's bytes are the staging's initial contents
    const unsigned listed = active ? Staging::UP : 0;
    enum { RAYS, STATE, HITS, BOUNCE, ACTIVE, NEXT, N_NEXT };
    Staging s(sc, {{rays, (size_t)n * sizeof(rt_ray), Staging::UP | Staging::DOWN},
                   {rng_state, (size_t)n * 4 * sizeof(uint64_t), Staging::UP | Staging::DOWN},
                   {hits, (size_t)n * sizeof(rt_hit), listed | Staging::DOWN},
                   {bounce, (size_t)n * sizeof(rt_bounce), listed | Staging::DOWN},
                   {active, (size_t)count * sizeof(uint32_t), Staging::UP},
                   {next_active, (size_t)n * sizeof(uint32_t), 0},      // (downloaded below)
                   {n_next, sizeof(uint32_t), Staging::DOWN}});
    StagedCall call(sc);
    if ((rc = hf.device()) || (rc = s.reserve("bounce buffers")) || (rc = call.begin()) || (rc = s.upload(call)) ||
        (rc = launch_bounce(sc, rq, s.dev(RAYS), n, s.dev(STATE), s.dev(ACTIVE), count, nullptr, s.dev(BOUNCE), s.dev(HITS), s.dev(NEXT),
                            s.dev(N_NEXT), call.st)) ||
        (rc = s.download(call)))
        return rc;
    if (next_active) {                                     // (the list's length is known only now)
        HIPCHK(hipStreamSynchronize(call.st));
        const size_t next_b = (size_t)std::min(*n_next, n) * sizeof(uint32_t);
        if (next_b) HIPCHK(hipMemcpyAsync(next_active, s.dev(NEXT), next_b, hipMemcpyDeviceToHost, call.st));
    }
    return call.finish(stats);
}

// ---- direct lighting of caller rays (rt_tile.h "direct lighting", rt_direct.hip.h) ------------------------------------------------
static int check_direct(rt_scene* sc, const rt_direct_request* rq, const void* hits, uint32_t n, const void* state, const void* active,
                        const void* n_active, const void* out) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    if (!rq) return fail(RT_ERR_BAD_ARG, "request is NULL");
    if (!hits || !state || !out) return fail(RT_ERR_BAD_ARG, "hits, rng_state or out is NULL");
    if (n == 0) return fail(RT_ERR_BAD_ARG, "n == 0");
    if (rq->reserved != 0) return fail(RT_ERR_BAD_ARG, "reserved must be 0");
    if ((active != nullptr) != (n_active != nullptr)) return fail(RT_ERR_BAD_ARG, "active and n_active: both or neither");
    return RT_OK;
}

// Enqueue one launch on `stream` (caller holds sc->mu, device current): persistent waves over the `count` entries of the active list
// (d_active == nullptr: records 0 .. count - 1), of which the kernel takes the first *d_n_active when that is given.
static int launch_direct(rt_scene* sc, const rt_direct_request* rq, const void* d_hits, uint32_t n, void* d_state, const void* d_active,
                         uint32_t count, const void* d_n_active, void* d_out, hipStream_t stream) {
    const rtplan::DirectPlan dp = rtplan::plan_direct(sc->shape, sc->n_lights, rq->flags);
    if (dp.too_many) return fail(RT_ERR_LIMIT, "more than 2^23 emitters");
    const rtplan::QueryPlan& qp = dp.query;
    rtk::DParams p;
    std::memset(&p, 0, sizeof p);
    p.hits = (const uint4*)d_hits;
    p.rng_state = (uint64_t*)d_state;
    p.active = (const uint32_t*)d_active;
    p.n_active = (const uint32_t*)d_n_active;
    p.out = (uint4*)d_out;
    p.n = n;
    p.count = count;
    material_refs(sc, p);
    light_refs(sc, p);
    p.t_min = rq->t_min;
    p.t_max = rq->t_max;
    return launch_rays(sc, qp, rtplan::QUERY_BLOCK, rtk::direct_kernel(qp.engine, qp.scan_mode, lights_by_power(rq->flags), lights_cone(sc)), "direct-lighting", p,
                       std::max<uint32_t>(count, 1u),
                       vtext("direct: engine %d  scan mode %d  lds %zu B  ", qp.engine, qp.scan_mode, qp.lds),
                       vtext("records %u  listed %s%u  lights %u%s%s", n, d_n_active ? "<= " : "", count, sc->n_lights,
                             lights_by_power(rq->flags) ? " by power" : "", lights_cone(sc) ? " cone" : ""),
                       0, stream);
}

static int rt_scene_light_count_impl(rt_scene* sc, uint32_t* n_lights) {
    if (!sc || !n_lights) return fail(RT_ERR_BAD_ARG, "scene or n_lights is NULL");
    *n_lights = sc->n_lights;
    return RT_OK;
}

// Host-only: the scene's own copy of the table, no device work, no synchronisation.
static int rt_scene_light_table_impl(rt_scene* sc, uint32_t flags, uint32_t* out_world_index, float* out_p, uint32_t capacity) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    const uint32_t M = sc->n_lights;
    if (capacity < M) return fail(RT_ERR_BAD_ARG, "capacity < rt_scene_light_count()");
    for (uint32_t k = 0; k < M; k++) {
        if (out_world_index) out_world_index[k] = sc->light_world[k];
        if (out_p) out_p[k] = lights_by_power(flags) ? sc->light_p[k] : 1.0f / (float)M;
    }
    return RT_OK;
}

// How the scene's sphere lights are sampled by the calls enqueued from now on; work already enqueued keeps its kernel instance.
static int rt_scene_set_light_sampling_impl(rt_scene* sc, uint32_t sampling) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    if (sampling > RT_LIGHTS_CONE) return fail(RT_ERR_BAD_ARG, "sampling is neither RT_LIGHTS_AREA nor RT_LIGHTS_CONE");
    std::lock_guard<std::mutex> lk(sc->mu);
    sc->light_sampling = sampling;
    return RT_OK;
}

static int rt_scene_light_sampling_impl(rt_scene* sc, uint32_t* out_sampling) {
    if (!sc || !out_sampling) return fail(RT_ERR_BAD_ARG, "scene or out_sampling is NULL");
    std::lock_guard<std::mutex> lk(sc->mu);
    *out_sampling = sc->light_sampling;
    return RT_OK;
}

// Whether RT_NEE_MIS takes light samples at glossy hits, for the calls enqueued from now on.
static int rt_scene_set_glossy_sampling_impl(rt_scene* sc, uint32_t sampling) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    if (sampling > RT_GLOSSY_MIS) return fail(RT_ERR_BAD_ARG, "sampling is neither RT_GLOSSY_BOUNCE nor RT_GLOSSY_MIS");
    std::lock_guard<std::mutex> lk(sc->mu);
    sc->glossy_sampling = sampling;
    return RT_OK;
}

static int rt_scene_glossy_sampling_impl(rt_scene* sc, uint32_t* out_sampling) {
    if (!sc || !out_sampling) return fail(RT_ERR_BAD_ARG, "scene or out_sampling is NULL");
    std::lock_guard<std::mutex> lk(sc->mu);
    *out_sampling = sc->glossy_sampling;
    return RT_OK;
}

static int rt_scene_direct_device_impl(rt_scene* sc, const rt_direct_request* rq, const void* d_hits, uint32_t n, void* d_state,
                                       const void* d_active, const void* d_n_active, void* d_out, void* hip_stream) {
    int rc = check_direct(sc, rq, d_hits, n, d_state, d_active, d_n_active, d_out);
    if (rc) return rc;
    return device_form(sc, hip_stream,
                       [&](hipStream_t st) { return launch_direct(sc, rq, d_hits, n, d_state, d_active, n, d_n_active, d_out, st); });
}

static int rt_scene_direct_impl(rt_scene* sc, const rt_direct_request* rq, const rt_hit* hits, uint32_t n, uint64_t* rng_state,
                                const uint32_t* active, uint32_t n_active, rt_direct* out, rt_tile_stats* stats) {
    // (the host form's n_active is a value: the both-or-neither rule is the device form's)
    int rc = check_direct(sc, rq, hits, n, rng_state, nullptr, nullptr, out);
    if (rc || (rc = check_active_list(active, n_active, n))) return rc;
    if (!active && n_active != 0) return fail(RT_ERR_BAD_ARG, "n_active without active");
    const uint32_t count = active ? n_active : n;
    HostForm hf(sc);
    // records that are not listed come back as they went in: the caller's bytes are the staging's initial contents
    Staging s(sc, {{hits, (size_t)n * sizeof(rt_hit), Staging::UP},
                   {rng_state, (size_t)n * 4 * sizeof(uint64_t), Staging::UP | Staging::DOWN},
                   {out, (size_t)n * sizeof(rt_direct), (active ? Staging::UP : 0u) | Staging::DOWN},
                   {active, (size_t)count * sizeof(uint32_t), Staging::UP}});
    StagedCall call(sc);
    if ((rc = hf.device()) || (rc = s.reserve("direct-lighting buffers")) || (rc = call.begin()) || (rc = s.upload(call)) ||
        (rc = launch_direct(sc, rq, s.dev(0), n, s.dev(1), s.dev(3), count, nullptr, s.dev(2), call.st)) || (rc = s.download(call)))
        return rc;
    return call.finish(stats);
}

// ---- next-event estimation for caller rays (rt_tile.h "next-event estimation", rt_nee.hip.h) ---------------------------------------
static int check_nee(rt_scene* sc, const rt_nee_request* rq, const void* rays, uint32_t n, const void* rgb) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    if (!rq) return fail(RT_ERR_BAD_ARG, "request is NULL");
    if (!rays || !rgb) return fail(RT_ERR_BAD_ARG, "rays or out_rgb is NULL");
    if (n == 0) return fail(RT_ERR_BAD_ARG, "n == 0");
    if (rq->spp == 0) return fail(RT_ERR_BAD_ARG, "spp == 0");
    if (rq->ray_form > RT_TRACE_RAY_AS_GIVEN) return fail(RT_ERR_BAD_ARG, "ray_form is neither RT_TRACE_RAY_NEW nor RT_TRACE_RAY_AS_GIVEN");
    if (rq->mode > RT_NEE_MIS) return fail(RT_ERR_BAD_ARG, "mode is neither RT_NEE_LIGHT_ONLY nor RT_NEE_MIS");
    if (rq->reserved != 0) return fail(RT_ERR_BAD_ARG, "reserved must be 0");
    if (rq->spp > RT_MAX_SPP) return fail(RT_ERR_LIMIT, "spp > RT_MAX_SPP");
    if (rq->max_bounces > RT_MAX_BOUNCES) return fail(RT_ERR_LIMIT, "max_bounces > RT_MAX_BOUNCES");
    if (rtplan::plan_nee(sc->shape, sc->n_lights, rq->flags).too_many) return fail(RT_ERR_LIMIT, "more than 2^23 emitters");
    return RT_OK;
}

// Enqueue one launch on `stream` (caller holds sc->mu, device current): persistent waves over the n rays.
static int launch_nee(rt_scene* sc, const rt_nee_request* rq, const void* d_rays, uint32_t n, void* d_state, void* d_rgb, void* d_segs,
                      void* d_shadow, hipStream_t stream) {
    const rtplan::QueryPlan qp = rtplan::plan_nee(sc->shape, sc->n_lights, rq->flags).query;
    rtk::NParams p;
    std::memset(&p, 0, sizeof p);
    p.rays = (const float4*)d_rays;
    p.rgb = (float*)d_rgb;
    p.segments = (uint32_t*)d_segs;
    p.shadow = (uint32_t*)d_shadow;
    p.rng_state = (uint64_t*)d_state;
    p.n = n;
    p.seed = rq->seed;
    p.spp = rq->spp;
    p.max_bounces = rq->max_bounces;
    p.as_given = rq->ray_form == RT_TRACE_RAY_AS_GIVEN ? 1u : 0u;
    p.mis = rq->mode == RT_NEE_MIS ? 1u : 0u;
    material_refs(sc, p);
    light_refs(sc, p);
    return launch_rays(sc, qp, rtplan::QUERY_BLOCK, rtk::nee_kernel(qp.engine, qp.scan_mode, lights_by_power(rq->flags), lights_cone(sc), glossy_mis(sc, rq)), "next-event-estimation", p, n,
                       vtext("nee: engine %d  scan mode %d  lds %zu B  ", qp.engine, qp.scan_mode, qp.lds),
                       vtext("rays %u  spp %u  bounces %u  mode %u  lights %u%s%s%s", n, rq->spp, rq->max_bounces, rq->mode, sc->n_lights,
                             lights_by_power(rq->flags) ? " by power" : "", lights_cone(sc) ? " cone" : "", glossy_mis(sc, rq) ? " glossy" : ""),
                       (uint64_t)n * rq->spp, stream);
}

static int rt_scene_trace_nee_device_impl(rt_scene* sc, const rt_nee_request* rq, const void* d_rays, uint32_t n, void* d_state,
                                          void* d_rgb, void* d_segs, void* d_shadow, void* hip_stream) {
    int rc = check_nee(sc, rq, d_rays, n, d_rgb);
    if (rc) return rc;
    return device_form(sc, hip_stream, [&](hipStream_t st) { return launch_nee(sc, rq, d_rays, n, d_state, d_rgb, d_segs, d_shadow, st); });
}

static int rt_scene_trace_nee_impl(rt_scene* sc, const rt_nee_request* rq, const rt_ray* rays, uint32_t n, uint64_t* rng_state,
                                   float* rgb, uint32_t* segs, uint32_t* shadow, rt_tile_stats* stats) {
    int rc = check_nee(sc, rq, rays, n, rgb);
    if (rc) return rc;
    HostForm hf(sc);
    Staging s(sc, {{rays, (size_t)n * sizeof(rt_ray), Staging::UP},
                   {rng_state, (size_t)n * 4 * sizeof(uint64_t), Staging::UP | Staging::DOWN},
                   {rgb, (size_t)n * 3 * sizeof(float), Staging::DOWN},
                   {segs, (size_t)n * sizeof(uint32_t), Staging::DOWN},
                   {shadow, (size_t)n * sizeof(uint32_t), Staging::DOWN}});
    StagedCall call(sc);
    if ((rc = hf.device()) || (rc = s.reserve("next-event-estimation buffers")) || (rc = call.begin()) || (rc = s.upload(call)) ||
        (rc = launch_nee(sc, rq, s.dev(0), n, s.dev(1), s.dev(2), s.dev(3), s.dev(4), call.st)) || (rc = s.download(call)))
        return rc;
    return call.finish(stats);
}

// ---- feature buffers of a strip (rt_tile.h "feature buffers", rt_aov.hip.h) -----------------------------------------------------
static uint32_t aov_mask(const rt_aov_planes& pl) {
    return (pl.albedo ? rtk::AOV_ALBEDO : 0u) | (pl.normal ? rtk::AOV_NORMAL : 0u) | (pl.depth ? rtk::AOV_DEPTH : 0u) |
           (pl.hits ? rtk::AOV_HITS : 0u) | (pl.index ? rtk::AOV_INDEX : 0u);
}

// Every entry of a call's plane array has the set of planes of entry 0 (*mask, by mask_of); name: the array's in the error text.
static int check_plane_sets(const rt_aov_planes* planes, uint32_t n, uint32_t (*mask_of)(const rt_aov_planes&), const char* name,
                            uint32_t* mask) {
    *mask = mask_of(planes[0]);
    for (uint32_t i = 1; i < n; i++)
        if (mask_of(planes[i]) != *mask) return fail(RT_ERR_BAD_ARG, std::string("the entries of ") + name + " differ in their set of planes");
    return RT_OK;
}

// The requests and planes of an AOV call (a batch of strips of one frame); *mask: the AOV_* bits of the planes every entry has.
static int check_aov(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, uint32_t begin, uint32_t end, const rt_aov_planes* planes,
                     uint32_t* mask) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    int rc = check_batch(rqs, n);
    if (rc) return rc;
    if ((rc = check_samples(begin, end, rqs[0].spp))) return rc;
    if (!planes) return fail(RT_ERR_BAD_ARG, "planes is NULL");
    if (aov_mask(planes[0]) == 0) return fail(RT_ERR_BAD_ARG, "every plane is NULL");
    return check_plane_sets(planes, n, aov_mask, "d_planes", mask);
}

// Enqueue the AOV launches of n strips (one per MAX_BATCH strips) on `stream` (caller holds sc->mu, device current): persistent waves
// over (strip, pixel).
static int launch_aov(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, uint32_t begin, uint32_t end, const rt_aov_planes* d_planes,
                      uint32_t mask, hipStream_t stream) {
    const rtplan::QueryPlan qp = rtplan::plan_query(sc->shape, rqs[0].flags);
    const rt_tile_request& rq = rqs[0];
    const uint32_t hs = rq.height / rq.divisions;
    rtk::AParams p;
    std::memset(&p, 0, sizeof p);
    frame_refs(sc, rq, begin, p);
    p.npix = hs * rq.width;
    p.s_end = end;
    p.planes = mask;
    scene_refs(sc, qp.full_chain, p);
    p.mat = sc->d_mat.get();
    for (uint32_t i0 = 0; i0 < n; i0 += rtk::MAX_BATCH) {
        const uint32_t m = std::min<uint32_t>(rtk::MAX_BATCH, n - i0);
        p.n_strips = m;
        for (uint32_t i = 0; i < m; i++) {
            const rt_aov_planes& pl = d_planes[i0 + i];
            rtk::AovStrip& sd = p.strips[i];
            sd.seed = rqs[i0 + i].seed;
            sd.albedo = pl.albedo;
            sd.normal = pl.normal;
            sd.depth = pl.depth;
            sd.hits = pl.hits;
            sd.index = pl.index;
            sd.y0 = hs * rqs[i0 + i].division_no;
        }
        int rc = launch_persistent(sc, qp.engine, qp.lds, rtplan::QUERY_BLOCK, rtk::aov_kernel(qp.engine, qp.scan_mode), "AOV", p,
                                   (uint64_t)p.npix * m, vtext("aov: engine %d  scan mode %d  lds %zu B  ", qp.engine, qp.scan_mode, qp.lds),
                                   vtext("strips %u  pixels %u  samples [%u, %u)  planes %#x", m, p.npix, begin, end, mask),
                                   (uint64_t)p.npix * (end - begin) * m, stream);
        if (rc) return rc;
    }
    return RT_OK;
}

static int rt_scene_render_aovs_device_impl(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, uint32_t begin, uint32_t end,
                                            const rt_aov_planes* d_planes, void* hip_stream) {
    uint32_t mask = 0;
    int rc = check_aov(sc, rqs, n, begin, end, d_planes, &mask);
    if (rc) return rc;
    return device_form(sc, hip_stream, [&](hipStream_t st) { return launch_aov(sc, rqs, n, begin, end, d_planes, mask, st); });
}

static int rt_scene_render_aov_impl(rt_scene* sc, const rt_tile_request* rq, uint32_t begin, uint32_t end, const rt_aov_planes* planes,
                                    rt_tile_stats* stats) {
    uint32_t mask = 0;
    int rc = check_aov(sc, rq, 1, begin, end, planes, &mask);
    if (rc) return rc;
    HostForm hf(sc);
    // albedo and normal (12 B), depth, hits and index (4 B) per pixel; a call from sample 0 reads no plane (the caller's buffers may be
    // uninitialised), a later one adds to what it is given
    const size_t npix = (size_t)(rq->height / rq->divisions) * rq->width;
    const size_t v3_b = npix * 3 * sizeof(float), s_b = npix * sizeof(uint32_t);
    const unsigned copy = (begin > 0 ? Staging::UP : 0u) | Staging::DOWN;
    Staging s(sc, {{planes->albedo, v3_b, copy}, {planes->normal, v3_b, copy}, {planes->depth, s_b, copy}, {planes->hits, s_b, copy},
                   {planes->index, s_b, copy}});
    StagedCall call(sc);
    auto launch = [&] {
        const rt_aov_planes dp = {(float*)s.dev(0), (float*)s.dev(1), (float*)s.dev(2), (uint32_t*)s.dev(3), (uint32_t*)s.dev(4)};
        return launch_aov(sc, rq, 1, begin, end, &dp, mask, call.st);
    };
    if ((rc = hf.device()) || (rc = s.reserve("AOV planes")) || (rc = call.begin()) || (rc = s.upload(call)) || (rc = launch()) ||
        (rc = s.download(call)))
        return rc;
    return call.finish(stats);
}

// ---- placed camera and the camera's rays (rt_tile.h "placed camera", rt_plan.h Pose, rt_camera.hip.h) -----------------------------
// *ps, *has: the pose of cam, or the reference camera for NULL; untouched on an error.
static int pose_of(const rt_camera* cam, rtplan::Pose* ps, bool* has) {
    if (!cam) {
        *has = false;
        return RT_OK;
    }
    if (!rtplan::make_pose(*cam, *ps))
        return fail(RT_ERR_BAD_ARG, "camera: a component is not finite, origin == target, up is parallel to the view direction, or flags / "
                                    "reserved are not 0");
    *has = true;
    return RT_OK;
}

static int rt_scene_set_camera_impl(rt_scene* sc, const rt_camera* cam) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    rtplan::Pose ps;
    bool has = false;
    int rc = pose_of(cam, &ps, &has);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(sc->mu);
    if (has) sc->pose = ps;
    sc->has_pose = has;
    return RT_OK;
}

static int check_camera_rays(rt_scene* sc, const rt_tile_request* rq, uint32_t begin, uint32_t end, const void* rays) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    int rc = check_batch(rq, 1);
    if (rc) return rc;
    if ((rc = check_samples(begin, end, rq->spp))) return rc;
    if (!rays) return fail(RT_ERR_BAD_ARG, "rays is NULL");
    return RT_OK;
}

// Enqueue the camera-ray launch of one strip on `stream` (caller holds sc->mu, device current): persistent waves over the records.
static int launch_camera_rays(rt_scene* sc, const rt_tile_request& rq, uint32_t begin, uint32_t end, void* d_rays, void* d_state,
                              hipStream_t stream) {
    const uint32_t hs = rq.height / rq.divisions;
    rtk::CParams p;
    std::memset(&p, 0, sizeof p);
    frame_refs(sc, rq, begin, p);
    p.y0 = hs * rq.division_no;
    p.n_smp = end - begin;
    p.total = (uint64_t)hs * rq.width * (end - begin);
    p.seed = rq.seed;
    p.rays = (float4*)d_rays;
    p.state = (ulonglong2*)d_state;
    return launch_persistent(sc, 0, 0, rtplan::QUERY_BLOCK, rtk::camera_rays_kernel(d_state != nullptr), "camera-ray", p, p.total,
                             vtext("camera rays: "),
                             vtext("records %llu  samples [%u, %u)  states %d", (unsigned long long)p.total, begin, end, d_state ? 1 : 0),
                             p.total, stream);
}

static int rt_scene_camera_rays_device_impl(rt_scene* sc, const rt_tile_request* rq, uint32_t begin, uint32_t end, void* d_rays,
                                            void* d_state, void* hip_stream) {
    int rc = check_camera_rays(sc, rq, begin, end, d_rays);
    if (rc) return rc;
    return device_form(sc, hip_stream, [&](hipStream_t st) { return launch_camera_rays(sc, *rq, begin, end, d_rays, d_state, st); });
}

static int rt_scene_camera_rays_impl(rt_scene* sc, const rt_tile_request* rq, uint32_t begin, uint32_t end, rt_ray* rays,
                                     uint64_t* rng_state, rt_tile_stats* stats) {
    int rc = check_camera_rays(sc, rq, begin, end, rays);
    if (rc) return rc;
    HostForm hf(sc);
    const size_t n = (size_t)(rq->height / rq->divisions) * rq->width * (end - begin);
    Staging s(sc, {{rays, n * sizeof(rt_ray), Staging::DOWN}, {rng_state, n * 4 * sizeof(uint64_t), Staging::DOWN}});
    StagedCall call(sc);
    if ((rc = hf.device()) || (rc = s.reserve("camera rays")) || (rc = call.begin()) || (rc = s.upload(call)) ||
        (rc = launch_camera_rays(sc, *rq, begin, end, s.dev(0), s.dev(1), call.st)) || (rc = s.download(call)))
        return rc;
    return call.finish(stats);
}

// ---- the a-trous denoiser (rt_tile.h "denoiser", rt_denoise.hip.h, rt_denoise_math.h) -------------------------------------------------
static uint32_t dn_mask(const rt_aov_planes& pl) {           // (the index plane is ignored)
    return (pl.albedo ? rtdn::P_ALBEDO : 0u) | (pl.normal ? rtdn::P_NORMAL : 0u) | (pl.depth ? rtdn::P_DEPTH : 0u) |
           (pl.hits ? rtdn::P_HITS : 0u);
}

// An optional output array: NULL, or n non-NULL entries.
static int check_out_array(const void* const* a, uint32_t n, const char* what) {
    if (!a) return RT_OK;
    for (uint32_t i = 0; i < n; i++)
        if (!a[i]) return fail(RT_ERR_BAD_ARG, std::string(what) + "[i] is NULL in a non-NULL array");
    return RT_OK;
}

// Every check of rt_tile.h "denoiser" but the device scratch; *mask: the rtdn::P_* of the planes every entry has.
static int check_denoise(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, const rt_denoise_request* dq, const void* const* acc,
                         const rt_aov_planes* planes, const void* const* rgb, size_t out_len, const void* const* f32,
                         const void* const* lin, uint32_t* mask) {
    if (!sc) return fail(RT_ERR_BAD_ARG, "scene is NULL");
    int rc = check_batch(rqs, n);
    if (rc) return rc;
    for (uint32_t i = 1; i < n; i++)
        if (rqs[i].division_no != rqs[0].division_no + i) return fail(RT_ERR_BAD_ARG, "strips must have consecutive division_no, ascending");
    if (!dq) return fail(RT_ERR_BAD_ARG, "denoise request is NULL");
    if ((rc = check_array(acc, n, "accum"))) return rc;
    if (!planes) return fail(RT_ERR_BAD_ARG, "planes is NULL");
    if ((rc = check_plane_sets(planes, n, dn_mask, "planes", mask))) return rc;
    if ((*mask & rtdn::P_DEPTH) && !(*mask & rtdn::P_HITS)) return fail(RT_ERR_BAD_ARG, "the depth plane needs the hits plane");
    if (!rgb && !f32 && !lin) return fail(RT_ERR_BAD_ARG, "no output");
    if ((rc = check_out_array(rgb, n, "out_rgb")) || (rc = check_out_array(f32, n, "out_f32")) ||
        (rc = check_out_array(lin, n, "out_linear")))
        return rc;
    const bool albedo = (*mask & rtdn::P_ALBEDO) != 0;
    if (dq->color_samples == 0 || (albedo && dq->aov_samples == 0)) return fail(RT_ERR_BAD_ARG, "color_samples and aov_samples must be >= 1");
    if (dq->color_samples > RT_MAX_SPP || (albedo && dq->aov_samples > RT_MAX_SPP))
        return fail(RT_ERR_LIMIT, "color_samples or aov_samples > RT_MAX_SPP");
    if (dq->iterations > RT_DENOISE_MAX_ITERATIONS) return fail(RT_ERR_BAD_ARG, "iterations > RT_DENOISE_MAX_ITERATIONS");
    if (dq->flags != 0 || dq->reserved != 0) return fail(RT_ERR_BAD_ARG, "flags and reserved must be 0");
    auto fin = [](float v) { return std::isfinite(v); };
    if (!fin(dq->k_color) || !(dq->k_color >= 0.f) || !fin(dq->k_normal) || !(dq->k_normal >= 0.f) || !fin(dq->k_depth) ||
        !(dq->k_depth >= 0.f))
        return fail(RT_ERR_BAD_ARG, "k_color, k_normal and k_depth must be finite and >= 0");
    if (!fin(dq->color_step_scale) || !(dq->color_step_scale > 0.f) || !fin(dq->albedo_eps) || !(dq->albedo_eps > 0.f))
        return fail(RT_ERR_BAD_ARG, "color_step_scale and albedo_eps must be finite and > 0");
    if (rgb && out_len < rt_tile_bytes(&rqs[0])) return fail(RT_ERR_BUFFER_TOO_SMALL, "out_len_each < (H/div)*W*3");
    const uint64_t rows = (uint64_t)(rqs[0].height / rqs[0].divisions) * n;
    if (rows > rqs[0].height) return fail(RT_ERR_BAD_ARG, "more strips than the frame has");
    if (rows >= (1u << 30) || rqs[0].width >= (1u << 30)) return fail(RT_ERR_LIMIT, "image of 2^30 rows or columns");   // (taps in int)
    return RT_OK;
}

static uint32_t dn_lds_max_step() {
    const int k = dbg(DBG_DENOISE_LDS_STEP);
    return k < 0 ? rtplan::DN_LDS_MAX_STEP : (uint32_t)k;
}

// Enqueue the launches of one denoise call on `stream` (caller holds sc->mu, device current, arguments checked): the entry kernel
// per band of DN_BAND strips, one step kernel per iteration over the whole image but the last, the last per band (or, with no
// iteration, the output kernel per band).  One event pair per launch.
static int launch_denoise(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, const rt_denoise_request& dq, uint32_t mask,
                          const void* const* acc, const rt_aov_planes* planes, void* const* rgb, void* const* f32, void* const* lin,
                          char* scratch, hipStream_t stream) {
    const rt_tile_request& rq = rqs[0];
    const uint32_t W = rq.width, Hs = rq.height / rq.divisions, R = Hs * n;
    const bool guided = (mask & (rtdn::P_NORMAL | rtdn::P_DEPTH | rtdn::P_HITS)) != 0;
    const rtplan::DenoisePlan pl = rtplan::plan_denoise(W, R, dq.iterations, guided, dn_lds_max_step());
    rtk::DnParams p;
    std::memset(&p, 0, sizeof p);
    p.W = W;
    p.R = R;
    p.Hs = Hs;
    p.planes = mask;
    p.e_f = (float)dq.color_samples;
    p.k_f = (float)dq.aov_samples;
    p.eps = dq.albedo_eps;
    p.kn = dq.k_normal;
    p.kd = dq.k_depth;
    p.guide = (float4*)(scratch + pl.off_guide);
    float4* buf[2] = {(float4*)(scratch + pl.off_color[0]), (float4*)(scratch + pl.off_color[1])};
    const uint32_t persist = (uint32_t)sc->ctx->n_cu * 8u;           // grid cap of the grid-stride kernels: 8 workgroups of 256 a CU
    auto launch = [&](rtk::DnFn kern, uint32_t blocks, size_t lds) { return enqueue(sc, stream, kern, blocks, rtplan::DN_BLOCK, lds, p); };
    // the band of strips [b0, b0 + m): its rows and its per-strip pointers
    auto band = [&](uint32_t b0, uint32_t m) {
        p.row0 = b0 * Hs;
        p.rows = m * Hs;
        p.n_strips = m;
        for (uint32_t i = 0; i < m; i++) {
            rtk::DnStrip& sd = p.strips[i];
            const rt_aov_planes& q = planes[b0 + i];
            sd.accum = (const float*)acc[b0 + i];
            sd.albedo = q.albedo;
            sd.normal = q.normal;
            sd.depth = q.depth;
            sd.hits = q.hits;
            sd.rgb = rgb ? (uint8_t*)rgb[b0 + i] : nullptr;
            sd.f32 = f32 ? (float*)f32[b0 + i] : nullptr;
            sd.lin = lin ? (float*)lin[b0 + i] : nullptr;
        }
    };
    auto grid_stride = [&](uint64_t pixels) { return (uint32_t)std::min<uint64_t>((pixels + 255) / 256, persist); };
    auto tiles = [&](uint32_t rows) { return pl.tiles_x * ((rows + rtplan::DN_TILE_Y - 1) / rtplan::DN_TILE_Y); };
    int rc;
    p.dst = buf[0];
    for (uint32_t b0 = 0; b0 < n; b0 += rtk::DN_BAND) {
        band(b0, std::min<uint32_t>(rtk::DN_BAND, n - b0));
        if ((rc = launch(rtk::dn_entry_kernel(), grid_stride((uint64_t)p.rows * W), 0))) return rc;
    }
    uint32_t cur = 0;
    float kc = dq.k_color;
    for (uint32_t i = 0; i < dq.iterations; i++) {
        p.s = pl.step[i];
        p.kc = kc;
        p.src = buf[cur];
        p.dst = buf[cur ^ 1u];
        const bool last = i + 1 == dq.iterations;
        const rtk::DnFn kern = rtk::dn_step_kernel(pl.lds[i] != 0, last);
        if (!last) {
            p.row0 = 0;
            p.rows = R;
            p.n_strips = 0;
            if ((rc = launch(kern, tiles(R), pl.lds[i]))) return rc;
        } else {
            for (uint32_t b0 = 0; b0 < n; b0 += rtk::DN_BAND) {
                band(b0, std::min<uint32_t>(rtk::DN_BAND, n - b0));
                if ((rc = launch(kern, tiles(p.rows), pl.lds[i]))) return rc;
            }
        }
        if (dbg(DBG_VERBOSE))
            fprintf(stderr, "[rt] denoise: iteration %u  step %u  lds %zu B  workgroups/CU %u  image %u x %u  planes %#x\n", i, p.s,
                    pl.lds[i], pl.wg_per_cu[i], W, R, mask);
        cur ^= 1u;
        kc = kc * dq.color_step_scale;
    }
    if (dq.iterations == 0) {
        p.src = buf[0];
        for (uint32_t b0 = 0; b0 < n; b0 += rtk::DN_BAND) {
            band(b0, std::min<uint32_t>(rtk::DN_BAND, n - b0));
            if ((rc = launch(rtk::dn_output_kernel(), grid_stride((uint64_t)p.rows * W), 0))) return rc;
        }
    }
    sc->last_engine = 0;
    sc->last_form = 0;
    return RT_OK;
}

static int rt_scene_denoise_device_impl(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, const rt_denoise_request* dq,
                                        const void* const* d_acc, const rt_aov_planes* d_planes, void* const* d_rgb, size_t out_len,
                                        void* const* d_f32, void* const* d_lin, void* d_scratch, size_t scratch_bytes,
                                        void* hip_stream) {
    uint32_t mask = 0;
    int rc = check_denoise(sc, rqs, n, dq, d_acc, d_planes, (const void* const*)d_rgb, out_len, (const void* const*)d_f32,
                           (const void* const*)d_lin, &mask);
    if (rc) return rc;
    const uint32_t R = rqs[0].height / rqs[0].divisions * n;
    if (!d_scratch) return fail(RT_ERR_BAD_ARG, "d_scratch is NULL");
    if (scratch_bytes < rtplan::plan_denoise(rqs[0].width, R, 0, false).scratch_bytes)
        return fail(RT_ERR_BAD_ARG, "scratch_bytes < rt_denoise_scratch_bytes(W, R)");
    return device_form(sc, hip_stream, [&](hipStream_t st) {
        return launch_denoise(sc, rqs, n, *dq, mask, d_acc, d_planes, d_rgb, d_f32, d_lin, (char*)d_scratch, st);
    });
}

static int rt_scene_denoise_impl(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, const rt_denoise_request* dq,
                                 const float* const* acc, const rt_aov_planes* planes, uint8_t* const* rgb, size_t out_len,
                                 float* const* f32, float* const* lin, rt_tile_stats* stats) {
    uint32_t mask = 0;
    int rc = check_denoise(sc, rqs, n, dq, (const void* const*)acc, planes, (const void* const*)rgb, out_len,
                           (const void* const*)f32, (const void* const*)lin, &mask);
    if (rc) return rc;
    HostForm hf(sc);
    Staging s(sc, rtplan::dn_stage_list(rqs[0], n, acc, planes, rgb, f32, lin));
    StagedCall call(sc);
    // the device side of every strip, as the device form takes it
    auto launch = [&] {
        std::vector<const void*> d_acc(n);
        std::vector<rt_aov_planes> d_pl(n);
        std::vector<void*> d_rgb(n), d_f32(n), d_lin(n);
        for (uint32_t i = 0; i < n; i++) {
            auto dev = [&](int k) { return s.dev(1 + (size_t)rtplan::DN_STAGE_STRIP * i + k); };
            d_acc[i] = dev(rtplan::DN_ACCUM);
            d_pl[i] = {(float*)dev(rtplan::DN_ALBEDO), (float*)dev(rtplan::DN_NORMAL), (float*)dev(rtplan::DN_DEPTH),
                       (uint32_t*)dev(rtplan::DN_HITS), nullptr};
            d_rgb[i] = dev(rtplan::DN_RGB);
            d_f32[i] = dev(rtplan::DN_F32);
            d_lin[i] = dev(rtplan::DN_LIN);
        }
        return launch_denoise(sc, rqs, n, *dq, mask, d_acc.data(), d_pl.data(), rgb ? d_rgb.data() : nullptr, f32 ? d_f32.data() : nullptr,
                              lin ? d_lin.data() : nullptr, s.dev(0), call.st);
    };
    if ((rc = hf.device()) || (rc = s.reserve("denoise staging")) || (rc = call.begin()) || (rc = s.upload(call)) || (rc = launch()) ||
        (rc = s.download(call)))
        return rc;
    return call.finish(stats);
}

// ---- Test / tool hooks.  NOT part of rt_tile.h and NOT in the product library: compiled only with -DRT_DEBUG_HOOKS, which
// build.py adds for lib/librt_s8_dbg.so (tests) and tools add to their instrumented variants.  tests/test_abi.py checks that
// librt_s8.so exports exactly the functions rt_tile.h declares.
#ifdef RT_DEBUG_HOOKS
// debug: raw read of the scene's device counter words (tools/phase_census.py)
extern "C" __attribute__((visibility("default"))) int rt_debug_read_counters(rt_scene* sc, uint32_t first, uint32_t n,
                                                                             unsigned long long* out) {
    return guarded([&]() -> int {
        if (!sc || !out || first > COUNTER_WORDS || n > COUNTER_WORDS - first) return fail(RT_ERR_BAD_ARG, "counter range");
        std::lock_guard<std::mutex> lk(sc->mu);
        HIPCHK(hipSetDevice(sc->ctx->dev));
        HIPCHK(hipMemcpy(out, sc->d_counters.get() + first, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}
// debug: sqrt_rn of the traversal kernels against the compiler's IEEE sequence on every f32 bit pattern in [from, from + n);
// *mismatches = patterns whose results differ.  Tests only; not part of rt_tile.h.
extern "C" __attribute__((visibility("default"))) int rt_debug_sqrt_selftest(int device, uint32_t from, unsigned long long n,
                                                                             unsigned long long* mismatches) {
    return guarded([&]() -> int {
        if (!mismatches || n > (1ull << 32) - from) return fail(RT_ERR_BAD_ARG, "sqrt self-test range");
        HIPCHK(hipSetDevice(device));
        DevArray<unsigned long long> d_bad;
        HIPCHK(d_bad.alloc(1));
        hipError_t e = hipMemset(d_bad.get(), 0, sizeof(unsigned long long));
        if (e == hipSuccess) {
            rtk::sqrt_selftest_launch(from, n, d_bad.get(), 0);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(mismatches, d_bad.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(RT_ERR_HIP, hipGetErrorString(e));
        return RT_OK;
    });
}
// debug: the device functions of the closest-hit arithmetic (rt_unit.hip.h) and of the light-sampling and scatter arithmetic
// (rt_unit_sampling.hip.h), one lane per record, as translation unit `unit` compiles them; a (unit, family) pair that is not
// instantiated is RT_ERR_BAD_ARG before any device work.  One launch, returns after synchronising.  Tests only; not in rt_tile.h.
extern "C" __attribute__((visibility("default"))) int rt_debug_unit(int device, int unit, int family, unsigned long long n,
                                                                    const void* in, void* out) {
    return guarded([&]() -> int {
        if (!rtk::unit_instantiated(unit, family)) return fail(RT_ERR_BAD_ARG, "unit / family");
        if (n == 0) return RT_OK;
        if (!in || !out || n > (1ull << 24)) return fail(RT_ERR_BAD_ARG, "unit records");
        const size_t bi = (size_t)n * rtk::unit_record_in(family) * 4, bo = (size_t)n * rtk::unit_record_out(family) * 4;
        HIPCHK(hipSetDevice(device));
        DevArray<uint32_t> d_in, d_out;
        hipError_t e = d_in.alloc(bi / 4);
        if (e == hipSuccess) e = d_out.alloc(bo / 4);
        if (e == hipSuccess) e = hipMemcpy(d_in.get(), in, bi, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(d_out.get(), 0, bo);
        if (e == hipSuccess) {
            rtk::unit_launch(unit, family, n, d_in.get(), d_out.get(), 0);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(out, d_out.get(), bo, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(RT_ERR_HIP, hipGetErrorString(e));
        return RT_OK;
    });
}
// debug: set one knob of the launch path (DebugKnob above) by its environment-variable name; returns the previous value,
// INT_MIN for an unknown name.  Tests and tools only; not part of rt_tile.h.
extern "C" __attribute__((visibility("default"))) int rt_debug_set(const char* name, int value) {
    dbg_load_env();
    if (!name) return INT32_MIN;
    if (!strcmp(name, "RT_LAST_VARIANT")) return g_last_variant.exchange(value);      // (the launch path's output, see there)
    for (int k = 0; k < DBG_N; k++)
        if (!strcmp(name, g_dbg_spec[k].env)) return g_dbg[k].exchange(value);
    return INT32_MIN;
}
// test hook (tests/test_abi.py): throw inside a guarded body; the status comes back, nothing unwinds
extern "C" __attribute__((visibility("default"))) int rt_debug_throw(int kind) {
    return guarded([&]() -> int {
        if (kind == 0) throw std::bad_alloc();
        if (kind == 1) throw std::runtime_error("rt_debug_throw");
        if (kind == 2) throw 42;
        if (kind == 3) { std::vector<char> v; v.reserve((size_t)-1 / 2); }      // a real failed allocation (length_error / bad_alloc)
        return RT_OK;
    });
}
#endif  // RT_DEBUG_HOOKS

static int rt_render_tile_impl(int device, const rt_tile_request* rq, const rt_sphere* sp, uint32_t ns,
                          const rt_triangle* tr, uint32_t nt, const uint32_t* world_index, uint8_t* out_rgb, size_t out_len,
                          float* out_f32, rt_tile_stats* stats) {
    int rc = check_request(rq);
    if (rc) return rc;
    if (!out_rgb) return fail(RT_ERR_BAD_ARG, "out_rgb is NULL");
    if (out_len < rt_tile_bytes(rq)) return fail(RT_ERR_BUFFER_TOO_SMALL, "out_len < (H/div)*W*3");
    rt_scene* sc = nullptr;
    rc = rt_scene_create_impl(device, sp, ns, tr, nt, world_index, &sc);
    if (rc) return rc;
    rc = rt_scene_render_tile_impl(sc, rq, out_rgb, out_len, out_f32, stats);
    std::string keep = g_err;
    rt_scene_destroy_impl(sc);
    if (rc) g_err = keep;
    return rc;
}

// =====================================================================================
// Frame context: the controller's dispatch + assembly (controller main.rs:47-75, 109-115) with everything a JOB needs kept
// alive between frames — one dispatcher thread per device entry, the world resident on every device, streams, strip
// buffers, and the page-locked registration of the caller's frame buffer.
// =====================================================================================
}  // extern "C"  (the struct below is a C++ type behind the opaque C handle)

struct FrameDev {
    int dev = 0;                        // device ordinal
    rt_scene* scene = nullptr;          // the job's world on this device (owned by the dispatcher thread)
    std::thread th;
    // strip-queue mode: two strips in flight, each on its own stream with its own device buffer (made on first use)
    Stream qs[2];
    GrowBuf qd[2];
    // result of the last command
    int rc = RT_OK;
    std::string err;
    rt_tile_stats st;
    float busy_ms = 0.f;                // dispatcher wall time of the last render
};

struct rt_frame_ctx {
    std::vector<FrameDev> fd;
    std::mutex call_mu;                 // one API call at a time per context
    std::mutex mu;                      // command hand-over
    std::condition_variable cv_work, cv_done;
    uint64_t gen = 0;
    int pending = 0;
    enum Cmd { CMD_NONE, CMD_UPLOAD, CMD_RENDER, CMD_STOP } cmd = CMD_NONE;
    // CMD_UPLOAD
    const HostScene* hs = nullptr;
    bool have_world = false;
    float scene_ms_pending = 0.f;       // duration of the last set_world, charged to the next frame's stats
    // ---- the job's state, kept from frame to frame
    // its camera (rt_frame_ctx_set_camera): handed to every entry's scene at the start of a frame
    rtplan::Pose pose;
    bool has_pose = false;
    rtframe::CostMemory costs;          // ray segments per strip of the job's last frame: the next frame is assigned by them
    // the caller's frame buffer, page-locked once
    void* pinned_ptr = nullptr;
    size_t pinned_len = 0;
    // ---- CMD_RENDER: the frame in flight (written by rt_frame_ctx_render before the hand-over, read by the dispatchers)
    rtframe::FramePlan plan;            // the kernels' request, the strip size, owner[k] = entry of strip k (rt_frame_plan.h)
    uint8_t* out = nullptr;
    std::atomic<uint32_t> next_strip{0};        // strip queue: the next strip to pull
    std::vector<unsigned long long> cost_now;   // filled by the dispatchers (each writes its own strips' entries)
};

namespace {

// Entry w's strips of the frame in flight (plan.owner: snake / longest-first by measured cost / k % n, rt_frame_plan.h) as one
// batch: one launch per <= MAX_BATCH strips, the last quarter as its own launch so that the downloads of the others run under it
// (controller main.rs:47-75 fires one request per division; Docker DNS round-robins them over the slaves).  Stitch by division_no:
// strip k lands at byte offset k * strip (controller main.rs:109-115).
int frame_dev_render_owned(rt_frame_ctx* fc, int w) {
    FrameDev& d = fc->fd[w];
    const rtframe::FramePlan& plan = fc->plan;
    std::vector<rt_tile_request> rqs;
    std::vector<uint8_t*> outs;
    for (uint32_t k = 0; k < plan.rq.divisions; k++) {
        if (plan.owner[k] != (uint32_t)w) continue;
        rt_tile_request rq = plan.rq;
        rq.division_no = k;
        rqs.push_back(rq);
        outs.push_back(fc->out + (size_t)k * plan.strip_bytes);
    }
    if (rqs.empty()) return RT_OK;
    std::vector<unsigned long long> cost(rqs.size(), 0ull);
    int r = rt_scene_render_tiles_impl(d.scene, rqs.data(), (uint32_t)rqs.size(), outs.data(), plan.strip_bytes, nullptr, &d.st, cost.data());
    if (r) return r;
    for (size_t i = 0; i < rqs.size(); i++) fc->cost_now[rqs[i].division_no] = cost[i];      // (disjoint entries per dispatcher)
    return RT_OK;
}

// Dynamic assignment: pull one strip at a time, the bottom of the frame first (its strips cost the most: longest-first keeps the
// devices' finish times within one cheap strip of each other).  Two strips in flight per entry, each on its own stream with its
// own device buffer: the launch tail and the download of one run under the other.  Streams and buffers belong to the context:
// made on the first queue-mode frame, grown when a frame has larger strips.
int frame_dev_render_queue(rt_frame_ctx* fc, int w) {
    FrameDev& d = fc->fd[w];
    const rt_tile_request& rq0 = fc->plan.rq;
    const size_t strip = fc->plan.strip_bytes;
    uint8_t* out_rgb = fc->out;
    rt_scene* sc = d.scene;
    HIPCHK(hipSetDevice(sc->ctx->dev));
    for (int i = 0; i < 2; i++)
        if (!d.qs[i]) HIPCHK(d.qs[i].create(hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
        int rc = reserve(d.qd[i], strip, "strip");
        if (rc) return rc;
    }
    bool busy[2] = {false, false};
    struct Settle {                       // an error return waits for what is already enqueued (it writes caller memory)
        FrameDev& d;
        bool* busy;
        ~Settle() {
            for (int i = 0; i < 2; i++)
                if (busy[i]) (void)hipStreamSynchronize(d.qs[i].get());
        }
    } settle{d, busy};
    for (uint32_t turn = 0;; turn++) {
        const int sl = (int)(turn & 1u);
        if (busy[sl]) {
            HIPCHK(hipStreamSynchronize(d.qs[sl].get()));
            busy[sl] = false;
        }
        const uint32_t i = fc->next_strip.fetch_add(1);
        if (i >= rq0.divisions) break;
        rt_tile_request rq = rq0;
        rq.division_no = rq0.divisions - 1u - i;
        void* d1[1] = {d.qd[sl].data()};
        int r = rt_scene_render_tiles_device_impl(sc, &rq, 1, d1, strip, nullptr, d.qs[sl].get());
        if (r) return r;
        HIPCHK(hipMemcpyAsync(out_rgb + (size_t)rq.division_no * strip, d.qd[sl].data(), strip, hipMemcpyDeviceToHost, d.qs[sl].get()));
        busy[sl] = true;
    }
    for (int i = 0; i < 2; i++)
        if (busy[i]) {
            HIPCHK(hipStreamSynchronize(d.qs[i].get()));
            busy[i] = false;
        }
    return rt_scene_collect_impl(sc, &d.st);
}

int frame_dev_render(rt_frame_ctx* fc, int w) {
    FrameDev& d = fc->fd[w];
    std::memset(&d.st, 0, sizeof d.st);
    rt_scene* sc = d.scene;
    if (!sc) return fail(RT_ERR_BAD_ARG, "rt_frame_ctx_render before rt_frame_ctx_set_world");
    {
        std::lock_guard<std::mutex> lk(sc->mu);          // the job's camera: this entry's launches of the frame read it
        sc->pose = fc->pose;
        sc->has_pose = fc->has_pose;
    }
    return fc->plan.mode == rtassign::QUEUE ? frame_dev_render_queue(fc, w) : frame_dev_render_owned(fc, w);
}

// On the dispatcher thread, with the entry's device current: the context itself is deleted on the caller's thread, with nothing left to free.
void frame_dev_release(FrameDev& d) {
    rt_scene_destroy_impl(d.scene);
    d.scene = nullptr;
    (void)hipSetDevice(d.dev);
    for (int i = 0; i < 2; i++) {
        if (d.qs[i]) (void)hipStreamSynchronize(d.qs[i].get());
        d.qs[i].reset();
        d.qd[i].reset();
    }
}

// dispatcher thread of entry w: sleeps on the context's condition variable between commands
void frame_dev_main(rt_frame_ctx* fc, int w) {
    FrameDev& d = fc->fd[w];
    uint64_t seen = 0;
    for (;;) {
        rt_frame_ctx::Cmd cmd;
        {
            std::unique_lock<std::mutex> lk(fc->mu);
            fc->cv_work.wait(lk, [&] { return fc->gen != seen; });
            seen = fc->gen;
            cmd = fc->cmd;
        }
        // an exception must not leave a thread function (std::terminate): same guard as the entry points
        const auto t0 = std::chrono::steady_clock::now();
        d.rc = guarded([&]() -> int {
            switch (cmd) {
                case rt_frame_ctx::CMD_UPLOAD: {
                    if (d.scene) {
                        rt_scene_destroy_impl(d.scene);
                        d.scene = nullptr;
                    }
                    return upload_scene(d.dev, *fc->hs, &d.scene);     // world uploaded once per device per job
                }
                case rt_frame_ctx::CMD_RENDER: return frame_dev_render(fc, w);
                case rt_frame_ctx::CMD_STOP: frame_dev_release(d); return RT_OK;
                default: return RT_OK;
            }
        });
        d.busy_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (d.rc) {
            try {
                d.err = g_err;
            } catch (...) {
            }
        }
        {
            std::lock_guard<std::mutex> lk(fc->mu);
            if (--fc->pending == 0) fc->cv_done.notify_all();
        }
        if (cmd == rt_frame_ctx::CMD_STOP) return;
    }
}

// hand one command to every dispatcher and wait for all of them; the first error (in entry order) is the call's
int frame_run(rt_frame_ctx* fc, rt_frame_ctx::Cmd cmd) {
    {
        std::lock_guard<std::mutex> lk(fc->mu);
        fc->cmd = cmd;
        fc->pending = (int)fc->fd.size();
        fc->gen++;
    }
    fc->cv_work.notify_all();
    {
        std::unique_lock<std::mutex> lk(fc->mu);
        fc->cv_done.wait(lk, [&] { return fc->pending == 0; });
    }
    for (FrameDev& d : fc->fd)
        if (d.rc) return fail(d.rc, d.err);
    return RT_OK;
}

void frame_unpin(rt_frame_ctx* fc) {
    if (fc->pinned_ptr) {
        if (!fc->fd.empty()) (void)hipSetDevice(fc->fd[0].dev);
        (void)hipHostUnregister(fc->pinned_ptr);
        fc->pinned_ptr = nullptr;
        fc->pinned_len = 0;
    }
}

int rt_frame_ctx_create_impl(const int* devices, int n_devices, rt_frame_ctx** out) {
    if (!out) return fail(RT_ERR_BAD_ARG, "out_ctx is NULL");
    *out = nullptr;
    if (!g_init) return fail(RT_ERR_NOT_INITIALIZED, "call rt_init() first");
    std::vector<int> devs;
    if (devices && n_devices > 0)
        devs.assign(devices, devices + n_devices);
    else
        for (size_t d = 0; d < g_ctx.size(); d++) devs.push_back((int)d);
    for (int d : devs)
        if (d < 0 || d >= (int)g_ctx.size()) return fail(RT_ERR_BAD_DEVICE, "bad device ordinal");
    rt_frame_ctx* fc = new rt_frame_ctx;
    fc->fd.resize(devs.size());
    size_t started = 0;
    try {
        for (; started < devs.size(); started++) {
            fc->fd[started].dev = devs[started];
            fc->fd[started].th = std::thread(frame_dev_main, fc, (int)started);
        }
    } catch (...) {
        // could not start every dispatcher: stop the ones that run (they wait for `pending` of their own count)
        fc->fd.resize(started);
        if (started) (void)frame_run(fc, rt_frame_ctx::CMD_STOP);
        for (FrameDev& d : fc->fd)
            if (d.th.joinable()) d.th.join();
        delete fc;
        throw;
    }
    *out = fc;
    return RT_OK;
}

int rt_frame_ctx_destroy_impl(rt_frame_ctx* fc) {
    if (!fc) return RT_OK;
    {
        std::lock_guard<std::mutex> call(fc->call_mu);
        (void)frame_run(fc, rt_frame_ctx::CMD_STOP);          // every dispatcher releases its world, streams and buffers
        for (FrameDev& d : fc->fd)
            if (d.th.joinable()) d.th.join();
        frame_unpin(fc);
    }
    delete fc;
    return RT_OK;
}

int rt_frame_ctx_set_world_impl(rt_frame_ctx* fc, const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt,
                                const uint32_t* world_index) {
    if (!fc) return fail(RT_ERR_BAD_ARG, "ctx is NULL");
    int rc = check_world(sp, ns, tr, nt, world_index);
    if (rc) return rc;
    if (!g_init) return fail(RT_ERR_NOT_INITIALIZED, "call rt_init() first");
    std::lock_guard<std::mutex> call(fc->call_mu);
    const auto t0 = std::chrono::steady_clock::now();
    // the world's host side once per job (the reference rebuilds the BVH per strip, slave main.rs:60)
    HostScene hs;
    rtscene::build_host_scene(sp, ns, tr, nt, world_index, dbg(DBG_REORDER) != 0, hs);
    fc->hs = &hs;
    fc->have_world = false;
    fc->costs.forget();                // another world: the strips' costs are to be measured again
    rc = frame_run(fc, rt_frame_ctx::CMD_UPLOAD);
    fc->hs = nullptr;
    if (rc) return rc;
    fc->have_world = true;
    fc->scene_ms_pending = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RT_OK;
}

int rt_frame_ctx_set_camera_impl(rt_frame_ctx* fc, const rt_camera* cam) {
    if (!fc) return fail(RT_ERR_BAD_ARG, "ctx is NULL");
    rtplan::Pose ps;
    bool has = false;
    int rc = pose_of(cam, &ps, &has);
    if (rc) return rc;
    std::lock_guard<std::mutex> call(fc->call_mu);
    if (has) fc->pose = ps;
    fc->has_pose = has;
    return RT_OK;
}

// The frame calls' arguments, in the one order both rt_render_frame and rt_frame_ctx_render report them: the request, the buffer,
// `world` (the one-shot call's world and rt_init, before any thread or upload; nothing for a context), the tiling, the length.
template <class WorldCheck>
int check_frame_args(const rt_tile_request* rq_in, const uint8_t* out_rgb, size_t out_len, WorldCheck&& world) {
    if (!rq_in) return fail(RT_ERR_BAD_ARG, "request is NULL");
    rt_tile_request rq0 = *rq_in;
    rq0.division_no = 0;
    int rc = check_request(&rq0);
    if (rc) return rc;
    if (!out_rgb) return fail(RT_ERR_BAD_ARG, "out_rgb is NULL");
    if ((rc = world())) return rc;
    // the controller's ImageBuffer::from_vec(width, height, ..).unwrap() (controller main.rs:117-119)
    // panics unless the strips tile the frame exactly
    if (rq0.height % rq0.divisions != 0) return fail(RT_ERR_FRAME_SIZE, "height % divisions != 0");
    if (out_len < rtframe::strip_bytes(rq0) * rq0.divisions) return fail(RT_ERR_BUFFER_TOO_SMALL, "out_len < H*W*3");
    return RT_OK;
}

int rt_frame_ctx_render_impl(rt_frame_ctx* fc, const rt_tile_request* rq_in, uint8_t* out_rgb, size_t out_len,
                             rt_frame_stats* stats) {
    if (!fc) return fail(RT_ERR_BAD_ARG, "ctx is NULL");
    int rc = check_frame_args(rq_in, out_rgb, out_len, [] { return RT_OK; });
    if (rc) return rc;
    std::lock_guard<std::mutex> call(fc->call_mu);
    if (!fc->have_world) return fail(RT_ERR_BAD_ARG, "rt_frame_ctx_render before rt_frame_ctx_set_world");
    const auto t0 = std::chrono::steady_clock::now();
    // page-lock the frame buffer ONCE: strip downloads become DMA that runs under the kernels.  The registration is kept
    // until another buffer comes (or release / destroy).  Best effort: a buffer the caller registered itself (or that
    // cannot be registered) is used as it is.
    float pin_ms = 0.f;
    const size_t frame_bytes = rtframe::strip_bytes(*rq_in) * rq_in->divisions;
    const rtframe::PinStep pin = rtframe::pin_step(!(rq_in->flags & RT_FLAG_FRAME_NO_PIN), fc->pinned_ptr, fc->pinned_len, out_rgb, frame_bytes);
    if (pin.release) frame_unpin(fc);
    if (pin.acquire) {
        (void)hipSetDevice(fc->fd[0].dev);                 // (not device 0 by accident: the context may exclude it)
        if (hipHostRegister(out_rgb, frame_bytes, hipHostRegisterPortable) == hipSuccess) {
            fc->pinned_ptr = out_rgb;
            fc->pinned_len = frame_bytes;
        } else {
            (void)hipGetLastError();
        }
        pin_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // the frame's strips and which entry renders which (rt_frame_plan.h)
    fc->plan = rtframe::plan_frame(*rq_in, (uint32_t)fc->fd.size(), fc->costs, fc->pose, fc->has_pose);
    fc->out = out_rgb;
    fc->next_strip.store(0);
    fc->cost_now.assign(fc->plan.rq.divisions, 0ull);
    rc = frame_run(fc, rt_frame_ctx::CMD_RENDER);
    if (rc) return rc;
    rtframe::remember_frame(fc->costs, fc->plan, fc->pose, fc->has_pose, fc->cost_now, dbg(DBG_STRIP_COST) != 0);
    std::vector<rtframe::EntryResult> res;
    for (const FrameDev& d : fc->fd) res.push_back({d.st, d.busy_ms});
    rt_frame_stats fs = rtframe::fold_frame_stats(res.data(), res.size(), fc->plan.mode == rtassign::QUEUE);
    fs.wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    fs.pin_ms = pin_ms;
    fs.scene_ms = fc->scene_ms_pending;
    fc->scene_ms_pending = 0.f;
    fs.host_ms = fs.wall_ms - fs.pin_ms - fs.kernel_ms - fs.d2h_exposed_ms;
    fs.n_devices = (uint32_t)fc->fd.size();
    fs.pinned = fc->pinned_ptr == (void*)out_rgb ? 1u : 0u;
    fs.assignment = (uint32_t)fc->plan.mode;
    if (stats) *stats = fs;
    return RT_OK;
}

int rt_frame_ctx_release_buffer_impl(rt_frame_ctx* fc) {
    if (!fc) return fail(RT_ERR_BAD_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> call(fc->call_mu);
    frame_unpin(fc);
    return RT_OK;
}

int rt_render_frame_impl(const int* devices, int n_devices, const rt_tile_request* rq_in, const rt_sphere* sp,
                         uint32_t ns, const rt_triangle* tr, uint32_t nt, const uint32_t* world_index, uint8_t* out_rgb,
                         size_t out_len, rt_tile_stats* stats) {
    // argument errors before any thread or upload
    int rc = check_frame_args(rq_in, out_rgb, out_len, [&] {
        int rw = check_world(sp, ns, tr, nt, world_index);
        if (rw) return rw;
        return g_init ? RT_OK : fail(RT_ERR_NOT_INITIALIZED, "call rt_init() first");
    });
    if (rc) return rc;
    rt_frame_ctx* fc = nullptr;
    rc = rt_frame_ctx_create_impl(devices, n_devices, &fc);
    if (rc) return rc;
    struct Destroy {
        rt_frame_ctx* fc;
        ~Destroy() {
            std::string keep = g_err;
            rt_frame_ctx_destroy_impl(fc);
            g_err = keep;
        }
    } destroy{fc};
    rc = rt_frame_ctx_set_world_impl(fc, sp, ns, tr, nt, world_index);
    if (rc) return rc;
    rt_frame_stats fs;
    rc = rt_frame_ctx_render_impl(fc, rq_in, out_rgb, out_len, &fs);
    if (rc) return rc;
    if (stats) *stats = fs.totals;
    return RT_OK;
}

}  // namespace

extern "C" {

// ---- the exported entry points: argument-for-argument the functions above, behind guarded() ----------------------
RT_API int rt_init(int* n_devices) { return guarded([&] { return rt_init_impl(n_devices); }); }
RT_API void rt_shutdown(void) { (void)guarded([&] { return rt_shutdown_impl(); }); }
RT_API int rt_scene_create(int device, const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt,
                           const uint32_t* world_index, rt_scene** out) {
    return guarded([&] { return rt_scene_create_impl(device, sp, ns, tr, nt, world_index, out); });
}
RT_API void rt_scene_destroy(rt_scene* sc) { (void)guarded([&] { return rt_scene_destroy_impl(sc); }); }
RT_API int rt_scene_render_tiles_device(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, void* const* d_out_rgb,
                                        size_t out_len_each, void* const* d_out_f32, void* hip_stream) {
    return guarded([&] { return rt_scene_render_tiles_device_impl(sc, rqs, n, d_out_rgb, out_len_each, d_out_f32, hip_stream); });
}
RT_API int rt_scene_render_tile_device(rt_scene* sc, const rt_tile_request* rq, void* d_out_rgb, size_t out_len,
                                       void* d_out_f32, void* hip_stream) {
    return guarded([&] { return rt_scene_render_tile_device_impl(sc, rq, d_out_rgb, out_len, d_out_f32, hip_stream); });
}
RT_API int rt_scene_collect(rt_scene* sc, rt_tile_stats* st) { return guarded([&] { return rt_scene_collect_impl(sc, st); }); }
RT_API int rt_scene_intersect(rt_scene* sc, const rt_ray* rays, uint32_t n, uint32_t mode, uint32_t flags, rt_hit* hits,
                              rt_tile_stats* stats) {
    return guarded([&] { return rt_scene_intersect_impl(sc, rays, n, mode, flags, hits, stats); });
}
RT_API int rt_scene_intersect_device(rt_scene* sc, const void* d_rays, uint32_t n, uint32_t mode, uint32_t flags, void* d_hits,
                                     void* hip_stream) {
    return guarded([&] { return rt_scene_intersect_device_impl(sc, d_rays, n, mode, flags, d_hits, hip_stream); });
}
RT_API int rt_scene_trace(rt_scene* sc, const rt_trace_request* rq, const rt_ray* rays, uint32_t n, uint64_t* rng_state, float* out_rgb,
                          uint32_t* out_segments, rt_tile_stats* stats) {
    return guarded([&] { return rt_scene_trace_impl(sc, rq, rays, n, rng_state, out_rgb, out_segments, stats); });
}
RT_API int rt_scene_trace_device(rt_scene* sc, const rt_trace_request* rq, const void* d_rays, uint32_t n, void* d_rng_state,
                                 void* d_out_rgb, void* d_out_segments, void* hip_stream) {
    return guarded([&] { return rt_scene_trace_device_impl(sc, rq, d_rays, n, d_rng_state, d_out_rgb, d_out_segments, hip_stream); });
}
RT_API int rt_scene_light_count(rt_scene* sc, uint32_t* n_lights) {
    return guarded([&] { return rt_scene_light_count_impl(sc, n_lights); });
}
RT_API int rt_scene_light_table(rt_scene* sc, uint32_t flags, uint32_t* out_world_index, float* out_p, uint32_t capacity) {
    return guarded([&] { return rt_scene_light_table_impl(sc, flags, out_world_index, out_p, capacity); });
}
RT_API int rt_scene_set_light_sampling(rt_scene* sc, uint32_t sampling) {
    return guarded([&] { return rt_scene_set_light_sampling_impl(sc, sampling); });
}
RT_API int rt_scene_light_sampling(rt_scene* sc, uint32_t* out_sampling) {
    return guarded([&] { return rt_scene_light_sampling_impl(sc, out_sampling); });
}
RT_API int rt_scene_set_glossy_sampling(rt_scene* sc, uint32_t sampling) {
    return guarded([&] { return rt_scene_set_glossy_sampling_impl(sc, sampling); });
}
RT_API int rt_scene_glossy_sampling(rt_scene* sc, uint32_t* out_sampling) {
    return guarded([&] { return rt_scene_glossy_sampling_impl(sc, out_sampling); });
}
RT_API int rt_scene_direct(rt_scene* sc, const rt_direct_request* rq, const rt_hit* hits, uint32_t n, uint64_t* rng_state, const uint32_t* active,
                           uint32_t n_active, rt_direct* out, rt_tile_stats* stats) {
    return guarded([&] { return rt_scene_direct_impl(sc, rq, hits, n, rng_state, active, n_active, out, stats); });
}
RT_API int rt_scene_direct_device(rt_scene* sc, const rt_direct_request* rq, const void* d_hits, uint32_t n, void* d_rng_state, const void* d_active,
                                  const void* d_n_active, void* d_out, void* hip_stream) {
    return guarded([&] {
        return rt_scene_direct_device_impl(sc, rq, d_hits, n, d_rng_state, d_active, d_n_active, d_out, hip_stream);
    });
}
RT_API int rt_scene_trace_nee(rt_scene* sc, const rt_nee_request* rq, const rt_ray* rays, uint32_t n, uint64_t* rng_state, float* out_rgb,
                              uint32_t* out_segments, uint32_t* out_shadow, rt_tile_stats* stats) {
    return guarded([&] { return rt_scene_trace_nee_impl(sc, rq, rays, n, rng_state, out_rgb, out_segments, out_shadow, stats); });
}
RT_API int rt_scene_trace_nee_device(rt_scene* sc, const rt_nee_request* rq, const void* d_rays, uint32_t n, void* d_rng_state, void* d_out_rgb,
                                     void* d_out_segments, void* d_out_shadow, void* hip_stream) {
    return guarded([&] {
        return rt_scene_trace_nee_device_impl(sc, rq, d_rays, n, d_rng_state, d_out_rgb, d_out_segments, d_out_shadow, hip_stream);
    });
}
RT_API int rt_scene_bounce(rt_scene* sc, const rt_bounce_request* rq, rt_ray* rays, uint32_t n, uint64_t* rng_state, const uint32_t* active,
                           uint32_t n_active, rt_bounce* out_bounce, rt_hit* out_hits, uint32_t* next_active, uint32_t* n_next,
                           rt_tile_stats* stats) {
    return guarded([&] { return rt_scene_bounce_impl(sc, rq, rays, n, rng_state, active, n_active, out_bounce, out_hits, next_active, n_next, stats); });
}
RT_API int rt_scene_bounce_device(rt_scene* sc, const rt_bounce_request* rq, void* d_rays, uint32_t n, void* d_rng_state, const void* d_active,
                                  const void* d_n_active, void* d_bounce, void* d_hits, void* d_next_active, void* d_n_next, void* hip_stream) {
    return guarded([&] {
        return rt_scene_bounce_device_impl(sc, rq, d_rays, n, d_rng_state, d_active, d_n_active, d_bounce, d_hits, d_next_active, d_n_next, hip_stream);
    });
}
RT_API int rt_scene_render_aov(rt_scene* sc, const rt_tile_request* rq, uint32_t sample_begin, uint32_t sample_end,
                               const rt_aov_planes* planes, rt_tile_stats* stats) {
    return guarded([&] { return rt_scene_render_aov_impl(sc, rq, sample_begin, sample_end, planes, stats); });
}
RT_API int rt_scene_render_aovs_device(rt_scene* sc, const rt_tile_request* reqs, uint32_t n, uint32_t sample_begin,
                                       uint32_t sample_end, const rt_aov_planes* d_planes, void* hip_stream) {
    return guarded([&] { return rt_scene_render_aovs_device_impl(sc, reqs, n, sample_begin, sample_end, d_planes, hip_stream); });
}
RT_API void rt_camera_defaults(rt_camera* cam) {
    if (!cam) return;
    std::memset(cam, 0, sizeof *cam);
    cam->target[2] = -1.0f;           // looking down -z (main.rs:42-50)
    cam->up[1] = 1.0f;
}
RT_API int rt_scene_set_camera(rt_scene* sc, const rt_camera* cam) { return guarded([&] { return rt_scene_set_camera_impl(sc, cam); }); }
RT_API int rt_scene_camera_rays(rt_scene* sc, const rt_tile_request* rq, uint32_t sample_begin, uint32_t sample_end, rt_ray* rays,
                                uint64_t* rng_state, rt_tile_stats* stats) {
    return guarded([&] { return rt_scene_camera_rays_impl(sc, rq, sample_begin, sample_end, rays, rng_state, stats); });
}
RT_API int rt_scene_camera_rays_device(rt_scene* sc, const rt_tile_request* rq, uint32_t sample_begin, uint32_t sample_end, void* d_rays,
                                       void* d_rng_state, void* hip_stream) {
    return guarded([&] { return rt_scene_camera_rays_device_impl(sc, rq, sample_begin, sample_end, d_rays, d_rng_state, hip_stream); });
}
RT_API void rt_denoise_request_defaults(rt_denoise_request* r) {
    if (!r) return;
    std::memset(r, 0, sizeof *r);
    r->color_samples = 1;
    r->aov_samples = 1;
    r->iterations = 5;
    r->k_color = 0.01f;            // (chosen on the quality test's c2 and quad_room inputs)
    r->color_step_scale = 4.0f;
    r->k_normal = 1.0f;
    r->k_depth = 4.0f;
    r->albedo_eps = 0.00390625f;
}
RT_API size_t rt_denoise_scratch_bytes(uint32_t width, uint32_t rows) {
    return rtplan::plan_denoise(width, rows, 0, false).scratch_bytes;
}
RT_API int rt_scene_denoise(rt_scene* sc, const rt_tile_request* reqs, uint32_t n, const rt_denoise_request* dreq,
                            const float* const* accum, const rt_aov_planes* planes, uint8_t* const* out_rgb, size_t out_len_each,
                            float* const* out_f32, float* const* out_linear, rt_tile_stats* stats) {
    return guarded([&] {
        return rt_scene_denoise_impl(sc, reqs, n, dreq, accum, planes, out_rgb, out_len_each, out_f32, out_linear, stats);
    });
}
RT_API int rt_scene_denoise_device(rt_scene* sc, const rt_tile_request* reqs, uint32_t n, const rt_denoise_request* dreq,
                                   const void* const* d_accum, const rt_aov_planes* d_planes, void* const* d_out_rgb,
                                   size_t out_len_each, void* const* d_out_f32, void* const* d_out_linear, void* d_scratch,
                                   size_t scratch_bytes, void* hip_stream) {
    return guarded([&] {
        return rt_scene_denoise_device_impl(sc, reqs, n, dreq, d_accum, d_planes, d_out_rgb, out_len_each, d_out_f32, d_out_linear,
                                            d_scratch, scratch_bytes, hip_stream);
    });
}
RT_API int rt_scene_render_tiles(rt_scene* sc, const rt_tile_request* rqs, uint32_t n, uint8_t* const* out_rgb,
                                 size_t out_len_each, float* const* out_f32, rt_tile_stats* stats) {
    return guarded([&] { return rt_scene_render_tiles_impl(sc, rqs, n, out_rgb, out_len_each, out_f32, stats); });
}
RT_API int rt_scene_render_tile_pass(rt_scene* sc, const rt_tile_request* rq, uint32_t sample_begin, uint32_t sample_end, float* accum,
                                     uint8_t* out_rgb, size_t out_len, float* out_f32, rt_tile_stats* stats) {
    return guarded([&] { return rt_scene_render_tile_pass_impl(sc, rq, sample_begin, sample_end, accum, out_rgb, out_len, out_f32, stats); });
}
RT_API int rt_scene_render_tiles_pass_device(rt_scene* sc, const rt_tile_request* reqs, uint32_t n, uint32_t sample_begin,
                                             uint32_t sample_end, void* const* d_accum, void* const* d_out_rgb, size_t out_len_each,
                                             void* const* d_out_f32, void* hip_stream) {
    return guarded([&] {
        return rt_scene_render_tiles_pass_device_impl(sc, reqs, n, sample_begin, sample_end, d_accum, d_out_rgb, out_len_each,
                                                      d_out_f32, hip_stream);
    });
}
RT_API int rt_scene_render_tile(rt_scene* sc, const rt_tile_request* rq, uint8_t* out_rgb, size_t out_len, float* out_f32,
                                rt_tile_stats* stats) {
    return guarded([&] { return rt_scene_render_tile_impl(sc, rq, out_rgb, out_len, out_f32, stats); });
}
RT_API int rt_render_tile(int device, const rt_tile_request* rq, const rt_sphere* sp, uint32_t ns, const rt_triangle* tr,
                          uint32_t nt, const uint32_t* world_index, uint8_t* out_rgb, size_t out_len, float* out_f32,
                          rt_tile_stats* stats) {
    return guarded([&] { return rt_render_tile_impl(device, rq, sp, ns, tr, nt, world_index, out_rgb, out_len, out_f32, stats); });
}
RT_API int rt_render_frame(const int* devices, int n_devices, const rt_tile_request* rq, const rt_sphere* sp, uint32_t ns,
                           const rt_triangle* tr, uint32_t nt, const uint32_t* world_index, uint8_t* out_rgb, size_t out_len,
                           rt_tile_stats* stats) {
    return guarded([&] { return rt_render_frame_impl(devices, n_devices, rq, sp, ns, tr, nt, world_index, out_rgb, out_len, stats); });
}
RT_API int rt_frame_ctx_create(const int* devices, int n_devices, rt_frame_ctx** out) {
    return guarded([&] { return rt_frame_ctx_create_impl(devices, n_devices, out); });
}
RT_API int rt_frame_ctx_set_world(rt_frame_ctx* fc, const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt,
                                  const uint32_t* world_index) {
    return guarded([&] { return rt_frame_ctx_set_world_impl(fc, sp, ns, tr, nt, world_index); });
}
RT_API int rt_frame_ctx_set_camera(rt_frame_ctx* fc, const rt_camera* cam) {
    return guarded([&] { return rt_frame_ctx_set_camera_impl(fc, cam); });
}
RT_API int rt_frame_ctx_render(rt_frame_ctx* fc, const rt_tile_request* rq, uint8_t* out_rgb, size_t out_len, rt_frame_stats* stats) {
    return guarded([&] { return rt_frame_ctx_render_impl(fc, rq, out_rgb, out_len, stats); });
}
RT_API int rt_frame_ctx_release_buffer(rt_frame_ctx* fc) { return guarded([&] { return rt_frame_ctx_release_buffer_impl(fc); }); }
RT_API void rt_frame_ctx_destroy(rt_frame_ctx* fc) { (void)guarded([&] { return rt_frame_ctx_destroy_impl(fc); }); }
// The file the library's HIP calls are bound to (rt_tile.h).  A process may hold two HIP runtimes — PyTorch wheels bundle their own
// libamdhip64.so (no SONAME), this library asks for ROCm's libamdhip64.so.7 — and the dynamic loader binds this library's hip*
// symbols to whichever came FIRST in the global scope (profiles/README.md, "two HIP runtimes in one process").  A host that makes
// its own streams or device buffers for the *_device entry points must make them with THIS runtime; the Python mirror uses it to
// refuse a process in which torch and the library would drive the device through different ones.
RT_API size_t rt_hip_runtime_path(char* buf, size_t cap) {
    Dl_info info;
    std::memset(&info, 0, sizeof info);
    if (!dladdr(reinterpret_cast<const void*>(&hipGetDeviceCount), &info) || !info.dli_fname) return 0;
    const size_t n = std::strlen(info.dli_fname);
    if (buf && cap) {
        const size_t m = n < cap - 1 ? n : cap - 1;
        std::memcpy(buf, info.dli_fname, m);
        buf[m] = 0;
    }
    return n;
}
}  // extern "C"
