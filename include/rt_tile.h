/*
 * rt_tile.h — C-ABI of the MI355X path-trace tile renderer.
 *
 * Drop-in boundary for ONE hot path of actuday6418/ray-tracer-s8: the body of the
 * slave's `worker()` NewJob arm (reference ray-tracer-slave/src/main.rs:37-83) and
 * everything it calls (`ray_color` main.rs:108-146, `Camera::get_ray` camera.rs:109-129,
 * `WorldRefList::intersect` shapes/mod.rs:158-191, Sphere/Triangle `get_roots`).
 *
 * The reference has no FFI; its seam is the controller->slave JSON `RenderInfo`
 * (ray-tracer-slave/src/lib.rs:10-15) answered by `ImageSlice` (lib.rs:17-22).  This
 * header carries exactly those fields as POD, plus the knobs the reference hard-codes
 * (main.rs:39,42-51; shapes/mod.rs:12-13) with the reference literals as defaults.
 *
 * Plain C: POD structs, pointers and sizes only.  A Rust `extern "C"` block, cgo or
 * ctypes can bind it verbatim.
 *
 * Every function returns an `rt_status` (0 = OK, negative = error) and never throws
 * or aborts across the boundary (the reference panics via `.unwrap()`).  Caller owns
 * every pointer before and after each call; the library copies in and retains nothing
 * outside an explicit `rt_scene` handle.
 */
#ifndef RT_TILE_H
#define RT_TILE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define RT_API
#else
#define RT_API __attribute__((visibility("default")))
#endif

#define RT_ABI_VERSION 4u      /* 2: rt_tile_stats.node_steps appended
                                  3: `world_index` (the position of every primitive in RenderInfo.world) on the entry
                                     points that take a world; the persistent frame context rt_frame_ctx_*;
                                     RT_FLAG_FRAME_QUEUE / RT_FLAG_FRAME_NO_PIN replace two environment variables
                                  4: the deterministic RNG is one stream per (pixel, SAMPLE) (see `seed` below: same seed,
                                     other images than ABI 3); RT_MAX_SPP; rt_hip_runtime_path(); the frame context assigns
                                     strips by measured cost and reports the balance (rt_frame_stats.balance_*,
                                     RT_FLAG_FRAME_STATIC)
                                  (4, additions only: ray queries rt_scene_intersect / rt_scene_intersect_device with
                                     rt_ray, rt_hit, RT_HIT_NONE, RT_QUERY_*; every earlier type and entry point unchanged)
                                  (4, additions only: path tracing of caller rays rt_scene_trace / rt_scene_trace_device with
                                     rt_trace_request, RT_TRACE_RAY_*)
                                  (4, additions only: feature buffers of a strip rt_scene_render_aov /
                                     rt_scene_render_aovs_device with rt_aov_planes)
                                  (4, additions only: the edge-avoiding a-trous denoiser rt_scene_denoise /
                                     rt_scene_denoise_device with rt_denoise_request, RT_DENOISE_MAX_ITERATIONS)
                                  (4, additions only: direct lighting of caller rays rt_scene_light_count / rt_scene_direct /
                                     rt_scene_direct_device with rt_direct_request, rt_direct, RT_DIRECT_*)
                                  (4, additions only: next-event estimation for caller rays rt_scene_trace_nee /
                                     rt_scene_trace_nee_device with rt_nee_request, RT_NEE_*)
                                  (4, additions only: light selection by power RT_FLAG_LIGHTS_BY_POWER for rt_scene_direct* and
                                     rt_scene_trace_nee*, rt_scene_light_table)
                                  (4, additions only: cone sampling of sphere lights RT_LIGHTS_AREA / RT_LIGHTS_CONE with
                                     rt_scene_set_light_sampling / rt_scene_light_sampling)
                                  (4, additions only: light samples at glossy hits RT_GLOSSY_BOUNCE / RT_GLOSSY_MIS with
                                     rt_scene_set_glossy_sampling / rt_scene_glossy_sampling) */

/* ---- status codes --------------------------------------------------------------- */
typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_BAD_ARG = -1,        /* null pointer, zero size, division_no >= divisions ...      */
    RT_ERR_NOT_INITIALIZED = -2,/* rt_init() not called / failed                              */
    RT_ERR_NO_DEVICE = -3,      /* no MI355X-class HIP device visible (no CPU fallback)       */
    RT_ERR_BAD_DEVICE = -4,     /* device ordinal out of range                                */
    RT_ERR_BUFFER_TOO_SMALL = -5,/* out_len < (H/div)*W*3                                     */
    RT_ERR_FRAME_SIZE = -6,     /* frame assembly asked with height % divisions != 0
                                   (reference controller panics: controller/src/main.rs:117-119) */
    RT_ERR_HIP = -7,            /* a HIP runtime call failed; see rt_last_error()             */
    RT_ERR_LIMIT = -8,          /* max_bounces > RT_MAX_BOUNCES, n_spheres too large ...      */
    RT_ERR_OOM = -9             /* host or device allocation failed                           */
} rt_status;

#define RT_MAX_BOUNCES 62u      /* path stack depth limit (reference literal is 10)           */
#define RT_MAX_SPP 4096u        /* samples per pixel limit (reference literal is 100)         */
#define RT_MAX_PRIMITIVES 0x3ffffffu /* spheres + triangles per scene: the kernels address nodes, geometry and
                                   materials with 32-bit byte offsets (64 B per tree node)    */

/* ---- scene primitives ----------------------------------------------------------- */

/* = reference `Sphere` (ray-tracer-slave/src/shapes/sphere.rs:12-20) minus `node_index`
 * (a BVH back-pointer the linear GPU scan does not use).  36 bytes, no padding. */
typedef struct rt_sphere {
    float cx, cy, cz;           /* center                                                     */
    float radius;
    float albedo_r, albedo_g, albedo_b; /* p_albedo_at                                        */
    float roughness;            /* p_roughness_at: 0 = Lambertian, 1 = mirror (main.rs:122)   */
    float emission;             /* p_emission_at: > 0 terminates the path (main.rs:116-117)   */
} rt_sphere;

/* = reference `Triangle` (ray-tracer-slave/src/shapes/mesh.rs:14-23) minus `node_index`.
 * 56 bytes, no padding. */
typedef struct rt_triangle {
    float a[3], b[3], c[3];
    float albedo_r, albedo_g, albedo_b;
    float roughness;
    float emission;
} rt_triangle;

/* ---- tile request = RenderMeta + division_no + the hard-coded knobs ------------- */

enum {
    RT_FLAG_NONE = 0u,
    /* Disable the conservative broad-phase filter: run the reference's exact root
     * computation against every primitive (slow; used by tests to prove the filter
     * never changes a result). */
    RT_FLAG_EXACT_SCAN = 1u << 0,
    /* Plain linear-scan semantics: do not apply the reference's BVH candidate culling
     * (bvh_impl.rs:373-398) to accepted hits and break distance ties by primitive index.
     * Default (flag clear) reproduces the reference: a hit counts only if BVH::traverse would
     * have returned the primitive, ties go to the earlier DFS leaf. */
    RT_FLAG_NO_BVH_CULL = 1u << 1,
    /* Force the 11-op "oc" broad phase even when the scene qualifies for the 8-op expanded
     * form (A/B testing; both are conservative and give identical images). */
    RT_FLAG_OC_BROAD_PHASE = 1u << 2,
    /* Walk the whole root-to-leaf AABB chain when validating a hit instead of using the
     * leaf-box monotonicity shortcut (A/B testing; identical images). */
    RT_FLAG_FULL_CHAIN = 1u << 3,
    /* Closest-hit engine.  Default: linear scan over the LDS-resident primitive list for scenes up to 32
     * spheres (and no mesh), per-lane traversal of the reference BVH above that.  Both give the
     * reference's result bit for bit; these force one or the other (A/B runs, tests). */
    RT_FLAG_BVH_TRAVERSE = 1u << 4,
    RT_FLAG_LINEAR_SCAN = 1u << 5,
    /* Traversal node format.  Default: the exact 64-byte nodes below 4096 primitives and for meshes, the
     * 32-byte conservatively quantised nodes (exact validation at the leaves) for larger sphere scenes.  Identical images;
     * these force one or the other (A/B runs, tests). */
    RT_FLAG_EXACT_NODES = 1u << 6,
    RT_FLAG_QUANT_NODES = 1u << 7,
    /* A tree whose exact nodes fit a CU's LDS (about 1000 primitives) is walked from an LDS-resident copy by default;
     * this flag keeps the nodes in HBM / L2 (A/B runs, tests).  Identical images. */
    RT_FLAG_NO_LDS_TREE = 1u << 8,
    /* Measurement aid (bench.py's roofline object): run the traversal kernel's counting twin, which also counts the
     * internal BVH nodes visited (rt_tile_stats.node_steps).  Same image; a few per cent slower, never the timed launch. */
    RT_FLAG_COUNT_STEPS = 1u << 9,
    /* Quantised walk, nearer child first, skipping every subtree whose box the ray enters beyond the running closest hit by
     * more than a proven slack (identical images).  Default for sphere scenes on the quantised nodes, and for scenes with
     * triangles on the exact nodes, that are dense enough for it to pay (c5, terrains); these force it on / off (A/B runs, tests). */
    RT_FLAG_CULL_WALK = 1u << 10,
    RT_FLAG_NO_CULL_WALK = 1u << 11,
    /* Frame-level flags (rt_render_frame / rt_frame_ctx_render only; the tile entry points ignore them).
     * FRAME_QUEUE: the devices pull strips one at a time, bottom of the frame (the expensive strips) first, from a shared
     * host-atomic queue, two launches in flight per device, instead of the static split strip k -> devices[k % n].
     * FRAME_NO_PIN: do not page-lock the caller's frame buffer (downloads then go through the runtime's staging). */
    RT_FLAG_FRAME_QUEUE = 1u << 12,
    RT_FLAG_FRAME_NO_PIN = 1u << 13,
    /* FRAME_STATIC: the plain split strip k -> devices[k % n] (rounds 1-3; A/B runs, tests) instead of the default, which
     * balances the devices by the strips' cost: see "Strip assignment" at rt_frame_ctx below. */
    RT_FLAG_FRAME_STATIC = 1u << 14,
    /* Light sampling (rt_scene_direct*, rt_scene_trace_nee* only; every other entry point ignores it): the emitter of a light sample
     * is picked by power, not uniformly: see "light selection by power" below. */
    RT_FLAG_LIGHTS_BY_POWER = 1u << 15
};

typedef struct rt_tile_request {
    /* RenderMeta (lib.rs:24-30); `id` (UUID) is opaque to the renderer, stays with caller */
    uint32_t width;             /* image width  W                                             */
    uint32_t height;            /* image height H                                             */
    uint32_t divisions;         /* number of horizontal strips; strip height Hs = H / div     */
    /* RenderInfo.division_no (lib.rs:14): strip index, 0 = TOP of the image (main.rs:66-71)  */
    uint32_t division_no;
    /* knobs the reference hard-codes; rt_tile_request_defaults() fills the literals         */
    uint32_t spp;               /* sample_count   = 100   (main.rs:51)                        */
    uint32_t max_bounces;       /* max_bounces    = 10    (main.rs:39); ray_color depth = +1  */
    float aperture;             /* 0.1            (main.rs:45)                                */
    float focus_distance;       /* 1.0            (main.rs:46)                                */
    float fov;                  /* PI/2 (f32)     (main.rs:47)                                */
    float focal_length;         /* 1.0            (main.rs:48)                                */
    float t_min;                /* 0.001          (shapes/mod.rs:12)                          */
    float t_max;                /* 1000.0         (shapes/mod.rs:13), half-open [t_min,t_max) */
    /* new: replaces `SmallRng::from_entropy()` per row (main.rs:69).  Sample s (0 .. spp-1) of the pixel in global row y,
     * column x of the frame draws from its own xoshiro256++ stream,
     *     SmallRng::seed_from_u64(seed + 4 * 0x9E3779B97F4A7C15 * ((y * width + x) * spp + s))      (wrapping u64)
     * i.e. the SplitMix64 sequence of `seed` cut into consecutive blocks of four outputs, one block per (pixel, sample);
     * the pixel is the f32 sum of its samples' colours in the order s = 0, 1, ... as main.rs:73-77 forms it.  Strips of a
     * frame rendered with one seed therefore stitch to exactly the single-strip frame.  DESIGN.md 3 "RNG";
     * tests/test_rng_distribution.py checks the images' distribution against the reference's stream-per-row structure. */
    uint64_t seed;
    uint32_t flags;             /* RT_FLAG_*                                                  */
    uint32_t reserved;          /* must be 0                                                  */
} rt_tile_request;

typedef struct rt_tile_stats {
    uint64_t ray_segments;      /* ray_color entries with depth > 0 (closest-hit queries)     */
    uint64_t primary_rays;      /* Hs * W * spp                                               */
    uint64_t broad_candidates;  /* primitives that passed the broad phase (0 in exact scan)   */
    uint64_t exact_fallbacks;   /* segments whose candidate list overflowed (exact rescans)   */
    float kernel_ms;            /* HIP-event time of the kernel(s) of this call               */
    float h2d_ms;               /* scene upload (0 when a resident rt_scene is used)          */
    float d2h_ms;               /* RGB8 strip download (0 for device output)                  */
    uint32_t n_launches;        /* kernel launches issued by this call                        */
    uint32_t engine;            /* closest-hit engine of the last launch: 0 linear scan (scene resident
                                   in LDS), 1 linear scan (scene streamed through LDS), 2 BVH traversal (exact nodes),
                                   3 BVH traversal (quantised nodes + exact leaf validation),
                                   4 BVH traversal, exact nodes resident in LDS,
                                   5 BVH traversal, quantised nodes, nearer child first with distance culling,
                                   6 BVH traversal, exact nodes, nearer child first with distance culling (scenes with triangles),
                                   7 BVH traversal, exact nodes resident in LDS, nearer child first with distance culling */
    uint32_t broad_form;        /* linear engines: 0 = oc form, 1 = expanded form   */
    uint64_t node_steps;        /* traversal engines under RT_FLAG_COUNT_STEPS: internal BVH nodes visited
                                   (each = two child-box slab tests); 0 otherwise.  broad_candidates = leaves
                                   reached = exact root tests for these engines */
} rt_tile_stats;

/* ---- lifecycle ------------------------------------------------------------------ */

/* Enumerate HIP devices, create one context (stream + events + counters) per device.
 * *n_devices may be NULL.  Returns RT_ERR_NO_DEVICE if none: there is NO CPU fallback. */
RT_API int rt_init(int* n_devices);
/* Refused (no effect; rt_last_error() says so) while any rt_scene is alive: destroy the scenes first. */
RT_API void rt_shutdown(void);
RT_API uint32_t rt_abi_version(void);
/* The libamdhip64 file this library's HIP calls are bound to (a process may map two HIP runtimes, e.g. a PyTorch wheel's
 * own next to ROCm's; the dynamic loader binds the library to whichever was loaded first).  A host that passes its own
 * hipStream_t / device pointers to the *_device entry points must make them with THIS runtime.  Copies at most cap - 1
 * characters and a terminator into buf (which may be NULL); returns the path's length, 0 if unknown. */
RT_API size_t rt_hip_runtime_path(char* buf, size_t cap);
RT_API const char* rt_strerror(int status);
/* Last error message of the calling thread ("" if none). */
RT_API const char* rt_last_error(void);

/* Fill the reference literals (main.rs:39-51, shapes/mod.rs:12-13, controller main.rs:33-39:
 * 1920x1080, 20 divisions); seed 0, flags 0. */
RT_API void rt_tile_request_defaults(rt_tile_request* req);

/* Bytes of one strip = (H / div) * W * 3  (main.rs:53-59).  0 on bad args. */
RT_API size_t rt_tile_bytes(const rt_tile_request* req);

/* ---- the world's order ------------------------------------------------------------ */
/* RenderInfo.world is ONE list, `Vec<Object>`, whose entries are spheres or triangles in any order
 * (ray-tracer-slave/src/lib.rs:11, shapes/mod.rs:23-27), and that order is observable: BVH::build numbers the shapes by
 * their position in it (bvh_impl.rs:421-427), so the halves of its `split_at(len / 2)` fallback (:277-291), the order of
 * the leaves BVH::traverse returns, and with it the winner among hits at exactly equal distance (`min_by` keeps the first,
 * shapes/mod.rs:177-182) all follow it.  The ABI carries the world as two typed arrays; `world_index` restores the order:
 * world_index[i] (i < n_spheres) is the position of spheres[i] in RenderInfo.world, world_index[n_spheres + j] that of
 * triangles[j]; it must be a permutation of 0 .. n_spheres + n_triangles - 1 (else RT_ERR_BAD_ARG).  NULL means the
 * spheres in their order followed by the triangles in theirs.  Copied during the call; the caller keeps ownership. */

/* ---- one strip, host buffers: replaces slave main.rs:53-83 ---------------------- */

/* Render strip `req->division_no` of the frame on `device` into out_rgb
 * (= ImageSlice.image: Hs*W*3 bytes, RGB8, row-major, top row of the strip first).
 * Synchronous.  Thread-safe across devices; calls on one device serialise.
 * Empty world (n_spheres + n_triangles == 0) renders the sky (the reference recurses
 * without bound in BVH::build, bvh_impl.rs:229-364).
 * Like the slave, accepts height % divisions != 0 and renders floor(H/div) rows.
 * out_f32 (optional, may be NULL): Hs*W*3 floats, post-gamma pre-quantise pixel values. */
RT_API int rt_render_tile(int device, const rt_tile_request* req,
                          const rt_sphere* spheres, uint32_t n_spheres,
                          const rt_triangle* triangles, uint32_t n_triangles,
                          const uint32_t* world_index,
                          uint8_t* out_rgb, size_t out_len,
                          float* out_f32, rt_tile_stats* stats);

/* ---- resident scene: upload the world once per device per job ------------------- */
/* (the reference re-sends and re-builds per strip: controller main.rs:58-62, slave main.rs:60) */

typedef struct rt_scene rt_scene;

RT_API int rt_scene_create(int device,
                           const rt_sphere* spheres, uint32_t n_spheres,
                           const rt_triangle* triangles, uint32_t n_triangles,
                           const uint32_t* world_index,
                           rt_scene** out_scene);
RT_API void rt_scene_destroy(rt_scene* scene);

/* Same as rt_render_tile, scene already in HBM. */
RT_API int rt_scene_render_tile(rt_scene* scene, const rt_tile_request* req,
                                uint8_t* out_rgb, size_t out_len,
                                float* out_f32, rt_tile_stats* stats);

/* Asynchronous, device-resident output: enqueue the strip on `hip_stream`
 * (a hipStream_t; NULL = the scene's own stream) writing RGB8 to device memory
 * d_out_rgb (>= rt_tile_bytes) and, if non-NULL, floats to d_out_f32.
 * Counters and HIP-event timings accumulate in the scene until rt_scene_collect().
 * Launches of one scene may be spread over several streams and overlap; the library chains only
 * those that share per-scene scratch (the capped-stack walk of trees deeper than the LDS stack). */
RT_API int rt_scene_render_tile_device(rt_scene* scene, const rt_tile_request* req,
                                       void* d_out_rgb, size_t out_len,
                                       void* d_out_f32, void* hip_stream);

/* Batched form: n strips of ONE frame (all fields equal except division_no and seed) are
 * rendered by a single launch of persistent waves that pull 64x1-pixel tiles of all n strips
 * from one queue — no per-strip launch tail.  d_out_rgb[i] receives strip i; d_out_f32 may
 * be NULL (or an array with NULL entries).  RT_ERR_BAD_ARG if the requests differ in any
 * frame-level field. */
RT_API int rt_scene_render_tiles_device(rt_scene* scene, const rt_tile_request* reqs, uint32_t n,
                                        void* const* d_out_rgb, size_t out_len_each,
                                        void* const* d_out_f32, void* hip_stream);

/* Host-buffer batched form (synchronous): one launch, then one D2H copy per strip. */
RT_API int rt_scene_render_tiles(rt_scene* scene, const rt_tile_request* reqs, uint32_t n,
                                 uint8_t* const* out_rgb, size_t out_len_each,
                                 float* const* out_f32, rt_tile_stats* stats);

/* ---- progressive rendering: a strip's samples in passes over a running sum ------- */
/* Replaces the one-shot sample loop of slave main.rs:73-81 (`for _ in 0..sample_count { pix_color += ray_color(..) }`, then
 * mean, gamma and quantise) with passes that a caller can preview, bound in time, stop or continue.
 *
 * A PASS renders samples [sample_begin, sample_end) of the S = req->spp sample image; 0 <= sample_begin < sample_end <= S,
 * else RT_ERR_BAD_ARG (and nothing is launched).  Every check of the one-pass entry points applies as well.
 *   - Sample s of a pixel draws from exactly the stream it draws from in one pass: seed + 4 PHI ((y W + x) S + s) (`seed`
 *     above), S being the JOB's spp, not sample_end - sample_begin.
 *   - accum: Hs*W*3 floats laid out like out_f32, in/out, the pixels' RAW colour sums (not means).  For sample_begin > 0 each
 *     pixel's sum starts from accum; for sample_begin == 0 it starts from 0 and accum is not read (it may be uninitialised).
 *     After the pass accum holds the sum over samples [0, sample_end), added one sample at a time in the order s = 0, 1, ...
 *     NULL: RT_ERR_BAD_ARG.
 *   - out_rgb / out_f32 (optional, as for rt_scene_render_tile) receive the preview sqrt(accum / sample_end), quantised as
 *     main.rs:78-81 does.
 *   - The f32 sum of a pixel after [0, k) is a prefix of the one-pass sum, so the pass with sample_end == S writes out_rgb and
 *     out_f32 BIT-IDENTICAL to rt_scene_render_tile of the same request, however [0, S) was split into passes.
 *   - A preview at sample_end < S is NOT the image of a one-pass render with spp = sample_end: that one draws from other
 *     streams (its stride is sample_end).
 *   - Counters cover the pass: primary_rays = Hs*W*(sample_end - sample_begin); the ray_segments of the passes add up to the
 *     one-pass count.
 * Scratch and every launch parameter are sized by the samples of the PASS: a job at RT_MAX_SPP in passes of 64 keeps the
 * sample-unit ring at its 64-sample size.   */

/* Host buffers, synchronous.  accum (Hs*W*3 floats) is uploaded when sample_begin > 0 and always downloaded. */
RT_API int rt_scene_render_tile_pass(rt_scene* scene, const rt_tile_request* req,
                                     uint32_t sample_begin, uint32_t sample_end, float* accum,
                                     uint8_t* out_rgb, size_t out_len,
                                     float* out_f32, rt_tile_stats* stats);

/* Batched device form: the strips of one frame in a single launch (per 64 strips), asynchronous on hip_stream, under the rules of
 * rt_scene_render_tiles_device (same frame-level fields, counters accumulate until rt_scene_collect).  d_accum[i] is the
 * device running sum of strip i (no NULL entry). */
RT_API int rt_scene_render_tiles_pass_device(rt_scene* scene, const rt_tile_request* reqs, uint32_t n,
                                             uint32_t sample_begin, uint32_t sample_end,
                                             void* const* d_accum,
                                             void* const* d_out_rgb, size_t out_len_each,
                                             void* const* d_out_f32, void* hip_stream);

/* Wait for all work enqueued on the scene, return accumulated counters / event time
 * since the previous collect, and reset them. */
RT_API int rt_scene_collect(rt_scene* scene, rt_tile_stats* stats);

/* ---- ray queries: closest hit and occlusion for the caller's rays ----------------- */
/* What `WorldRefList::intersect` (ray-tracer-slave/src/shapes/mod.rs:158-191) returns for one ray after `BVH::traverse`
 * (bvh_impl.rs:373-398) has picked its candidates, for a batch of rays on a resident scene: picking, shadow and visibility
 * rays, collision probes, an integrator of the caller's own on this BVH and these root tests.
 *
 *   - Ray i is Ray::new(origin, direction) (B/ray.rs:133-143): the direction is normalised by DIVISION by its length, so a
 *     zero or non-finite direction gives NaN components (and no hit).  A root counts when it lies in the ray's own half-open
 *     window [t_min, t_max) (shapes/mod.rs:106-129); t_min >= t_max admits nothing, t_max may be +inf.
 *   - RT_QUERY_CLOSEST: the primitive WorldRefList::intersect picks, with its tie rule (min_by keeps the FIRST minimum of
 *     |P - origin| over the traversal's candidates, i.e. the earlier depth-first leaf; under RT_FLAG_NO_BVH_CULL the earlier
 *     position in the world).
 *       index     the primitive's position in RenderInfo.world: world_index[i] of the scene's rt_scene_create when one was
 *                 given, else the spheres (0 .. n_spheres - 1) followed by the triangles;
 *       p*        the hit point o + t d (Ray::at, ray.rs:147-149);
 *       distance  length(P - o), the value the reference compares (shapes/mod.rs:177-182);
 *       n*        the normal the reference computes: normalize_or_zero(P - centre) for a sphere (sphere.rs:49-51),
 *                 normalize_or_zero((a - b) x (a - c)) for a triangle (mesh.rs:163-165).
 *     A miss: index = RT_HIT_NONE, distance = +inf, every other field 0.
 *   - RT_QUERY_ANY (occlusion): index != RT_HIT_NONE exactly when the closest query would hit; the walk may stop at the first
 *     admitted hit, so the index is that of SOME admitted primitive and the other fields are unspecified.
 *   - flags: the RT_FLAG_* bits of the tile entry points, same meaning.  Default: BVH semantics (a hit counts only if
 *     BVH::traverse would return the primitive), walked over the exact nodes.  RT_FLAG_NO_BVH_CULL: plain scan in world order.
 *     RT_FLAG_EXACT_SCAN / RT_FLAG_LINEAR_SCAN: BVH semantics by a scan of every primitive with per-hit validation.
 *     RT_FLAG_FULL_CHAIN: the crate's literal slab test throughout.  RT_FLAG_BVH_TRAVERSE, RT_FLAG_NO_LDS_TREE: the walk (the
 *     default).  Flags naming an engine the query path does not have (RT_FLAG_QUANT_NODES, RT_FLAG_EXACT_NODES,
 *     RT_FLAG_CULL_WALK, RT_FLAG_NO_CULL_WALK, RT_FLAG_COUNT_STEPS, RT_FLAG_OC_BROAD_PHASE, the RT_FLAG_FRAME_* bits) are
 *     accepted and ignored: every engine gives the same hits.
 *   - RT_ERR_BAD_ARG, and nothing launched: a NULL scene, rays or hits pointer, n == 0, mode > RT_QUERY_ANY.
 *   - Counters (rt_tile_stats): primary_rays = ray_segments = n; broad_candidates = exact root tests run; kernel_ms; h2d_ms
 *     (the rays) and d2h_ms (the hits) of the host form; n_launches; engine = the engine that ran (numbered as
 *     rt_tile_stats.engine: 1 the scan, 2 the exact-node walk).
 *  */
typedef struct rt_ray { float ox, oy, oz, t_min; float dx, dy, dz, t_max; } rt_ray;          /* 32 bytes */
typedef struct rt_hit { float px, py, pz, distance; float nx, ny, nz; uint32_t index; } rt_hit; /* 32 bytes */
#define RT_HIT_NONE 0xffffffffu
enum { RT_QUERY_CLOSEST = 0u, RT_QUERY_ANY = 1u };

/* Host buffers (n rays in, n hits out), synchronous; stats may be NULL. */
RT_API int rt_scene_intersect(rt_scene* scene, const rt_ray* rays, uint32_t n, uint32_t mode, uint32_t flags,
                              rt_hit* hits, rt_tile_stats* stats);
/* Device buffers (n rt_ray, n rt_hit), asynchronous on hip_stream (NULL = the scene's stream); counters and event times
 * accumulate in the scene until rt_scene_collect(). */
RT_API int rt_scene_intersect_device(rt_scene* scene, const void* d_rays, uint32_t n, uint32_t mode, uint32_t flags,
                                     void* d_hits, void* hip_stream);

/* ---- path tracing of caller rays: the colour a ray sees ---------------------------- */
/* The reference's integrator on the caller's rays, for a batch of rays (rt_ray above) on a resident scene: any camera (a placed or
 * rotated pinhole, orthographic, panoramic, stereo, a custom lens), light probes and irradiance samples, sample scheduling of the
 * caller's own.
 *
 *   - Per sample: sample s of ray i is ray_color(ray_i, max_bounces + 1, rng) (ray-tracer-slave/src/main.rs:108-146): the closest
 *     hit as rt_scene_intersect finds it; on an emitter em * albedo; on any other hit a UnitSphere draw and the scattered ray
 *     diffuse + roughness (glossy - diffuse) (main.rs:119-127), which is drawn also when the depth runs out (the reference draws
 *     before ray_color(.., 0) returns black); no hit: the sky of normalize_or_zero(d).y (main.rs:135-144); the albedos multiplied
 *     right to left (main.rs:123).  Every segment of the path uses the ray's own window [t_min, t_max), as the tile request's
 *     window serves every segment of a strip.
 *   - ray_form RT_TRACE_RAY_NEW: the first ray is Ray::new(o, d) (B/ray.rs:133-143), the direction normalised by division (as
 *     rt_scene_intersect).  RT_TRACE_RAY_AS_GIVEN: the direction is taken bit for bit, as the value Camera::get_ray
 *     (camera.rs:109-129) or a bounce hands to ray_color (normalising twice is not idempotent in f32).
 *   - RNG: rng_state == NULL: sample s of ray i draws from SmallRng::seed_from_u64(seed + 4 * 0x9E3779B97F4A7C15 * (i * spp + s))
 *     (wrapping u64; the tile's stream per (pixel, sample) with the pixel index replaced by the ray index).  Otherwise rng_state
 *     holds 4 * n u64, the xoshiro256++ state (s[0..3]) of each ray, read and written back: the ray's spp samples draw one after
 *     the other from that one stream, and the state after the last draw is stored.
 *   - out_rgb (3 * n floats, required): the f32 sum of the ray's sample colours, added in the order s = 0, 1, ... starting from
 *     0 — not the mean, not gamma-corrected (the `accum` of the progressive entry points).  out_segments (n u32, optional): the
 *     ray's ray_color entries with depth > 0, summed over its samples.
 *   - flags: as for rt_scene_intersect.  Default: BVH semantics over the exact-node walk; RT_FLAG_NO_BVH_CULL the plain scan;
 *     RT_FLAG_EXACT_SCAN / RT_FLAG_LINEAR_SCAN the scan with BVH semantics; RT_FLAG_FULL_CHAIN the literal slab test; a tree
 *     deeper than the walk's stack takes the scan.  The tile-only flags are accepted and ignored.
 *   - RT_ERR_BAD_ARG, and nothing launched: a NULL scene, request, rays or out_rgb, n == 0, spp == 0, ray_form > 1.
 *     RT_ERR_LIMIT: spp > RT_MAX_SPP, max_bounces > RT_MAX_BOUNCES.
 *   - Counters (rt_tile_stats): primary_rays = n * spp; ray_segments = the sum of all segments; broad_candidates = exact root
 *     tests; kernel_ms; h2d_ms (rays and states) and d2h_ms (colours, segments, states) of the host form; n_launches; engine (as
 *     for rt_scene_intersect).
 * No per-scene scratch on the device: launches on different streams may overlap.   */
typedef struct rt_trace_request {
    uint32_t spp;               /* samples per ray, 1 .. RT_MAX_SPP                                        */
    uint32_t max_bounces;       /* 0 .. RT_MAX_BOUNCES; ray_color depth = max_bounces + 1 (as rt_tile_request) */
    uint64_t seed;              /* the seeded streams, when no RNG states are passed                       */
    uint32_t flags;             /* RT_FLAG_*, as for rt_scene_intersect                                    */
    uint32_t ray_form;          /* RT_TRACE_RAY_NEW | RT_TRACE_RAY_AS_GIVEN                                */
} rt_trace_request;             /* 24 bytes */
enum { RT_TRACE_RAY_NEW = 0u, RT_TRACE_RAY_AS_GIVEN = 1u };

/* Host buffers, synchronous; rng_state, out_segments and stats may be NULL. */
RT_API int rt_scene_trace(rt_scene* scene, const rt_trace_request* req, const rt_ray* rays, uint32_t n,
                          uint64_t* rng_state, float* out_rgb, uint32_t* out_segments, rt_tile_stats* stats);
/* Device buffers (n rt_ray, 4 n u64 or NULL, 3 n f32, n u32 or NULL), asynchronous on hip_stream (NULL = the scene's stream);
 * counters and event times accumulate in the scene until rt_scene_collect(). */
RT_API int rt_scene_trace_device(rt_scene* scene, const rt_trace_request* req, const void* d_rays, uint32_t n,
                                 void* d_rng_state, void* d_out_rgb, void* d_out_segments, void* hip_stream);

/* ---- path steps: one ray_color bounce for the caller's rays, with compaction -------- */
/* ONE entry of ray_color with depth > 0 (ray-tracer-slave/src/main.rs:108-146) as a call of its own: the hit, the shade and the
 * scatter of one segment of every active ray of a batch, for an integrator of the caller's own between the segments — next-event
 * estimation with RT_QUERY_ANY shadow rays, Russian roulette, per-bounce feature buffers, path-length filters, throughput clamps,
 * another sky — on this library's BVH, root tests and shading arithmetic.  The ray and its RNG state are updated in place, and a
 * device-side list of the rays that scattered comes back: the next step's active list, so that every wave of every step is full
 * of live rays.  K steps folded by the caller reproduce rt_scene_trace bit for bit (below).
 *
 * Per active ray i (rt_ray above); the window [t_min, t_max) is the ray's own and is kept:
 *   - Closest hit: the hit rt_scene_intersect finds under the same flags.  ray_form RT_TRACE_RAY_NEW: the direction is normalised
 *     by division first (Ray::new, B/ray.rs:133-143); RT_TRACE_RAY_AS_GIVEN: it is taken bit for bit.  The ray a step writes back
 *     must be stepped AS_GIVEN (normalising twice is not idempotent in f32).
 *   - RT_BOUNCE_MISSED: rgb = the sky of normalize_or_zero(d).y (main.rs:135-144).  The ray and the state are unchanged.
 *   - RT_BOUNCE_EMITTED (emission > 0, main.rs:116-117): rgb = albedo * emission.  The ray and the state are unchanged.
 *   - RT_BOUNCE_SCATTERED: rgb = the albedo.  One UnitSphere draw is taken from state i (main.rs:119); the scattered direction is
 *     diffuse + roughness (glossy - diffuse) (main.rs:120-122) through try_normalize with the normal as the fallback (main.rs:126),
 *     then Ray::new's normalisation; its origin is exactly the hit point P.  The scattered ray is written over ray i, the advanced
 *     state over state i: operation for operation what rt_scene_trace does between two segments.
 *   - out_hits (optional): the rt_hit of RT_QUERY_CLOSEST for the INCOMING ray; on a miss the miss record.
 *   - seed_states = 1: state i = SmallRng::seed_from_u64(seed + 4 * 0x9E3779B97F4A7C15 * i) (wrapping u64: the seeded stream of
 *     rt_scene_trace at spp = 1) is written over state i of every active ray first, whatever its status, and then stepped.
 *     rng_state is required either way.
 *   - Active list: active == NULL steps all n rays; otherwise n_active indices < n.  A ray that is not listed has no byte of its
 *     ray, state, bounce or hit record touched.  Naming a ray twice is the caller's error.  The host form checks every index and
 *     returns RT_ERR_BAD_ARG; the device form reads the length from *d_n_active ON THE DEVICE (no host synchronisation between
 *     steps), steps min(n, *d_n_active) entries and skips an index >= n.  d_active and d_n_active are both NULL (all n rays) or
 *     both given (n is then the upper bound the launch is sized from).
 *   - Compaction: next_active (optional, capacity n) receives the indices of the SCATTERED rays and *n_next their number; n_next
 *     alone counts them.  The library zeroes *n_next on the stream before the launch.  The SET is specified, its order is not (one
 *     atomic append per wave); every per-ray result lives at the ray's own index, so no result depends on that order.
 *   - Folding: the reference multiplies the albedos right to left (main.rs:123).  A caller who wants rt_scene_trace's bits keeps
 *     the rgb of every step and folds a1 * (a2 * (... (ak * term))), term the rgb of the step that MISSED or EMITTED; a ray still
 *     alive after the caller's last step folds term = 0, as the reference draws and then returns black (main.rs:119, 109-111).
 *     max_bounces = K - 1 of rt_scene_trace is K steps.
 *   - flags: as for rt_scene_intersect (a tree deeper than the walk's stack takes the scan; tile-only flags are ignored).
 *   - RT_ERR_BAD_ARG, and nothing launched: a NULL scene, request, rays, rng_state or out_bounce; n == 0; ray_form > 1;
 *     seed_states > 1; reserved != 0; next_active without n_next; one of active / n_active without the other; in the host form an
 *     index >= n or n_active > n.
 *   - Counters (rt_tile_stats): ray_segments = rays stepped; broad_candidates = exact root tests; primary_rays = 0; kernel_ms;
 *     h2d_ms (rays, states, the active list) and d2h_ms (rays, states, bounces, hits, the next list and its count) of the host
 *     form; n_launches; engine (as for rt_scene_intersect).
 * No per-scene scratch on the device: launches on different streams may overlap.   */
typedef struct rt_bounce { float r, g, b; uint32_t status; } rt_bounce;                       /* 16 bytes */
enum { RT_BOUNCE_SCATTERED = 0u, RT_BOUNCE_EMITTED = 1u, RT_BOUNCE_MISSED = 2u };
typedef struct rt_bounce_request {
    uint32_t flags;             /* RT_FLAG_*, as for rt_scene_intersect                                    */
    uint32_t ray_form;          /* RT_TRACE_RAY_NEW | RT_TRACE_RAY_AS_GIVEN                                */
    uint32_t seed_states;       /* 1: first write state i = seed_from_u64(seed + 4*PHI*i), then step       */
    uint32_t reserved;          /* 0                                                                       */
    uint64_t seed;
} rt_bounce_request;            /* 24 bytes */

/* Host buffers, synchronous: rays (n) and rng_state (4 n u64) are read and written back; out_bounce (n) is required; active
 * (n_active indices), out_hits (n), next_active (n) with n_next, and stats may be NULL.  Records of rays that are not active come
 * back as they went in; out_bounce / out_hits entries of such rays are not written. */
RT_API int rt_scene_bounce(rt_scene* scene, const rt_bounce_request* req, rt_ray* rays, uint32_t n, uint64_t* rng_state,
                           const uint32_t* active, uint32_t n_active, rt_bounce* out_bounce, rt_hit* out_hits,
                           uint32_t* next_active, uint32_t* n_next, rt_tile_stats* stats);
/* Device buffers (n rt_ray, 4 n u64, n_active-capacity u32 list and its u32 length or both NULL, n rt_bounce, n rt_hit or NULL,
 * n u32 or NULL, one u32 or NULL), asynchronous on hip_stream (NULL = the scene's stream); counters and event times accumulate in
 * the scene until rt_scene_collect().  Ping-pong two lists: d_next_active / d_n_next of one step are d_active / d_n_active of the
 * next. */
RT_API int rt_scene_bounce_device(rt_scene* scene, const rt_bounce_request* req, void* d_rays, uint32_t n, void* d_rng_state,
                                  const void* d_active, const void* d_n_active, void* d_bounce, void* d_hits,
                                  void* d_next_active, void* d_n_next, void* hip_stream);

/* ---- direct lighting: one light sample per hit of the caller's rays ------------------------- */
/* Next-event estimation for an integrator built from the path steps above: for every active hit record (the rt_hit a step wrote to
 * out_hits) the library picks one emitter of the scene, draws a point on it from the ray's own RNG state, traces the shadow ray and
 * returns the Lambertian direct-light estimate, in one launch, one lane per record, the state advanced in place.  Every operation
 * below is one IEEE f32 rounding in the order written (no fused multiply-add, correctly rounded division and sqrt); a dot product
 * a.b is (ax*bx + ay*by) + az*bz; u01 is the f32 in [0, 1) of gen_range(0.0..1.0) on the ray's xoshiro256++ state.
 *
 *   - Emitters: the primitives with emission > 0 (a NaN emits nothing), listed in ascending position in RenderInfo.world (the value
 *     rt_hit.index reports); M = rt_scene_light_count() is their number.  The list is made once by rt_scene_create.
 *   - Active list: as for rt_scene_bounce*.  active == NULL (device form: d_active and d_n_active both NULL) takes all n records;
 *     otherwise n_active indices < n.  A record that is not listed has no byte of its state or of its rt_direct touched.  The host
 *     form checks every index (RT_ERR_BAD_ARG); the device form reads the length from *d_n_active ON THE DEVICE, takes
 *     min(n, *d_n_active) entries and skips an index >= n: the next_active / n_next of a bounce step are valid arguments as they stand.
 *   - Skipped records: a listed record with hits[i].index == RT_HIT_NONE gets status RT_DIRECT_SKIPPED, light = RT_HIT_NONE and every
 *     other field 0; it takes no draw and its state is unchanged.  Otherwise, when M == 0: RT_DIRECT_NO_LIGHTS on the same terms.
 *   - Draws, all from state i, the advanced state written back for every record that drew:
 *       u = u01; the emitter is k = min((uint32_t)(u * (float)M), M - 1) of the list;
 *       a sphere light (centre c, radius r): one UnitSphere draw us = (x1*f, x2*f, 1 - 2*s), s = x1*x1 + x2*x2 the accepted pair of
 *         Uniform(-1, 1) draws (rejected while s >= 1), f = 2 * sqrt(1 - s): the draw of a scattering hit (main.rs:119);
 *         L = c + r * us per component, nl = us;
 *       a triangle light (a, b, c): u1 = u01, u2 = u01; if u1 + u2 > 1 then u1 = 1 - u1 and u2 = 1 - u2;
 *         L = a + (u1 * (b - a) + u2 * (c - a)) per component; nl = normalize_or_zero((a - b) x (a - c)), the normal rt_hit reports.
 *   - Geometry: P = hits[i].p*, n = hits[i].n* as given (not flipped: the reference's diffuse lobe is about that normal);
 *       v = L - P; d2 = (vx*vx + vy*vy) + vz*vz; w = v / sqrt(d2); cs = n.w;
 *       cl = -(nl.w) for a sphere light, |nl.w| for a triangle light (ray_color returns em * albedo from either side of a triangle).
 *     If !(cs > 0) or !(cl > 0) or d2 is 0 or not finite: status RT_DIRECT_FACING_AWAY, rgb = 0, light and l* written, no ray traced.
 *   - Visibility: the shadow ray is Ray::new(P, v) (the direction normalised by division: it is w) in the window
 *     [req->t_min, req->t_max); its closest hit is found as rt_scene_intersect finds it under req->flags (same engines, a tree
 *     deeper than the walk's stack takes the scan, tile-only flags are ignored).  RT_DIRECT_LIT exactly when that hit's primitive is
 *     emitter k; otherwise RT_DIRECT_OCCLUDED with rgb = 0.
 *   - Estimate (without the surface albedo: the caller multiplies by the rt_bounce.rgb of the step and by its throughput):
 *       rgb = (albedo_k * emission_k) * W per channel;
 *       sphere light:   W = ((cs * cl) * ((4 * (r*r)) * (float)M)) / d2      (the pi of the area and of the Lambertian 1/pi cancel);
 *       triangle light: W = ((cs * cl) * (A * (float)M)) / (PI * d2), A = 0.5 * sqrt(c.c) of c = (a - b) x (a - c), PI the f32 pi.
 *   - rt_direct: rgb; light = the world position of emitter k; l* = L; status.
 *   - RT_ERR_BAD_ARG, and nothing launched: a NULL scene, request, hits, rng_state or out; n == 0; reserved != 0; one of active /
 *     n_active given without the other; in the host form an index >= n or n_active > n.  RT_ERR_LIMIT: M > 2^23.
 *   - Counters (rt_tile_stats): ray_segments = shadow rays traced; primary_rays = 0; broad_candidates = exact root tests; kernel_ms;
 *     h2d_ms (hits, states, the list) and d2h_ms (states, samples) of the host form; n_launches; engine (as for rt_scene_intersect).
 *   - Limits: the estimate equals ray_color's next bounce in expectation only at a hit of roughness 0.  A hit point inside an emissive
 *     sphere sees that sphere as dark (cl <= 0).  A caller who adds the estimate drops the RT_BOUNCE_EMITTED term of the FOLLOWING
 *     step, or the light is counted twice.  The area estimator's cs * cl / d2 has no bound next to a light; for sphere lights that
 *     limit is lifted under RT_LIGHTS_CONE (below).
 *   - Light selection by power: the emitter above is picked uniformly.  With RT_FLAG_LIGHTS_BY_POWER in req->flags it is picked from
 *     the scene's light table, made once by rt_scene_create.  For emitter k = 0 .. M - 1 of the list, in its order:
 *       lum_k = ((ar + ag) + ab) * emission;  area_k = (4 * (r*r)) * PI for a sphere, A + A for a triangle (A as in the estimate: it
 *       emits from both sides);  q_k = lum_k * area_k, and q_k = 0 if !(q_k > 0) (a NaN, an albedo sum <= 0, radius 0, a degenerate
 *       triangle);  c_k = c_(k-1) + q_k with c_(-1) = 0;  total = c_(M-1).
 *     The table is DEGENERATE when !(total > 0 && total < inf) (every q_k zero, an overflowing sum, an infinite q_k): then
 *     p_k = 1/M, ip_k = (float)M and the pick is the uniform one above, so the flag changes no bit.  Otherwise
 *       w_k = c_k - c_(k-1);  p_k = 0.5f * (1.0f / (float)M) + 0.5f * (w_k / total);  ip_k = 1.0f / p_k
 *     — a mixture, half uniform and half by power, that is part of the contract: p_k >= 1/(2M) also for a light whose power the f32
 *     running sum rounded away, so every emitter is sampled and the weight is bounded.  The pick takes the same single u = u01:
 *       u < 0.5:   k = min((uint32_t)((u + u) * (float)M), M - 1);
 *       otherwise: x = ((u - 0.5f) + (u - 0.5f)) * total;  k = the smallest index with x < c_k, or M - 1 when there is none.
 *     ip_k takes the place of (float)M in W, and nothing else changes:
 *       sphere light:   W = ((cs * cl) * ((4 * (r*r)) * ip_k)) / d2;      triangle light: W = ((cs * cl) * (A * ip_k)) / (PI * d2).
 *     rt_scene_light_table() reports every p_k.
 *   - Cone sampling of sphere lights: how a sphere light is sampled is a property of the SCENE, like its camera:
 *     rt_scene_set_light_sampling(scene, RT_LIGHTS_AREA | RT_LIGHTS_CONE).  The default is RT_LIGHTS_AREA, the sample above, every
 *     byte of every output.  The setting is read when a call is enqueued and only selects the kernel instance: work already enqueued
 *     keeps the setting it was enqueued with; rt_scene_set_light_sampling must not race with other calls on the same scene.  Only
 *     rt_scene_direct* and rt_scene_trace_nee* read it; every other call ignores it.  Under RT_LIGHTS_CONE everything not listed
 *     here is as above — the pick, uniform or by power; the active list; the statuses; the shadow ray's window and flags:
 *       A triangle light is untouched in every byte.  A sphere light (c, r) takes the same draws: the accepted pair x1, x2 with
 *       s = x1*x1 + x2*x2, so the state written back never depends on the setting.
 *       Regime: a = c - P per component; dc2 = a.a; r2 = r*r; q = r2 / dc2.  The sample is a CONE sample when q >= 0x1p-10f && q < 1.0f;
 *         otherwise it is the area sample above in every field (a NaN, a hit point inside or on the sphere, radius 0, a far small
 *         light, dc2 equal to 0 or inf).
 *       Cone: ctm = sqrt(1 - q); omc = q / (1 + ctm) (1 - cos(theta_max) without cancellation); e = s * omc; ct = 1 - e;
 *         st = sqrt(e * (2 - e)); rs = sqrt(s); cp = s > 0 ? x1 / rs : 0; sp = s > 0 ? x2 / rs : 0.
 *       Frame about the axis (Duff et al. 2017, branch-free): dc = sqrt(dc2); w = a / dc per component; sg = copysignf(1, w.z);
 *         A = -1 / (sg + w.z); B = (w.x * w.y) * A; t1 = (1 + (sg * (w.x * w.x)) * A, sg * B, -(sg * w.x));
 *         t2 = (B, sg + (w.y * w.y) * A, -w.y).
 *       Direction: ka = st * cp; kb = st * sp; v = (ka * t1 + kb * t2) + ct * w per component.  The shadow ray is Ray::new(P, v); its
 *         direction wn is v normalised by division, as everywhere.  cs = n.wn; !(cs > 0): RT_DIRECT_FACING_AWAY, no ray traced.  There
 *         is no cl test: every direction of the cone meets the front of the sphere.
 *       Visibility: unchanged, RT_DIRECT_LIT exactly when the closest hit is emitter k.
 *       Weight: W = (cs * (omc + omc)) * ip, ip = (float)M, or ip_k under RT_FLAG_LIGHTS_BY_POWER; rgb = (albedo * emission) * W.
 *         W is cs * Omega / pi / p_k with Omega the cone's solid angle: W <= 2 * ip always.
 *       l*: where the direction meets the sphere: h = r2 - dc2 * (st * st); h = h > 0 ? h : 0; ts = dc * ct - sqrt(h);
 *         L = P + ts * wn per component; written for every status that writes l* above.
 *     Consequences: the written-back states equal RT_LIGHTS_AREA's; a scene with no sphere emitter gives RT_LIGHTS_AREA's bytes.
 *     Limit: rounding can push a direction on the very rim of the cone past the sphere; that sample reads RT_DIRECT_OCCLUDED although
 *     nothing occludes it, which slightly darkens the estimate.  The regime's threshold keeps the share of such samples below 2^-14
 *     (tests/test_cone_host.py measures it); below the threshold the area sample, which has no such rim, is used.
 * No per-scene scratch on the device: launches on different streams may overlap.   */
typedef struct rt_direct_request { uint32_t flags; uint32_t reserved; float t_min, t_max; } rt_direct_request; /* 16 bytes */
typedef struct rt_direct { float r, g, b; uint32_t light; float lx, ly, lz; uint32_t status; } rt_direct;      /* 32 bytes */
enum { RT_DIRECT_LIT = 0u, RT_DIRECT_OCCLUDED = 1u, RT_DIRECT_FACING_AWAY = 2u, RT_DIRECT_NO_LIGHTS = 3u, RT_DIRECT_SKIPPED = 4u };

/* The number M of emitters of the scene. */
RT_API int rt_scene_light_count(rt_scene* scene, uint32_t* n_lights);
/* The emitter list with the probability each emitter is picked with under `flags`: for k < M, out_world_index[k] = the world position
 * of emitter k (the value rt_direct.light reports) and out_p[k] = p_k of the light table with RT_FLAG_LIGHTS_BY_POWER, 1.0f / (float)M
 * without it.  Either array may be NULL.  capacity < M or a NULL scene: RT_ERR_BAD_ARG.  Host only: no GPU work, no synchronisation. */
RT_API int rt_scene_light_table(rt_scene* scene, uint32_t flags, uint32_t* out_world_index, float* out_p, uint32_t capacity);
/* Host buffers, synchronous: hits (n) are read; rng_state (4 n u64) is read and written back; out (n) is required; active (n_active
 * indices) and stats may be NULL.  Records that are not listed come back as they went in. */
RT_API int rt_scene_direct(rt_scene* scene, const rt_direct_request* req, const rt_hit* hits, uint32_t n, uint64_t* rng_state,
                           const uint32_t* active, uint32_t n_active, rt_direct* out, rt_tile_stats* stats);
/* Device buffers (n rt_hit, 4 n u64, a u32 list and its u32 length or both NULL, n rt_direct), asynchronous on hip_stream (NULL = the
 * scene's stream); counters and event times accumulate in the scene until rt_scene_collect(). */
RT_API int rt_scene_direct_device(rt_scene* scene, const rt_direct_request* req, const void* d_hits, uint32_t n, void* d_rng_state,
                                  const void* d_active, const void* d_n_active, void* d_out, void* hip_stream);
/* How rt_scene_direct* and rt_scene_trace_nee* sample the scene's sphere lights ("cone sampling of sphere lights" above): over the
 * whole sphere (the default), or over the cone it subtends from the hit point.  sampling > 1 or a NULL scene: RT_ERR_BAD_ARG.  Host
 * only: no GPU work, no synchronisation. */
enum { RT_LIGHTS_AREA = 0u, RT_LIGHTS_CONE = 1u };
RT_API int rt_scene_set_light_sampling(rt_scene* scene, uint32_t sampling);
RT_API int rt_scene_light_sampling(rt_scene* scene, uint32_t* out_sampling);

/* ---- next-event estimation: the integrator of the path steps and the light samples, in one kernel -------- */
/* The integrator a caller composes from rt_scene_bounce* and rt_scene_direct* — a path of at most K = max_bounces + 1 segments with one
 * light sample after every hit but the last — as ONE launch, one lane per ray, nothing written to memory between the steps.  It also
 * carries the two rules the composed recipe cannot: it knows each hit's roughness, and in RT_NEE_MIS it combines the light sample and
 * the bounce by the balance heuristic.  Every operation below is one IEEE f32 rounding in the order written (no fused multiply-add,
 * correctly rounded division and sqrt); products and sums of colours are per channel.
 *
 *   - RNG and sums, as rt_scene_trace: rng_state == NULL: sample s of ray i draws from SmallRng::seed_from_u64(seed +
 *     4 * 0x9E3779B97F4A7C15 * (i * spp + s)); otherwise rng_state holds the xoshiro256++ state of each ray, read and written back, its
 *     spp samples drawing one after the other.  out_rgb (3 * n floats) is the f32 sum of the ray's sample colours c, added in the
 *     order s = 0, 1, ... starting from 0.
 *   - One sample: T = (1, 1, 1), c = (0, 0, 0), sampled = false.  For k = 0 .. max_bounces one path step exactly as rt_scene_bounce
 *     specifies it: the closest hit under `flags` in the ray's own window [t_min, t_max); ray_form applies to k = 0, every later
 *     segment is RT_TRACE_RAY_AS_GIVEN; the same UnitSphere draw and scattered ray.
 *       RT_BOUNCE_MISSED:     c = c + T * sky (one multiplication, then one addition).  The sample ends.
 *       RT_BOUNCE_SCATTERED   at primitive j (albedo a, roughness rho, point P and normal n as rt_hit reports them): T = T * a.  If
 *                             k == max_bounces the sample ends: the scatter draw has been taken, as the reference takes it, and no
 *                             light sample is.  Otherwise sampled = (rho == 0 && M > 0), M = rt_scene_light_count().  If sampled: one
 *                             light sample exactly as rt_scene_direct specifies it for the record (P, n, j), from the state as the step
 *                             left it, with the ray's own window and the request's flags; when a shadow ray is traced it is counted
 *                             in out_shadow; when the sample is RT_DIRECT_LIT with estimate D and weight W,
 *                               RT_NEE_LIGHT_ONLY:  c = c + T * D;
 *                               RT_NEE_MIS:         wl = 1.0f / (1.0f + W);  c = c + T * (D * wl);
 *                             and no addition for any other status.  If not sampled, no draw is taken.  n is kept for the next step.
 *       RT_BOUNCE_EMITTED     at emitter j, e = albedo * emission.  If k == 0 or !sampled: c = c + T * e.  Otherwise the light
 *                             strategy's view of this hit point, from the previous hit's normal n, the segment's unit direction d, this
 *                             hit's rt_hit normal nh and its rt_hit.distance: cs' = n.d; cl' = -(nh.d) for a sphere, |nh.d| for a
 *                             triangle; d2' = distance * distance; W' = the W of rt_scene_direct for (cs', cl', the radius or area of
 *                             j, M, d2').  The point is SAMPLABLE when cs' > 0 and cl' > 0 and d2' > 0 and d2' is finite.
 *                               not samplable (an emissive sphere hit from inside):  c = c + T * e;
 *                               samplable, RT_NEE_LIGHT_ONLY:  nothing is added (the light sample of the step before stood for it);
 *                               samplable, RT_NEE_MIS:         wb = 1.0f - 1.0f / (1.0f + W');  c = c + T * (e * wb).
 *                             The sample ends.
 *     W is (cs / pi) / p_light = p_bsdf / p_light, so wl and wb are the balance heuristic's weights, and the area estimator's unbounded
 *     cs * cl / d2 becomes Le * W / (1 + W) <= Le.  RT_NEE_LIGHT_ONLY keeps the unbounded term; for sphere lights that limit is lifted
 *     under RT_LIGHTS_CONE (below), where W <= 2 * ip.
 *   - RT_NEE_LIGHT_ONLY is, bit for bit, the fold above over rt_scene_bounce and rt_scene_direct called per step.
 *   - out_segments (n u32, optional): the ray's path segments, summed over its samples; with M == 0 they and the written-back states
 *     are rt_scene_trace's for the same arguments.  out_shadow (n u32, optional): its shadow rays.
 *   - flags: as for rt_scene_intersect (a tree deeper than the walk's stack takes the scan; tile-only flags are ignored).
 *   - RT_ERR_BAD_ARG, and nothing launched: a NULL scene, request, rays or out_rgb; n == 0; spp == 0; ray_form > 1; mode > 1;
 *     reserved != 0.  RT_ERR_LIMIT: spp > RT_MAX_SPP, max_bounces > RT_MAX_BOUNCES, M > 2^23.
 *   - Counters (rt_tile_stats): primary_rays = n * spp; ray_segments = path segments + shadow rays; broad_candidates = exact root
 *     tests; kernel_ms; h2d_ms (rays and states) and d2h_ms (colours, counts, states) of the host form; n_launches = 1; engine (as for
 *     rt_scene_intersect).
 *   - Light selection by power: with RT_FLAG_LIGHTS_BY_POWER in `flags` every light sample is rt_scene_direct's under that flag (the
 *     pick from the light table, ip_k in W), and in the RT_BOUNCE_EMITTED branch W' takes ip_j of the emitter j that was hit in the
 *     place of (float)M.  wl and wb are unchanged: W is still p_bsdf / p_light.  RT_NEE_LIGHT_ONLY stays, bit for bit, the fold over
 *     rt_scene_bounce and rt_scene_direct with the flag.
 *   - Cone sampling of sphere lights: when the scene's setting is RT_LIGHTS_CONE (rt_scene_set_light_sampling) every light sample is
 *     rt_scene_direct's under that setting, and the RT_BOUNCE_EMITTED branch, for an emitter j that is a sphere (c_j, r) with k != 0
 *     and sampled, views the point as the cone sample of the hit before saw it.  With o the segment's origin, which is exactly the
 *     previous hit point: a' = c_j - o; dc2' = a'.a'; q' = (r*r) / dc2'.  If q' is in the cone regime (q' >= 0x1p-10f && q' < 1.0f):
 *     cs' = n.d; the point is SAMPLABLE exactly when cs' > 0; omc' = q' / (1 + sqrt(1 - q')); W' = (cs' * (omc' + omc')) * ip_j
 *     (ip_j = (float)M without RT_FLAG_LIGHTS_BY_POWER).  Otherwise, and for triangles, the view above applies unchanged.  The regime
 *     depends only on the point and the emitter, so the sample taken at P and the view from o = P speak of the same p_light; wl and
 *     wb stay the balance heuristic's weights.  RT_NEE_LIGHT_ONLY under RT_LIGHTS_CONE stays, bit for bit, the fold over
 *     rt_scene_bounce and rt_scene_direct under RT_LIGHTS_CONE.  out_segments and the written-back states equal RT_LIGHTS_AREA's: the
 *     path never depends on the light sample; out_shadow and the colours differ.  A scene with no sphere emitter gives RT_LIGHTS_AREA's
 *     bytes.  The rim limit of rt_scene_direct's cone sample applies.
 *   - Light samples at glossy hits: whether a hit of roughness rho > 0 takes a light sample is a property of the SCENE:
 *     rt_scene_set_glossy_sampling(scene, RT_GLOSSY_BOUNCE | RT_GLOSSY_MIS).  The default is RT_GLOSSY_BOUNCE, everything above, every
 *     byte of every output.  The setting is read when a call is enqueued and only selects the kernel instance: work already enqueued
 *     keeps the setting it was enqueued with; rt_scene_set_glossy_sampling must not race with other calls on the same scene.  Only
 *     rt_scene_trace_nee* in mode RT_NEE_MIS reads it: RT_NEE_LIGHT_ONLY (so its fold identity stays), rt_scene_direct* (which has
 *     neither the roughness nor the incoming direction) and every other call ignore it in every byte.  The light sample alone has
 *     no finite variance at such a hit (below); under the balance heuristic its term is Le * W / (1 + W) <= Le.
 *     ray_color scatters along pre = diffuse + rho * (glossy - diffuse) = c + r * us, us uniform on the unit sphere: the direction
 *     from the origin to a uniform point of the sphere of radius r = 1 - rho about c = r * n + rho * g, g the mirrored direction.
 *     With b = c.w and kappa = c.c - r*r the density of the unit direction w is p(w) = (b*b + D) / (2 pi r sqrt(D)), D = b*b - kappa,
 *     for b > 0 and D > 0, else 0 (both intersections contribute, each t*t / |cos|; the origin lies outside the sphere, kappa > 0, at
 *     every front-face hit with 0 < rho < 1).  cg = pi * p(w) stands where the Lambertian cs stands above.  Under RT_GLOSSY_MIS, in
 *     mode RT_NEE_MIS, everything not listed here is as above:
 *       Class of an RT_BOUNCE_SCATTERED hit with k != max_bounces and M > 0: d the segment's direction as the step used it,
 *         g = d - (2 * (d.n)) * n the glossy_dir the step formed (the same bits), gn = n.g, gg = g.g.
 *           rho == 0:                          the diffuse sample exactly as above (cs; the lobe formula is not used);
 *           0 < rho && rho < 1 && gn >= 0:     LOBE-SAMPLED;
 *           anything else (rho >= 1, rho < 0, a NaN, a back-face hit gn < 0, where the origin may lie inside the sphere): no light
 *                                              sample and no draw, as above.
 *       Lobe of a lobe-sampled hit: r = 1 - rho; c = r * n + rho * g per component (two products, one sum);
 *         kappa = rho * (rho * gg + (r + r) * gn).
 *       Lobe factor of a unit direction w: b = c.w; D = b * b - kappa; w is IN THE LOBE iff b > 0 && D > 0;
 *         cg = (b * b + D) / ((r + r) * sqrt(D)).
 *       Light sample at a lobe-sampled hit: the draws, the pick (uniform or by power), the point or the cone pair and the regime rule
 *         of the scene's RT_LIGHTS_CONE are rt_scene_direct's, from the state as the step left it.  Every rejection above stays
 *         (cs > 0, cl > 0, d2 finite and not 0; cs > 0 alone for a cone sample).  One is added: with wn the shadow ray's unit
 *         direction (v normalised by division) and W the W of rt_scene_direct with cg(wn) in the place of cs —
 *           area sphere: ((cg * cl) * ((4 * (r_l*r_l)) * ip)) / d2;  triangle: ((cg * cl) * (A * ip)) / (PI * d2);
 *           cone: (cg * (omc + omc)) * ip;  ip = (float)M, or ip_k under RT_FLAG_LIGHTS_BY_POWER —
 *         if wn is not in the lobe or !(W < inf), no ray is traced, nothing is added and out_shadow does not count it; the draws
 *         have been taken.  Otherwise wl = 1.0f / (1.0f + W) and, when the shadow ray is RT_DIRECT_LIT, c = c + T * (D * wl) with
 *         D = (albedo * emission) * W.
 *       Lobe factor of the direction the scatter itself took, formed at the lobe-sampled hit from the UnitSphere vector us of its
 *         scatter draw (the scattered point is X = c + r * us, and this is cg(X / |X|) without the cancellation of b * b - kappa on the
 *         rim): m = r * (c.us + r); t = sqrt(kappa + (m + m)); cgb = ((kappa + m) * (kappa + m) + m * m) / (((r + r) * |m|) * t);
 *         that direction is IN THE LOBE iff cgb > 0 (not for m == 0, a NaN, an overflowing scatter).
 *       RT_BOUNCE_EMITTED after a lobe-sampled hit: the view above, by area or by cone under the same regime rule, with cgb of the
 *         previous hit in the place of cs' in W'; the point is SAMPLABLE when it is samplable above (cs' = n.d > 0 and the rest)
 *         and cgb > 0.  W' = inf gives wb = 1, the full term.  Not samplable: c = c + T * e.
 *     Consequences: a lobe-sampled hit advances the RNG by the light sample's draws, so the segments, the written-back states and
 *     the colours of a ray that meets such a hit differ from RT_GLOSSY_BOUNCE's; a ray that meets only hits of rho == 0 or
 *     rho >= 1 (and a scene with M == 0) gives RT_GLOSSY_BOUNCE's bytes.  The estimator stays unbiased: wl and wb are the balance
 *     heuristic's weights of p_scatter / p_light.
 *   - Limits: under RT_GLOSSY_BOUNCE a hit with roughness > 0 takes no light sample (it falls back to the bounce, which is unbiased);
 *     under RT_GLOSSY_MIS that holds for rho >= 1 and for back-face hits.  p(w) has a 1 / sqrt(D) singularity on the rim of the lobe,
 *     so the light sample alone (Le * W) has a logarithmically divergent variance there: the setting exists for RT_NEE_MIS only.
 *     Rim: D = b * b - kappa of an f32 direction cancels on the rim, where up to 2^-9 of the scatter's own directions would read
 *     D <= 0; that is why the bounce's factor is formed from its draw, cgb above, which leaves fewer than 2^-14 of them outside
 *     the lobe (tests/test_lobe_density.py measures both).  A bounce direction outside the lobe has its emitter
 *     added in full, and a light sample whose direction rounds to D <= 0 is dropped.
 * No per-scene scratch on the device: launches on different streams may overlap.   */
typedef struct rt_nee_request {
    uint32_t spp;               /* samples per ray, 1 .. RT_MAX_SPP                                        */
    uint32_t max_bounces;       /* 0 .. RT_MAX_BOUNCES; at most max_bounces + 1 path segments, as rt_scene_trace */
    uint64_t seed;              /* the seeded streams, when no RNG states are passed                       */
    uint32_t flags;             /* RT_FLAG_*, as for rt_scene_intersect                                    */
    uint32_t ray_form;          /* RT_TRACE_RAY_NEW | RT_TRACE_RAY_AS_GIVEN (the first segment only)       */
    uint32_t mode;              /* RT_NEE_LIGHT_ONLY | RT_NEE_MIS                                          */
    uint32_t reserved;          /* 0                                                                       */
} rt_nee_request;               /* 32 bytes */
enum { RT_NEE_LIGHT_ONLY = 0u, RT_NEE_MIS = 1u };

/* Host buffers, synchronous; rng_state, out_segments, out_shadow and stats may be NULL. */
RT_API int rt_scene_trace_nee(rt_scene* scene, const rt_nee_request* req, const rt_ray* rays, uint32_t n, uint64_t* rng_state,
                              float* out_rgb, uint32_t* out_segments, uint32_t* out_shadow, rt_tile_stats* stats);
/* Device buffers (n rt_ray, 4 n u64 or NULL, 3 n f32, n u32 or NULL, n u32 or NULL), asynchronous on hip_stream (NULL = the scene's
 * stream); counters and event times accumulate in the scene until rt_scene_collect(). */
RT_API int rt_scene_trace_nee_device(rt_scene* scene, const rt_nee_request* req, const void* d_rays, uint32_t n, void* d_rng_state,
                                     void* d_out_rgb, void* d_out_segments, void* d_out_shadow, void* hip_stream);
/* Whether rt_scene_trace_nee* in mode RT_NEE_MIS takes a light sample at hits of roughness 0 < rho < 1 ("light samples at glossy hits"
 * above): not (the default: such a hit falls back to the bounce), or weighted by the density of the reference's scatter lobe.
 * sampling > 1 or a NULL scene: RT_ERR_BAD_ARG.  Host only: no GPU work, no synchronisation. */
enum { RT_GLOSSY_BOUNCE = 0u, RT_GLOSSY_MIS = 1u };
RT_API int rt_scene_set_glossy_sampling(rt_scene* scene, uint32_t sampling);
RT_API int rt_scene_glossy_sampling(rt_scene* scene, uint32_t* out_sampling);

/* ---- feature buffers (AOVs) of a strip: what the camera rays of the beauty image first hit ---- */
/* Per-pixel feature buffers for a denoiser, edge-aware filters, picking and compositing, ALIGNED with the beauty image: they
 * come from the very camera rays (sub-pixel and lens samples) whose colours the tile entry points average, so the planes after
 * samples [0, e) line up with the progressive preview after [0, e).
 *
 *   - Samples: a call covers samples s in [sample_begin, sample_end) of the S = req->spp sample job, with the rules and checks of
 *     rt_scene_render_tile_pass.  The camera ray of sample s of the pixel at global row y, column x is exactly the ray the tile
 *     kernel traces first for that sample: Camera::get_ray (camera.rs:109-129) drawing from
 *     SmallRng::seed_from_u64(seed + 4 * 0x9E3779B97F4A7C15 * ((y W + x) S + s)) (wrapping u64): the UnitDisc rejection pair,
 *     then the u and v jitter draws; the direction that results is used as given (no second normalisation).
 *   - The sample's first hit is the closest hit in [req->t_min, req->t_max) as rt_scene_intersect finds it, with its tie rule
 *     and its RT_FLAG_* semantics: BVH semantics over the exact-node walk by default; the plain scan under RT_FLAG_NO_BVH_CULL;
 *     the scan with BVH semantics under RT_FLAG_EXACT_SCAN / RT_FLAG_LINEAR_SCAN; RT_FLAG_FULL_CHAIN the literal slab test.
 *     Tile-only flags are accepted and ignored.
 *   - Planes (Hs*W pixels laid out like out_f32; a NULL plane is not computed):
 *       albedo  Hs*W*3 floats: the f32 sum over the call's samples of the first hit's albedo (p_albedo_at, whether or not the
 *               primitive emits); a miss adds the sky colour ray_color returns for that ray (main.rs:135-144);
 *       normal  Hs*W*3 floats: the sum of the normal at the first hit, the value of rt_hit.n* (not flipped toward the ray);
 *       depth   Hs*W floats: the sum of |P - o| (rt_hit.distance; o is the lens point);
 *       hits    Hs*W u32: the number of samples whose camera ray hit something;
 *       index   Hs*W u32: the world position (rt_hit.index) hit by sample 0 of the pixel, or RT_HIT_NONE.  Written only by a
 *               call with sample_begin == 0, left untouched by the others.
 *   - Sums: a sum starts at +0.0f when sample_begin == 0, else from the plane's current contents (hits likewise, as a u32).
 *     Each contributing sample is added with one f32 addition in the order s = sample_begin, sample_begin + 1, ...  A miss adds
 *     nothing to normal and depth (no addition at all: a -0.0 survives).  So the planes after any cut of [0, k) into calls are
 *     bit-identical to one call over [0, k), and strips of one frame stitch to the planes of a single strip (the streams are
 *     per global pixel).  Means after [0, e): albedo / e, normal normalised, depth / hits.
 *   - RT_ERR_BAD_ARG, and nothing launched: a NULL scene, request or planes; every plane NULL; sample_begin >= sample_end or
 *     sample_end > spp; every check of the tile entry points; in the device form, requests that differ in a frame-level field
 *     (as rt_scene_render_tiles_device) or entries with different sets of non-NULL planes.  RT_ERR_LIMIT: spp > RT_MAX_SPP.
 *   - Counters (rt_tile_stats): primary_rays = ray_segments = Hs*W*(sample_end - sample_begin) per strip; broad_candidates =
 *     exact root tests; engine as for rt_scene_intersect (2 the walk, 1 the scan); kernel_ms; n_launches; h2d_ms (planes
 *     uploaded) and d2h_ms (planes downloaded) of the host form.
 * No per-scene scratch on the device: launches on different streams may overlap.  The beauty launch does not write these planes
 * (a separate pass re-traces the first segment of each sample; callers bound its cost by taking the planes over fewer samples
 * than the beauty).   */
typedef struct rt_aov_planes {
    float*    albedo;           /* Hs*W*3 */
    float*    normal;           /* Hs*W*3 */
    float*    depth;            /* Hs*W   */
    uint32_t* hits;             /* Hs*W   */
    uint32_t* index;            /* Hs*W   */
} rt_aov_planes;                /* 40 bytes */

/* Host buffers, synchronous: the non-NULL planes are uploaded when sample_begin > 0 and always downloaded; stats may be NULL. */
RT_API int rt_scene_render_aov(rt_scene* scene, const rt_tile_request* req, uint32_t sample_begin, uint32_t sample_end,
                               const rt_aov_planes* planes, rt_tile_stats* stats);
/* Batched device form: n strips of one frame, one launch per 64 strips, asynchronous on hip_stream (NULL = the scene's stream),
 * counters and event times accumulating until rt_scene_collect().  d_planes: n entries of device pointers, every entry with
 * the same set of non-NULL planes. */
RT_API int rt_scene_render_aovs_device(rt_scene* scene, const rt_tile_request* reqs, uint32_t n,
                                       uint32_t sample_begin, uint32_t sample_end,
                                       const rt_aov_planes* d_planes, void* hip_stream);

/* ---- denoiser: edge-avoiding a-trous wavelet filter guided by the feature buffers ---- */
/* Dammertz et al. 2010: a 5x5 B3-spline kernel dilated by 2^i at iteration i, with edge stopping on colour, normal and depth and
 * optional albedo demodulation, over the progressive accum of a frame's strips and their rt_aov_planes.  Every operation below is
 * one IEEE f32 rounding in the order written (no fused multiply-add, correctly rounded division and sqrt, no exp), so the result
 * is reproducible bit for bit off the GPU.
 *
 *   - Image: reqs[0..n) are strips of one frame with consecutive division_no, ascending, that agree on every frame-level field
 *     (the check of rt_scene_render_tiles_device).  Their union, stacked top to bottom, is the image P: W columns, R = n*Hs rows.
 *     The top and bottom rows of P are image borders: strips denoised in separate calls show seams; n = divisions denoises the
 *     whole frame.  The strip count is not limited to 64.  No scene data is read: the world is irrelevant.
 *   - Inputs per pixel (finite and non-negative, as the renderer writes them; otherwise the result is unspecified):
 *       c = C / e per channel, C = accum[i] (Hs*W*3 floats laid out like out_f32), e = color_samples;
 *       albedo given: a = A / k (k = aov_samples), d = a + albedo_eps, r0 = c / d; without albedo r0 = c;
 *       normal given: L = sqrt((Nx*Nx + Ny*Ny) + Nz*Nz), n = L > 0 ? (Nx/L, Ny/L, Nz/L) : 0;
 *       depth given (requires hits): z = hits > 0 ? D / (float)hits : 0, and q = z > 0 ? 1 / z : 0;
 *       hits given: g = hits > 0, else g = 1.  index is ignored.
 *   - Iteration i = 0 .. I-1, step s = 2^i, kc_0 = k_color, kc_{i+1} = kc_i * color_step_scale:
 *       taps (dy, dx) in {-2..2}^2, dy outer, dx inner, both ascending; tap pixel q = p + s*(dx, dy);
 *       a tap is skipped if q lies outside P or g_q != g_p;
 *       the centre tap (0, 0) has t = 1; any other tap:
 *         D = r_q - r_p per channel, x = ((Dr*Dr + Dg*Dg) + Db*Db) * kc_i;
 *         normal given, unless n_p and n_q are both 0: dot = (np_x*nq_x + np_y*nq_y) + np_z*nq_z, x = x + (1 - dot) * k_normal;
 *         depth given: x = x + (|z_q - z_p| * q_p) * k_depth;
 *         t = 1 - x if that is > 0, else +0 (Tukey's biweight: compact support, an exact 0 across a strong edge);
 *       w = H[dy]*H[dx] * (t*t), H = (1/16, 1/4, 3/8, 1/4, 1/16), the dyadic product first;
 *       Sw += w, Sc += w * r_q from +0.0 in tap order; r_{i+1} = Sc / Sw per channel (Sw >= 9/64: the centre tap).
 *   - Outputs, each optional (at least one), laid out like out_f32 per strip: m = albedo ? r_I * d : r_I, the linear mean;
 *       out_linear  m (Hs*W*3 floats);
 *       out_f32     sqrt(m) (Hs*W*3 floats: post-gamma, pre-quantise, as the tile's out_f32);
 *       out_rgb     the tile's quantisation of sqrt(m) * 255.999f (Hs*W*3 bytes, out_len_each >= rt_tile_bytes).
 *     So with iterations == 0 and no albedo, out_f32 and out_rgb are the progressive pass's preview after [0, e), bit for bit.
 *     Outputs must not overlap inputs.
 *   - RT_ERR_BAD_ARG, and nothing launched: a NULL scene, request, dreq, accum (or entry) or planes (an entry whose every plane is
 *     NULL is allowed: plain colour a-trous); no output; depth without hits; a field of dreq out of range; strips that are not
 *     consecutive or differ in a frame-level field; entries with different sets of non-NULL planes or outputs; in the device
 *     form scratch_bytes < rt_denoise_scratch_bytes(W, R) or a NULL d_scratch.  RT_ERR_BUFFER_TOO_SMALL: out_len_each <
 *     rt_tile_bytes.  RT_ERR_LIMIT: color_samples or aov_samples > RT_MAX_SPP.
 *   - Counters (rt_tile_stats): kernel_ms, n_launches, h2d_ms (inputs uploaded) and d2h_ms (outputs downloaded) of the host form;
 *     the ray counters add 0; engine reports 0 (no closest-hit engine runs).
 *  */
#define RT_DENOISE_MAX_ITERATIONS 8u
typedef struct rt_denoise_request {
    uint32_t color_samples;     /* e: accum holds samples [0, e)                                   1 .. RT_MAX_SPP          */
    uint32_t aov_samples;       /* k: the albedo plane holds samples [0, k)              1 .. RT_MAX_SPP (when albedo given) */
    uint32_t iterations;        /* I: 0 .. RT_DENOISE_MAX_ITERATIONS                                                        */
    uint32_t flags;             /* must be 0                                                                                 */
    float k_color;              /* >= 0, finite                                                                              */
    float color_step_scale;     /* > 0, finite: k_color of iteration i+1 = (that of i) * this                               */
    float k_normal;             /* >= 0, finite                                                                              */
    float k_depth;              /* >= 0, finite                                                                              */
    float albedo_eps;           /* > 0, finite                                                                               */
    uint32_t reserved;          /* must be 0                                                                                 */
} rt_denoise_request;           /* 40 bytes */

/* The defaults; color_samples and aov_samples are set to 1: the caller sets both. */
RT_API void rt_denoise_request_defaults(rt_denoise_request* r);
/* Device scratch of rt_scene_denoise_device for an image of width x rows pixels (any iteration count and set of planes). */
RT_API size_t rt_denoise_scratch_bytes(uint32_t width, uint32_t rows);
/* Host buffers, synchronous: accum[i], planes[i] and the outputs are host pointers of strip i; stats may be NULL. */
RT_API int rt_scene_denoise(rt_scene* scene, const rt_tile_request* reqs, uint32_t n, const rt_denoise_request* dreq,
                            const float* const* accum, const rt_aov_planes* planes,
                            uint8_t* const* out_rgb, size_t out_len_each, float* const* out_f32, float* const* out_linear,
                            rt_tile_stats* stats);
/* Device buffers, asynchronous on hip_stream (NULL = the scene's stream), counters until rt_scene_collect(); the scratch is the
 * caller's (no per-scene device scratch: calls on different streams with separate scratch may overlap).  out_rgb, out_f32 and
 * out_linear: NULL or n device pointers. */
RT_API int rt_scene_denoise_device(rt_scene* scene, const rt_tile_request* reqs, uint32_t n, const rt_denoise_request* dreq,
                                   const void* const* d_accum, const rt_aov_planes* d_planes,
                                   void* const* d_out_rgb, size_t out_len_each, void* const* d_out_f32,
                                   void* const* d_out_linear, void* d_scratch, size_t scratch_bytes, void* hip_stream);

/* ---- placed camera: a pose for the strips' camera rays ------------------------------- */
/* The reference's Camera sits at Point3::ZERO, looks down -z with y up (main.rs:42-50), and can be moved (Camera::set_origin,
 * camera.rs:73-83).  An rt_camera places and turns the same pinhole / thin-lens camera: its eye, a point it looks at, a roll
 * reference.  Field of view, focal length, aperture and focus distance stay the request's.
 *
 *   - Scope: the camera belongs to the JOB, like the world (the slave makes one Camera per job, main.rs:42-50): it is set on the
 *     rt_scene (or the rt_frame_ctx, below), not carried by rt_tile_request.  NULL restores the reference camera.
 *   - When it is read: when a call is enqueued; it travels by value in the kernel arguments, so work already enqueued keeps the
 *     camera it was enqueued with.  rt_scene_set_camera must not race with other calls on the same scene.
 *   - Who reads it: every entry point that generates camera rays: rt_scene_render_tile, _tile_device, _tiles, _tiles_device,
 *     _tile_pass, _tiles_pass_device, rt_scene_render_aov, _aovs_device, rt_scene_camera_rays*, rt_frame_ctx_render (the context's
 *     camera).  rt_render_tile and rt_render_frame keep the reference camera; rt_scene_intersect*, rt_scene_trace* and
 *     rt_scene_denoise* do not depend on it.  The closest-hit engine does not depend on the pose.
 *   - No camera set (or reset with NULL): exactly the code path and the bytes of a library without placed cameras.
 *   - Arithmetic of a pose.  Each operation is one IEEE f32 rounding in the order written, no fused multiply-add:
 *       basis    w = (origin - target) / |origin - target|, division by the length as Ray::new does (ray.rs:133-143), a length being
 *                sqrt((x*x + y*y) + z*z);  u = c / |c| with c = up x w;  v = w x u;  a cross product component is a*b - c*d with the
 *                two products rounded separately ((a x b).x = a.y*b.z - a.z*b.y, and cyclic);
 *       vectors  vh = 2 tan(fov / 2), vw = (W / H) vh, lens_radius = aperture / 2 as Camera::new computes them (camera.rs:19-47);
 *                hor = vw * u, ver = vh * v, foc = focal_length * w;
 *                llc[i] = ((origin[i] - hor[i] / 2) - ver[i] / 2) - foc[i];  lens_u = lens_radius * u, lens_v = lens_radius * v;
 *       sample   the lens offset of Camera::get_ray (camera.rs:109-129) is offset[i] = x1 * lens_u[i] + x2 * lens_v[i] (two products,
 *                one sum) for the UnitDisc draw (x1, x2); everything else of get_ray is unchanged.
 *     The reference camera is lens_u = (lens_radius, 0, 0), lens_v = (0, lens_radius, 0) written literally; rt_camera_defaults gives
 *     the same vectors through the arithmetic above for every positive vw, vh and focal_length.
 *   - RT_ERR_BAD_ARG, and the previous camera stays: a NULL scene or context; a component that is not finite; |origin - target| or
 *     |up x w| equal to 0 or not finite (up parallel to the view direction); flags or reserved not 0.
 *  */
typedef struct rt_camera {
    float origin[3];            /* the eye (Camera::origin)                                    */
    float target[3];            /* a point looked at                                           */
    float up[3];                /* roll reference                                              */
    uint32_t flags;             /* must be 0                                                   */
    uint32_t reserved;          /* must be 0                                                   */
} rt_camera;                    /* 44 bytes */

/* The reference camera as a pose: origin (0,0,0), target (0,0,-1), up (0,1,0). */
RT_API void rt_camera_defaults(rt_camera* cam);
/* cam == NULL: back to the reference camera. */
RT_API int rt_scene_set_camera(rt_scene* scene, const rt_camera* cam);

/* The camera rays of a strip, for an integrator of the caller's own on rt_scene_trace_device / rt_scene_intersect_device that starts
 * from exactly the rays the tile kernel traces first, without a host round trip.
 *   - Samples [sample_begin, sample_end) of the S = req->spp sample job, with the checks of rt_scene_render_tile_pass.  The record of
 *     sample s of the strip's pixel (row, x) is written at (row*W + x) * (sample_end - sample_begin) + (s - sample_begin).
 *   - rays: (o, t_min) (d, t_max): o the lens point, d the direction as Camera::get_ray hands it to ray_color (for
 *     RT_TRACE_RAY_AS_GIVEN), t_min / t_max the request's.
 *   - rng_state (optional, may be NULL): 4 u64 per record, the xoshiro256++ state after get_ray's draws: what ray_color continues
 *     from (the rng_state of rt_scene_trace with spp = 1).
 *   - Counters: primary_rays = records written, kernel_ms, n_launches, d2h_ms (host form); ray_segments adds 0. */
RT_API int rt_scene_camera_rays(rt_scene* scene, const rt_tile_request* req, uint32_t sample_begin, uint32_t sample_end,
                                rt_ray* rays, uint64_t* rng_state, rt_tile_stats* stats);
/* Device buffers (Hs*W*(sample_end - sample_begin) rt_ray; 4 u64 per record or NULL), asynchronous on hip_stream (NULL = the scene's
 * stream); counters and event times accumulate in the scene until rt_scene_collect(). */
RT_API int rt_scene_camera_rays_device(rt_scene* scene, const rt_tile_request* req, uint32_t sample_begin, uint32_t sample_end,
                                       void* d_rays, void* d_rng_state, void* hip_stream);

/* ---- whole frame: replaces controller dispatch + assembly ----------------------- */
/* (controller main.rs:47-75 `for division_no in 0..divisions` and :109-115 stitch.)
 *
 * rt_frame_ctx is the controller's state for a JOB: a set of devices, each with one dispatcher thread, the job's world
 * resident in its HBM, its streams and its strip buffers, plus the page-locked registration of the caller's frame buffer.
 * Everything is created once — the context by rt_frame_ctx_create, the world by rt_frame_ctx_set_world, the registration
 * by the first rt_frame_ctx_render that sees a buffer — and reused: a second frame of the job (same world, same buffer)
 * registers, allocates, uploads and spawns nothing.  rt_render_frame is the one-shot wrapper (create, set world, render
 * one frame, destroy).
 *
 * Strip assignment.  Strips are not equally expensive (sky rows: one segment per sample; ground rows bounce), and a frame
 * is done when its slowest device is.  Default: the first frame of a job goes out in SNAKE order — strip k to entry k % n
 * in even rows of n strips, to n-1 - k % n in odd ones: every entry gets one strip of each row, which evens out any cost
 * profile that is close to linear in the strip's position — and the kernels count the ray segments of every strip; every
 * later frame of the job (same world, same frame geometry) is assigned LONGEST-FIRST by those counts, each strip to the
 * entry with the least load so far.  For these two assignments the context cuts the frame into its own strips — at least
 * six per entry, whole rows, the next count from max(divisions, 6 n) up that divides the height — since `divisions` is the
 * reference's wire format, not a property of the image: every cut into whole rows renders the same bytes (`seed` above).  All strips of an entry go out in one launch (above 64 MiB of pixels per device: two,
 * the last quarter of the strips running under the downloads of the rest).  RT_FLAG_FRAME_STATIC in req->flags: the plain
 * split strip k -> devices[k % n]; RT_FLAG_FRAME_QUEUE: the devices pull strips one at a time, bottom of the frame first,
 * two launches in flight per device.  The RGB8 strips are stitched by division_no into out_rgb (H*W*3).  Same bytes
 * whatever the assignment.  No collective, no peer traffic: strips are independent.
 * req->division_no is ignored.  height % divisions must be 0 (the controller's from_vec(..).unwrap() panics otherwise). */

typedef struct rt_frame_ctx rt_frame_ctx;
#define RT_FRAME_STATS_ENTRIES 16u

/* Where the wall time of one rt_frame_ctx_render call went (milliseconds).  Devices run concurrently: kernel_ms and
 * d2h_exposed_ms are those of the device that finished last. */
typedef struct rt_frame_stats {
    rt_tile_stats totals;       /* counters summed over the devices; kernel_ms / d2h_ms = the largest per-device value */
    float wall_ms;              /* the whole call, steady clock                                                        */
    float pin_ms;               /* page-locking out_rgb in this call (0 when the buffer was already registered)       */
    float scene_ms;             /* host-side world preparation + uploads charged to this frame: the duration of the
                                   rt_frame_ctx_set_world since the previous frame (0 for every later frame of the job) */
    float kernel_ms;            /* HIP-event time of the launches of the device that finished last                    */
    float d2h_exposed_ms;       /* last launch done -> last strip byte on the host, same device                       */
    float host_ms;              /* wall_ms - pin_ms - kernel_ms - d2h_exposed_ms: dispatch, thread wake-up, joins      */
    uint32_t n_devices;
    uint32_t pinned;            /* 1: out_rgb is page-locked (strip downloads are direct DMA)                          */
    uint32_t assignment;        /* 0: static k % n, 1: snake (no costs yet), 2: longest-first by the previous frame's
                                   per-strip ray segments, 3: strip queue                                              */
    float balance_max_over_mean;/* ray segments of the busiest entry / mean over the entries, THIS frame (1 = even)    */
    uint64_t entry_segments[RT_FRAME_STATS_ENTRIES];   /* ray segments per entry (the first RT_FRAME_STATS_ENTRIES)    */
} rt_frame_stats;

/* devices == NULL (or n_devices <= 0) means all devices.  A device may be listed more than once (several dispatcher
 * threads sharing it).  Starts one dispatcher thread per entry. */
RT_API int rt_frame_ctx_create(const int* devices, int n_devices, rt_frame_ctx** out_ctx);
/* Make this world the job's: host-side preparation once (device layouts, the candidate-filter BVH), one upload per
 * device.  Replaces the previous world of the context.  Must not race with rt_frame_ctx_render on the same context. */
RT_API int rt_frame_ctx_set_world(rt_frame_ctx* ctx,
                                  const rt_sphere* spheres, uint32_t n_spheres,
                                  const rt_triangle* triangles, uint32_t n_triangles,
                                  const uint32_t* world_index);
/* The job's camera ("placed camera" above): every later frame of the context is rendered from it; NULL: the reference camera.
 * A new pose starts from the snake assignment again (the strips' costs were measured from another viewpoint).  Must not race with
 * rt_frame_ctx_render on the same context. */
RT_API int rt_frame_ctx_set_camera(rt_frame_ctx* ctx, const rt_camera* cam);
/* Render one frame of the job into out_rgb (>= H*W*3 bytes).  The context page-locks out_rgb (hipHostRegister) the
 * first time it sees it and keeps the registration until another buffer is passed or the context is destroyed — pass the
 * same buffer for every frame of a job and only the first pays pin_ms.  The caller must not free a buffer the context
 * still holds: call rt_frame_ctx_release_buffer (or destroy the context) first.  Synchronous; one call at a time per
 * context.  stats may be NULL. */
RT_API int rt_frame_ctx_render(rt_frame_ctx* ctx, const rt_tile_request* req,
                               uint8_t* out_rgb, size_t out_len, rt_frame_stats* stats);
/* Drop the page-locked registration of the last frame buffer (no-op if none). */
RT_API int rt_frame_ctx_release_buffer(rt_frame_ctx* ctx);
/* Stops the dispatcher threads, releases the worlds, buffers, streams and the registration. */
RT_API void rt_frame_ctx_destroy(rt_frame_ctx* ctx);

/* One-shot: a context over `devices`, this world, one frame, everything released again. */
RT_API int rt_render_frame(const int* devices, int n_devices, const rt_tile_request* req,
                           const rt_sphere* spheres, uint32_t n_spheres,
                           const rt_triangle* triangles, uint32_t n_triangles,
                           const uint32_t* world_index,
                           uint8_t* out_rgb, size_t out_len, rt_tile_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* RT_TILE_H */
