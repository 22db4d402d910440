"""The caller-ray kernels (ray queries rt_query.hip.h, path tracing of caller rays rt_trace.hip.h, feature buffers rt_aov.hip.h)
against the batch ray oracle (oracle.intersect_batch / oracle.trace_batch, pinned on the CPU by tests/test_oracle_batch.py), ray by
ray and bit for bit, every ray of every case:
(a) a differential fuzz over the scene generators of tests/test_gpu_fuzz.py — per case a ray population drawn from the scene's
    bounds with windows of the rays' own (tests/_ray_cases.py), one of test_gpu_query.CONFIGS, and four calls: closest hit, any hit,
    the trace with a state per ray (colour sums, segments, written-back states; BVH semantics included) and the seeded trace on a
    subset; then the feature buffers of a strip of the scene.  Deterministic: case i is reproducible from its number;
(b) the branches of plan_query / plan_trace that only the CPU plan harnesses had seen: path32 and the 128-lane workgroup (70 000
    primitives at 62 bounces), full_chain forced by inverted sphere boxes, thousands of coincident primitives, trees as deep as
    the walk's stack holds and deeper (the scan), a walk stack plus path stack beyond 64 KiB at 256 lanes, batch sizes around the
    workgroup size with the path stack of the last partial workgroup live.
The conditions that keep a case from passing vacuously (hits and misses, real ties, narrow windows that change a hit, deep paths)
are asserted from the oracle's answers before the GPU is asked (tests/_ray_cases.py fuzz_case, and the assertions here)."""
import os

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

import _ray_cases as R
from test_gpu_aov import _assert_planes_equal, _camera_samples
from test_gpu_query import CONFIGS
from test_gpu_trace import _same_bits

pytestmark = pytest.mark.gpu

F = _abi
NONE = _abi.RT_HIT_NONE
WALK, SCAN = 2, 1
DEFAULT_COUNTS = (60, 6, 8)
N_SMALL = int(os.environ.get("RT_RAY_FUZZ_CASES", DEFAULT_COUNTS[0]))      # RT_RAY_FUZZ_CASES=1000 for a long soak
N_BIG = int(os.environ.get("RT_RAY_FUZZ_BIG", DEFAULT_COUNTS[1]))
N_MIXED = int(os.environ.get("RT_RAY_FUZZ_MIXED", DEFAULT_COUNTS[2]))
N_SEEDED = 160                                                              # rays of the seeded trace (a subset, from the front)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _eq(a, b):
    """Elementwise: equal bit for bit, NaN matching NaN."""
    a, b = _f32(a), _f32(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def check_closest(hits, rays, ref, what):
    """rt_hit records against the oracle's batch: a miss is (NONE, +inf, zeros); a hit has the oracle's world position, point and
    normal, and the distance of a float32 restatement of length(P - o)."""
    hit = ref["hit"]
    idx_ok = hits["index"] == ref["index"]
    assert idx_ok.all(), (what, "index", np.nonzero(~idx_ok)[0][:5], hits[~idx_ok][:3], ref["index"][~idx_ok][:3], rays[~idx_ok][:3])
    miss = hits[~hit]
    assert np.all(np.isposinf(miss["distance"])) and all(np.all(miss[k].view(np.uint32) == 0) for k in ("px", "py", "pz", "nx", "ny", "nz")), what
    h, r, o = hits[hit], {k: v[hit] for k, v in ref.items()}, rays[hit]
    for j, k in enumerate(("px", "py", "pz")):
        ok = _eq(h[k], r["point"][:, j])
        assert ok.all(), (what, k, np.nonzero(hit)[0][~ok][:5])
    for j, k in enumerate(("nx", "ny", "nz")):
        ok = _eq(h[k], r["normal"][:, j])
        assert ok.all(), (what, k, np.nonzero(hit)[0][~ok][:5])
    with np.errstate(all="ignore"):
        x, y, z = (_f32(h[a]) - _f32(o[b]) for a, b in (("px", "ox"), ("py", "oy"), ("pz", "oz")))
        dist = np.sqrt(_f32(_f32(_f32(x * x) + _f32(y * y)) + _f32(z * z)))
    ok = _eq(h["distance"], dist)
    assert ok.all(), (what, "distance", np.nonzero(hit)[0][~ok][:5])


def check_query(sc, rays, ref, flags, engine, what):
    o, d = R.od(rays)
    hits, st = sc.intersect(o, d, rays["t_min"], rays["t_max"], flags=flags)
    assert st.engine == engine and st.n_launches == 1 and st.primary_rays == st.ray_segments == len(rays), (what, st.engine)
    check_closest(hits, rays, ref, what)
    anyh, st_any = sc.intersect(o, d, rays["t_min"], rays["t_max"], any_hit=True, flags=flags)
    got = anyh["index"] != NONE
    assert np.array_equal(got, ref["hit"]), (what, "any hit", np.nonzero(got != ref["hit"])[0][:10])
    assert st_any.engine == engine


def check_trace(sc, rays, want, spp, mb, flags, engine, what, states=None, seed=None, as_given=False):
    """rt_scene_trace against oracle.trace_batch's (rgb, segments, states): every ray."""
    o, d = R.od(rays)
    if states is not None:
        rgb, segs, st, st1 = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=spp, max_bounces=mb, rng_state=states, flags=flags,
                                      as_given=as_given)
        assert np.array_equal(st1, want[2]), (what, "states", np.nonzero(np.any(st1 != want[2], 1))[0][:5])
    else:
        rgb, segs, st = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=spp, max_bounces=mb, seed=seed, flags=flags, as_given=as_given)
    ok = np.all(_eq(rgb, want[0]), 1)
    assert ok.all(), (what, "rgb", np.nonzero(~ok)[0][:5], rgb[~ok][:3], want[0][~ok][:3], rays[~ok][:3])
    assert np.array_equal(segs, want[1]), (what, "segments", np.nonzero(segs != want[1])[0][:5])
    assert st.engine == engine and st.n_launches == 1, (what, st.engine)
    assert st.primary_rays == len(rays) * spp and st.ray_segments == int(want[1].sum()), what


def aov_request(rq, flags):
    """The generator's strip when it is small, else the same camera on a smaller frame (at most about 6 000 camera rays)."""
    r = rq.copy()
    r.flags = flags
    r.spp = min(r.spp, 8)
    while (r.height // r.divisions) * r.width * r.spp > 6000 and (r.width > 8 or r.height > 2 * r.divisions):
        r.width = max(8, r.width * 2 // 3)
        r.height = max(r.divisions, r.height * 2 // 3)
    return r


def expected_planes(oracle, sph, tri, wi, rq, backend):
    """The feature buffers the contract defines, composed from intersect_batch(ray_as_given) over the tile's camera rays."""
    hs, W, S = rq.height // rq.divisions, rq.width, rq.spp
    o, d = _camera_samples(oracle, rq)
    rays = R.make_rays(o, d, rq.t_min, rq.t_max)
    e = oracle.intersect_batch(sph, tri, rays, backend=backend, world_index=wi, ray_as_given=True)
    hit = e["hit"]
    alb = e["albedo"].copy()
    for j in np.nonzero(~hit)[0]:
        alb[j] = oracle.sky(d[j])
    x, y, z = ((e["point"][:, k] - o[:, k]).astype(np.float32) for k in range(3))
    dist = np.where(hit, np.sqrt(_f32(_f32(_f32(x * x) + _f32(y * y)) + _f32(z * z))), np.float32(0)).astype(np.float32)
    n = hs * W
    per = lambda a: a.reshape((n, S) + a.shape[1:])
    planes = {"albedo": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32), "depth": np.zeros(n, np.float32)}
    hit_s, nrm_s, alb_s, dist_s = per(hit), per(e["normal"]), per(alb), per(dist)
    for s in range(S):                                           # in sample order; a miss adds nothing to normal and depth
        planes["albedo"] = (planes["albedo"] + alb_s[:, s]).astype(np.float32)
        planes["normal"] = np.where(hit_s[:, s, None], (planes["normal"] + nrm_s[:, s]).astype(np.float32), planes["normal"])
        planes["depth"] = np.where(hit_s[:, s], (planes["depth"] + dist_s[:, s]).astype(np.float32), planes["depth"])
    planes["hits"] = hit_s.sum(1).astype(np.uint32)
    planes["index"] = per(e["index"])[:, 0].copy()
    return {k: v.reshape((hs, W, 3) if v.ndim == 2 else (hs, W)) for k, v in planes.items()}, hit


def check_aov(oracle, sc, sph, tri, wi, rq, backend, engine, what):
    want, hit = expected_planes(oracle, sph, tri, wi, rq, backend)
    planes, st = sc.render_aov(rq)
    _assert_planes_equal(planes, want, what)
    assert st.engine == engine and st.primary_rays == len(hit), (what, st.engine)
    return hit


def _run_case(oracle, kind, i):
    c = R.fuzz_case(oracle, kind, i, CONFIGS)                    # the oracle's answers and the case's conditions, before any launch
    what = (kind, i, c["cfg"])
    sph, tri, wi, rays = c["sph"], c["tri"], c["wi"], c["rays"]
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        check_query(sc, rays, c["hits"], c["flags"], c["engine"], what)
        check_trace(sc, rays, c["trace"], c["spp"], c["mb"], c["flags"], c["engine"], what + ("states", c["mb"], c["spp"]), states=c["states"])
        sub = rays[:N_SEEDED]
        seeded = oracle.trace_batch(sph, tri, sub, spp=c["spp"], max_bounces=c["mb"], backend=c["backend"], world_index=wi, seed=c["seed"])
        check_trace(sc, sub, seeded, c["spp"], c["mb"], c["flags"], c["engine"], what + ("seeded",), seed=c["seed"])
        rq = aov_request(c["rq"], c["flags"])
        if rq.height // rq.divisions > 0:                        # (a zero-row strip has no feature buffers: the rest of the case ran)
            check_aov(oracle, sc, sph, tri, wi, rq, c["backend"], c["engine"], what + ("aov",))


@pytest.mark.parametrize("i", range(N_SMALL))
def test_ray_fuzz_case(ndev, oracle, i):
    _run_case(oracle, "small", i)


@pytest.mark.parametrize("i", range(N_BIG))
def test_ray_fuzz_big_scene(ndev, oracle, i):
    _run_case(oracle, "big", i)


@pytest.mark.parametrize("i", range(N_MIXED))
def test_ray_fuzz_big_mixed_scene(ndev, oracle, i):
    _run_case(oracle, "mixed", i)


# ---------------------------------------------------------------- (b) the plan branches
def _branch_rays(oracle, sph, seed, n=600, wi=None, extra=None):
    g = np.random.default_rng(seed)
    rays, narrow, _ = R.ray_population(oracle, g, sph, np.zeros(0, _abi.TRIANGLE_DTYPE), n, wi)
    return rays if extra is None else np.concatenate([extra, rays])


@pytest.fixture(scope="module")
def field(oracle):
    """70 000 spheres: the scene, its tree depth, the rays (mirror rays first) and the oracle's traces under BVH semantics."""
    sph, mirrors = R.field70000()
    depth = R.tree_depth(sph, None)
    g = np.random.default_rng(70)
    rays = _branch_rays(oracle, sph, 71, n=600, extra=R.mirror_rays(g, sph, mirrors))
    st0 = R.states(len(rays), 72)
    want = {mb: oracle.trace_batch(sph, None, rays, spp=1, max_bounces=mb, backend=1, states=st0) for mb in (62, 10)}
    return sph, depth, rays, st0, want


def test_path32_and_the_128_lane_workgroup(ndev, oracle, field):
    sph, depth, rays, st0, want = field
    n = len(sph)
    p62, p10 = R.trace_plan(n, 0, depth, False, 0, 62), R.trace_plan(n, 0, depth, False, 0, 10)
    assert p62["path32"] and p62["block"] == 128 and p62["engine"] == WALK, p62
    assert p10["path32"] and p10["block"] == 256 and p10["engine"] == WALK, p10
    assert R.trace_plan(n, 0, depth, False, F.RT_FLAG_EXACT_SCAN, 62)["engine"] == SCAN
    assert int(want[62][1].max()) > 16 and int(want[10][1].max()) == 11, "no path uses the deep entries of the path stack"
    hits = oracle.intersect_batch(sph, None, rays, backend=1)
    assert hits["hit"].any() and not hits["hit"].all()
    with rt.Scene(0, rt.World(sph)) as sc:
        check_query(sc, rays, hits, 0, WALK, "field70000")
        for mb in (62, 10):
            for flags, engine in ((0, WALK), (F.RT_FLAG_EXACT_SCAN, SCAN)):
                check_trace(sc, rays, want[mb], 1, mb, flags, engine, ("field70000", mb, flags), states=st0)


@pytest.mark.parametrize("n", [1, 100, 255, 256, 257])
def test_batch_edges_with_a_live_path_stack(ndev, field, n):
    """Batches around the workgroup sizes at 62 bounces on the 70 000-sphere scene, mirror rays first: the lanes of the last,
    partial workgroup push and pop their path stacks to the full depth."""
    sph, depth, rays, st0, want = field
    assert int(want[62][1][:n].max()) > 16
    sub = tuple(a[:n] for a in want[62])
    with rt.Scene(0, rt.World(sph)) as sc:
        check_trace(sc, rays[:n], sub, 1, 62, 0, WALK, ("edge", n), states=st0[:n])


def test_inverted_sphere_boxes_force_the_full_chain(ndev, oracle):
    sph = R.odd_radii_world()
    depth = R.tree_depth(sph, None)
    assert R.query_plan(len(sph), 0, depth, True, 0)["full_chain"] and R.trace_plan(len(sph), 0, depth, True, 0, 10)["full_chain"]
    assert np.any(sph["radius"] < 0)                             # what the host derives the plan's `inverted` from
    rays = _branch_rays(oracle, sph, 81)
    st0 = R.states(len(rays), 82)
    rq = _abi.default_request(width=64, height=36, divisions=2, division_no=1, spp=2, seed=83)
    with rt.Scene(0, rt.World(sph)) as sc:
        for cfg in ("default", "exact_scan", "no_bvh_cull"):
            flags, engine, backend = CONFIGS[cfg]
            hits = oracle.intersect_batch(sph, None, rays, backend=backend)
            assert hits["hit"].any() and not hits["hit"].all()
            check_query(sc, rays, hits, flags, engine, ("odd radii", cfg))
            want = oracle.trace_batch(sph, None, rays, spp=2, max_bounces=10, backend=backend, states=st0)
            assert int(want[1].max()) >= 4
            check_trace(sc, rays, want, 2, 10, flags, engine, ("odd radii", cfg), states=st0)
            r = rq.copy()
            r.flags = flags
            hit = check_aov(oracle, sc, sph, None, None, r, backend, engine, ("odd radii", cfg, "aov"))
            assert hit.any() and not hit.all()


@pytest.mark.parametrize("permuted", [False, True])
def test_thousands_of_coincident_spheres(ndev, oracle, permuted):
    """Every hit on the pile is an exact tie among 2 000 candidates: the first leaf in depth-first order wins (backend 1), the
    earliest world position under the plain scan."""
    sph = R.pile_world()
    wi = np.random.default_rng(6).permutation(len(sph)).astype(np.uint32) if permuted else None
    g = np.random.default_rng(91)
    rays, _, _ = R.ray_population(oracle, g, sph, np.zeros(0, _abi.TRIANGLE_DTYPE), 400, wi, aim_at=[0, 2000])
    st0 = R.states(len(rays), 92)
    pos = np.arange(len(sph), dtype=np.uint32) if wi is None else wi
    winners = {}
    with rt.Scene(0, rt.World(sph, None, wi)) as sc:
        for cfg in ("default", "exact_scan", "no_bvh_cull"):
            flags, engine, backend = CONFIGS[cfg]
            hits = oracle.intersect_batch(sph, None, rays, backend=backend, world_index=wi)
            on_pile = np.isin(hits["index"], pos[:4000])
            assert on_pile.sum() >= 20 and not hits["hit"].all()
            winners[backend] = hits["index"]
            check_query(sc, rays, hits, flags, engine, ("pile", permuted, cfg))
            want = oracle.trace_batch(sph, None, rays, spp=2, max_bounces=10, backend=backend, world_index=wi, states=st0)
            check_trace(sc, rays, want, 2, 10, flags, engine, ("pile", permuted, cfg), states=st0)
    assert np.any(winners[0] != winners[1])                      # the two tie rules name different copies


@pytest.mark.parametrize("n,walks", [(40, True), (64, True), (66, False)])
def test_trees_as_deep_as_the_walk_stack_and_deeper(ndev, oracle, n, walks):
    """chain_world(n): a tree of depth n - 1.  39: walk stack plus path stack of a 62-bounce trace beyond 64 KiB at 256 lanes;
    63 = TRAV_STACK - 1: the deepest tree the walk takes, every entry of its stack used, 128 lanes at 62 bounces; 65: the scan with
    BVH semantics (scan_mode 2) whatever the flags say.  All against backend 1."""
    sph = R.chain_world(n)
    depth = R.tree_depth(sph, None)
    top = R.trav_stack()
    assert depth == n - 1 and (depth < top) == walks
    engine = WALK if walks else SCAN
    q, p62 = R.query_plan(n, 0, depth, False, 0), R.trace_plan(n, 0, depth, False, 0, 62)
    assert q["engine"] == engine and q["scan_mode"] == 2 and p62["engine"] == engine and p62["scan_mode"] == 2
    if n == 40:
        assert p62["block"] == 256 and p62["lds"] > 64 * 1024, p62
    if n == 64:
        assert depth == top - 1 and p62["block"] == 128, p62
    g = np.random.default_rng(100 + n)
    rays = R.chain_rays(g, sph, 700)
    hits = oracle.intersect_batch(sph, None, rays, backend=1)
    assert hits["hit"].any() and not hits["hit"].all()
    assert len(np.unique(hits["index"][hits["hit"]])) > n // 2    # leaves all along the chain are reached
    st0 = R.states(len(rays), n)
    rq = _abi.default_request(width=48, height=32, divisions=2, division_no=0, spp=2, seed=n, fov=2.2, t_max=np.inf)
    with rt.Scene(0, rt.World(sph)) as sc:
        check_query(sc, rays, hits, 0, engine, ("chain", n))
        for mb in (62, 10):
            want = oracle.trace_batch(sph, None, rays, spp=1, max_bounces=mb, backend=1, states=st0)
            assert int(want[1].max()) >= 4
            check_trace(sc, rays, want, 1, mb, 0, engine, ("chain", n, mb), states=st0)
        check_aov(oracle, sc, sph, None, None, rq, 1, engine, ("chain", n, "aov"))
