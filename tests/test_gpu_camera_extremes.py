"""Camera rays on the GPU at extreme poses, knobs and film geometry (the corpus of tests/_camera_cases.py), against the
numpy restatement of the placed camera (tests/_camera_np.py) and, through it, the batch oracle:
a. rays and states of every case from the camera-ray kernel, host form (with and without states, a sample sub-range) and device form
   (sentinel guards around the outputs);
b. a launch with more records than one grid holds: the persistent loop strides;
c. the tile kernels: the accum of a strip is the in-order f32 sum of the batch oracle's ray_color over the restated rays, and every
   forced engine renders the oracle's image;
d. the feature buffers against the batch oracle's first hits over the restated rays.
The rule everywhere: a float is NaN in one exactly where it is NaN in the other, every other float is bit-equal (signed zeros and
infinities included), integers and RNG states are equal."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

import _camera_cases as cc
import _camera_np as cnp
from test_gpu_camera import ENGINE_FLAGS, _quantise, _sum_in_order
from test_gpu_query import _world

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
F = _abi
BOUNCES = 3

# (name, request, pose, (begin, end)): the knob cases at all their samples, the geometry cases at their sample range under P0
KNOB_RUNS = [(name, cc.request(knobs, max_bounces=BOUNCES), pose, (0, cc.FRAME["spp"])) for name, knobs, pose, _ in cc.CASES]
GEOMETRY_RUNS = [(name, _abi.default_request(**knobs, max_bounces=BOUNCES), cc.P0, rng) for name, knobs, rng in cc.GEOMETRY + cc.COUNTS]
TALL_RUNS = [r for r in GEOMETRY_RUNS if r[0].startswith("tall_")]
WIDE_RUN = (cc.WIDE[0], _abi.default_request(**cc.WIDE[1], max_bounces=BOUNCES), cc.P0, cc.WIDE[2])
RUNS = {r[0]: r for r in KNOB_RUNS + GEOMETRY_RUNS + [WIDE_RUN]}
SMALL_RUNS = [r[0] for r in KNOB_RUNS + GEOMETRY_RUNS]                      # at most a few thousand records each
SENTINEL = 0x7FC5A5A5                                                       # (a NaN as a float: no kernel computes this pattern)
GUARD = 64                                                                  # records kept free at each end of a device output


def _cam(pose):
    return None if pose is None else _abi.Camera.look_at(*pose)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rows_that_differ(got, want):
    """The rows of two float32 arrays (n, k) that differ under the rule: NaN where NaN, every other value bit-equal."""
    got, want = (np.ascontiguousarray(a, np.float32).reshape(len(a), -1) for a in (got, want))
    assert got.shape == want.shape, (got.shape, want.shape)
    ng, nw = np.isnan(got), np.isnan(want)
    bad = (ng != nw) | (~ng & ~nw & (_u32(got) != _u32(want)))
    return np.nonzero(bad.any(1))[0]


def _show(v):
    v = np.atleast_1d(np.ascontiguousarray(v))
    return " ".join(f"{x!r}[{b:08x}]" for x, b in zip(v.tolist(), _u32(v.astype(np.float32)).tolist())) if v.dtype.kind == "f" \
        else " ".join(str(x) for x in v.tolist())


def _fail(oracle, run, what, rows, got, want, per_row):
    """Print the first mismatching rows — the case, the row's records with (x, row, sample), both values with their bits, the restated
    dot1 and dot2 — and fail.  per_row: the records of one row of got / want (1 for rays, the samples of the call for pixel planes)."""
    name, rq, pose, (b, e) = run
    recs = cnp.strip_records(rq, b, e)
    dots = cc.restated(oracle, rq, pose, b, e)[2]
    for r in rows[:4]:
        print(f"{name}: {what} row {r}\n  got  {_show(got[r])}\n  want {_show(want[r])}")
        for i in range(r * per_row, (r + 1) * per_row):
            print(f"  record {i} (x, row, sample) = {recs[i]}  dot1 {_show(dots[i, 0])}  dot2 {_show(dots[i, 1])}")
    raise AssertionError(f"{name}: {what}: {len(rows)} rows differ, first {rows[:8].tolist()}")


def _check_floats(oracle, run, what, got, want, per_row=1):
    rows = _rows_that_differ(got, want)
    if len(rows):
        _fail(oracle, run, what, rows, np.asarray(got).reshape(len(got), -1), np.asarray(want).reshape(len(want), -1), per_row)


def _check_ints(oracle, run, what, got, want, per_row=1):
    got, want = (np.ascontiguousarray(a).reshape(len(a), -1) for a in (got, want))
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    rows = np.nonzero((got != want).any(1))[0]
    if len(rows):
        _fail(oracle, run, what, rows, got, want, per_row)


def _ray_words(rays):
    return np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)


def _check_rays(oracle, run, what, rays, states, erays, estates):
    _check_floats(oracle, run, what + " rays", _ray_words(rays), _ray_words(erays))
    if states is not None:
        _check_ints(oracle, run, what + " states", states, estates)


@pytest.fixture(scope="module")
def scene(ndev):
    sph, tri = _world("cornell16")
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        yield sc


# ------------------------------------------------------------------------------------------------------- a. rays and states


def _check_host_forms(oracle, sc, run):
    name, rq, pose, (b, e) = run
    erays, estates, _ = cc.restated(oracle, rq, pose, b, e)
    n = e - b
    sc.set_camera(_cam(pose))
    rays, states, st = sc.camera_rays(rq, b, e)                                   # the twin that stores the states
    _check_rays(oracle, run, "host form", rays, states, erays, estates)
    assert st.primary_rays == len(erays) and st.n_launches == 1
    rays, none, _ = sc.camera_rays(rq, b, e, want_states=False)                   # ... and the one that does not
    assert none is None
    _check_rays(oracle, run, "host form, no states", rays, None, erays, None)
    # a sample sub-range: the same records, cut out (the last sample alone; with three or more, the ones after the first as well)
    for sb, se in {(e - 1, e), (b + 1, e)} if n > 1 else ():
        cut = slice(sb - b, se - b)
        part, pstates, _ = sc.camera_rays(rq, sb, se, want_states=se - sb == 1)
        sub = (name + f"[{sb},{se})", rq, pose, (sb, se))
        _check_rays(oracle, sub, "sub-range", part, pstates, erays.reshape(-1, n)[:, cut].reshape(-1),
                    estates.reshape(-1, n, 4)[:, cut].reshape(-1, 4))


@pytest.mark.parametrize("name", SMALL_RUNS)
def test_camera_rays_equal_the_restatement(oracle, scene, name):
    run = RUNS[name]
    _check_host_forms(oracle, scene, run)
    _, rq, pose, (b, e) = run
    if pose is None:
        # the reference camera: the oracle's camera_ray is a second reference
        rays, states, _ = scene.camera_rays(rq, b, e)
        want = np.zeros((len(rays), 6), np.float32)
        wstates = np.zeros((len(rays), 4), np.uint64)
        for i, (x, yg, s) in enumerate(cnp.strip_records(rq, b, e)):
            wstates[i] = cnp.sample_state(oracle, rq, x, yg, s)
            want[i] = np.concatenate(oracle.camera_ray(rq, x, rq.height - 1 - yg, wstates[i]))
        _check_floats(oracle, run, "oracle camera_ray", _ray_words(rays)[:, [0, 1, 2, 4, 5, 6]], want)
        _check_ints(oracle, run, "oracle states", states, wstates)


def test_camera_rays_of_the_last_row_of_a_wide_film(oracle, scene):
    """One row of 32768 records at the last row of a 32768 x 65535 film, sample 4095 of 4096: stream indices up to 2^43."""
    _check_host_forms(oracle, scene, WIDE_RUN)


def _device_form_body():
    """In a child process that imported torch first: every run through camera_rays_device into tensors GUARD records longer than needed
    at each end, filled with SENTINEL; the records equal the restatement's, the guards keep the sentinel."""
    import torch
    from oracle import oracle as orc
    orc.load()
    dev = torch.device("cuda:0")
    sph, tri = _world("cornell16")
    guard_words = np.full(GUARD * 8, SENTINEL, np.uint32)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for run in RUNS.values():
            name, rq, pose, (b, e) = run
            sc.set_camera(_cam(pose))
            if run is WIDE_RUN:                                                   # (restated once, by the host-form test: here the host form's)
                erays, estates, _ = sc.camera_rays(rq, b, e)
            else:
                erays, estates, _ = cc.restated(orc, rq, pose, b, e)
            n = len(erays)
            for with_states in (True, False):
                d_rays = torch.full(((n + 2 * GUARD) * 8,), SENTINEL, dtype=torch.int32, device=dev)
                d_states = torch.full(((n + 2 * GUARD) * 8,), SENTINEL, dtype=torch.int32, device=dev)   # 4 uint64 = 8 words a record
                torch.cuda.synchronize()
                sc.camera_rays_device(rq, b, e, d_rays.data_ptr() + GUARD * 32,
                                      d_states.data_ptr() + GUARD * 32 if with_states else 0)
                st = sc.collect()
                assert st.primary_rays == n and st.n_launches == 1, (name, st.primary_rays, st.n_launches)
                r = d_rays.cpu().numpy().view(np.uint32)
                s = d_states.cpu().numpy().view(np.uint32)
                for what, a in (("rays", r), ("states", s)):
                    assert np.array_equal(a[:GUARD * 8], guard_words) and np.array_equal(a[-GUARD * 8:], guard_words), \
                        (name, what, "a guard lost its sentinel")
                body = slice(GUARD * 8, -GUARD * 8)
                _check_rays(orc, run, "device form", r[body].view(np.float32).reshape(-1, 8),
                            s[body].view(np.uint64).reshape(-1, 4) if with_states else None, erays, estates)
                if not with_states:
                    assert (s == SENTINEL).all(), (name, "states written without a states pointer")


_CHILD = r"""
import sys
import torch                                                      # first: the library then binds to torch's HIP runtime
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_camera_extremes as T
T.{body}()
print("ok")
"""


def _run_child(body):
    code = _CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), body=body)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_camera_rays_device_form_keeps_its_guards(ndev):
    _run_child("_device_form_body")


# ------------------------------------------------------------------------------------------------------ b. the striding launch


def test_a_launch_larger_than_the_grid_strides(oracle, scene):
    """More records than the device holds in one grid (multi_processor_count x 8 workgroups of 256): the persistent loop of the
    camera-ray kernel goes round.  The records equal the ones made 16 samples at a time, byte for byte, and 2000 of them, drawn
    with a fixed seed, the restatement."""
    n_cu = _multi_processor_count()
    one_grid = n_cu * 8 * 256
    W, H = 96, 54
    spp = 16 * (one_grid // (W * H * 16) + 1)
    assert W * H * spp > one_grid and spp <= 4096, (n_cu, spp)
    print(f"compute units {n_cu}: one grid holds {one_grid} records, the call makes {W * H * spp} ({spp} spp)")
    rq = _abi.default_request(width=W, height=H, divisions=1, spp=spp, seed=0xE57, aperture=0.3, focus_distance=2.5)
    scene.set_camera(_cam(cc.P0))
    rays, states, st = scene.camera_rays(rq)
    assert st.primary_rays == len(rays) == W * H * spp and st.n_launches == 1
    r3, s3 = rays.reshape(W * H, spp), states.reshape(W * H, spp, 4)
    for b in range(0, spp, 16):
        part, pstates, _ = scene.camera_rays(rq, b, b + 16)
        assert part.tobytes() == np.ascontiguousarray(r3[:, b:b + 16]).tobytes(), ("samples", b)
        assert pstates.tobytes() == np.ascontiguousarray(s3[:, b:b + 16]).tobytes(), ("samples", b)
    g = np.random.default_rng(0x57D1DE)
    pick = np.sort(g.choice(len(rays), 2000, replace=False))
    pick[-1] = len(rays) - 1                                                      # the last record among them
    assert (pick >= one_grid).sum() > 100                                         # ... and many beyond the first round
    recs = [((i // spp) % W, (i // spp) // W, i % spp) for i in pick.tolist()]
    erays, estates = cnp.rays_of(oracle, rq, cc.P0, recs)
    bad = _rows_that_differ(_ray_words(rays[pick]), _ray_words(erays))
    assert len(bad) == 0, ("records", pick[bad][:8], [recs[i] for i in bad[:8]], rays[pick][bad[:2]], erays[bad[:2]])
    assert np.array_equal(states[pick], estates), ("states of records", pick[(states[pick] != estates).any(1)][:8])


def _multi_processor_count():
    """The device's compute units, asked of torch in a child process (torch needs a process of its own, imported first)."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return int(r.stdout.strip().splitlines()[-1])


# ------------------------------------------------------------------------------------------------------ c. the tile kernels


_TRACED = {}


def _traced(oracle, world, run, backend):
    """(the in-order f32 sum per pixel of the batch oracle's ray_color over the restated rays of `run`, its segments, its rays),
    computed once per world and backend and shared: leave it unchanged."""
    name, rq, pose, (b, e) = run
    key = (world, name, backend)
    if key not in _TRACED:
        sph, tri = _world(world)
        erays, estates, _ = cc.restated(oracle, rq, pose, b, e)
        ergb, esegs, _ = oracle.trace_batch(sph, tri, erays, spp=1, max_bounces=rq.max_bounces, backend=backend, ray_as_given=True,
                                            states=estates)
        _TRACED[key] = _sum_in_order(ergb.reshape(-1, e - b, 3)), int(esegs.sum()), len(erays)
    return _TRACED[key]


def _check_tile(oracle, sc, world, run, flags, backend, cuts=None):
    """The strip of `run` through render_tile_pass (in the passes `cuts`, default one) against the batch oracle over the restated rays."""
    name, rq, pose, (b, e) = run
    rq = rq.copy()
    rq.flags = flags
    total, esegs, n_rays = _traced(oracle, world, run, backend)
    n = e - b
    accum = np.zeros((rq.height // rq.divisions, rq.width, 3), np.float32)
    segs = primary = 0
    for cb, ce in cuts or [(b, e)]:
        rgb, f32, accum, st = sc.render_tile_pass(rq, cb, ce, accum, want_f32=True)
        segs += st.ray_segments
        primary += st.primary_rays
    what = f"tile flags {flags:#x} cuts {cuts}"
    _check_floats(oracle, run, what + " accum", accum.reshape(-1, 3), total, n)
    with np.errstate(invalid="ignore"):
        prev = np.sqrt((total / np.float32(e)).astype(np.float32)).astype(np.float32)
    _check_floats(oracle, run, what + " f32", f32.reshape(-1, 3), prev, n)
    _check_ints(oracle, run, what + " rgb", rgb.reshape(-1, 3), _quantise(prev), n)
    assert esegs == segs and primary == n_rays, (name, what, esegs, segs, primary)
    return st.engine


@pytest.mark.parametrize("world", ["cornell16", "quad_room"])
def test_tile_accum_equals_the_batch_oracle(ndev, oracle, world):
    sph, tri = _world(world)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for name in SMALL_RUNS:
            run = RUNS[name]
            sc.set_camera(_cam(run[2]))
            for flags, backend in ((0, 1), (F.RT_FLAG_NO_BVH_CULL, 0)):
                _check_tile(oracle, sc, world, run, flags, backend)


def test_huge_film_passes_compose(ndev, oracle):
    """The six samples of the huge-film strips in two passes, [4090, 4093) and [4093, 4096), onto a running accum."""
    world = "cornell16"
    sph, tri = _world(world)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_camera(_cam(cc.P0))
        for run in TALL_RUNS:
            b, e = run[3]
            for flags, backend in ((0, 1), (F.RT_FLAG_NO_BVH_CULL, 0)):
                _check_tile(oracle, sc, world, run, flags, backend, cuts=[(b, b + 3), (b + 3, e)])


@pytest.mark.parametrize("world", ["rand1024", "field9000", "terrain"])      # the worlds of test_posed_frame_is_the_same_under_every_engine
def test_every_engine_renders_the_oracles_image(ndev, oracle, world):
    """Every entry of ENGINE_FLAGS on every corpus case: each compiled instance of the tile kernel has its own copy of the camera arm."""
    sph, tri = _world(world)
    engines = {}
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for run in KNOB_RUNS:
            sc.set_camera(_cam(run[2]))
            for flag_name, fl in ENGINE_FLAGS.items():
                engines[flag_name] = _check_tile(oracle, sc, world, run, fl, 1)
    print(world, "engines that ran:", engines)
    assert len(set(engines.values())) >= 3, engines


# --------------------------------------------------------------------------------------------------- d. the feature buffers


def _expected_planes(oracle, sph, tri, rays, n, backend):
    """The feature buffers of a strip from the batch oracle's first hits over its rays (n samples a pixel), as
    test_gpu_camera.test_posed_feature_buffers_equal_the_batch_oracle computes them.  (They are compared under this file's rule, not
    with test_gpu_aov._assert_planes_equal: the corpus puts NaNs into the planes, whose payload is no part of the contract.)"""
    h = oracle.intersect_batch(sph, tri, rays, backend=backend, ray_as_given=True)
    hit = h["hit"].reshape(-1, n)
    d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)
    o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)
    sky = np.array([oracle.sky(x) for x in d], np.float32)
    with np.errstate(all="ignore"):
        alb = np.where(h["hit"][:, None], h["albedo"], sky).astype(np.float32).reshape(-1, n, 3)
        dp = (h["point"] - o).astype(np.float32)
        dist = np.sqrt(((dp[:, 0] * dp[:, 0]).astype(np.float32) + (dp[:, 1] * dp[:, 1]).astype(np.float32)).astype(np.float32)
                       + (dp[:, 2] * dp[:, 2]).astype(np.float32)).astype(np.float32).reshape(-1, n)
        nrm = h["normal"].reshape(-1, n, 3)
        e_alb = _sum_in_order(alb)
        e_nrm = np.zeros((len(hit), 3), np.float32)                               # a miss adds nothing to normal and depth
        e_dep = np.zeros(len(hit), np.float32)
        for s in range(n):
            m = hit[:, s]
            e_nrm[m] = (e_nrm[m] + nrm[m, s]).astype(np.float32)
            e_dep[m] = (e_dep[m] + dist[m, s]).astype(np.float32)
    return dict(albedo=e_alb, normal=e_nrm, depth=e_dep, hits=hit.sum(1).astype(np.uint32), index=h["index"].reshape(-1, n)[:, 0])


@pytest.mark.parametrize("world", ["cornell16", "quad_room"])
def test_feature_buffers_equal_the_batch_oracle(ndev, oracle, world):
    sph, tri = _world(world)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for run in KNOB_RUNS + TALL_RUNS:
            name, rq0, pose, (b, e) = run
            erays, _, _ = cc.restated(oracle, rq0, pose, b, e)
            hs, w, n = rq0.height // rq0.divisions, rq0.width, e - b
            sc.set_camera(_cam(pose))
            for flags, backend in ((0, 1), (F.RT_FLAG_NO_BVH_CULL, 0)):
                rq = rq0.copy()
                rq.flags = flags
                out = None
                if b:                                                             # a later pass: onto sums that are zero so far
                    out = dict(albedo=np.zeros((hs, w, 3), np.float32), normal=np.zeros((hs, w, 3), np.float32),
                               depth=np.zeros((hs, w), np.float32), hits=np.zeros((hs, w), np.uint32),
                               index=np.full((hs, w), SENTINEL, np.uint32))
                planes, st = sc.render_aov(rq, b, e, out=out)
                want = _expected_planes(oracle, sph, tri, erays, n, backend)
                what = f"aov flags {flags:#x} "
                for k in ("albedo", "normal", "depth"):
                    _check_floats(oracle, run, what + k, planes[k].reshape(hs * w, -1), want[k].reshape(hs * w, -1), n)
                _check_ints(oracle, run, what + "hits", planes["hits"].reshape(-1), want["hits"], n)
                if b == 0:
                    _check_ints(oracle, run, what + "index", planes["index"].reshape(-1), want["index"], n)
                else:
                    assert (planes["index"] == SENTINEL).all(), (name, "index written by a later pass")
                assert st.primary_rays == len(erays), (name, flags)
