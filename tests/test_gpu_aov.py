"""Feature buffers of a strip on the GPU (rt_scene_render_aov, rt_scene_render_aovs_device), bit for bit throughout:
1. against the CPU oracle's composition, per (pixel, sample): the tile's camera ray (oracle.camera_ray from the stream of the
   sample), its closest hit (oracle.intersect: backend 1 = BVH semantics, 0 = plain scan) or the sky (oracle.sky), summed in
   sample order — for every scene of test_gpu_query.SCENES and the empty world, under every flag config that picks an engine;
2. passes: any cut of [0, S) gives the one-pass planes, and the index plane is left alone by passes that start after sample 0;
3. strips: a frame as 1 strip and as 4 strips stitches to the same planes;
4. the device form on torch tensors (one launch per 64 strips, a subset of the planes);
5. argument errors, with nothing launched;
6. a full-size strip of c3 spot-checked against the oracle;
7. alignment with the beauty image: pixels whose samples all missed have an albedo sum equal to the progressive accum;
8. the host forms of the AOV, trace, query and progressive entry points interleaved on one scene, the staging grown in turn:
   every result repeats;
9. the host forms that share the scene's one staging buffer — AOV, camera rays, denoiser, query, trace — and the tile pass
   interleaved on one scene, sizes growing and shrinking: each gives the bytes of the same call on a fresh scene."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes

from test_gpu_query import SCENES, _world

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
F = _abi
NONE = _abi.RT_HIT_NONE
WALK, SCAN = 2, 1
# flags -> (engine that must run, oracle backend)
CONFIGS = {
    "default": (0, WALK, 1),
    "full_chain": (F.RT_FLAG_FULL_CHAIN, WALK, 1),
    "exact_scan": (F.RT_FLAG_EXACT_SCAN, SCAN, 1),
    "linear_scan": (F.RT_FLAG_LINEAR_SCAN, SCAN, 1),
    "no_bvh_cull": (F.RT_FLAG_NO_BVH_CULL, SCAN, 0),
}
ALL_SCENES = SCENES + ["empty"]
PLANES = _abi.AOV_PLANES


def _scene_world(name):
    if name == "empty":
        return np.zeros(0, _abi.SPHERE_DTYPE), None
    return _world(name)


def _strip_request(flags=0, seed=0x7AC3, **kw):
    args = dict(width=24, height=16, divisions=2, division_no=1, spp=3, max_bounces=10, seed=seed, flags=flags)
    args.update(kw)
    return _abi.default_request(**args)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_planes_equal(got, want, what):
    for k in want:
        g, w = _bits(got[k]), _bits(want[k])
        bad = np.argwhere(g != w)
        assert g.shape == w.shape and len(bad) == 0, (what, k, bad[:5], got[k][tuple(bad[0])] if len(bad) else None,
                                                      want[k][tuple(bad[0])] if len(bad) else None)


def _preimage(d):
    """For camera directions d (N, 3) float32 — the value Ray::new hands over — directions d' with Ray::new(d') == d bit for bit
    (oracle.intersect applies Ray::new to the direction it is given; the library traces d as it is).  d is Ray::new of a vector
    within two ulps of it per component, so the search over those neighbours always succeeds."""
    d = np.ascontiguousarray(d, np.float32)
    steps = {}
    for k in range(-2, 3):
        v = d.copy()
        for _ in range(abs(k)):
            v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf)).astype(np.float32)
        steps[k] = v
    out = np.full_like(d, np.nan)
    found = np.zeros(len(d), bool)
    combos = sorted(((a, b, c) for a in range(-2, 3) for b in range(-2, 3) for c in range(-2, 3)),
                    key=lambda t: (abs(t[0]) + abs(t[1]) + abs(t[2]), t))
    for a, b, c in combos:
        cand = np.stack([steps[a][:, 0], steps[b][:, 1], steps[c][:, 2]], 1)
        x, y, z = cand[:, 0], cand[:, 1], cand[:, 2]
        ln = np.sqrt((x * x + y * y) + z * z)                    # glam length: (x x + y y) + z z, then a division (Ray::new)
        with np.errstate(divide="ignore", invalid="ignore"):
            nd = cand / ln[:, None]
        ok = ~found & np.all(_bits(nd) == _bits(d), 1)
        out[ok] = cand[ok]
        found |= ok
        if found.all():
            break
    assert found.all(), np.nonzero(~found)[0][:5]
    return out


def _camera_samples(oracle, rq, pixels=None, begin=0, end=None):
    """The tile's camera rays of samples [begin, end) of the strip's pixels ((row, x) pairs; None: all, row-major), pixel-major."""
    hs, S = rq.height // rq.divisions, rq.spp
    end = S if end is None else end
    if pixels is None:
        pixels = [(yl, x) for yl in range(hs) for x in range(rq.width)]
    o, d = [], []
    for yl, x in pixels:
        yg = hs * rq.division_no + yl
        for s in range(begin, end):
            state = oracle.seed_from_u64(oracle.sample_seed(rq.seed, yg * rq.width + x, S, s))
            a, b = oracle.camera_ray(rq, x, rq.height - 1 - yg, state)
            o.append(a)
            d.append(b)
    return np.array(o, np.float32).reshape(-1, 3), np.array(d, np.float32).reshape(-1, 3)


def _expected(oracle, sph, tri, rq, backend, pixels=None):
    """The planes the contract defines, from the oracle: per pixel, the in-order f32 sums over samples [0, S)."""
    hs, W, S = rq.height // rq.divisions, rq.width, rq.spp
    if pixels is None:
        pixels = [(yl, x) for yl in range(hs) for x in range(W)]
    o, d = _camera_samples(oracle, rq, pixels)
    dp = _preimage(d)
    n = len(pixels)
    alb, nrm = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    dep, hits, idx = np.zeros(n, np.float32), np.zeros(n, np.uint32), np.full(n, NONE, np.uint32)
    s_arg = sph if len(sph) else None
    t_arg = tri if tri is not None and len(tri) else None
    for i in range(n):
        for s in range(S):
            j = i * S + s
            e = oracle.intersect(s_arg, t_arg, o[j], dp[j], float(rq.t_min), float(rq.t_max), backend=backend)
            if e is None:
                alb[i] = alb[i] + oracle.sky(d[j])
                continue
            alb[i] = alb[i] + e["albedo"]
            nrm[i] = nrm[i] + e["normal"]
            x, y, z = (np.float32(e["point"][k]) - np.float32(o[j][k]) for k in range(3))
            dep[i] = dep[i] + np.sqrt(np.float32(np.float32(x * x) + np.float32(y * y)) + np.float32(z * z))
            hits[i] += 1
            if s == 0:
                idx[i] = e["index"]
    return {"albedo": alb, "normal": nrm, "depth": dep, "hits": hits, "index": idx}


def _grid(flat, hs, w):
    return {k: v.reshape((hs, w, 3) if v.ndim == 2 else (hs, w)) for k, v in flat.items()}


@pytest.fixture(scope="module")
def expected(oracle):
    """Per scene and oracle backend: the planes of _strip_request() (the oracle rebuilds its BVH per call: computed once)."""
    out = {}
    rq = _strip_request()
    hs = rq.height // rq.divisions
    for name in ALL_SCENES:
        sph, tri = _scene_world(name)
        for backend in (0, 1):
            out[name, backend] = _grid(_expected(oracle, sph, tri, rq, backend), hs, rq.width)
    return out


@pytest.mark.parametrize("scene", ALL_SCENES)
def test_planes_match_the_oracle_on_every_engine(ndev, expected, scene):
    sph, tri = _scene_world(scene)
    n_prims = len(sph) + (0 if tri is None else len(tri))
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for cfg, (flags, engine, backend) in CONFIGS.items():
            rq = _strip_request(flags)
            npix = (rq.height // rq.divisions) * rq.width
            planes, st = sc.render_aov(rq)
            want = expected[scene, backend]
            _assert_planes_equal(planes, want, (scene, cfg))
            assert st.engine == (engine if n_prims else SCAN), (cfg, st.engine)
            assert st.n_launches == 1 and st.primary_rays == st.ray_segments == npix * rq.spp
            if st.engine == SCAN:
                assert st.broad_candidates == npix * rq.spp * n_prims          # the scan tests every primitive
            else:
                assert 0 < st.broad_candidates < npix * rq.spp * max(n_prims, 2)
            assert st.kernel_ms > 0 and st.d2h_ms >= 0
    if scene == "empty":
        want = expected[scene, 1]
        assert np.all(want["hits"] == 0) and np.all(want["index"] == NONE)
        assert np.all(_bits(want["normal"]) == 0) and np.all(_bits(want["depth"]) == 0)     # +0.0: no addition at all
        assert np.all(want["albedo"] > 0)                                                    # the sky sums
    else:
        hit_frac = np.mean(expected[scene, 1]["hits"] > 0)
        assert hit_frac > 0, scene


def _run_passes(sc, rq, cuts, sentinel=None):
    out = None
    for b, e in cuts:
        planes, st = sc.render_aov(rq, b, e, out=out)
        out = planes
        assert st.primary_rays == st.ray_segments == (rq.height // rq.divisions) * rq.width * (e - b)
        if b == 0 and sentinel is not None:
            out["index"][...] = sentinel
    return out


@pytest.mark.parametrize("scene", ["terrain", "quad_room"])
def test_passes_give_the_one_pass_planes(ndev, scene):
    sph, tri = _scene_world(scene)
    S = 7
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for flags in (0, F.RT_FLAG_NO_BVH_CULL):
            rq = _strip_request(flags, spp=S, width=40, height=20)
            one, _ = sc.render_aov(rq, 0, S)
            for cuts in ([(0, 1), (1, 3), (3, S)], [(s, s + 1) for s in range(S)], [(0, 4), (4, S)]):
                got = _run_passes(sc, rq, cuts)
                _assert_planes_equal(got, one, (scene, flags, cuts))
                got = _run_passes(sc, rq, cuts, sentinel=0x5E17)
                assert np.all(got["index"] == 0x5E17), (scene, cuts)       # only a pass from sample 0 writes the index
            # a prefix [0, k) in passes equals one call over [0, k)
            k = 4
            pre, _ = sc.render_aov(rq, 0, k)
            _assert_planes_equal(_run_passes(sc, rq, [(0, 2), (2, k)]), pre, (scene, flags, "prefix"))
            assert np.any(one["hits"] > 0) and np.any(one["hits"] < S)


def test_strips_stitch_to_the_single_strip_planes(ndev):
    sph, tri = _scene_world("quad_room")
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for flags in (0, F.RT_FLAG_EXACT_SCAN):
            full = _abi.default_request(width=36, height=24, divisions=1, spp=3, seed=0xF7A3E, flags=flags)
            whole, _ = sc.render_aov(full)
            parts = []
            for k in range(4):
                rq = _abi.default_request(width=36, height=24, divisions=4, division_no=k, spp=3, seed=0xF7A3E, flags=flags)
                p, st = sc.render_aov(rq)
                assert st.primary_rays == 6 * 36 * 3
                parts.append(p)
            stitched = {k: np.concatenate([p[k] for p in parts], 0) for k in PLANES}
            _assert_planes_equal(stitched, whole, ("stitch", flags))


_DEVICE_CHILD = r"""
import numpy as np
import torch                                                      # first: the library then binds to torch's HIP runtime
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes
rt.init()
dev = torch.device("cuda", 0)
NAMES = _abi.AOV_PLANES
SHAPE3 = ("albedo", "normal")


def tensors(hs, w, names, fill):
    out = {}
    for k in names:
        shape = (hs, w, 3) if k in SHAPE3 else (hs, w)
        dt = torch.float32 if k in ("albedo", "normal", "depth") else torch.int32
        out[k] = torch.full(shape, fill, dtype=dt, device=dev)
    return out


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


sph, tri = scenes.quad_room()
with rt.Scene(0, rt.World(sph, tri)) as sc:
    for flags, engine in ((0, 2), (_abi.RT_FLAG_NO_BVH_CULL, 1)):
        for n_strips, w, h, S, cut in ((4, 40, 24, 5, 2), (66, 16, 132, 2, 1)):
            reqs = [_abi.default_request(width=w, height=h, divisions=n_strips, division_no=k, spp=S, seed=0xD37 + 3 * k, flags=flags)
                    for k in range(n_strips)]
            hs = h // n_strips
            ref = [sc.render_aov(rq)[0] for rq in reqs]
            t = [tensors(hs, w, NAMES, -7) for _ in reqs]
            stream = torch.cuda.Stream(device=dev)
            torch.cuda.synchronize()
            sc.collect()
            sc.render_aovs_device(reqs, 0, cut, [{k: v.data_ptr() for k, v in tt.items()} for tt in t], stream=stream.cuda_stream)
            sc.render_aovs_device(reqs, cut, S, [{k: v.data_ptr() for k, v in tt.items()} for tt in t], stream=stream.cuda_stream)
            torch.cuda.synchronize()
            st = sc.collect()
            per_call = (n_strips + 63) // 64
            assert st.n_launches == 2 * per_call, (n_strips, st.n_launches)
            assert st.primary_rays == st.ray_segments == n_strips * hs * w * S, st.primary_rays
            assert st.engine == engine and st.kernel_ms > 0 and st.broad_candidates > 0
            for k in range(n_strips):
                for name in NAMES:
                    assert host(t[k][name]).tobytes() == ref[k][name].tobytes(), (flags, n_strips, k, name)
        # a subset of the planes: only those are computed, the others are not touched
        reqs = [_abi.default_request(width=40, height=24, divisions=4, division_no=k, spp=3, seed=0xD37 + 3 * k, flags=flags)
                for k in range(4)]
        ref = [sc.render_aov(rq)[0] for rq in reqs]
        t = [tensors(6, 40, NAMES, -7) for _ in reqs]
        torch.cuda.synchronize()
        sc.render_aovs_device(reqs, 0, 3, [{"albedo": tt["albedo"].data_ptr(), "hits": tt["hits"].data_ptr()} for tt in t])
        torch.cuda.synchronize()
        st = sc.collect()
        assert st.n_launches == 1 and st.primary_rays == 4 * 6 * 40 * 3
        for k in range(4):
            assert host(t[k]["albedo"]).tobytes() == ref[k]["albedo"].tobytes()
            assert host(t[k]["hits"]).tobytes() == ref[k]["hits"].tobytes()
            for name in ("normal", "depth", "index"):
                assert torch.all(t[k][name] == -7).item(), name
print("DEVICE OK")
"""


def test_device_form_equals_host_form(ndev):
    """rt_scene_render_aovs_device on torch tensors, in passes, 4 and 66 strips (one launch per 64), a subset of the planes (in a
    child process that imports torch first: one HIP runtime for both)."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _DEVICE_CHILD], capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=300)
    assert r.returncode == 0 and "DEVICE OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_argument_errors_launch_nothing(ndev):
    lib = _abi.load()
    hs, w = 8, 24
    alb = np.full((hs, w, 3), -7.0, np.float32)
    hit = np.full((hs, w), 7, np.uint32)
    good = _abi.AovPlanes(alb.ctypes.data, None, None, hit.ctypes.data, None)
    empty = _abi.AovPlanes(None, None, None, None, None)

    def rq(**kw):
        return C.byref(_strip_request(**kw))

    def rqs(*kws):
        return (_abi.TileRequest * len(kws))(*[_strip_request(**k) for k in kws])

    BAD, LIMIT = _abi.RT_ERR_BAD_ARG, _abi.RT_ERR_LIMIT
    with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
        sc.collect()
        h = sc._h
        g = C.byref(good)
        assert lib.rt_scene_render_aov(None, rq(), 0, 3, g, None) == BAD
        assert lib.rt_scene_render_aov(h, None, 0, 3, g, None) == BAD
        assert lib.rt_scene_render_aov(h, rq(), 0, 3, None, None) == BAD
        assert lib.rt_scene_render_aov(h, rq(), 0, 3, C.byref(empty), None) == BAD
        assert lib.rt_scene_render_aov(h, rq(), 2, 2, g, None) == BAD
        assert lib.rt_scene_render_aov(h, rq(), 3, 1, g, None) == BAD
        assert lib.rt_scene_render_aov(h, rq(), 0, 4, g, None) == BAD                 # sample_end > spp
        assert lib.rt_scene_render_aov(h, rq(division_no=2), 0, 3, g, None) == BAD
        assert lib.rt_scene_render_aov(h, rq(width=0), 0, 3, g, None) == BAD
        assert lib.rt_scene_render_aov(h, rq(spp=0), 0, 1, g, None) == BAD
        assert lib.rt_scene_render_aov(h, rq(spp=4097), 0, 3, g, None) == LIMIT
        assert lib.rt_scene_render_aov(h, rq(max_bounces=63), 0, 3, g, None) == LIMIT
        two = (_abi.AovPlanes * 2)(good, good)
        mixed = (_abi.AovPlanes * 2)(good, _abi.AovPlanes(alb.ctypes.data, None, None, None, None))
        assert lib.rt_scene_render_aovs_device(None, rqs({}, {}), 2, 0, 3, two, None) == BAD
        assert lib.rt_scene_render_aovs_device(h, rqs({}, {}), 0, 0, 3, two, None) == BAD
        assert lib.rt_scene_render_aovs_device(h, rqs({}, {}), 2, 0, 3, None, None) == BAD
        assert lib.rt_scene_render_aovs_device(h, rqs({}, {}), 2, 0, 3, mixed, None) == BAD
        assert lib.rt_scene_render_aovs_device(h, rqs({}, {"width": 32}), 2, 0, 3, two, None) == BAD     # frame fields differ
        assert lib.rt_scene_render_aovs_device(h, rqs({}, {"flags": F.RT_FLAG_NO_BVH_CULL}), 2, 0, 3, two, None) == BAD
        assert lib.rt_scene_render_aovs_device(h, rqs({}, {}), 2, 1, 1, two, None) == BAD
        assert lib.rt_scene_render_aovs_device(h, rqs({}, {}), 2, 0, 9, two, None) == BAD
        assert lib.rt_scene_render_aovs_device(h, rqs({"spp": 5000}, {"spp": 5000}), 2, 0, 3, two, None) == LIMIT
        st = sc.collect()
        assert st.n_launches == 0 and st.primary_rays == 0 and st.ray_segments == 0
        assert np.all(alb == -7.0) and np.all(hit == 7)
        # the limits themselves are legal
        planes, st = sc.render_aov(_strip_request(spp=4096, width=2, height=2, divisions=1, division_no=0), 4095, 4096,
                                   out={"albedo": np.zeros((2, 2, 3), np.float32)}, planes=("albedo",))
        assert st.n_launches == 1 and st.primary_rays == 4
        with pytest.raises(ValueError):
            sc.render_aov(_strip_request(), 1, 3)                                      # a continuation needs the sums
        with pytest.raises(ValueError):
            sc.render_aov(_strip_request(), planes=("colour",))


def test_full_size_strip_spot_checked_against_the_oracle(ndev, oracle):
    sph, rq = scenes.config("c3")
    rq.width, rq.height, rq.divisions, rq.division_no, rq.spp = 1920, 1080, 20, 7, 8
    hs = rq.height // rq.divisions
    with rt.Scene(0, rt.World(sph)) as sc:
        planes, st = sc.render_aov(rq)
    assert st.engine == WALK and st.primary_rays == hs * rq.width * rq.spp and st.n_launches == 1
    g = np.random.default_rng(0xA0F)
    pick = g.choice(hs * rq.width, 2000, replace=False)
    pixels = [(int(p) // rq.width, int(p) % rq.width) for p in pick]
    want = _expected(oracle, sph, None, rq, 1, pixels)
    ys, xs = np.array([p[0] for p in pixels]), np.array([p[1] for p in pixels])
    got = {k: v[ys, xs] for k, v in planes.items()}
    _assert_planes_equal(got, want, "c3 full-size strip")
    assert 0 < np.mean(want["hits"] > 0) < 1


@pytest.mark.parametrize("scene", ["terrain", "tie_world"])
def test_sky_pixels_align_with_the_beauty_accum(ndev, scene):
    """No oracle: after [0, S), a pixel with hits == 0 missed on every sample, so the beauty image's running sum is the in-order
    sum of the same sky colours as the albedo plane — equal bit for bit only if both come from the same rays and streams."""
    sph, tri = _scene_world(scene)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for flags in (0, F.RT_FLAG_NO_BVH_CULL, F.RT_FLAG_EXACT_SCAN):
            rq = _abi.default_request(width=64, height=32, divisions=2, division_no=1, spp=5, max_bounces=6, seed=0xB1EA, flags=flags)
            _, _, accum, _ = sc.render_tile_pass(rq, 0, rq.spp)
            planes, _ = sc.render_aov(rq, planes=("albedo", "hits"))
            sky = planes["hits"] == 0
            assert sky.sum() >= 16 and (~sky).sum() >= 16, (scene, flags, int(sky.sum()))
            assert np.array_equal(_bits(accum[sky]), _bits(planes["albedo"][sky])), (scene, flags)


def test_staging_buffers_of_other_entry_points_leave_the_planes_alone(ndev):
    """One scene, the host forms of every entry point that stages through a scene buffer, each grown between two AOV calls: the
    planes, the traced colours and the hits come out the same bit for bit (the AOV, trace and query forms carve the scene's one
    staging buffer anew on every call and leave nothing in flight behind them; the tile pass has buffers of its own)."""
    sph, tri = _scene_world("quad_room")
    g = np.random.default_rng(0x57A6)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        small = _strip_request(spp=4)
        big = _abi.default_request(width=160, height=96, divisions=2, division_no=0, spp=2, seed=0x5B16)
        n0 = 512
        o = g.uniform(-2, 2, size=(60000, 3)).astype(np.float32)
        d = g.normal(size=(60000, 3)).astype(np.float32)
        first, _ = sc.render_aov(small)
        rgb0, segs0, _ = sc.trace(o[:n0], d[:n0], spp=2, max_bounces=4, seed=3)
        hits0, _ = sc.intersect(o[:n0], d[:n0])
        again, _ = sc.render_aov(small)
        _assert_planes_equal(again, first, "aov after the first trace and query")
        sc.trace(o, d, spp=1, max_bounces=2, seed=4)                      # trace buffer grows
        after_trace, _ = sc.render_aov(small)
        _assert_planes_equal(after_trace, first, "aov after a larger trace")
        sc.intersect(o, d)                                                # query buffers grow
        sc.render_tile_pass(big, 0, big.spp)                              # progressive sums and strips grow
        after_all, _ = sc.render_aov(small)
        _assert_planes_equal(after_all, first, "aov after larger query and tile calls")
        big_planes, _ = sc.render_aov(big)                                # the AOV buffer grows
        assert big_planes["albedo"].shape == (48, 160, 3)
        rgb1, segs1, _ = sc.trace(o[:n0], d[:n0], spp=2, max_bounces=4, seed=3)
        hits1, _ = sc.intersect(o[:n0], d[:n0])
        assert rgb1.tobytes() == rgb0.tobytes() and np.array_equal(segs1, segs0)
        assert hits1.tobytes() == hits0.tobytes()
        _assert_planes_equal(sc.render_aov(small)[0], first, "aov after its own buffer grew")
        sc.trace(o, d, spp=1, max_bounces=2, seed=4)
        _assert_planes_equal(sc.render_aov(big)[0], big_planes, "large aov after another trace")


def _result_arrays(out):
    """The arrays of a host-form call's result (tuples, lists and dicts of them), the stats left out, as bytes."""
    if isinstance(out, np.ndarray):
        return [np.ascontiguousarray(out).tobytes()]
    if isinstance(out, dict):
        out = list(out.values())
    if isinstance(out, (tuple, list)):
        return [b for v in out for b in _result_arrays(v)]
    return []


def test_interleaved_strip_host_forms_share_one_staging_buffer(ndev):
    """The host forms of the feature buffers, the camera rays and the denoiser stage their arrays in the buffer the caller-ray calls
    use, carved anew by every call.  Calls of all these kinds and a tile pass interleaved on one scene, with staged sizes that grow
    and shrink, planes and outputs that come and go, and uploads that depend on the sample range, each give the bytes of the same
    call on a fresh scene of the same world: no stale offset, no missed upload, no wrong copy direction, nothing left over."""
    sph, tri = _scene_world("quad_room")
    g = np.random.default_rng(0x57A7)
    o = g.uniform(-2, 2, size=(1000, 3)).astype(np.float32)
    d = g.normal(size=(1000, 3)).astype(np.float32)
    small = _abi.default_request(width=64, height=48, divisions=2, division_no=1, spp=4, max_bounces=6, seed=0x5A11)
    big = _abi.default_request(width=160, height=96, divisions=2, division_no=0, spp=2, max_bounces=6, seed=0x5B16)
    strips = [_abi.default_request(width=64, height=48, divisions=4, division_no=k, spp=4, max_bounces=6, seed=0xD0 + k) for k in (1, 2, 3)]
    # the inputs of the calls that continue or filter something, made once on a scene of their own
    with rt.Scene(0, rt.World(sph, tri)) as prep:
        half, _ = prep.render_aov(small, 0, 2)
        acc = [prep.render_tile_pass(rq, 0, rq.spp)[2] for rq in strips]
        guides = [prep.render_aov(rq)[0] for rq in strips]
    two = _abi.DenoiseRequest.defaults(iterations=2)
    none = _abi.DenoiseRequest.defaults(iterations=0)
    all_out = ("rgb", "linear", "f32")
    calls = [
        ("aov small [0, 2)", lambda sc: sc.render_aov(small, 0, 2)),
        ("aov small [2, 4) on those planes", lambda sc: sc.render_aov(small, 2, 4, out={k: v.copy() for k, v in half.items()})),
        ("intersect 1000", lambda sc: sc.intersect(o, d)),
        ("aov small, depth and hits", lambda sc: sc.render_aov(small, planes=("depth", "hits"))),
        ("aov big", lambda sc: sc.render_aov(big)),
        ("trace 257", lambda sc: sc.trace(o[:257], d[:257], spp=2, max_bounces=3, seed=3)),
        ("camera rays [1, 3), no states", lambda sc: sc.camera_rays(small, 1, 3, want_states=False)),
        ("denoise 1 strip, all guides, all outputs, 2 iterations", lambda sc: sc.denoise(strips[0], acc[0], guides[0], 4, 4, two, all_out)),
        ("tile pass", lambda sc: sc.render_tile_pass(big, 0, big.spp)),
        ("camera rays [1, 4), states", lambda sc: sc.camera_rays(small, 1, 4)),
        ("denoise 3 strips, no guide, linear, 0 iterations", lambda sc: sc.denoise(strips, acc, [{}] * 3, 4, 4, none, ("linear",))),
        ("intersect 63", lambda sc: sc.intersect(o[:63], d[:63])),
        ("denoise 3 strips, all guides, all outputs, 2 iterations", lambda sc: sc.denoise(strips, acc, guides, 4, 4, two, all_out)),
        ("denoise 1 strip, no guide, linear, 2 iterations", lambda sc: sc.denoise(strips[2], acc[2], {}, 4, 4, two, ("linear",))),
        ("aov small [0, 2) again", lambda sc: sc.render_aov(small, 0, 2)),
    ]
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        results = [call(sc) for _, call in calls]
    shared = [_result_arrays(r) for r in results]
    assert all(len(a) >= 1 for a in shared), [len(a) for a in shared]
    assert [len(a) for a in shared] == [5, 5, 1, 2, 5, 2, 1, 3, 2, 2, 3, 1, 9, 1, 5]
    assert shared[0] == _result_arrays(half) and shared[-1] == shared[0]
    assert shared[1] != shared[0]                                          # the second half added to the first
    # the filter did something: after 2 iterations the linear colour is not the mean it was given
    for k, which in ((7, [0]), (12, [0, 1, 2]), (13, [2])):
        outs = results[k][0] if isinstance(results[k][0], list) else [results[k][0]]
        for out, i in zip(outs, which):
            assert np.abs(out["linear"] - acc[i] / np.float32(4)).max() > 1e-3, calls[k][0]
    for (what, call), got in zip(calls, shared):
        with rt.Scene(0, rt.World(sph, tri)) as fresh:
            assert got == _result_arrays(call(fresh)), what
