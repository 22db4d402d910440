"""Path tracing of caller rays on the GPU (rt_scene_trace, rt_scene_trace_device), bit for bit throughout:
1. against the CPU oracle's ray_color (oracle.ray_color: plain-scan semantics) under RT_FLAG_NO_BVH_CULL, ray by ray: the colour
   sum, the segments and the written-back RNG state, for random, camera and adversarial rays, several bounce limits and spp;
2. composed with the tile renderer, for BVH semantics (no per-ray oracle exists): the camera rays of a strip traced
   RT_TRACE_RAY_AS_GIVEN from the tile's own RNG states, summed per pixel in sample order, are the strip's progressive `accum`;
3. the seeded streams and the chained state form against single-sample calls;
4. the device form on torch tensors, two streams in flight, collect() counters;
5. argument errors and limits, with nothing launched;
6. the plain-C client examples/trace_rays.c."""
import ctypes as C
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

from test_gpu_query import SCENES, _adversarial_rays, _camera_rays, _rays, _world

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
F = _abi
WALK, SCAN = 2, 1
M64 = (1 << 64) - 1


def _od(rays):
    return np.stack([rays["ox"], rays["oy"], rays["oz"]], 1), np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)


def _random_rays(sph, tri, n, seed):
    g = np.random.default_rng(seed)
    pts = []
    if len(sph):
        pts.append(np.stack([sph["cx"], sph["cy"], sph["cz"]], 1))
    if tri is not None and len(tri):
        pts.append(np.asarray(tri["a"], np.float32))
    p = np.concatenate(pts)
    lo, hi = p.min(0) - 2, p.max(0) + 2
    o = g.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = g.normal(size=(n, 3)).astype(np.float32)
    return _rays(o, d)


def _states(n, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)


def _same_bits(a, b):
    """Equal bit for bit, NaN matching NaN."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _oracle_trace(oracle, sph, tri, rays, spp, max_bounces, states=None, seed=None):
    """rgb sums, segments and final states of the oracle's ray_color, sample after sample, per ray."""
    n = len(rays)
    rgb = np.zeros((n, 3), np.float32)
    segs = np.zeros(n, np.uint64)
    out_states = np.zeros((n, 4), np.uint64)
    t = tri if tri is not None and len(tri) else None
    for i, r in enumerate(rays):
        st = None if states is None else states[i].copy()
        acc = np.zeros(3, np.float32)
        for s in range(spp):
            if states is None:
                st = oracle.seed_from_u64(oracle.sample_seed(seed, i, spp, s))
            c, k = oracle.ray_color(sph, t, (r["ox"], r["oy"], r["oz"]), (r["dx"], r["dy"], r["dz"]), max_bounces + 1, st,
                                    float(r["t_min"]), float(r["t_max"]))
            acc = (acc + np.asarray(c, np.float32)).astype(np.float32)
            segs[i] += k
        rgb[i] = acc
        out_states[i] = st
    return rgb, segs, out_states


@pytest.fixture(scope="module")
def ray_sets(oracle):
    out = {}
    for name in SCENES:
        sph, tri = _world(name)
        cam = _camera_rays(oracle, 8, 5)
        rnd = _random_rays(sph, tri, 40, seed=len(name))
        adv = _adversarial_rays(sph, tri if tri is not None else np.zeros(0, _abi.TRIANGLE_DTYPE))
        out[name] = (sph, tri, np.concatenate([cam, rnd, adv]))
    return out


# (max_bounces, spp) pairs: every bounce limit with one spp and 0 / 10 with the other
SETTINGS = [(0, 3), (1, 1), (10, 3), (10, 1), (62, 1)]


@pytest.mark.parametrize("scene", SCENES)
def test_rays_match_the_oracle_ray_color(ndev, oracle, ray_sets, scene):
    sph, tri, rays = ray_sets[scene]
    o, d = _od(rays)
    n_prims = len(sph) + (0 if tri is None else len(tri))
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for mb, spp in SETTINGS:
            st0 = _states(len(rays), mb * 7 + spp)
            rgb, segs, stats, st1 = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=spp, max_bounces=mb, rng_state=st0,
                                             flags=F.RT_FLAG_NO_BVH_CULL)
            ergb, esegs, est = _oracle_trace(oracle, sph, tri, rays, spp, mb, states=st0)
            bad = [i for i in range(len(rays)) if not _same_bits(rgb[i], ergb[i])]
            assert not bad, (scene, mb, spp, bad[:5], rgb[bad[:3]], ergb[bad[:3]], rays[bad[:3]])
            assert np.array_equal(segs, esegs), (scene, mb, spp, np.nonzero(segs != esegs)[0][:5])
            assert np.array_equal(st1, est), (scene, mb, spp)
            assert stats.engine == SCAN and stats.n_launches == 1
            assert stats.primary_rays == len(rays) * spp and stats.ray_segments == int(esegs.sum())
            assert stats.broad_candidates == stats.ray_segments * n_prims          # the scan tests every primitive per segment
            if mb == 10 and spp == 3:                                              # the seeded streams
                seed = 0xDEADBEEF12345678 + len(scene)
                rgb, segs, _ = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=spp, max_bounces=mb, seed=seed,
                                        flags=F.RT_FLAG_NO_BVH_CULL)
                ergb, esegs, _ = _oracle_trace(oracle, sph, tri, rays, spp, mb, seed=seed)
                assert _same_bits(rgb, ergb) and np.array_equal(segs, esegs), scene
        assert np.any(esegs > 1)                                                   # some paths bounce


def _strip_request(flags, seed=0x7AC3):
    return _abi.default_request(width=24, height=16, divisions=2, division_no=1, spp=3, max_bounces=10, seed=seed, flags=flags)


def _strip_rays(oracle, rq):
    """The tile's camera rays of every (pixel, sample) of the strip and the RNG state after Camera::get_ray, pixel-major."""
    hs = rq.height // rq.divisions
    o, d, st = [], [], []
    for yl in range(hs):
        yg = hs * rq.division_no + yl
        for x in range(rq.width):
            for s in range(rq.spp):
                state = oracle.seed_from_u64(oracle.sample_seed(rq.seed, yg * rq.width + x, rq.spp, s))
                a, b = oracle.camera_ray(rq, x, rq.height - 1 - yg, state)
                o.append(a)
                d.append(b)
                st.append(state)
    return np.array(o, np.float32), np.array(d, np.float32), np.array(st, np.uint64)


COMPOSE = {
    "default": (0, 0, WALK),
    "full_chain": (F.RT_FLAG_FULL_CHAIN, 0, WALK),
    "exact_scan": (F.RT_FLAG_EXACT_SCAN, 0, SCAN),
    "linear_scan": (F.RT_FLAG_LINEAR_SCAN, 0, SCAN),
    "no_bvh_cull": (F.RT_FLAG_NO_BVH_CULL, F.RT_FLAG_NO_BVH_CULL, SCAN),
}


@pytest.mark.parametrize("scene", SCENES)
def test_camera_rays_as_given_compose_to_the_tile_accum(ndev, oracle, scene):
    sph, tri = _world(scene)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for cfg, (trace_flags, tile_flags, engine) in COMPOSE.items():
            rq = _strip_request(tile_flags)
            hs, S = rq.height // rq.divisions, rq.spp
            _, _, accum, tst = sc.render_tile_pass(rq, 0, S)
            o, d, st0 = _strip_rays(oracle, rq)
            rgb, segs, stats, _ = sc.trace(o, d, rq.t_min, rq.t_max, spp=1, max_bounces=rq.max_bounces, rng_state=st0,
                                           as_given=True, flags=trace_flags)
            assert stats.engine == engine, (cfg, stats.engine)
            per = rgb.reshape(hs, rq.width, S, 3)
            total = np.zeros((hs, rq.width, 3), np.float32)
            for s in range(S):
                total = (total + per[:, :, s, :]).astype(np.float32)
            assert _same_bits(total, accum), (scene, cfg, np.argwhere(total.view(np.uint32) != accum.view(np.uint32))[:5])
            assert int(segs.sum()) == tst.ray_segments, (scene, cfg, int(segs.sum()), tst.ray_segments)


def test_seeded_streams_and_chained_states(ndev, ray_sets):
    sph, tri, rays = ray_sets["cornell16"]
    o, d = _od(rays)
    n, k, seed = len(rays), 4, 0x51EED
    from oracle import oracle as orc
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for flags in (0, F.RT_FLAG_NO_BVH_CULL):
            rgb, segs, st = sc.trace(o, d, spp=k, max_bounces=10, seed=seed, flags=flags)
            # k * n single-sample rays with the seeded streams' states, summed in sample order
            states = np.array([orc.seed_from_u64(orc.sample_seed(seed, i, k, s)) for i in range(n) for s in range(k)], np.uint64)
            rgb1, segs1, _, _ = sc.trace(np.repeat(o, k, 0), np.repeat(d, k, 0), spp=1, max_bounces=10, rng_state=states, flags=flags)
            tot = np.zeros((n, 3), np.float32)
            per = rgb1.reshape(n, k, 3)
            for s in range(k):
                tot = (tot + per[:, s]).astype(np.float32)
            assert _same_bits(rgb, tot) and np.array_equal(segs, segs1.reshape(n, k).sum(1)), flags
            assert st.primary_rays == n * k and st.ray_segments == int(segs.sum())
            # chained: spp = k from one state equals k calls of spp = 1 passing the state along
            s0 = _states(n, 99)
            rgb_k, segs_k, _, s_k = sc.trace(o, d, spp=k, max_bounces=10, rng_state=s0, flags=flags)
            s = s0.copy()
            tot = np.zeros((n, 3), np.float32)
            seg_tot = np.zeros(n, np.uint64)
            for _ in range(k):
                c, g, _, s = sc.trace(o, d, spp=1, max_bounces=10, rng_state=s, flags=flags)
                tot = (tot + c).astype(np.float32)
                seg_tot += g
            assert _same_bits(rgb_k, tot) and np.array_equal(segs_k, seg_tot) and np.array_equal(s_k, s), flags
            assert not np.array_equal(s_k, s0)


def test_argument_errors_launch_nothing(ndev):
    lib = _abi.load()
    rays = _rays([(0, 0, 0)] * 4, [(0, 0, -1)] * 4)
    rgb = np.full(12, -7.0, np.float32)
    rp = rays.ctypes.data_as(C.POINTER(_abi.Ray))
    fp = rgb.ctypes.data_as(C.POINTER(C.c_float))

    def rq(**kw):
        r = _abi.TraceRequest(1, 10, 0, 0, 0)
        for k_, v in kw.items():
            setattr(r, k_, v)
        return C.byref(r)

    from ray_tracer_s8_amd import scenes
    with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
        sc.collect()
        h = sc._h
        assert lib.rt_scene_trace(h, rq(), rp, 0, None, fp, None, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_trace(h, rq(spp=0), rp, 4, None, fp, None, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_trace(h, rq(ray_form=2), rp, 4, None, fp, None, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_trace(h, None, rp, 4, None, fp, None, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_trace(h, rq(), None, 4, None, fp, None, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_trace(h, rq(), rp, 4, None, None, None, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_trace(h, rq(spp=4097), rp, 4, None, fp, None, None) == _abi.RT_ERR_LIMIT
        assert lib.rt_scene_trace(h, rq(max_bounces=63), rp, 4, None, fp, None, None) == _abi.RT_ERR_LIMIT
        vr, vf = C.c_void_p(rays.ctypes.data), C.c_void_p(rgb.ctypes.data)
        assert lib.rt_scene_trace_device(h, rq(), vr, 0, None, vf, None, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_trace_device(h, rq(ray_form=5), vr, 4, None, vf, None, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_trace_device(h, rq(), None, 4, None, vf, None, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_trace_device(h, rq(), vr, 4, None, None, None, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_trace_device(h, rq(spp=5000), vr, 4, None, vf, None, None) == _abi.RT_ERR_LIMIT
        assert lib.rt_scene_trace_device(h, rq(max_bounces=100), vr, 4, None, vf, None, None) == _abi.RT_ERR_LIMIT
        st = sc.collect()
        assert st.n_launches == 0 and st.primary_rays == 0 and st.ray_segments == 0
        assert np.all(rgb == -7.0)
        # the limits themselves are legal
        out, segs, st = sc.trace(np.zeros((2, 3)), [(0, 0, -1), (0.3, 0.1, -1)], spp=1, max_bounces=62)
        assert st.n_launches == 1 and st.primary_rays == 2 and np.all(segs >= 1)
        out, segs, st = sc.trace(np.zeros((1, 3)), [(0, 0, -1)], spp=4096, max_bounces=0)
        assert st.primary_rays == 4096 and segs[0] == 4096
        with pytest.raises(ValueError):
            sc.trace(np.zeros((3, 3)), np.zeros((4, 3)))
        with pytest.raises(ValueError):
            sc.trace(np.zeros((3, 3)), np.zeros((3, 3)), rng_state=np.zeros((2, 4), np.uint64))


_DEVICE_CHILD = r"""
import numpy as np
import torch                                                      # first: the library then binds to torch's HIP runtime
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes
rt.init()
g = np.random.default_rng(12)
n = 40001
o = g.uniform((-20, -1, -40), (20, 8, 0), size=(n, 3)).astype(np.float32)
d = g.normal(size=(n, 3)).astype(np.float32)
rays = np.empty(n, _abi.RAY_DTYPE)
rays["ox"], rays["oy"], rays["oz"] = o.T
rays["dx"], rays["dy"], rays["dz"] = d.T
rays["t_min"], rays["t_max"] = 0.001, 1000.0
s0 = g.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64)
dev = torch.device("cuda", 0)
d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).to(dev)
with rt.Scene(0, rt.World(scenes.rand1024())) as sc:
    for flags in (0, _abi.RT_FLAG_NO_BVH_CULL):
        ref_rgb, ref_segs, _ = sc.trace(o, d, spp=3, max_bounces=6, seed=5, flags=flags)
        ref_rgb_s, ref_segs_s, _, ref_state = sc.trace(o, d, spp=2, max_bounces=6, rng_state=s0, flags=flags)
        # two streams in flight at once: the seeded form on one, the state form on the other
        s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        rgb1 = torch.empty((n, 3), dtype=torch.float32, device=dev)
        rgb2 = torch.empty((n, 3), dtype=torch.float32, device=dev)
        seg1 = torch.empty(n, dtype=torch.int32, device=dev)
        st2 = torch.from_numpy(s0.view(np.int64).copy()).to(dev)
        rgb3 = torch.empty((n, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        sc.trace_device(d_rays.data_ptr(), n, rgb1.data_ptr(), d_segments=seg1.data_ptr(), spp=3, max_bounces=6, seed=5,
                        flags=flags, stream=s1.cuda_stream)
        sc.trace_device(d_rays.data_ptr(), n, rgb2.data_ptr(), d_rng_state=st2.data_ptr(), spp=2, max_bounces=6, flags=flags,
                        stream=s2.cuda_stream)
        sc.trace_device(d_rays.data_ptr(), n, rgb3.data_ptr(), spp=3, max_bounces=6, seed=5, flags=flags, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        st = sc.collect()
        assert st.n_launches == 3 and st.primary_rays == 8 * n, (st.n_launches, st.primary_rays)
        assert st.ray_segments == 2 * int(ref_segs.sum()) + int(ref_segs_s.sum()), st.ray_segments
        assert st.engine == (1 if flags else 2) and st.kernel_ms > 0 and st.broad_candidates > 0, st.engine
        assert rgb1.cpu().numpy().tobytes() == ref_rgb.tobytes()
        assert rgb3.cpu().numpy().tobytes() == ref_rgb.tobytes()
        assert seg1.cpu().numpy().view(np.uint32).tobytes() == ref_segs.tobytes()
        assert rgb2.cpu().numpy().tobytes() == ref_rgb_s.tobytes()
        assert st2.cpu().numpy().view(np.uint64).tobytes() == ref_state.tobytes()
print("DEVICE OK")
"""


def test_device_form_equals_host_form(ndev):
    """rt_scene_trace_device on torch tensors, on two streams at once, counters through rt_scene_collect (in a child process that
    imports torch first: one HIP runtime for both)."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _DEVICE_CHILD], capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=300)
    assert r.returncode == 0 and "DEVICE OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_plain_c_trace_client(ndev, tmp_path):
    """examples/trace_rays.c through the C-ABI only (no Python binding in the loop)."""
    exe = tmp_path / "trace_rays"
    lib = _abi.lib_path().parent
    r = subprocess.run([shutil.which("gcc"), "-std=c99", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "trace_rays.c"),
                        f"-L{lib}", "-lrt_s8", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "TRACE_OK" in run.stdout, run.stdout + run.stderr
