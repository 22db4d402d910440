"""Ray queries on the GPU (rt_scene_intersect, rt_scene_intersect_device) against the CPU oracle's WorldRefList::intersect
(oracle.intersect: backend 1 = BVH semantics, 0 = plain scan), ray by ray and bit for bit: index, hit point and normal, and the
distance against a float32 restatement of length(P - o).  Every engine the query path has is forced by flags, the default
included; camera rays, bounce rays and adversarial rays (origins on and inside spheres, tangent rays, axis-aligned directions
with +-0 components, shared triangle edges, empty windows, infinite t_max, zero and NaN directions)."""
import ctypes as C
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes

from _world_cases import interleave, tie_world

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NONE = _abi.RT_HIT_NONE
WALK, SCAN = 2, 1
F = _abi
# flags -> (engine that must run, oracle backend)
CONFIGS = {
    "default": (0, WALK, 1),
    "bvh_traverse": (F.RT_FLAG_BVH_TRAVERSE | F.RT_FLAG_NO_LDS_TREE, WALK, 1),
    "full_chain": (F.RT_FLAG_FULL_CHAIN, WALK, 1),
    "exact_scan": (F.RT_FLAG_EXACT_SCAN, SCAN, 1),
    "linear_scan": (F.RT_FLAG_LINEAR_SCAN | F.RT_FLAG_FULL_CHAIN, SCAN, 1),
    "no_bvh_cull": (F.RT_FLAG_NO_BVH_CULL, SCAN, 0),
    "ignored_flags": (F.RT_FLAG_QUANT_NODES | F.RT_FLAG_CULL_WALK | F.RT_FLAG_COUNT_STEPS | F.RT_FLAG_FRAME_QUEUE, WALK, 1),
}


def _world(name):
    if name == "single_sphere":
        return scenes.single_sphere(), None
    if name == "cornell16":
        return scenes.cornell16(), None
    if name == "rand1024":
        return scenes.rand1024(), None
    if name == "field9000":
        return scenes.rand65536(n=9000), None
    if name == "quad_room":
        return scenes.quad_room()
    if name == "terrain":
        return scenes.tri_terrain()
    if name == "tie_world":
        return tie_world()
    raise KeyError(name)


SCENES = ["single_sphere", "cornell16", "rand1024", "field9000", "quad_room", "terrain", "tie_world"]


def _rays(o, d, t_min=0.001, t_max=1000.0):
    o = np.asarray(o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    r = np.empty(len(o), _abi.RAY_DTYPE)
    r["ox"], r["oy"], r["oz"] = o.T
    r["dx"], r["dy"], r["dz"] = d.T
    r["t_min"] = np.broadcast_to(np.asarray(t_min, np.float32), (len(o),))
    r["t_max"] = np.broadcast_to(np.asarray(t_max, np.float32), (len(o),))
    return r


def _camera_rays(oracle, w, h, seed=0x51CE):
    rq = _abi.default_request(width=w, height=h, divisions=1, spp=1, seed=seed)
    o, d = [], []
    for y in range(h):
        for x in range(w):
            st = oracle.seed_from_u64(oracle.sample_seed(seed, y * w + x, 1, 0))
            a, b = oracle.camera_ray(rq, x, h - 1 - y, st)
            o.append(a)
            d.append(b)
    return _rays(o, d)


def _oracle_hits(oracle, sph, tri, rays, backend):
    out = []
    for r in rays:
        out.append(oracle.intersect(sph, tri if tri is not None and len(tri) else None, (r["ox"], r["oy"], r["oz"]),
                                    (r["dx"], r["dy"], r["dz"]), float(r["t_min"]), float(r["t_max"]), backend=backend))
    return out


def _bounce_rays(ref, rays, seed):
    """From the hit points of `rays` (oracle results), seeded random directions, the reference's t_min."""
    g = np.random.default_rng(seed)
    pts = [h["point"] for h in ref if h is not None]
    if not pts:
        return _rays(np.zeros((0, 3)), np.zeros((0, 3)))
    d = g.normal(size=(len(pts), 3)).astype(np.float32)
    return _rays(np.array(pts), d)


def _adversarial_rays(sph, tri):
    o, d, tmin, tmax = [], [], [], []

    def add(a, b, t0=0.001, t1=1000.0):
        o.append(a)
        d.append(b)
        tmin.append(t0)
        tmax.append(t1)

    for s in sph[:12]:
        c, r = np.array([s["cx"], s["cy"], s["cz"]], np.float32), np.float32(s["radius"])
        add(c, (0.3, -0.2, 1.0))                                             # from the centre (inside)
        add(c + np.array([r, 0, 0], np.float32), (1.0, 0.0, 0.0))            # on the surface, outwards
        add(c + np.array([r, 0, 0], np.float32), (-1.0, 0.0, 0.0))           # on the surface, inwards
        add(c + np.array([0, r, 5 * r + 1], np.float32), (0.0, 0.0, -1.0))   # tangent, axis-aligned
        add(c + np.array([0, 0, 4 * r + 1], np.float32), (-0.0, 0.0, -1.0))  # straight at the centre, a -0 component
        add(c + np.array([0, 0, 4 * r + 1], np.float32), (0.0, -0.0, -1.0), 0.001, np.inf)
    for t in tri[:12]:
        a, b, c = (np.asarray(t[k], np.float32) for k in ("a", "b", "c"))
        for p in ((a + b) / 2, (b + c) / 2, (a + c) / 2, a):                # shared edges and a vertex
            add(p + np.array([0.05, 2.0, 0.1], np.float32), p - (p + np.array([0.05, 2.0, 0.1], np.float32)))
        n = np.cross(b - a, c - a)
        add((a + b + c) / 3 + n, -n)                                         # head-on, and grazing along the face
        add((a + b + c) / 3 - (b - a), b - a)
    add((0, 0, 0), (0, 0, -1))
    add((0, 0, 0), (0, 0, -1), 5.0, 5.0)                                     # t_min == t_max: nothing admitted
    add((0, 0, 0), (0, 0, -1), 10.0, 1.0)                                    # t_min > t_max
    add((0, 0, 0), (0.1, -0.2, -1), 0.001, np.inf)
    add((0, 0, 0), (0, 0, 0))                                                # zero direction: NaN after Ray::new
    add((0, 0, 0), (np.nan, 0, -1))
    add((np.nan, 0, 0), (0, 0, -1))
    add((0, 0, 0), (-0.0, -0.0, -1.0))
    add((0, 0, 0), (1.0, 0.0, 0.0))
    return _rays(o, d, tmin, tmax)


def _same(a, b):
    a, b = np.float32(a), np.float32(b)
    return a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b))


def _check_closest(hits, rays, ref, what):
    assert len(hits) == len(ref)
    for i, (h, e) in enumerate(zip(hits, ref)):
        if e is None:
            assert h["index"] == NONE, (what, i, rays[i], h)
            assert np.isinf(h["distance"]) and h["distance"] > 0 and all(h[k] == 0 for k in ("px", "py", "pz", "nx", "ny", "nz")), (what, i)
            continue
        assert h["index"] == e["index"], (what, i, rays[i], h, e)
        for k, j in (("px", 0), ("py", 1), ("pz", 2)):
            assert _same(h[k], e["point"][j]), (what, i, k, h, e)
        for k, j in (("nx", 0), ("ny", 1), ("nz", 2)):
            assert _same(h[k], e["normal"][j]), (what, i, k, h, e)
        x = np.float32(h["px"]) - np.float32(rays[i]["ox"])
        y = np.float32(h["py"]) - np.float32(rays[i]["oy"])
        z = np.float32(h["pz"]) - np.float32(rays[i]["oz"])
        dist = np.sqrt(np.float32(np.float32(x * x) + np.float32(y * y)) + np.float32(z * z))
        assert _same(h["distance"], dist), (what, i, h["distance"], dist)


def _check_any(hits, ref, what):
    got = hits["index"] != NONE
    want = np.array([e is not None for e in ref])
    assert np.array_equal(got, want), (what, np.nonzero(got != want)[0][:10])


@pytest.fixture(scope="module")
def ray_sets(oracle):
    """Per scene: the rays and the oracle's hits under both backends (the oracle rebuilds its BVH per call: computed once)."""
    out = {}
    for name in SCENES:
        sph, tri = _world(name)
        w, h = (16, 9) if name == "field9000" else (32, 18)
        cam = _camera_rays(oracle, w, h)
        cam_ref = _oracle_hits(oracle, sph, tri, cam, 1)
        bounce = _bounce_rays(cam_ref, cam, seed=len(name))
        adv = _adversarial_rays(sph, tri if tri is not None else np.zeros(0, _abi.TRIANGLE_DTYPE))
        rays = np.concatenate([cam, bounce, adv])
        out[name] = (sph, tri, rays, {1: cam_ref + _oracle_hits(oracle, sph, tri, np.concatenate([bounce, adv]), 1),
                                      0: _oracle_hits(oracle, sph, tri, rays, 0)})
    return out


@pytest.mark.parametrize("scene", SCENES)
def test_closest_and_any_hit_match_the_oracle_on_every_engine(ndev, ray_sets, scene):
    sph, tri, rays, ref = ray_sets[scene]
    n_prims = len(sph) + (0 if tri is None else len(tri))
    assert any(e is not None for e in ref[1]) and any(e is None for e in ref[1])
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for cfg, (flags, engine, backend) in CONFIGS.items():
            o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)
            d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)
            hits, st = sc.intersect(o, d, rays["t_min"], rays["t_max"], flags=flags)
            _check_closest(hits, rays, ref[backend], (scene, cfg))
            assert st.engine == engine and st.n_launches == 1, (cfg, st.engine, st.n_launches)
            assert st.primary_rays == st.ray_segments == len(rays)
            if engine == SCAN:
                assert st.broad_candidates == len(rays) * n_prims        # the scan tests every primitive
            else:
                assert 0 < st.broad_candidates < len(rays) * max(n_prims, 2)
            anyh, st_any = sc.intersect(o, d, rays["t_min"], rays["t_max"], any_hit=True, flags=flags)
            _check_any(anyh, ref[backend], (scene, cfg, "any"))
            assert st_any.engine == engine and st_any.broad_candidates <= st.broad_candidates
            hit = anyh["index"] != NONE
            assert np.all(anyh["index"][hit] < n_prims)


def test_batch_sizes_give_the_same_hits(ndev, ray_sets):
    sph, tri, rays, _ = ray_sets["rand1024"]
    lib = _abi.load()
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        full = np.empty(len(rays), _abi.HIT_DTYPE)
        assert lib.rt_scene_intersect(sc._h, rays.ctypes.data_as(C.POINTER(_abi.Ray)), len(rays), 0, 0,
                                      full.ctypes.data_as(C.POINTER(_abi.Hit)), None) == 0
        for n in (1, 63, 65):
            for start in (0, 7, len(rays) - n):
                part = np.empty(n, _abi.HIT_DTYPE)
                sub = np.ascontiguousarray(rays[start:start + n])
                assert lib.rt_scene_intersect(sc._h, sub.ctypes.data_as(C.POINTER(_abi.Ray)), n, 0, 0,
                                              part.ctypes.data_as(C.POINTER(_abi.Hit)), None) == 0
                assert part.tobytes() == full[start:start + n].tobytes(), (n, start)


def test_a_batch_of_4m_rays_equals_batches_of_4096(ndev, oracle):
    sph = scenes.rand1024()
    g = np.random.default_rng(0x4D)
    n = 1 << 22
    o = g.uniform((-20, -1, -40), (20, 8, 0), size=(n, 3)).astype(np.float32)
    d = g.normal(size=(n, 3)).astype(np.float32)
    rays = _rays(o, d)
    lib = _abi.load()
    with rt.Scene(0, rt.World(sph)) as sc:
        big, st = sc.intersect(o, d)
        assert st.primary_rays == n and st.n_launches == 1 and st.engine == WALK
        parts = np.empty(n, _abi.HIT_DTYPE)
        for i0 in range(0, n, 4096):
            sub = rays[i0:i0 + 4096]
            assert lib.rt_scene_intersect(sc._h, sub.ctypes.data_as(C.POINTER(_abi.Ray)), len(sub), 0, 0,
                                          parts[i0:].ctypes.data_as(C.POINTER(_abi.Hit)), None) == 0
    assert big.tobytes() == parts.tobytes()
    hit_frac = np.mean(big["index"] != NONE)
    assert 0.05 < hit_frac < 0.95, hit_frac
    pick = np.sort(g.choice(n, 1500, replace=False))
    _check_closest(big[pick], rays[pick], _oracle_hits(oracle, sph, None, rays[pick], 1), "4M sample")


@pytest.mark.parametrize("kind", ["spheres", "triangles"])
def test_world_index_positions(ndev, oracle, kind):
    """A permuted world: the index is the position in the world, and the hits are the oracle's on the reordered arrays."""
    if kind == "spheres":
        sph, tri = np.concatenate([scenes.cornell16(), tie_world(with_tris=False)[0]]), None
        n = len(sph)
    else:
        sph, tri = np.zeros(0, _abi.SPHERE_DTYPE), scenes.tri_terrain()[1]
        n = len(tri)
    perm = np.random.default_rng(5).permutation(n).astype(np.uint32)
    arr = sph if kind == "spheres" else tri
    reordered = np.empty_like(arr)
    reordered[perm] = arr
    rays = np.concatenate([_camera_rays(oracle, 24, 14), _adversarial_rays(sph, tri if tri is not None else np.zeros(0, _abi.TRIANGLE_DTYPE))])
    rs, rt_ = (reordered, None) if kind == "spheres" else (None, reordered)
    with rt.Scene(0, rt.World(sph, tri, world_index=perm)) as sc:
        o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)
        d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)
        for flags, backend in ((0, 1), (F.RT_FLAG_EXACT_SCAN, 1), (F.RT_FLAG_NO_BVH_CULL, 0)):
            hits, _ = sc.intersect(o, d, rays["t_min"], rays["t_max"], flags=flags)
            _check_closest(hits, rays, _oracle_hits(oracle, rs, rt_, rays, backend), (kind, flags))


def test_interleaved_world_returns_world_positions(ndev, oracle):
    sph, tri = tie_world()
    n = len(sph) + len(tri)
    wi = interleave(len(sph), len(tri), 9)
    rays = _camera_rays(oracle, 32, 18)
    o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)
    d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)
    with rt.Scene(0, rt.World(sph, tri, world_index=wi)) as sc:
        for flags in (0, F.RT_FLAG_NO_BVH_CULL, F.RT_FLAG_EXACT_SCAN):
            hits, _ = sc.intersect(o, d, flags=flags)
            got = hits["index"][hits["index"] != NONE]
            assert len(got) > 0 and np.all(got < n)
            # the hit point lies on the object at that world position
            inv = np.empty(n, np.int64)
            inv[wi] = np.arange(n)
            for h in hits[hits["index"] != NONE][:200]:
                k = int(inv[h["index"]])
                if k < len(sph):
                    s = sph[k]
                    r = np.sqrt((h["px"] - s["cx"]) ** 2 + (h["py"] - s["cy"]) ** 2 + (h["pz"] - s["cz"]) ** 2)
                    assert abs(r - s["radius"]) < 1e-3, (h, s)
                else:
                    assert abs(h["py"] - tri[k - len(sph)]["a"][1]) < 1e-4, h


def test_argument_errors_launch_nothing(ndev):
    lib = _abi.load()
    rays = _rays([(0, 0, 0)] * 4, [(0, 0, -1)] * 4)
    hits = np.zeros(4, _abi.HIT_DTYPE)
    rp, hp = rays.ctypes.data_as(C.POINTER(_abi.Ray)), hits.ctypes.data_as(C.POINTER(_abi.Hit))
    with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
        sc.collect()
        assert lib.rt_scene_intersect(sc._h, rp, 0, 0, 0, hp, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_intersect(sc._h, rp, 4, 2, 0, hp, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_intersect(sc._h, None, 4, 0, 0, hp, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_intersect(sc._h, rp, 4, 0, 0, None, None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_intersect_device(sc._h, C.c_void_p(rays.ctypes.data), 0, 0, 0, C.c_void_p(hits.ctypes.data), None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_intersect_device(sc._h, None, 4, 0, 0, C.c_void_p(hits.ctypes.data), None) == _abi.RT_ERR_BAD_ARG
        assert lib.rt_scene_intersect_device(sc._h, C.c_void_p(rays.ctypes.data), 4, 7, 0, None, None) == _abi.RT_ERR_BAD_ARG
        st = sc.collect()
        assert st.n_launches == 0 and st.primary_rays == 0 and st.ray_segments == 0
        assert np.all(hits["index"] == 0)
        with pytest.raises(ValueError):
            sc.intersect(np.zeros((3, 3)), np.zeros((4, 3)))


_DEVICE_CHILD = r"""
import numpy as np
import torch                                                      # first: the library then binds to torch's HIP runtime
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes
rt.init()
g = np.random.default_rng(11)
n = 100003
rays = np.empty(n, _abi.RAY_DTYPE)
o = g.uniform((-20, -1, -40), (20, 8, 0), size=(n, 3)).astype(np.float32)
d = g.normal(size=(n, 3)).astype(np.float32)
rays["ox"], rays["oy"], rays["oz"] = o.T
rays["dx"], rays["dy"], rays["dz"] = d.T
rays["t_min"], rays["t_max"] = 0.001, 1000.0
dev = torch.device("cuda", 0)
d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).to(dev)
stream = torch.cuda.current_stream().cuda_stream
with rt.Scene(0, rt.World(scenes.rand1024())) as sc:
    for any_hit, flags in ((False, 0), (True, 0), (False, _abi.RT_FLAG_NO_BVH_CULL)):
        d_hits = torch.empty((n, 8), dtype=torch.int32, device=dev)
        sc.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), any_hit=any_hit, flags=flags, stream=stream)
        sc.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), any_hit=any_hit, flags=flags, stream=stream)
        torch.cuda.synchronize()
        st = sc.collect()
        assert st.n_launches == 2 and st.primary_rays == 2 * n == st.ray_segments, (st.n_launches, st.primary_rays)
        assert st.engine == (1 if flags else 2) and st.kernel_ms > 0, st.engine
        ref, _ = sc.intersect(o, d, any_hit=any_hit, flags=flags)
        got = d_hits.cpu().numpy().tobytes()
        if any_hit:
            assert np.array_equal(np.frombuffer(got, _abi.HIT_DTYPE)["index"] != 0xFFFFFFFF, ref["index"] != 0xFFFFFFFF)
        else:
            assert got == ref.tobytes()
print("DEVICE OK")
"""


def test_device_form_equals_host_form(ndev):
    """rt_scene_intersect_device on torch tensors, counters through rt_scene_collect (in a child process that imports torch first:
    one HIP runtime for both)."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _DEVICE_CHILD], capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=300)
    assert r.returncode == 0 and "DEVICE OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_plain_c_query_client(ndev, tmp_path):
    """examples/query_rays.c through the C-ABI only (no Python binding in the loop)."""
    exe = tmp_path / "query_rays"
    lib = _abi.lib_path().parent
    r = subprocess.run([shutil.which("gcc"), "-std=c99", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "query_rays.c"),
                        f"-L{lib}", "-lrt_s8", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "QUERY_OK" in run.stdout, run.stdout + run.stderr
