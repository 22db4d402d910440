"""The host layer's device resources on the GPU (csrc/rt_device.h as rt_api.hip uses it; the owners themselves are tested on the CPU
by tests/test_device_host.py): the sample-unit rings shared by more streams than there are rings and grown under them, scenes
created and destroyed over and over with rt_shutdown / rt_init around them, and a host form whose staging grows between calls.
Small frames (128 x 80), a few hundred spheres, at most 8 samples: every result is the oracle's, byte for byte."""
import ctypes as C
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes

from test_gpu_ray_fuzz import check_closest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
W, H = 128, 80


def _field():
    return scenes.rand1024(n=300)


def test_more_streams_than_rings_and_rings_that_grow_under_them(ndev, oracle, capfd):
    """One scene, six caller streams (the scene has four rings): a strip on each at 1 sample per pixel, then a strip on each of the
    same six at 8.  The first round's strips are an eighth of the frame, the second round's the whole frame: a launch of the second
    round has eight times the tiles, so its ring is larger than any the first round left, and every ring grows while the other
    rings belong to other streams' launches.  The launch lines of RT_VERBOSE give the ring sizes."""
    sph = _field()
    rounds = [_abi.default_request(width=W, height=H, divisions=8, spp=1, max_bounces=4), _abi.default_request(width=W, height=H, divisions=1, spp=8, max_bounces=4)]
    with _abi.debug_library():               # (RT_VERBOSE is a hook of the TEST library)
        rt.init()
        hip = _abi.hip_runtime()
        prev = _abi.debug_set("RT_VERBOSE", 1)
        try:
            with rt.Scene(0, rt.World(sph)) as sc:
                streams, jobs = [], []
                for _ in range(6):
                    s = C.c_void_p()
                    assert hip.hipStreamCreate(C.byref(s)) == 0
                    streams.append(s)
                for base in rounds:                  # (every buffer first: nothing but launches between the launches)
                    for i in range(6):
                        rq = base.copy()
                        rq.seed = 7 + i
                        rq.division_no = i % rq.divisions
                        nb = W * (H // rq.divisions) * 3
                        d = C.c_void_p()
                        assert hip.hipMalloc(C.byref(d), C.c_size_t(nb)) == 0
                        jobs.append((rq, d, nb))
                capfd.readouterr()
                for k, (rq, d, nb) in enumerate(jobs):
                    sc.render_tiles_device([rq], [d.value], nb, streams[k % 6].value)
                assert hip.hipDeviceSynchronize() == 0
                st = sc.collect()
                got = []
                for rq, d, nb in jobs:
                    h = np.zeros(nb, np.uint8)
                    assert hip.hipMemcpy(h.ctypes.data_as(C.c_void_p), d, C.c_size_t(nb), 2) == 0      # hipMemcpyDeviceToHost
                    got.append(h)
                    hip.hipFree(d)
                for s in streams:
                    hip.hipStreamDestroy(s)
        finally:
            _abi.debug_set("RT_VERBOSE", prev)
    assert st.n_launches == 12
    ring = [int(b) for b in re.findall(r"sample-unit ring (\d+) B", capfd.readouterr().err)]
    assert len(ring) == 12 and len(set(ring[:6])) == 1 and len(set(ring[6:])) == 1 and ring[6] > ring[0] > 0, ring
    for (rq, _, _), h in zip(jobs, got):
        want, _, _ = oracle.render(rq, sph, backend=1)
        assert np.array_equal(h, want), (rq.spp, rq.division_no, rq.seed)


_LIFETIME_CHILD = r"""
import ctypes as C
import numpy as np
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes
lib = _abi.load()
lib.rt_last_error.restype = C.c_char_p
assert rt.init() >= 1
sph = scenes.rand1024(n=300)
rq = _abi.default_request(width=128, height=80, divisions=1, spp=2, max_bounces=4, seed=11)
first = None
for i in range(40):
    with rt.Scene(0, rt.World(sph)) as sc:
        rgb, _, st = sc.render_tile(rq)
    assert st.n_launches == 1
    if first is None:
        first = rgb.copy()
    assert np.array_equal(rgb, first), i
lib.rt_shutdown()                                   # no scene is alive: accepted, so the library is as before rt_init
h = C.c_void_p()
sp = np.ascontiguousarray(sph)
rc = lib.rt_scene_create(0, sp.ctypes.data, len(sp), None, 0, None, C.byref(h))
assert rc == _abi.RT_ERR_NOT_INITIALIZED and not h.value, (rc, lib.rt_last_error())
n = C.c_int(0)
assert lib.rt_init(C.byref(n)) == 0 and n.value >= 1
with rt.Scene(0, rt.World(sph)) as sc:
    again, _, _ = sc.render_tile(rq)
assert np.array_equal(again, first)
np.save(OUT, first)
print("LIFETIME OK")
"""


def test_forty_scenes_then_shutdown_and_init_again(ndev, oracle, tmp_path):
    """Create, render, destroy, 40 times on one device; then rt_shutdown is accepted (a scene cannot be created any more), rt_init
    works again and a render gives the first one's bytes, which are the oracle's.  In a child process: rt_shutdown is the whole
    process's, and another test's scene still alive here would have it refused."""
    out = tmp_path / "first.npy"
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", f"OUT = {str(out)!r}\n" + _LIFETIME_CHILD], capture_output=True, text=True, cwd=str(ROOT), env=env,
                       timeout=300)
    assert r.returncode == 0 and "LIFETIME OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    rq = _abi.default_request(width=W, height=H, divisions=1, spp=2, max_bounces=4, seed=11)
    want, _, _ = oracle.render(rq, _field(), backend=1)
    assert np.array_equal(np.load(out), want)


def test_host_form_grows_its_staging_and_goes_on(ndev, oracle):
    """rt_scene_intersect with 64 rays, then 4096, then 64 on one scene: the one staging buffer of the host forms is made, grown
    (freed and allocated again) and then larger than needed.  The hits are the oracle's each time."""
    sph = _field()
    g = np.random.default_rng(0x6B0F)
    n = 4096
    o = g.uniform((-20, -1, -40), (20, 8, 0), size=(n, 3)).astype(np.float32)
    d = g.normal(size=(n, 3)).astype(np.float32)
    rays = np.empty(n, _abi.RAY_DTYPE)
    rays["ox"], rays["oy"], rays["oz"] = o.T
    rays["dx"], rays["dy"], rays["dz"] = d.T
    rays["t_min"], rays["t_max"] = 0.001, 1000.0
    ref = oracle.intersect_batch(sph, None, rays, backend=1)
    assert 0.05 < ref["hit"].mean() < 0.95
    with rt.Scene(0, rt.World(sph)) as sc:
        for lo, hi in ((0, 64), (0, 4096), (4032, 4096)):
            hits, st = sc.intersect(o[lo:hi], d[lo:hi])
            assert st.n_launches == 1 and st.primary_rays == hi - lo
            check_closest(hits, rays[lo:hi], {k: v[lo:hi] for k, v in ref.items()}, (lo, hi))
