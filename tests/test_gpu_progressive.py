"""Progressive passes on the GPU (rt_scene_render_tile_pass, rt_scene_render_tiles_pass_device): a strip rendered in passes over
a running f32 sum ends bit-identical to the one-pass strip, through every closest-hit engine; the running sum is the oracle's
sequential per-sample sum; the argument checks launch nothing."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

T, E, Q = _abi.RT_FLAG_BVH_TRAVERSE, _abi.RT_FLAG_EXACT_NODES, _abi.RT_FLAG_QUANT_NODES
# engine -> (scene, request flags)
ENGINES = {
    0: ("cornell16", _abi.RT_FLAG_LINEAR_SCAN),                                # scan, scene resident in LDS
    1: ("field9000", _abi.RT_FLAG_LINEAR_SCAN),                                # scan, scene streamed through LDS
    2: ("rand1024", T | E | _abi.RT_FLAG_NO_LDS_TREE),
    3: ("field9000", T | Q | _abi.RT_FLAG_NO_CULL_WALK),
    4: ("rand1024", T | E | _abi.RT_FLAG_NO_CULL_WALK),                        # LDS-resident tree
    5: ("field9000", T | Q | _abi.RT_FLAG_CULL_WALK),
    6: ("terrain", T | E | _abi.RT_FLAG_CULL_WALK | _abi.RT_FLAG_NO_LDS_TREE),
    7: ("rand1024", T | E | _abi.RT_FLAG_CULL_WALK),                           # LDS-resident tree, culled
}
# (spp, width, height, divisions, division_no, passes): a ragged 96-pixel row (a whole and a part tile), a strip below the top
SPLITS = {
    "s100": (100, 96, 12, 2, 1, [(0, 1), (1, 8), (8, 37), (37, 100)]),
    "s8": (8, 96, 12, 2, 1, [(0, 3), (3, 8)]),
    "s1": (1, 96, 12, 2, 1, [(0, 1)]),
    "s4096": (4096, 8, 2, 1, 0, [(0, 1000), (1000, 4096)]),
}


def _world(name):
    if name == "cornell16":
        return rt.World(scenes.cornell16())
    if name == "field9000":
        return rt.World(scenes.rand65536(n=9000))
    if name == "rand1024":
        return rt.World(scenes.rand1024())
    # a terrain of 25 088 small triangles: within the culled walk's bound (tri_terrain's large ones fall back to engine 2)
    return rt.World(None, scenes.mesh_world(112, 112))


def _request(spp, w, h, div, no, flags=0, seed=0x9A55):
    return _abi.default_request(width=w, height=h, divisions=div, division_no=no, spp=spp, max_bounces=4, seed=seed, flags=flags)


def _run_passes(sc, rq, passes, want_f32=True):
    """The passes in order, one running sum; checks the per-pass counters.  Returns the last (rgb, f32, accum) and the summed
    ray segments."""
    hs = rq.height // rq.divisions
    acc, segs = None, 0
    for b, e in passes:
        rgb, f32, acc, st = sc.render_tile_pass(rq, b, e, acc, want_f32=want_f32)
        assert st.primary_rays == hs * rq.width * (e - b) and st.n_launches == 1
        segs += st.ray_segments
    return rgb, f32, acc, segs, st


def _expected_engine(engine, got):
    # the quantised nodes need a grid fine enough for the scene; where it is not, the request falls back to the exact nodes
    # (tests/test_gpu_parity.py accepts the same)
    if engine in (3, 5) and got in (2, 4):
        return got
    return engine


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("engine", list(ENGINES))
def test_last_pass_is_the_one_pass_strip(ndev, engine, split):
    scene, flags = ENGINES[engine]
    spp, w, h, div, no, passes = SPLITS[split]
    rq = _request(spp, w, h, div, no, flags)
    with rt.Scene(0, _world(scene)) as sc:
        ref, ref_f, ref_st = sc.render_tile(rq, want_f32=True)
        rgb, f32, acc, segs, st = _run_passes(sc, rq, passes)
    assert ref_st.engine == _expected_engine(engine, ref_st.engine) and st.engine == ref_st.engine
    assert np.array_equal(rgb, ref), f"engine {engine}, {split}: {int((rgb != ref).sum())} RGB8 bytes differ"
    assert np.array_equal(f32.view(np.uint32), ref_f.view(np.uint32)), f"engine {engine}, {split}: f32 not bit-identical"
    assert segs == ref_st.ray_segments
    # the preview is sqrt(sum / end) of the running sum the pass handed back
    assert np.array_equal(f32.view(np.uint32), np.sqrt(acc.reshape(-1) / np.float32(spp)).view(np.uint32))


def test_full_width_1080p_strip_in_two_passes(ndev):
    sph, rq = scenes.config("c2")
    rq.spp, rq.division_no = 100, 10
    with rt.Scene(0, rt.World(sph)) as sc:
        ref, ref_f, ref_st = sc.render_tile(rq, want_f32=True)
        rgb, f32, _, segs, _ = _run_passes(sc, rq, [(0, 37), (37, 100)])
    assert np.array_equal(rgb, ref) and np.array_equal(f32.view(np.uint32), ref_f.view(np.uint32))
    assert segs == ref_st.ray_segments


def test_running_sum_is_the_oracles_sequential_sum(ndev, oracle):
    """After a middle pass, accum holds exactly the f32 sum over samples [0, end) that the oracle forms for the pixel one sample
    at a time, each sample from its own stream seed + 4 PHI (p S + s) with S the job's spp; the preview is sqrt(sum / end).
    cornell16 is closed (no primary ray sees the sky): the pixels include one on the light (paths of one segment) and bounced
    ones, on both tiles of a ragged row."""
    W, H, div, S = 72, 36, 3, 12
    rq = _request(S, W, H, div, 0, _abi.RT_FLAG_NO_BVH_CULL, seed=77)            # plain linear scan = the oracle's backend 0
    sph = scenes.cornell16()
    with rt.Scene(0, rt.World(sph)) as sc:
        acc = np.full((H // div, W, 3), np.nan, np.float32)                        # (not read by a pass from sample 0)
        _, _, acc, _ = sc.render_tile_pass(rq, 0, 5, acc)
        _, f32, acc, _ = sc.render_tile_pass(rq, 5, 9, acc, want_f32=True)
    end = 9
    one_segment = 0
    for x, y in [(35, 10), (36, 11), (2, 0), (40, 6), (70, 11), (71, 3)]:
        s = np.zeros(3, np.float32)
        for k in range(end):
            st = oracle.seed_from_u64(oracle.sample_seed(rq.seed, y * W + x, S, k))
            o, d = oracle.camera_ray(rq, x, H - y - 1, st)
            c, segs = oracle.ray_color(sph, None, o, d, rq.max_bounces + 1, st)
            s = (s + c).astype(np.float32)
            one_segment += segs == 1
        assert np.array_equal(acc[y, x].view(np.uint32), s.view(np.uint32)), (x, y, acc[y, x], s)
        assert np.array_equal(f32.reshape(acc.shape)[y, x].view(np.uint32),
                              np.sqrt(s / np.float32(end)).astype(np.float32).view(np.uint32)), (x, y)
    assert one_segment >= end // 2                                                # the light pixels
    assert np.array_equal(f32.view(np.uint32), np.sqrt(acc.reshape(-1) / np.float32(end)).view(np.uint32))


_BATCHED_CHILD = r"""
import sys
import numpy as np
import torch                                                      # first: the library then binds to torch's HIP runtime
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes
rt.init()
W, H, div, S = 200, 50, 4, 10                                     # 50 % 4 != 0: strips of 12 rows, the last two rows dropped
reqs = [_abi.default_request(width=W, height=H, divisions=div, division_no=k, spp=S, max_bounces=4, seed=31 + k) for k in range(div)]
nb = (H // div) * W * 3
dev = torch.device("cuda", 0)
out = [torch.empty(nb, dtype=torch.uint8, device=dev) for _ in reqs]
outf = [torch.empty(nb, dtype=torch.float32, device=dev) for _ in reqs]
acc = [torch.empty(nb, dtype=torch.float32, device=dev) for _ in reqs]
stream = torch.cuda.current_stream().cuda_stream
with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
    segs = 0
    for b, e in [(0, 3), (3, 4), (4, 10)]:
        sc.render_tiles_pass_device(reqs, b, e, [a.data_ptr() for a in acc], [o.data_ptr() for o in out], nb,
                                    [f.data_ptr() for f in outf], stream)
        torch.cuda.synchronize()
        st = sc.collect()
        assert st.n_launches == 1 and st.primary_rays == div * nb // 3 * (e - b), (st.n_launches, st.primary_rays)
        segs += st.ray_segments
    ref, ref_f, ref_st = sc.render_tiles(reqs, want_f32=True)
got = np.concatenate([o.cpu().numpy() for o in out])
got_f = np.concatenate([f.cpu().numpy() for f in outf])
assert np.array_equal(got, np.concatenate(ref)), int((got != np.concatenate(ref)).sum())
assert np.array_equal(got_f.view(np.uint32), np.concatenate(ref_f).view(np.uint32))
assert segs == ref_st.ray_segments, (segs, ref_st.ray_segments)
print("BATCHED OK")
"""


def test_batched_device_passes_on_a_ragged_frame(ndev):
    """All strips of a frame whose height the divisions do not divide, one rt_scene_render_tiles_pass_device per pass, device
    buffers from torch (in a child process that imports torch first: one HIP runtime for both)."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _BATCHED_CHILD], capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=300)
    assert r.returncode == 0 and "BATCHED OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("cull", [0, _abi.RT_FLAG_CULL_WALK])
def test_capped_stack_kernels(ndev, cull):
    """The capped-stack walks (stack entries beyond three LDS slots in HBM): still bit-identical."""
    with _abi.debug_library():
        rt.init()
        prev = [_abi.debug_set("RT_FORCE_CAPPED", 1), _abi.debug_set("RT_STACK_LDS", 3)]
        try:
            rq = _request(8, 96, 12, 2, 1, T | Q | cull)
            with rt.Scene(0, _world("field9000")) as sc:
                ref, ref_f, ref_st = sc.render_tile(rq, want_f32=True)
                rgb, f32, _, segs, st = _run_passes(sc, rq, [(0, 3), (3, 8)])
        finally:
            _abi.debug_set("RT_FORCE_CAPPED", prev[0])
            _abi.debug_set("RT_STACK_LDS", prev[1])
    assert ref_st.engine == (5 if cull else 3) and st.engine == ref_st.engine
    assert np.array_equal(rgb, ref) and np.array_equal(f32.view(np.uint32), ref_f.view(np.uint32))
    assert segs == ref_st.ray_segments


def test_argument_errors_launch_nothing(ndev):
    rq = _request(8, 96, 12, 2, 1)
    nb = 6 * 96 * 3
    lib = _abi.load()
    acc = np.zeros(nb, np.float32)
    out = np.zeros(nb, np.uint8)
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    with rt.Scene(0, _world("cornell16")) as sc:
        sc.collect()

        def host(b, e, a):
            return lib.rt_scene_render_tile_pass(sc._h, C.byref(rq), b, e, a, out.ctypes.data_as(bp), nb, None, None)

        assert host(3, 3, acc.ctypes.data_as(fp)) == _abi.RT_ERR_BAD_ARG               # begin >= end
        assert host(5, 2, acc.ctypes.data_as(fp)) == _abi.RT_ERR_BAD_ARG
        assert host(0, 9, acc.ctypes.data_as(fp)) == _abi.RT_ERR_BAD_ARG               # end > spp
        assert host(0, 8, None) == _abi.RT_ERR_BAD_ARG                                 # NULL accum
        # the device form: device pointers are never dereferenced on a refused call, the checks come first
        d = C.c_void_p(0x1000)
        reqs = (_abi.TileRequest * 2)(rq, rq)
        reqs[1].division_no = 0

        def dev(b, e, accs):
            return lib.rt_scene_render_tiles_pass_device(sc._h, reqs, 2, b, e, accs, (C.c_void_p * 2)(d, d), nb, None, None)

        good = (C.c_void_p * 2)(d, d)
        assert dev(4, 4, good) == _abi.RT_ERR_BAD_ARG
        assert dev(0, 9, good) == _abi.RT_ERR_BAD_ARG
        assert dev(0, 8, None) == _abi.RT_ERR_BAD_ARG
        assert dev(0, 8, (C.c_void_p * 2)(d, None)) == _abi.RT_ERR_BAD_ARG
        st = sc.collect()
    assert st.n_launches == 0 and st.primary_rays == 0


def test_render_progressive_generator(ndev):
    rq = _request(64, 96, 12, 2, 1)
    with rt.Scene(0, _world("cornell16")) as sc:
        ref, _, _ = sc.render_tile(rq)
        steps = list(sc.render_progressive(rq, 16))
    assert [e for e, _, _ in steps] == [16, 32, 48, 64]
    assert all(st.primary_rays == 6 * 96 * 16 for _, _, st in steps)
    assert np.array_equal(steps[-1][1], ref)
    assert not np.array_equal(steps[0][1], ref)                                   # a preview, not yet the image
