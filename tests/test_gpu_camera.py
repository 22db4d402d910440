"""The placed camera on the GPU (rt_scene_set_camera, rt_frame_ctx_set_camera, rt_scene_camera_rays*), bit for bit throughout:
1. rays: rt_scene_camera_rays equals the numpy restatement of a pose (tests/_camera_np.py), rays and RNG states, host and device
   form; with no camera set it equals the oracle's camera_ray;
2. tile = oracle: the accum of a posed strip is the in-order f32 sum of the batch oracle's ray_color over the restated rays, under
   BVH semantics (backend 1) and the plain scan (RT_FLAG_NO_BVH_CULL, backend 0), every pose on every scene;
3. engines agree: a posed frame renders the same bytes under every forced engine;
4. stitching, passes and the batched device form;
5. the feature buffers under a pose against the batch oracle's first hits, and the denoiser's pass-through of the posed preview;
6. state: NULL restores the reference camera, the default pose is the reference camera, enqueued work keeps its camera, the frame
   context's camera and its cost cache."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes

import _camera_np as cnp
from test_gpu_query import SCENES, _world

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
F = _abi
W, H, DIV, SPP = 48, 27, 3, 4

# (origin, target, up); None: no camera set.  The default pose; a pure translation; an oblique look-at with a rolled up; an eye
# inside the scenes' bounding boxes looking up.
POSES = {
    "default": ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)),
    "translated": ((0.75, 0.5, 1.5), (0.75, 0.5, 0.5), (0.0, 1.0, 0.0)),
    "oblique_rolled": ((2.5, 1.75, 1.0), (-0.25, 0.1, -2.0), (0.3, 1.0, -0.2)),
    "inside_looking_up": ((0.1, -0.2, -1.2), (0.15, 3.0, -1.3), (0.0, 0.2, -1.0)),
}


def _request(division_no=0, flags=0, seed=0xC0FFEE, **kw):
    return _abi.default_request(width=W, height=H, divisions=DIV, division_no=division_no, spp=SPP, max_bounces=6, seed=seed,
                                flags=flags, **kw)


def _cam(pose):
    return None if pose is None else _abi.Camera.look_at(*pose)


_RAYS = {}


def _restated(oracle, pose_name, division_no):
    """The restated rays and states of a strip of the standard frame under a pose (cached: the numpy restatement is slow)."""
    key = (pose_name, division_no)
    if key not in _RAYS:
        _RAYS[key] = cnp.strip_rays(oracle, _request(division_no), POSES[pose_name])
    return _RAYS[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _quantise(f):
    """The tile's quantisation (color.rs:13-19): (c * 255.999) as u8, truncating, saturating, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        v = np.asarray(f, np.float32) * np.float32(255.999)
        return np.where(np.isnan(v), 0, np.clip(np.floor(v), 0, 255)).astype(np.uint8)


def _sum_in_order(per):
    """per: (pixels, samples, k) -> the f32 sum over the samples in order, from +0."""
    tot = np.zeros((per.shape[0], per.shape[2]), np.float32)
    for s in range(per.shape[1]):
        tot = (tot + per[:, s]).astype(np.float32)
    return tot


# ------------------------------------------------------------------------------------------------------------------ 1. rays


@pytest.mark.parametrize("pose", POSES)
def test_camera_rays_equal_the_restatement(ndev, oracle, pose):
    sph, tri = _world("cornell16")
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_camera(_cam(POSES[pose]))
        for k in range(DIV):
            rq = _request(k)
            rays, states, st = sc.camera_rays(rq)
            erays, estates = _restated(oracle, pose, k)
            assert rays.tobytes() == erays.tobytes(), (pose, k, np.nonzero(rays != erays)[0][:5])
            assert np.array_equal(states, estates), (pose, k)
            assert st.primary_rays == len(erays) and st.n_launches == 1 and st.ray_segments == 0
        # a sample range: the same records, cut out; no states asked for
        rq = _request(1)
        part, none, st = sc.camera_rays(rq, 1, 3, want_states=False)
        erays, _ = _restated(oracle, pose, 1)
        assert none is None and part.tobytes() == erays.reshape(-1, SPP)[:, 1:3].tobytes()
        assert st.primary_rays == len(part) == (H // DIV) * W * 2


def test_camera_rays_without_a_camera_are_the_oracles(ndev, oracle):
    sph, _ = _world("single_sphere")
    rq = _request(2, aperture=0.4, focus_distance=2.5, fov=1.2)
    hs = H // DIV
    with rt.Scene(0, rt.World(sph)) as sc:
        rays, states, _ = sc.camera_rays(rq)
        sc.set_camera(_abi.Camera.look_at((1, 2, 3), (0, 0, 0)))
        sc.set_camera(None)
        again, sagain, _ = sc.camera_rays(rq)
    assert rays.tobytes() == again.tobytes() and np.array_equal(states, sagain)
    i = 0
    for yl in range(hs):
        yg = hs * rq.division_no + yl
        for x in range(W):
            for s in range(SPP):
                st = oracle.seed_from_u64(oracle.sample_seed(rq.seed, yg * W + x, SPP, s))
                o, d = oracle.camera_ray(rq, x, H - 1 - yg, st)
                r = rays[i]
                got = np.array([r["ox"], r["oy"], r["oz"], r["dx"], r["dy"], r["dz"]], np.float32)
                assert _same_bits(got, np.concatenate([o, d])), (x, yg, s)
                assert np.array_equal(states[i], st) and r["t_min"] == np.float32(rq.t_min) and r["t_max"] == np.float32(rq.t_max)
                i += 1


_DEVICE_CHILD = r"""
import sys
import numpy as np
import torch                                                      # first: the library then binds to torch's HIP runtime
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes
W, H, DIV, SPP = 48, 27, 3, 4
pose = ((2.5, 1.75, 1.0), (-0.25, 0.1, -2.0), (0.3, 1.0, -0.2))
rq = _abi.default_request(width=W, height=H, divisions=DIV, division_no=1, spp=SPP, max_bounces=6, seed=0xC0FFEE)
n = (H // DIV) * W * SPP
dev = torch.device("cuda:0")
with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
    sc.set_camera(_abi.Camera.look_at(*pose))
    rays, states, _ = sc.camera_rays(rq)
    d_rays = torch.zeros(n * 8, dtype=torch.float32, device=dev)
    d_states = torch.zeros(n * 4, dtype=torch.int64, device=dev)
    d_rgb = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    # the camera's rays on the device, traced there from the states the camera left: no host round trip
    sc.camera_rays_device(rq, 0, SPP, d_rays.data_ptr(), d_states.data_ptr())
    # a camera set AFTER the launch was enqueued does not reach it
    sc.set_camera(None)
    st = sc.collect()
    assert st.n_launches == 1 and st.primary_rays == n, (st.n_launches, st.primary_rays)
    assert d_rays.cpu().numpy().tobytes() == rays.tobytes()
    assert d_states.cpu().numpy().view(np.uint64).reshape(n, 4).tobytes() == states.tobytes()
    sc.trace_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), d_rng_state=d_states.data_ptr(), spp=1, max_bounces=rq.max_bounces,
                    as_given=True)
    sc.collect()
    # ... and the colours sum to the posed strip's accum
    sc.set_camera(_abi.Camera.look_at(*pose))
    _, _, accum, _ = sc.render_tile_pass(rq, 0, SPP)
    per = d_rgb.cpu().numpy().reshape(-1, SPP, 3)
    tot = np.zeros((per.shape[0], 3), np.float32)
    for s in range(SPP):
        tot = (tot + per[:, s]).astype(np.float32)
    assert tot.view(np.uint32).tobytes() == accum.view(np.uint32).tobytes()
    # states are optional in the device form too
    d_rays.zero_()
    sc.camera_rays_device(rq, 0, SPP, d_rays.data_ptr())
    sc.collect()
    assert d_rays.cpu().numpy().tobytes() == rays.tobytes()
print("ok")
"""


def test_camera_rays_device_form(ndev):
    """torch needs a process of its own in which it is imported first (two HIP runtimes, _abi.check_single_hip_runtime)."""
    r = subprocess.run([sys.executable, "-c", _DEVICE_CHILD], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------ 2. tile = oracle


@pytest.mark.parametrize("pose", POSES)
@pytest.mark.parametrize("scene", SCENES)
def test_posed_tile_equals_the_batch_oracle(ndev, oracle, scene, pose):
    sph, tri = _world(scene)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_camera(_cam(POSES[pose]))
        for flags, backend in ((0, 1), (F.RT_FLAG_NO_BVH_CULL, 0)):
            for k in range(DIV):
                rq = _request(k, flags)
                rays, states = _restated(oracle, pose, k)
                rgb, f32, accum, st = sc.render_tile_pass(rq, 0, SPP, want_f32=True)
                ergb, esegs, _ = oracle.trace_batch(sph, tri, rays, spp=1, max_bounces=rq.max_bounces, backend=backend,
                                                    ray_as_given=True, states=states)
                total = _sum_in_order(ergb.reshape(-1, SPP, 3))
                assert _same_bits(total, accum.reshape(-1, 3)), (scene, pose, flags, k,
                                                                 np.argwhere(_bits(total) != _bits(accum.reshape(-1, 3)))[:5])
                with np.errstate(invalid="ignore"):
                    prev = np.sqrt((total / np.float32(SPP)).astype(np.float32)).astype(np.float32)
                assert _same_bits(prev.reshape(-1), f32), (scene, pose, flags, k)
                assert np.array_equal(_quantise(prev).reshape(-1), rgb), (scene, pose, flags, k)
                assert int(esegs.sum()) == st.ray_segments, (scene, pose, flags, k)
                assert st.primary_rays == len(rays)


# ----------------------------------------------------------------------------------------------------------- 3. engines agree

ENGINE_FLAGS = {
    "linear": F.RT_FLAG_LINEAR_SCAN,
    "traverse": F.RT_FLAG_BVH_TRAVERSE,
    "exact_nodes": F.RT_FLAG_BVH_TRAVERSE | F.RT_FLAG_EXACT_NODES,
    "exact_nodes_l2": F.RT_FLAG_BVH_TRAVERSE | F.RT_FLAG_EXACT_NODES | F.RT_FLAG_NO_LDS_TREE,
    "exact_nodes_cull": F.RT_FLAG_BVH_TRAVERSE | F.RT_FLAG_EXACT_NODES | F.RT_FLAG_CULL_WALK,
    "exact_nodes_no_cull": F.RT_FLAG_BVH_TRAVERSE | F.RT_FLAG_EXACT_NODES | F.RT_FLAG_NO_CULL_WALK,
    "exact_nodes_l2_cull": F.RT_FLAG_BVH_TRAVERSE | F.RT_FLAG_EXACT_NODES | F.RT_FLAG_NO_LDS_TREE | F.RT_FLAG_CULL_WALK,
    "quant_nodes_cull": F.RT_FLAG_BVH_TRAVERSE | F.RT_FLAG_QUANT_NODES | F.RT_FLAG_CULL_WALK,
    "quant_nodes_no_cull": F.RT_FLAG_BVH_TRAVERSE | F.RT_FLAG_QUANT_NODES | F.RT_FLAG_NO_CULL_WALK,
    "no_lds_tree": F.RT_FLAG_NO_LDS_TREE,
}


@pytest.mark.parametrize("scene", ["rand1024", "field9000", "terrain"])     # LDS-tree size, above 4096 spheres, a mesh
def test_posed_frame_is_the_same_under_every_engine(ndev, scene):
    sph, tri = _world(scene)
    rq = _abi.default_request(width=96, height=54, divisions=1, spp=3, max_bounces=8, seed=77)
    engines = {}
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_camera(_cam(POSES["oblique_rolled"]))
        ref, ref_f, ref_st = sc.render_tile(rq, want_f32=True)
        assert ref.std() > 1.0
        for name, fl in ENGINE_FLAGS.items():
            r = rq.copy()
            r.flags = fl
            rgb, f32, st = sc.render_tile(r, want_f32=True)
            engines[name] = st.engine
            assert np.array_equal(rgb, ref) and np.array_equal(_bits(f32), _bits(ref_f)), (scene, name, st.engine)
            assert st.ray_segments == ref_st.ray_segments, (scene, name)
        # the pose does not choose the engine
        sc.set_camera(None)
        for name, fl in ENGINE_FLAGS.items():
            r = rq.copy()
            r.flags = fl
            assert sc.render_tile(r)[2].engine == engines[name], (scene, name)
        assert sc.render_tile(rq)[2].engine == ref_st.engine
    assert len(set(engines.values())) >= 3, engines


# ------------------------------------------------------------------------------------------------- 4. stitching, passes, batches


@pytest.mark.parametrize("pose", ["translated", "oblique_rolled"])
def test_posed_strips_stitch_and_passes_compose(ndev, pose):
    sph, tri = _world("quad_room")
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_camera(_cam(POSES[pose]))
        one = _abi.default_request(width=W, height=H, divisions=1, spp=SPP, max_bounces=6, seed=0xC0FFEE)
        whole, whole_f, whole_st = sc.render_tile(one, want_f32=True)
        strips = [sc.render_tile(_request(k), want_f32=True) for k in range(DIV)]
        assert np.array_equal(np.concatenate([s[0] for s in strips]), whole)
        assert np.array_equal(_bits(np.concatenate([s[1] for s in strips])), _bits(whole_f))
        assert sum(s[2].ray_segments for s in strips) == whole_st.ray_segments
        batched, _, bst = sc.render_tiles([_request(k) for k in range(DIV)])
        assert np.array_equal(np.concatenate(batched), whole) and bst.ray_segments == whole_st.ray_segments
        for cuts in ([(0, 1), (1, 2), (2, 3), (3, 4)], [(0, 3), (3, 4)], [(0, 1), (1, 4)]):
            accum, segs = None, 0
            for b, e in cuts:
                rgb, f32, accum, st = sc.render_tile_pass(_request(1), b, e, accum, want_f32=True)
                segs += st.ray_segments
            assert np.array_equal(rgb, strips[1][0]) and np.array_equal(_bits(f32), _bits(strips[1][1])), cuts
            assert segs == strips[1][2].ray_segments


_TILES_DEVICE_CHILD = r"""
import numpy as np
import torch
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes
W, H, DIV, SPP = 48, 27, 3, 4
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=6, seed=0xC0FFEE) for k in range(DIV)]
nb = (H // DIV) * W * 3
dev = torch.device("cuda:0")
with rt.Scene(0, rt.World(scenes.rand1024())) as sc:
    sc.set_camera(_abi.Camera.look_at((2.5, 1.75, 1.0), (-0.25, 0.1, -2.0), (0.3, 1.0, -0.2)))
    per = [sc.render_tile(r)[0] for r in rqs]
    outs = [torch.zeros(nb, dtype=torch.uint8, device=dev) for _ in rqs]
    accs = [torch.zeros(nb, dtype=torch.float32, device=dev) for _ in rqs]
    torch.cuda.synchronize()
    sc.render_tiles_device(rqs, [o.data_ptr() for o in outs], nb)
    sc.set_camera(None)                                      # enqueued work keeps the camera it was enqueued with
    sc.collect()
    for o, p in zip(outs, per):
        assert np.array_equal(o.cpu().numpy(), p)
    ref = [sc.render_tile(r)[0] for r in rqs]                # the reference camera again
    assert any(not np.array_equal(a, b) for a, b in zip(ref, per))
    sc.set_camera(_abi.Camera.look_at((2.5, 1.75, 1.0), (-0.25, 0.1, -2.0), (0.3, 1.0, -0.2)))
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    sc.render_tiles_pass_device(rqs, 0, 2, [a.data_ptr() for a in accs], [o.data_ptr() for o in outs], nb)
    sc.render_tiles_pass_device(rqs, 2, SPP, [a.data_ptr() for a in accs], [o.data_ptr() for o in outs], nb)
    sc.collect()
    for o, p in zip(outs, per):
        assert np.array_equal(o.cpu().numpy(), p)
print("ok")
"""


def test_posed_batched_device_forms(ndev):
    r = subprocess.run([sys.executable, "-c", _TILES_DEVICE_CHILD], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------------- 5. AOV


@pytest.mark.parametrize("pose", ["oblique_rolled", "inside_looking_up"])
@pytest.mark.parametrize("scene", ["cornell16", "quad_room", "tie_world"])
def test_posed_feature_buffers_equal_the_batch_oracle(ndev, oracle, scene, pose):
    sph, tri = _world(scene)
    hs = H // DIV
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_camera(_cam(POSES[pose]))
        for flags, backend in ((0, 1), (F.RT_FLAG_NO_BVH_CULL, 0)):
            rq = _request(1, flags)
            rays, _ = _restated(oracle, pose, 1)
            planes, st = sc.render_aov(rq)
            h = oracle.intersect_batch(sph, tri, rays, backend=backend, ray_as_given=True)
            hit = h["hit"].reshape(-1, SPP)
            d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)
            o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)
            sky = np.array([oracle.sky(x) for x in d], np.float32)
            alb = np.where(h["hit"][:, None], h["albedo"], sky).astype(np.float32).reshape(-1, SPP, 3)
            dp = (h["point"] - o).astype(np.float32)
            dist = np.sqrt(((dp[:, 0] * dp[:, 0]).astype(np.float32) + (dp[:, 1] * dp[:, 1]).astype(np.float32)).astype(np.float32)
                           + (dp[:, 2] * dp[:, 2]).astype(np.float32)).astype(np.float32).reshape(-1, SPP)
            nrm = h["normal"].reshape(-1, SPP, 3)
            e_alb = _sum_in_order(alb)
            # a miss adds nothing to normal and depth (no addition at all)
            e_nrm = np.zeros((len(hit), 3), np.float32)
            e_dep = np.zeros(len(hit), np.float32)
            for s in range(SPP):
                m = hit[:, s]
                e_nrm[m] = (e_nrm[m] + nrm[m, s]).astype(np.float32)
                e_dep[m] = (e_dep[m] + dist[m, s]).astype(np.float32)
            assert _same_bits(planes["albedo"].reshape(-1, 3), e_alb), (scene, pose, flags)
            assert _same_bits(planes["normal"].reshape(-1, 3), e_nrm), (scene, pose, flags)
            assert _same_bits(planes["depth"].reshape(-1), e_dep), (scene, pose, flags)
            assert np.array_equal(planes["hits"].reshape(-1), hit.sum(1).astype(np.uint32))
            assert np.array_equal(planes["index"].reshape(-1), h["index"].reshape(-1, SPP)[:, 0])
            assert st.primary_rays == hs * W * SPP


def test_denoiser_passes_the_posed_preview_through(ndev):
    sph, tri = _world("cornell16")
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_camera(_cam(POSES["oblique_rolled"]))
        rqs = [_request(k) for k in range(DIV)]
        passes = [sc.render_tile_pass(r, 0, SPP, want_f32=True) for r in rqs]
        planes = [sc.render_aov(r, planes=("normal", "depth", "hits"))[0] for r in rqs]
        dq = _abi.DenoiseRequest.defaults(iterations=0)
        outs, _ = sc.denoise(rqs, [p[2] for p in passes], planes, SPP, SPP, dreq=dq)
        for o, p in zip(outs, passes):
            assert np.array_equal(o["rgb"].reshape(-1), p[0]) and np.array_equal(_bits(o["f32"].reshape(-1)), _bits(p[1]))


# ----------------------------------------------------------------------------------------------------------------- 6. state


def test_null_restores_and_defaults_are_the_reference_camera(ndev):
    sph, tri = _world("rand1024")
    for rq in (_abi.default_request(width=64, height=36, divisions=2, division_no=1, spp=3, seed=9),
               _request(1, aperture=0.4, fov=2.4, focal_length=1.5, focus_distance=3.5), _request(0, aperture=0.0)):
        with rt.Scene(0, rt.World(sph, tri)) as never:
            ref, ref_f, ref_st = never.render_tile(rq, want_f32=True)
            ref_aov, _ = never.render_aov(rq)
        with rt.Scene(0, rt.World(sph, tri)) as sc:
            sc.set_camera(_cam(POSES["oblique_rolled"]))
            posed, _, _ = sc.render_tile(rq)
            assert not np.array_equal(posed, ref)
            for cam in (None, _abi.Camera.defaults()):
                sc.set_camera(_cam(POSES["translated"]))
                sc.set_camera(cam)
                rgb, f32, st = sc.render_tile(rq, want_f32=True)
                assert np.array_equal(rgb, ref) and np.array_equal(_bits(f32), _bits(ref_f)), cam
                assert st.ray_segments == ref_st.ray_segments and st.engine == ref_st.engine
                aov, _ = sc.render_aov(rq)
                for n in ref_aov:
                    assert aov[n].tobytes() == ref_aov[n].tobytes(), (n, cam)


def test_bad_cameras_leave_the_previous_one(ndev):
    sph, tri = _world("cornell16")
    rq = _request(1)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_camera(_cam(POSES["translated"]))
        want = sc.render_tile(rq)[0]
        bad = [_abi.Camera.look_at((1, 1, 1), (1, 1, 1)), _abi.Camera.look_at((0, 0, 0), (0, 2, 0)),
               _abi.Camera.look_at((float("nan"), 0, 0), (0, 0, -1)), _abi.Camera.look_at((0, 0, 0), (0, 0, -1), (0, float("inf"), 0))]
        flagged = _abi.Camera.defaults()
        flagged.flags = 1
        res = _abi.Camera.defaults()
        res.reserved = 1
        for cam in bad + [flagged, res]:
            with pytest.raises(_abi.RtError) as e:
                sc.set_camera(cam)
            assert e.value.status == _abi.RT_ERR_BAD_ARG
            assert np.array_equal(sc.render_tile(rq)[0], want)
        with rt.FrameContext([0], rt.World(sph, tri)) as fc:
            with pytest.raises(_abi.RtError) as e:
                fc.set_camera(bad[0])
            assert e.value.status == _abi.RT_ERR_BAD_ARG
        # the sample range and request checks of the camera rays are the pass's
        for b, e_ in ((2, 2), (3, 1), (0, SPP + 1)):
            with pytest.raises(_abi.RtError) as e:
                sc.camera_rays(rq, b, e_)
            assert e.value.status == _abi.RT_ERR_BAD_ARG


def test_frame_context_camera(ndev):
    sph, tri = _world("rand1024")
    rq = _abi.default_request(width=W, height=H, divisions=DIV, spp=SPP, max_bounces=6, seed=0xC0FFEE)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        ref = np.concatenate([sc.render_tile(_request(k))[0] for k in range(DIV)])
        sc.set_camera(_cam(POSES["oblique_rolled"]))
        posed = np.concatenate([sc.render_tile(_request(k))[0] for k in range(DIV)])
        sc.set_camera(_cam(POSES["translated"]))
        moved = np.concatenate([sc.render_tile(_request(k))[0] for k in range(DIV)])
    assert not np.array_equal(ref, posed)
    with rt.FrameContext([0, 0], rt.World(sph, tri)) as fc:           # two entries on one device: the balanced assignments run
        img, fs = fc.render(rq)
        assert np.array_equal(img.reshape(-1), ref) and fs.assignment == 1
        img, fs = fc.render(rq)
        assert np.array_equal(img.reshape(-1), ref) and fs.assignment == 2
        fc.set_camera(_cam(POSES["oblique_rolled"]))
        img, fs = fc.render(rq)
        assert np.array_equal(img.reshape(-1), posed) and fs.assignment == 1      # a new pose: the snake assignment again
        img, fs = fc.render(rq)
        assert np.array_equal(img.reshape(-1), posed) and fs.assignment == 2
        fc.set_camera(_cam(POSES["oblique_rolled"]))                               # the same pose again keeps the costs
        img, fs = fc.render(rq)
        assert np.array_equal(img.reshape(-1), posed) and fs.assignment == 2
        fc.set_camera(_cam(POSES["translated"]))
        img, fs = fc.render(rq)
        assert np.array_equal(img.reshape(-1), moved) and fs.assignment == 1
        fc.set_camera(None)
        img, fs = fc.render(rq)
        assert np.array_equal(img.reshape(-1), ref) and fs.assignment == 1
        # the strip queue and the static split render the same posed frame
        fc.set_camera(_cam(POSES["oblique_rolled"]))
        for fl in (F.RT_FLAG_FRAME_QUEUE, F.RT_FLAG_FRAME_STATIC):
            r = rq.copy()
            r.flags = fl
            assert np.array_equal(fc.render(r)[0].reshape(-1), posed), fl


def test_example_render_posed(ndev, tmp_path):
    """examples/render_posed.c: a plain-C client that orbits c2 in a few frames through the frame context."""
    from ray_tracer_s8_amd import build
    exe = tmp_path / "render_posed"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "render_posed.c"),
                    "-o", str(exe), f"-L{build.LIB_PATH.parent}", "-lrt_s8", f"-Wl,-rpath,{build.LIB_PATH.parent}", "-lm"], check=True)
    r = subprocess.run([str(exe), "4", str(tmp_path / "orbit")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    frames = sorted(tmp_path.glob("orbit_*.ppm"))
    assert len(frames) == 4
    data = [f.read_bytes() for f in frames]
    assert len(set(data)) == 4                                       # every viewpoint its own image
    assert "assignment" in r.stdout
