"""The batch forms of the ray oracle (oracle.intersect_batch, oracle.trace_batch: the scene and its BVH built once, the rays spread
over threads) pinned on the CPU, bit for bit:
1. against the single-ray oracle (oracle.intersect, oracle.ray_color) on the ray sets of the GPU query and trace tests;
2. under BVH semantics against the tile oracle: the camera rays of a strip traced as given compose to oracle.render's f32 image and
   segment count — the per-ray oracle for path tracing under backend 1 that did not exist before;
3. world_index against the arrays reordered by hand; ray_as_given against Ray::new of a pre-image; 1 thread against all threads;
   the closest hit against the independent numpy restatement (oracle/restate_np.py);
4. the conditions of the GPU fuzz's default case set that span cases (tests/test_gpu_ray_fuzz.py), from the oracle alone;
5. the plan arithmetic: no legal input reaches the 64-lane trace workgroup."""
import numpy as np
import pytest

from ray_tracer_s8_amd import _abi, scenes

import _ray_cases as R
from _world_cases import tie_world
from test_gpu_aov import _camera_samples, _preimage
from test_gpu_aov import _strip_request as _aov_request
from test_gpu_fuzz import _random_case, _world_order
from test_gpu_query import CONFIGS, SCENES, _adversarial_rays, _bounce_rays, _camera_rays, _oracle_hits, _world
from test_gpu_trace import SETTINGS, _oracle_trace, _random_rays, _same_bits, _states, _strip_rays

NO_TRI = np.zeros(0, _abi.TRIANGLE_DTYPE)
FLOATS = ("point", "normal", "albedo", "roughness", "emission")


def _bits_equal(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)) for k in FLOATS) \
        and np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["index"], b["index"])


def _check_against_single(batch, single, what):
    assert len(single) == len(batch["hit"])
    for i, e in enumerate(single):
        if e is None:
            assert not batch["hit"][i] and batch["index"][i] == R.NONE, (what, i)
            assert all(np.all(np.asarray(batch[k][i]).view(np.uint32) == 0) for k in FLOATS), (what, i)
            continue
        assert batch["hit"][i] and batch["index"][i] == e["index"], (what, i, batch["index"][i], e["index"])
        for k in ("point", "normal", "albedo"):
            assert _same_bits(batch[k][i], e[k]), (what, i, k)
        for k in ("roughness", "emission"):
            assert _same_bits(batch[k][i], np.float32(e[k])), (what, i, k)


def _query_rays(oracle, name):
    """The ray set of test_gpu_query.ray_sets for one scene: camera, bounce and adversarial rays."""
    sph, tri = _world(name)
    w, h = (16, 9) if name == "field9000" else (32, 18)
    cam = _camera_rays(oracle, w, h)
    cam_ref = _oracle_hits(oracle, sph, tri, cam, 1)
    bounce = _bounce_rays(cam_ref, cam, seed=len(name))
    adv = _adversarial_rays(sph, tri if tri is not None else NO_TRI)
    return sph, tri, np.concatenate([cam, bounce, adv]), cam_ref


@pytest.mark.parametrize("scene", SCENES)
def test_intersect_batch_equals_the_single_ray_oracle(oracle, scene):
    sph, tri, rays, cam_ref = _query_rays(oracle, scene)
    for backend in (0, 1):
        single = _oracle_hits(oracle, sph, tri, rays[len(cam_ref):], backend)
        single = (cam_ref if backend == 1 else _oracle_hits(oracle, sph, tri, rays[:len(cam_ref)], 0)) + single
        batch = oracle.intersect_batch(sph, tri, rays, backend=backend)
        _check_against_single(batch, single, (scene, backend))
        assert any(e is not None for e in single) and any(e is None for e in single)


@pytest.mark.parametrize("scene", SCENES)
def test_trace_batch_equals_the_single_ray_trace(oracle, scene):
    """Backend 0, the ray set of test_gpu_trace.ray_sets, its SETTINGS, both RNG forms."""
    sph, tri = _world(scene)
    rays = np.concatenate([_camera_rays(oracle, 8, 5), _random_rays(sph, tri, 40, seed=len(scene)),
                           _adversarial_rays(sph, tri if tri is not None else NO_TRI)])
    for mb, spp in SETTINGS:
        st0 = _states(len(rays), mb * 7 + spp)
        ergb, esegs, est = _oracle_trace(oracle, sph, tri, rays, spp, mb, states=st0)
        rgb, segs, st1 = oracle.trace_batch(sph, tri, rays, spp=spp, max_bounces=mb, states=st0)
        assert _same_bits(rgb, ergb) and np.array_equal(segs, esegs) and np.array_equal(st1, est), (scene, mb, spp)
        seed = 0xDEADBEEF12345678 + len(scene)
        ergb, esegs, _ = _oracle_trace(oracle, sph, tri, rays, spp, mb, seed=seed)
        rgb, segs, none = oracle.trace_batch(sph, tri, rays, spp=spp, max_bounces=mb, seed=seed)
        assert _same_bits(rgb, ergb) and np.array_equal(segs, esegs) and none is None, (scene, mb, spp, "seeded")
    assert np.any(esegs > 1)


def _permuted_world():
    """A _world_order-style world: the first case of test_gpu_fuzz with a permuted world, duplicates and at least 30 primitives."""
    for i in range(1, 400, 3):
        sph, tri, _, _ = _random_case(i)
        if len(sph) + len(tri) >= 30:
            sph, tri, wi = _world_order(i, sph, tri)
            assert wi is not None and R.duplicated(sph, tri)
            return sph, tri, wi
    raise AssertionError("no such case")


def _compose_world(name):
    if name == "permuted":
        return _permuted_world()
    sph, tri = _world(name)
    return sph, tri, None


@pytest.mark.parametrize("scene", ["cornell16", "rand1024", "quad_room", "tie_world", "permuted"])
@pytest.mark.parametrize("backend", [1, 0])
def test_trace_batch_composes_to_the_tile_oracle(oracle, scene, backend):
    """The camera rays of a strip (oracle.camera_ray, the state after get_ray), traced as given with spp = 1, summed per pixel in
    sample order: sqrt(sum / spp) is oracle.render's f32 image, and the segments add up to its count."""
    sph, tri, wi = _compose_world(scene)
    rq = _abi.default_request(width=24, height=16, divisions=2, division_no=1, spp=3, max_bounces=10, seed=0x7AC3)
    _, ref_f, info = oracle.render(rq, sph if len(sph) else None, tri if tri is not None and len(tri) else None, backend=backend,
                                   want_f32=True, world_index=wi)
    o, d, st0 = _strip_rays(oracle, rq)
    rays = R.make_rays(o, d, rq.t_min, rq.t_max)
    rgb, segs, _ = oracle.trace_batch(sph, tri, rays, spp=1, max_bounces=rq.max_bounces, backend=backend, world_index=wi,
                                      ray_as_given=True, states=st0)
    hs, S = rq.height // rq.divisions, rq.spp
    per = rgb.reshape(hs, rq.width, S, 3)
    total = np.zeros((hs, rq.width, 3), np.float32)
    for s in range(S):
        total = (total + per[:, :, s, :]).astype(np.float32)
    img = np.sqrt((total / np.float32(S)).astype(np.float32)).astype(np.float32)
    assert _same_bits(img.reshape(-1), ref_f), (scene, backend)
    assert int(segs.sum()) == info["ray_segments"]
    assert np.any(segs > 1)


def test_backends_differ_where_the_order_decides(oracle):
    """The permuted world with duplicates: the plain scan and the BVH semantics pick different copies for some ray, so the
    composition above under backend 1 could not pass with backend 0's hits."""
    sph, tri, wi = _permuted_world()
    g = np.random.default_rng(3)
    rays, _, _ = R.ray_population(oracle, g, sph, tri, 512, wi, aim_at=R.duplicated(sph, tri))
    a = oracle.intersect_batch(sph, tri, rays, backend=0, world_index=wi)
    b = oracle.intersect_batch(sph, tri, rays, backend=1, world_index=wi)
    assert np.any(a["index"] != b["index"])


@pytest.mark.parametrize("kind", ["spheres", "triangles"])
def test_world_index_equals_the_arrays_reordered_by_hand(oracle, kind):
    if kind == "spheres":
        arr = np.concatenate([scenes.cornell16(), tie_world(with_tris=False)[0]])
    else:
        arr = np.concatenate([scenes.tri_terrain()[1], tie_world()[1]])
    n = len(arr)
    perm = np.random.default_rng(5).permutation(n).astype(np.uint32)
    reordered = np.empty_like(arr)
    reordered[perm] = arr                                         # primitive i stands at world position perm[i]
    sph, tri = (arr, None) if kind == "spheres" else (None, arr)
    rs, rt_ = (reordered, None) if kind == "spheres" else (None, reordered)
    rays = np.concatenate([_camera_rays(oracle, 24, 14), _adversarial_rays(arr if kind == "spheres" else np.zeros(0, _abi.SPHERE_DTYPE),
                                                                          arr if kind == "triangles" else NO_TRI)])
    st0 = _states(len(rays), 17)
    for backend in (0, 1):
        a = oracle.intersect_batch(sph, tri, rays, backend=backend, world_index=perm)
        b = oracle.intersect_batch(rs, rt_, rays, backend=backend)
        assert _bits_equal(a, b), (kind, backend)                 # the index is the position in the world
        assert a["hit"].any() and not a["hit"].all()
        ta = oracle.trace_batch(sph, tri, rays, spp=2, max_bounces=10, backend=backend, world_index=perm, states=st0)
        tb = oracle.trace_batch(rs, rt_, rays, spp=2, max_bounces=10, backend=backend, states=st0)
        assert _same_bits(ta[0], tb[0]) and np.array_equal(ta[1], tb[1]) and np.array_equal(ta[2], tb[2]), (kind, backend)
    with pytest.raises(ValueError):
        oracle.intersect_batch(sph, tri, rays, world_index=np.zeros(n, np.uint32))


@pytest.mark.parametrize("scene", ["cornell16", "quad_room", "terrain"])
def test_ray_as_given_equals_ray_new_of_a_preimage(oracle, scene):
    sph, tri = _world(scene)
    rq = _aov_request()
    o, d = _camera_samples(oracle, rq)
    given = R.make_rays(o, d, rq.t_min, rq.t_max)
    pre = R.make_rays(o, _preimage(d), rq.t_min, rq.t_max)
    for backend in (0, 1):
        a = oracle.intersect_batch(sph, tri, given, backend=backend, ray_as_given=True)
        b = oracle.intersect_batch(sph, tri, pre, backend=backend)
        assert _bits_equal(a, b) and a["hit"].any(), (scene, backend)
        st0 = _states(len(given), 5)
        ta = oracle.trace_batch(sph, tri, given, spp=1, max_bounces=6, backend=backend, ray_as_given=True, states=st0)
        tb = oracle.trace_batch(sph, tri, pre, spp=1, max_bounces=6, backend=backend, states=st0)
        assert _same_bits(ta[0], tb[0]) and np.array_equal(ta[1], tb[1]) and np.array_equal(ta[2], tb[2])
    # a direction that is NOT unit length is taken as it is: the hit point moves along it by t times its length
    far = R.make_rays([(0, 0, 0)], [(0, 0, -2)], 0.001, 1000.0)
    one = scenes.single_sphere()
    a = oracle.intersect_batch(one, None, far, ray_as_given=True)
    b = oracle.intersect_batch(one, None, far)
    assert a["hit"][0] and b["hit"][0] and not np.array_equal(a["point"], b["point"])


def test_the_result_does_not_depend_on_the_thread_count(oracle):
    sph, tri, wi = _permuted_world()
    g = np.random.default_rng(8)
    rays, _, _ = R.ray_population(oracle, g, sph, tri, 1000, wi)
    st0 = _states(len(rays), 3)
    for backend in (0, 1):
        ref = oracle.intersect_batch(sph, tri, rays, backend=backend, world_index=wi, nthreads=1)
        tref = oracle.trace_batch(sph, tri, rays, spp=3, max_bounces=25, backend=backend, world_index=wi, states=st0, nthreads=1)
        sref = oracle.trace_batch(sph, tri, rays, spp=3, max_bounces=25, backend=backend, world_index=wi, seed=77, nthreads=1)
        for nthreads in (0, 3, 64):
            got = oracle.intersect_batch(sph, tri, rays, backend=backend, world_index=wi, nthreads=nthreads)
            assert all(got[k].tobytes() == ref[k].tobytes() for k in ref), (backend, nthreads)
            t = oracle.trace_batch(sph, tri, rays, spp=3, max_bounces=25, backend=backend, world_index=wi, states=st0, nthreads=nthreads)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(t, tref)), (backend, nthreads)
            s = oracle.trace_batch(sph, tri, rays, spp=3, max_bounces=25, backend=backend, world_index=wi, seed=77, nthreads=nthreads)
            assert s[0].tobytes() == sref[0].tobytes() and s[1].tobytes() == sref[1].tobytes()
    assert np.array_equal(st0, _states(len(rays), 3))            # the caller's states are not written


def test_intersect_batch_equals_the_numpy_restatement(oracle):
    """oracle/restate_np.py (independent of the C++ oracle): World.intersect in world order = backend 0, ray by ray."""
    from oracle import restate_np as rs
    sph, tri = _world("quad_room")
    wi = np.random.default_rng(2).permutation(len(sph) + len(tri)).astype(np.uint32)
    g = np.random.default_rng(4)
    rays, _, _ = R.ray_population(oracle, g, sph, tri, 160, wi)
    batch = oracle.intersect_batch(sph, tri, rays, backend=0, world_index=wi)
    world = rs.World(sph, tri, world_index=wi)
    n_hit = 0
    with np.errstate(all="ignore"):
        for i, r in enumerate(rays):
            world.t_min, world.t_max = np.float32(r["t_min"]), np.float32(r["t_max"])
            o, d = rs.ray_new(tuple(np.float32(r[k]) for k in ("ox", "oy", "oz")), tuple(np.float32(r[k]) for k in ("dx", "dy", "dz")))
            e = world.intersect(o, d)
            assert (e is not None) == bool(batch["hit"][i]), i
            if e is None:
                continue
            n_hit += 1
            p, nrm, alb, rough, emis = e
            assert _same_bits(np.array(p, np.float32), batch["point"][i]) and _same_bits(np.array(nrm, np.float32), batch["normal"][i]), i
            assert _same_bits(np.array(alb, np.float32), batch["albedo"][i]), i
            assert _same_bits(np.float32(rough), batch["roughness"][i]) and _same_bits(np.float32(emis), batch["emission"][i]), i
    assert 10 < n_hit < len(rays) - 10


# ---------------------------------------------------------------- the GPU fuzz's default case set, from the oracle alone
def test_every_config_is_used_by_the_default_case_set():
    import test_gpu_ray_fuzz as fz
    used = [R.case_config(kind, i) for kind, n in (("small", fz.N_SMALL), ("big", fz.N_BIG), ("mixed", fz.N_MIXED)) for i in range(n)]
    if (fz.N_SMALL, fz.N_BIG, fz.N_MIXED) == fz.DEFAULT_COUNTS:
        for cfg in CONFIGS:
            assert used.count(cfg) >= 3, (cfg, used.count(cfg))
    assert set(R.CONFIG_NAMES) == set(CONFIGS)
    # every config meets every scene size of the small generator's draw
    sizes = {}
    for i in range(fz.DEFAULT_COUNTS[0]):
        sph, tri, _, _ = R.case_scene("small", i)
        sizes.setdefault(R.case_config("small", i), set()).add(len(sph) + len(tri) > 100)
    assert all(v == {True, False} for v in sizes.values()), sizes


def test_the_backends_disagree_somewhere_in_the_default_case_set(oracle):
    """Over the permuted cases of the default set, the plain scan and the BVH semantics pick different primitives for some ray:
    the adversarial population is not too tame to tell a kernel with the wrong tie rule from a right one."""
    import test_gpu_ray_fuzz as fz
    differ = 0
    for i in range(1, fz.DEFAULT_COUNTS[0], 3):
        c = R.fuzz_case(oracle, "small", i, CONFIGS)
        if c["wi"] is None:
            continue
        other = oracle.intersect_batch(c["sph"], c["tri"], c["rays"], backend=1 - c["backend"], world_index=c["wi"])
        differ += int(np.sum(other["index"] != c["hits"]["index"]))
    assert differ > 0


def test_no_legal_input_takes_the_64_lane_trace_workgroup():
    """plan_trace over the whole legal range (tree depth 0 .. TRAV_STACK, 0 .. RT_MAX_BOUNCES, both path widths, walk and scan): a
    lane needs at most (64 + 63) x 4 = 508 bytes and 2 x 508 x 128 < 160 KiB, so the 64-lane entry of TRACE_BLOCKS is a guard for
    larger limits, not a branch a scene can reach; the 128-lane one is reached, and two workgroups always share a CU."""
    top = R.trav_stack()
    blocks = set()
    for n_sph in (1, 65536, 65537):
        for depth in range(0, top + 1):
            for mb in range(0, _abi.RT_MAX_BOUNCES + 1):
                for flags in (0, _abi.RT_FLAG_EXACT_SCAN):
                    p = R.trace_plan(n_sph, 0, depth, False, flags, mb)
                    blocks.add(p["block"])
                    assert 2 * p["lds"] <= 160 * 1024
    assert blocks == {256, 128}
