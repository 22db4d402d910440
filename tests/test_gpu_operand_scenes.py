"""The directed operand corpus (tests/_operand_cases.py) as rays on scenes of ONE primitive: what tests/test_gpu_operands.py proves
of the device functions by themselves is tied here to the engines that inline them.  The records are grouped by primitive, the groups
that hold the exact-equality classes (disc == 0, |.| == 2, a root on a window end; det == +-eps, u == 0 / 1, u + v == 1) first; every
group's rays go through Scene.intersect (closest and any hit; default flags, RT_FLAG_NO_BVH_CULL, RT_FLAG_LINEAR_SCAN) — Ray::new's
direction — and through Scene.trace(as_given=True, max_bounces=0) — the direction bit for bit — against oracle.intersect_batch /
trace_batch, with the comparison helpers of tests/test_gpu_ray_fuzz.py.  Normalising a direction moves a record between classes, so
the groups are chosen, and every exact-equality class is counted (at least FLOOR records), under BOTH ray conventions."""
import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

import _operand_cases as OC
import _ray_cases as R
from test_gpu_ray_fuzz import _eq, check_closest

pytestmark = pytest.mark.gpu

NONE = _abi.RT_HIT_NONE
N_SCENES = 16
FLAG_SETS = (0, _abi.RT_FLAG_NO_BVH_CULL, _abi.RT_FLAG_LINEAR_SCAN)
SEED = 0x0BE5


def sphere_scenes():
    rec = OC.sphere_directed()
    given, new = OC.classify_sphere(rec, False), OC.classify_sphere(rec, True)
    both = {(k, n): c[k] for k in OC.SPHERE_EXACT for n, c in enumerate((given, new))}      # each class under each ray convention
    out = []
    for prim, idx in OC.primitive_groups(rec, [6, 7, 8, 9], both, tuple(both), N_SCENES):
        sph = np.zeros(1, _abi.SPHERE_DTYPE)
        sph["cx"], sph["cy"], sph["cz"], sph["radius"] = prim
        sph["albedo_r"], sph["albedo_g"], sph["albedo_b"], sph["roughness"], sph["emission"] = 0.75, 0.5, 0.25, 0.5, 2.0
        out.append((sph, None, rec[idx], rec[idx, 10], rec[idx, 11]))
    return out, rec, given, new


def triangle_scenes():
    rec = OC.triangle_directed()
    given, new = OC.classify_triangle(rec, False), OC.classify_triangle(rec, True)
    both = {(k, n): c[k] for k in OC.TRIANGLE_EXACT for n, c in enumerate((given, new))}
    out = []
    for prim, idx in OC.primitive_groups(rec, list(range(6, 15)), both, tuple(both), N_SCENES):
        tri = np.zeros(1, _abi.TRIANGLE_DTYPE)
        tri["a"], tri["b"], tri["c"] = prim[0:3], prim[3:6], prim[6:9]
        tri["albedo_r"], tri["albedo_g"], tri["albedo_b"], tri["roughness"], tri["emission"] = 0.25, 0.5, 0.75, 0.5, 2.0
        out.append((None, tri, rec[idx], rec[idx, 15], rec[idx, 16]))
    return out, rec, given, new


def covered(scenes, rec, classes, exact):
    """records of each exact-equality class among the scenes' rays (a record is found again by its words)"""
    words = {r.tobytes() for sc in scenes for r in np.ascontiguousarray(sc[2])}
    used = np.array([r.tobytes() in words for r in np.ascontiguousarray(rec)])
    return {k: int((classes[k] & used).sum()) for k in exact}


def run_scene(oracle, sph, tri, rec, t_min, t_max, what):
    rays = R.make_rays(rec[:, 0:3], rec[:, 3:6], t_min, t_max)
    o, d = R.od(rays)
    hits_n = 0
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        for flags in FLAG_SETS:
            backend = 0 if flags == _abi.RT_FLAG_NO_BVH_CULL else 1
            ref = oracle.intersect_batch(sph, tri, rays, backend=backend)
            hits, _ = sc.intersect(o, d, rays["t_min"], rays["t_max"], flags=flags)
            check_closest(hits, rays, ref, what + ("closest", flags))
            anyh, _ = sc.intersect(o, d, rays["t_min"], rays["t_max"], any_hit=True, flags=flags)
            got = anyh["index"] != NONE
            assert np.array_equal(got, ref["hit"]), (what, "any hit", flags, np.nonzero(got != ref["hit"])[0][:10], rays[got != ref["hit"]][:3])
            hits_n += int(ref["hit"].sum())
            want = oracle.trace_batch(sph, tri, rays, spp=1, max_bounces=0, backend=backend, ray_as_given=True, seed=SEED)
            rgb, segs, _ = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=0, seed=SEED, as_given=True, flags=flags)
            ok = np.all(_eq(rgb, want[0]), 1)
            assert ok.all(), (what, "trace rgb", flags, np.nonzero(~ok)[0][:5], rgb[~ok][:3], want[0][~ok][:3], rays[~ok][:3])
            assert np.array_equal(segs, want[1]), (what, "trace segments", flags)
    return hits_n, len(rays)


def test_directed_sphere_records_as_rays_on_one_sphere(ndev, oracle):
    scenes, rec, given, new = sphere_scenes()
    for name, c in (("as given", given), ("Ray::new", new)):
        cov = covered(scenes, rec, c, OC.SPHERE_EXACT)
        assert all(v >= OC.FLOOR for v in cov.values()), (name, cov)
    hits = rays = 0
    for i, (sph, tri, r, t0, t1) in enumerate(scenes):
        h, n = run_scene(oracle, sph, tri, r, t0, t1, ("sphere scene", i, sph[["cx", "cy", "cz", "radius"]].tolist()))
        hits, rays = hits + h, rays + n
    assert hits >= 1000 and 3 * rays - hits >= 1000, (hits, rays)


def test_directed_triangle_records_as_rays_on_one_triangle(ndev, oracle):
    scenes, rec, given, new = triangle_scenes()
    for name, c in (("as given", given), ("Ray::new", new)):
        cov = covered(scenes, rec, c, OC.TRIANGLE_EXACT)
        assert all(v >= OC.FLOOR for v in cov.values()), (name, cov)
    hits = rays = 0
    for i, (sph, tri, r, t0, t1) in enumerate(scenes):
        h, n = run_scene(oracle, sph, tri, r, t0, t1, ("triangle scene", i, tri[["a", "b", "c"]].tolist()))
        hits, rays = hits + h, rays + n
    assert hits >= 1000 and 3 * rays - hits >= 1000, (hits, rays)
