"""The variants of the LDS-tree kernels (ISECT 5 and 6; DESIGN.md 4.8 "round 5") render the oracle's bytes.

* the sphere-only instantiation the host picks for a world without triangles (rtplan::Plan::tris), against the general one forced
  by RT_LTREE_GENERAL, on a ragged 130 x 8 frame at 1, 3, 8 and 24 samples per pixel (grp > 1, one pixel per slot, the 24-unit
  slot); a world of spheres and triangles must keep the general kernel;
* the plain-frame copy of the commit (KParams::plain) against the launches that must not take it: an f32 plane, two progressive
  passes, RT_PLAIN_FRAME=0;
* the shapes at which a block of steps runs mostly at no walking lane — what an early exit from a block (measured and dropped in
  round 5, tools/experiments/r05_ltree_block_exit.patch) or an overlap of the tree's staging with the first units (not built) would
  have to get right: worlds whose walks end within two steps on frames of one tile, and a frame whose rays all run down the
  camera's axis — direction (+-0, +-0, -1), so every block is the SLOW variant.

Which variant a launch took is read back from RT_LAST_VARIANT (csrc/rt_api.hip: bit 0 sphere-only kernel, bit 1 plain frame).
Every comparison is a bit comparison; the references are computed once per module."""
import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes
from test_gpu_knobs import knobs
from test_gpu_progressive import _run_passes

pytestmark = pytest.mark.gpu

T, E = _abi.RT_FLAG_BVH_TRAVERSE, _abi.RT_FLAG_EXACT_NODES
# ISECT -> (engine, request flags)
ISECTS = {5: (4, T | E | _abi.RT_FLAG_NO_CULL_WALK), 6: (7, T | E | _abi.RT_FLAG_CULL_WALK)}
SPHERE_ONLY, PLAIN = 1, 2                      # bits of RT_LAST_VARIANT
GROUND = scenes._sph((0.0, -101.0, -6.0), 100.0, (0.5, 0.5, 0.5))


def _field(n, seed=0x17EE5):
    """n spheres: one large ground sphere and a field close in front of the camera (most primary rays hit something)."""
    return scenes._rand_field(n, seed, ((-4, 4), (-1, 3), (-9, -3)), (0.2, 0.6), GROUND)


def _worlds():
    axis = np.array([scenes._sph((0.0, 0.0, -4.0), 0.7, (0.8, 0.4, 0.3), 0.4)], dtype=_abi.SPHERE_DTYPE)
    two = np.array([scenes._sph((-0.6, 0.0, -3.0), 0.5, (0.8, 0.3, 0.3)), scenes._sph((0.7, 0.1, -3.5), 0.6, (0.3, 0.8, 0.3), 0.5)],
                   dtype=_abi.SPHERE_DTYPE)
    return {
        "spheres40": rt.World(_field(40)),
        "mixed": rt.World(_field(20), scenes.quad_room()[1][:12]),
        "one": rt.World(scenes.single_sphere()),
        "two": rt.World(two),
        "axis": rt.World(np.concatenate([_field(40), axis])),
    }


WORLDS = _worlds()


def _rq(w, h, spp, flags, div=1, no=0, **kw):
    kw.setdefault("fov", 0.1)                  # (frames a few rows high are very wide: a narrow view keeps the rays on the spheres)
    return _abi.default_request(width=w, height=h, divisions=div, division_no=no, spp=spp, max_bounces=4, seed=0x51AB, flags=flags, **kw)


@pytest.fixture(scope="module")
def want(oracle):
    """want(world name, request) -> the oracle's (rgb, f32, ray segments), computed once per (world, frame) and read-only."""
    cache = {}

    def get(name, rq):
        key = (name, rq.width, rq.height, rq.divisions, rq.division_no, rq.spp, rq.fov, rq.aperture)
        if key not in cache:
            w = WORLDS[name]
            rgb, f32, info = oracle.render(rq, w.spheres if len(w.spheres) else None, w.triangles if len(w.triangles) else None,
                                           backend=1, want_f32=True)
            rgb.setflags(write=False)
            f32.setflags(write=False)
            cache[key] = (rgb, f32, info["ray_segments"])
        return cache[key]

    return get


def _bits(a):
    return np.asarray(a).view(np.uint32)


def _render(sc, rq, want_f32=False):
    """One strip; returns (rgb, f32, stats, RT_LAST_VARIANT of its launch)."""
    _abi.debug_set("RT_LAST_VARIANT", 0)
    rgb, f32, st = sc.render_tile(rq, want_f32=want_f32)
    return rgb, f32, st, _abi.debug_set("RT_LAST_VARIANT", 0)


@pytest.mark.parametrize("spp", [1, 3, 8, 24])
@pytest.mark.parametrize("isect", list(ISECTS))
def test_sphere_only_kernel_against_the_general_one(ndev, want, isect, spp):
    engine, flags = ISECTS[isect]
    rq = _rq(130, 8, spp, flags)
    ref, ref_f, ref_segs = want("spheres40", rq)
    with _abi.debug_library():
        rt.init()
        with rt.Scene(0, WORLDS["spheres40"]) as sc:
            rgb, _, st, v = _render(sc, rq)
            with knobs({"RT_LTREE_GENERAL": 1}):
                rgb_g, _, st_g, v_g = _render(sc, rq)
                _, f32_g, _, _ = _render(sc, rq, want_f32=True)
            _, f32, _, _ = _render(sc, rq, want_f32=True)
    assert st.engine == st_g.engine == engine
    assert v & SPHERE_ONLY and not v_g & SPHERE_ONLY, (v, v_g)
    assert bool(v & PLAIN) == (spp == 8) and bool(v_g & PLAIN) == (spp == 8), (v, v_g)       # (24: not a power of two)
    assert np.array_equal(rgb, ref), f"sphere-only: {int((rgb != ref).sum())} RGB8 bytes differ"
    assert np.array_equal(rgb_g, ref), f"general: {int((rgb_g != ref).sum())} RGB8 bytes differ"
    assert np.array_equal(_bits(f32), _bits(ref_f)) and np.array_equal(_bits(f32_g), _bits(ref_f))
    assert st.ray_segments == st_g.ray_segments == ref_segs


def test_mixed_world_keeps_the_general_kernel(ndev, want):
    with _abi.debug_library():
        rt.init()
        with rt.Scene(0, WORLDS["mixed"]) as sc:
            for isect, (engine, flags) in ISECTS.items():
                rq = _rq(130, 8, 8, flags)
                ref, ref_f, ref_segs = want("mixed", rq)
                rgb, _, st, v = _render(sc, rq)
                _, f32, _, _ = _render(sc, rq, want_f32=True)
                assert st.engine in (4, 7), st.engine                    # (the culled walk needs every triangle within its bound)
                assert not v & SPHERE_ONLY, (isect, v)
                assert np.array_equal(rgb, ref), f"ISECT {isect}: {int((rgb != ref).sum())} RGB8 bytes differ"
                assert np.array_equal(_bits(f32), _bits(ref_f)) and st.ray_segments == ref_segs


@pytest.mark.parametrize("isect", list(ISECTS))
def test_plain_frame_commit_against_the_general_one(ndev, want, isect):
    engine, flags = ISECTS[isect]
    rq = _rq(130, 8, 8, flags)
    ref, ref_f, ref_segs = want("spheres40", rq)
    with _abi.debug_library():
        rt.init()
        with rt.Scene(0, WORLDS["spheres40"]) as sc:
            rgb, _, st, v = _render(sc, rq)
            rgb_f, f32, st_f, v_f = _render(sc, rq, want_f32=True)
            _abi.debug_set("RT_LAST_VARIANT", 0)
            rgb_p, f32_p, acc, segs_p, st_p = _run_passes(sc, rq, [(0, 3), (3, 8)])
            v_p = _abi.debug_set("RT_LAST_VARIANT", 0)
            with knobs({"RT_PLAIN_FRAME": 0}):
                rgb_0, _, st_0, v_0 = _render(sc, rq)
    assert st.engine == st_f.engine == st_p.engine == st_0.engine == engine
    assert v & PLAIN and not v_f & PLAIN and not v_p & PLAIN and not v_0 & PLAIN, (v, v_f, v_p, v_0)
    for what, got in (("plain", rgb), ("f32 plane", rgb_f), ("two passes", rgb_p), ("RT_PLAIN_FRAME=0", rgb_0)):
        assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} RGB8 bytes differ"
    assert np.array_equal(_bits(f32), _bits(ref_f)) and np.array_equal(_bits(f32_p), _bits(ref_f))
    # the running sum the last pass handed back is the one the image is the mean of
    assert np.array_equal(_bits(f32_p), _bits(np.sqrt(acc.reshape(-1) / np.float32(8))))
    assert st.ray_segments == st_f.ray_segments == segs_p == st_0.ray_segments == ref_segs


@pytest.mark.parametrize("isect", list(ISECTS))
def test_short_walks_on_one_tile(ndev, want, isect):
    """Walks of at most two steps (one sphere: a single leaf, no tree to stage — such a world takes another engine, rendered all the
    same; two spheres: one node) on frames of ONE tile, where the first walk follows the first acquisition at once: the literal
    64 x 1 frame (its v_den is 0: the oracle's arithmetic either way) and the top strip of a 64 x 2 frame."""
    engine, flags = ISECTS[isect]
    with _abi.debug_library():
        rt.init()
        for name in ("one", "two"):
            with rt.Scene(0, WORLDS[name]) as sc:
                for rq in (_rq(64, 1, 1, flags), _rq(64, 2, 1, flags, div=2, no=0, fov=0.03), _rq(64, 2, 8, flags, div=2, no=1, fov=0.03)):
                    ref, ref_f, ref_segs = want(name, rq)
                    rgb, f32, st, v = _render(sc, rq, want_f32=True)
                    if name == "two":
                        assert st.engine == engine and v & SPHERE_ONLY, (st.engine, v)
                    assert np.array_equal(rgb, ref), f"{name} {rq.width}x{rq.height}: {int((rgb != ref).sum())} RGB8 bytes differ"
                    assert np.array_equal(_bits(f32), _bits(ref_f)) and st.ray_segments == ref_segs


@pytest.mark.parametrize("isect", list(ISECTS))
def test_rays_down_the_camera_axis_walk_the_slow_step(ndev, want, isect):
    """fov 0, aperture 0: every camera ray is (+-0, +-0, -1) — two inverse direction components are infinite, so every block of
    steps of the first segments is the SLOW variant; the bounces off the sphere on the axis walk the fast one."""
    engine, flags = ISECTS[isect]
    rq = _rq(130, 8, 3, flags, fov=0.0, aperture=0.0)
    ref, ref_f, ref_segs = want("axis", rq)
    with _abi.debug_library():
        rt.init()
        with rt.Scene(0, WORLDS["axis"]) as sc:
            rgb, f32, st, v = _render(sc, rq, want_f32=True)
    assert st.engine == engine and v & SPHERE_ONLY
    assert ref_segs > 130 * 8 * 3 and ref.std() > 0.0                  # (the rays hit the sphere and bounce)
    assert np.array_equal(rgb, ref), f"{int((rgb != ref).sum())} RGB8 bytes differ"
    assert np.array_equal(_bits(f32), _bits(ref_f)) and st.ray_segments == ref_segs
