"""The LDS-tree kernels (ISECT 5 and 6) after round 6 render the oracle's bytes and count its ray segments.

Round 6 moved instructions of the closest-hit loop without touching an IEEE operation: the first step of a block stays inside its
variant (slow / fast), the stack top, the list's end and its head live as LDS addresses from the query's start to its last root
test, the head of a block forms its wave-uniform inputs once per round and the walking lanes from the reference, and the stack
pointer's step is a sum of two selects.  (Measured and dropped, but what the cases were also chosen for: the child reference selected
from the halves of the node's reference word, and a copy of the unit acquisition for plain frames with shifts where the divisions
were.)  The cases are the shapes at which one of these can go wrong:

* 70 x 3 pixels (70 is no multiple of 64: a short last tile and a ragged slot), 40 random spheres and the ground, depth 8, at 8
  samples per pixel (plain; most blocks are fast blocks, entered at their first and at their later steps), at 3 and 12 (not plain:
  the general acquisition and commit), at 16 (plain, another shift), and at 8 through the pass entry point with s_begin > 0 (not
  plain);
* the camera's rays running exactly down -z from the origin (fov 0, aperture 0: direction components +-0, so the wave takes the SLOW
  block, whose first step moved as well);
* 24 spheres piled on one centre with radii 1.00 ... 1.23, 64 x 1 pixels, depth 2: a lane's leaf list passes maxl - STEPS in
  mid-walk, so flush() runs between two blocks — on the list's addresses now;
* 2 spheres, 64 x 1 pixels, depth 1: the smallest tree, one internal node, where node DONE and the NaN field are reached from the
  first step of the first block.

Every case is rendered by both engines, each through its sphere-only and (RT_LTREE_GENERAL) its general instantiation.  Every
comparison is a bit comparison; the references are computed once per module."""
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


def _worlds():
    field = scenes._rand_field(41, 0x6A11, ((-4, 4), (-1, 3), (-9, -3)), (0.2, 0.6), GROUND)      # 40 spheres and the ground
    axis = np.array([scenes._sph((0.0, 0.0, -4.0), 0.7, (0.8, 0.4, 0.3), 0.4)], dtype=_abi.SPHERE_DTYPE)
    pile = np.array([scenes._sph((0.0, 0.0, -4.0), 1.0 + 0.01 * i, (0.3 + 0.02 * i, 0.5, 0.9 - 0.02 * i), 0.1 * (i % 3))
                     for i in range(24)], dtype=_abi.SPHERE_DTYPE)
    two = np.array([scenes._sph((-0.6, 0.0, -3.0), 0.5, (0.8, 0.3, 0.3)), scenes._sph((0.7, 0.1, -3.5), 0.6, (0.3, 0.8, 0.3), 0.5)],
                   dtype=_abi.SPHERE_DTYPE)
    return {"field": rt.World(field), "axis": rt.World(np.concatenate([field, axis])), "pile": rt.World(pile), "two": rt.World(two)}


WORLDS = _worlds()


def _rq(w, h, spp, depth, flags, **kw):
    kw.setdefault("fov", 0.1)                  # (frames a few rows high are very wide: a narrow view keeps the rays on the spheres)
    kw.setdefault("divisions", 1)
    return _abi.default_request(width=w, height=h, division_no=0, spp=spp, max_bounces=depth, seed=0x6B0B, flags=flags, **kw)


def _rq_one_row(spp, depth, flags):
    """64 x 1 pixels: the top strip of a 64 x 2 frame (a frame one row high has v_den 0 and no ray that hits anything)."""
    return _rq(64, 2, spp, depth, flags, divisions=2, fov=0.01)


@pytest.fixture(scope="module")
def want(oracle):
    """want(world name, request) -> the oracle's (rgb, ray segments), computed once per (world, frame) and read-only."""
    cache = {}

    def get(name, rq):
        key = (name, rq.width, rq.height, rq.divisions, rq.spp, rq.max_bounces, rq.fov, rq.aperture)
        if key not in cache:
            rgb, info = oracle.render(rq, WORLDS[name].spheres, None, backend=1)[::2]
            rgb.setflags(write=False)
            cache[key] = (rgb, info["ray_segments"])
        return cache[key]

    return get


def _render(sc, rq):
    """One strip; returns (rgb, stats, RT_LAST_VARIANT of its launch)."""
    _abi.debug_set("RT_LAST_VARIANT", 0)
    rgb, _, st = sc.render_tile(rq)
    return rgb, st, _abi.debug_set("RT_LAST_VARIANT", 0)


def _both_instantiations(name, rq, engine, want, plain, passes=None):
    """The frame through the sphere-only and the general instantiation of one engine, against the oracle."""
    ref, ref_segs = want(name, rq)
    with _abi.debug_library():
        rt.init()
        with rt.Scene(0, WORLDS[name]) as sc:
            for general in (0, 1):
                with knobs({"RT_LTREE_GENERAL": general}):
                    if passes is None:
                        rgb, st, v = _render(sc, rq)
                        segs = st.ray_segments
                    else:
                        _abi.debug_set("RT_LAST_VARIANT", 0)
                        rgb, _, _, segs, st = _run_passes(sc, rq, passes, want_f32=False)
                        v = _abi.debug_set("RT_LAST_VARIANT", 0)
                what = f"{name} {rq.width}x{rq.height // rq.divisions} spp {rq.spp}, {'general' if general else 'sphere-only'} kernel"
                assert st.engine == engine, (what, st.engine)
                assert bool(v & SPHERE_ONLY) == (not general) and bool(v & PLAIN) == plain, (what, v)
                assert np.array_equal(rgb, ref), f"{what}: {int((rgb != ref).sum())} RGB8 bytes differ"
                assert segs == ref_segs, (what, segs, ref_segs)
    return ref, ref_segs


@pytest.mark.parametrize("spp", [3, 8, 12, 16])
@pytest.mark.parametrize("isect", list(ISECTS))
def test_ragged_frame_plain_and_general_acquisition(ndev, want, isect, spp):
    engine, flags = ISECTS[isect]
    ref, segs = _both_instantiations("field", _rq(70, 3, spp, 8, flags), engine, want, plain=spp in (8, 16))
    assert 2 * segs > 3 * 70 * 3 * spp and ref.std() > 1.0        # (more than half of the rays hit and bounce: the walks are real ones)


@pytest.mark.parametrize("isect", list(ISECTS))
def test_ragged_frame_through_a_later_pass(ndev, want, isect):
    """Samples 0-2, then 3-7 through the pass entry point: s_begin > 0 and a running sum in and out, so neither launch is plain."""
    engine, flags = ISECTS[isect]
    _both_instantiations("field", _rq(70, 3, 8, 8, flags), engine, want, plain=False, passes=[(0, 3), (3, 8)])


@pytest.mark.parametrize("isect", list(ISECTS))
def test_rays_down_minus_z_take_the_slow_block(ndev, want, isect):
    engine, flags = ISECTS[isect]
    ref, segs = _both_instantiations("axis", _rq(70, 3, 8, 8, flags, fov=0.0, aperture=0.0), engine, want, plain=True)
    assert segs > 70 * 3 * 8 and ref.std() > 0.0                  # (the rays hit the sphere on the axis and bounce)


@pytest.mark.parametrize("isect", list(ISECTS))
def test_pile_fills_the_leaf_list_in_mid_walk(ndev, want, isect):
    """Every ray through the pile reaches the 24 concentric spheres' leaves one after the other: more candidates than the list
    holds less a block of appends (at most 16 - 8), so the list is flushed between two blocks of the same walk."""
    engine, flags = ISECTS[isect]
    ref, segs = _both_instantiations("pile", _rq_one_row(8, 2, flags), engine, want, plain=True)
    assert segs > 64 * 8 and ref.std() > 0.0


@pytest.mark.parametrize("isect", list(ISECTS))
def test_smallest_tree(ndev, want, isect):
    engine, flags = ISECTS[isect]
    ref, segs = _both_instantiations("two", _rq_one_row(8, 1, flags), engine, want, plain=True)
    assert segs > 64 * 8 and ref.std() > 0.0
