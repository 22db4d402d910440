"""The camera corpus on the CPU (tests/_camera_cases.py):
1. every case has the class it is named for — the kinds of the two squared lengths its records normalise, and its NaN directions —
   so that the device tests of tests/test_gpu_camera_extremes.py reach what they are meant to reach;
2. every (request, pose) of the corpus through the host planner (csrc/rt_plan.h, the g++ harness of tests/test_camera_plan.py) gives
   the restatement's camera vectors bit for bit;
3. make_pose refuses a pose exactly where the restatement's basis does, on both sides of the underflow and the overflow of the two
   squared lengths it divides by;
4. without a pose the restatement's rays are the oracle's camera_ray."""
import numpy as np
import pytest

from ray_tracer_s8_amd import _abi

import _camera_cases as cc
import _camera_np as cnp
from test_camera_plan import SCALARS, VECS, _host, lib  # noqa: F401  (lib: the fixture that builds the harness)

CASES = {c[0]: c for c in cc.CASES}
ALL_GEOMETRY = cc.GEOMETRY + [cc.WIDE] + cc.COUNTS


def _dirs(rays):
    return np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)


# ------------------------------------------------------------------------------------------------------------------ 1. classes


@pytest.mark.parametrize("name", CASES)
def test_case_has_its_class(oracle, name):
    _, knobs, pose, cls = CASES[name]
    rq = cc.request(knobs)
    rays, states, dots = cc.restated(oracle, rq, pose)
    n = (rq.height // rq.divisions) * rq.width * rq.spp
    assert len(rays) == n == sum(cls["dot1"].values()) == sum(cls["dot2"].values())
    got = dict(dot1=cc.kinds(dots[:, 0]), dot2=cc.kinds(dots[:, 1]), nan=int(np.isnan(_dirs(rays)).any(1).sum()))
    assert got == cls, (name, got, cls)
    # a mixed case has both of its kinds in one aligned run of 64 records, a wave (for a fast-path kind and another: a wave whose
    # ballot in sqrt_rn is not uniform)
    for stage, pair in cc.MIXED.get(name, {}).items():
        m = cc.kind_masks(dots[:, ("dot1", "dot2").index(stage)])
        a, b = (m[:, cc.KINDS.index(k)] for k in pair)
        assert any(a[i:i + 64].any() and b[i:i + 64].any() for i in range(0, n, 64)), (name, stage, pair)
    if cls["nan"] == 0:
        # (a cap, not a tolerance) and the rays are not all one ray
        assert not np.isnan(_dirs(rays)).any()
        assert len(np.unique(_dirs(rays).view(np.uint32), axis=0)) >= n // 2, name
    # the states are the draws' only: they do not depend on the camera
    plain = cc.restated(oracle, cc.request({k: v for k, v in knobs.items() if k in ("width", "height", "divisions", "division_no")}),
                        cc.P0)[1]
    assert np.array_equal(states, plain)


def test_mixed_cases_are_in_the_corpus():
    assert set(cc.MIXED) <= set(CASES) and len(CASES) == len(cc.CASES)


@pytest.mark.parametrize("name", [g[0] for g in ALL_GEOMETRY if g is not cc.WIDE])
def test_geometry_case_is_finite_and_reaches_its_index(oracle, name):
    _, knobs, (b, e) = next(g for g in ALL_GEOMETRY if g[0] == name)
    rq = _abi.default_request(**knobs)
    rays, states, dots = cc.restated(oracle, rq, cc.P0, b, e)
    assert len(rays) == (rq.height // rq.divisions) * rq.width * (e - b)
    if rq.width == 1:                                                         # u_den = 0, as in the case W1
        assert cc.kinds(dots[:, 0]) == {"inf": len(rays)} and np.isnan(_dirs(rays)).all()
    else:
        assert np.isfinite(_dirs(rays)).all() and cc.kinds(dots) == {"norm": dots.size}
    assert len(np.unique(states, axis=0)) == len(states)
    if name.startswith("tall_"):
        assert float(cnp.camera_vectors(rq, *cc.P0)["u_den"]) == 1.0
        if rq.division_no:
            x, yg, s = cnp.strip_records(rq, b, e)[0]
            assert (yg * rq.width + x) * rq.spp + s >= 2 ** 42
    if name in ("tall_first", "tall_middle"):
        y_cam = rq.height - 1 - rq.division_no
        assert y_cam > 2 ** 24 and int(np.float32(y_cam)) != y_cam            # (float) of the camera row rounds


def test_wide_case_geometry():
    _, knobs, (b, e) = cc.WIDE
    rq = _abi.default_request(**knobs)
    assert rq.width * rq.height == 2 ** 31 - 32768 and e - b == 1
    x, yg, s = cnp.strip_records(rq, b, e)[-1]
    assert (yg * rq.width + x) * rq.spp + s >= 2 ** 42


# ------------------------------------------------------------------------------------------------------------ 2. the host planner


def _same_nan(a, b):
    """Bit-equal, or NaN in both."""
    a, b = np.atleast_1d(np.asarray(a, np.float32)), np.atleast_1d(np.asarray(b, np.float32))
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def test_host_planner_equals_the_restatement_on_the_corpus(lib):
    pairs = [(name, cc.request(knobs), pose) for name, knobs, pose, _ in cc.CASES]
    pairs += [(name, _abi.default_request(**knobs), cc.P0) for name, knobs, _ in ALL_GEOMETRY]
    for name, rq, pose in pairs:
        host = _host(lib, rq, None if pose is None else _abi.Camera.look_at(*pose))
        assert host is not None, name
        ref = cnp.camera_vectors(rq, *(pose if pose is not None else (None, None, None)))
        for n in VECS + SCALARS:
            assert _same_nan(host[n], ref[n]), (name, n, host[n], ref[n])


# ------------------------------------------------------------------------------------------------- 3. make_pose's refusal boundary

# the scale of the vector whose squared length make_pose divides by, and whether the pose is refused: the squared length is zero after
# underflow, subnormal, near the top of the range, infinite
SCALES = [(1e-30, True), (1e-21, False), (1e18, False), (1e30, True)]


@pytest.mark.parametrize("scale, refused", SCALES)
@pytest.mark.parametrize("which", ["eye_to_target", "up_cross_w"])
def test_make_pose_refuses_where_the_restatement_does(lib, which, scale, refused):
    rq = cc.request({})
    s = np.float32(scale)
    for direction in ((1.0, 0.0, 0.0), (0.6, -0.3, 0.8), (-0.5, 0.5, 0.7)):
        d = tuple(float(np.float32(c) * s) for c in direction)
        with np.errstate(all="ignore"):
            if which == "eye_to_target":
                pose = (d, (0.0, 0.0, 0.0), (0.1, 1.0, 0.2))
                sq = cnp._dot3(np.asarray(d, np.float32))
            else:
                pose = ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), d)                   # w = (0, 0, 1): up x w = (d.y, -d.x, 0)
                sq = cnp._dot3(np.asarray([d[1], -d[0], 0.0], np.float32))
            kind = cc.kinds(np.asarray([sq]))
        assert kind == {{1e-30: "zero", 1e-21: "sub", 1e18: "norm", 1e30: "inf"}[scale]: 1}, (which, scale, kind)
        none = cnp.basis(*pose) is None
        assert (_host(lib, rq, _abi.Camera.look_at(*pose)) is None) == none == refused, (which, scale, direction)


# ---------------------------------------------------------------------------------------------------- 4. no pose: the oracle's rays


@pytest.mark.parametrize("name", [c[0] for c in cc.REF])
def test_reference_camera_cases_equal_the_oracle(oracle, name):
    _, knobs, pose, _ = CASES[name]
    rq = cc.request(knobs)
    rays, states, _ = cc.restated(oracle, rq, None)
    for i, (x, yg, s) in enumerate(cnp.strip_records(rq)):
        st = cnp.sample_state(oracle, rq, x, yg, s)
        o, d = oracle.camera_ray(rq, x, rq.height - 1 - yg, st)
        r = rays[i]
        got = np.array([r["ox"], r["oy"], r["oz"], r["dx"], r["dy"], r["dz"]], np.float32)
        assert _same_nan(got, np.concatenate([o, d])), (name, i, x, yg, s, got, o, d)
        assert np.array_equal(states[i], st), (name, i)
