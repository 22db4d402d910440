"""The corpus of camera cases at extreme poses, knobs and film geometry (tests/test_camera_cases.py on the CPU,
tests/test_gpu_camera_extremes.py on the device).  Importable without a GPU.

A knob case is (name, request knobs, pose or None, class) at the standard frame FRAME.  The class is what the numpy restatement
(tests/_camera_np.py) gives for the two squared lengths Camera::get_ray normalises, per record of the case:
    dot1 of llc + u hor + v ver - org, dot2 of focal_point - o,
counted by kind (KINDS), and the number of records whose direction has a NaN.  tests/test_camera_cases.py asserts the class of every
case, so no case passes without reaching what it is named for: the kinds other than "norm" are the operands that leave the fast
path of the device's sqrt_rn (valid from 2^-96 up to, not including, infinity)."""
import math

import numpy as np

from ray_tracer_s8_amd import _abi

import _camera_np as cnp

FRAME = dict(width=24, height=12, divisions=3, division_no=1, spp=2, seed=7)          # 4 rows x 24 x 2 = 192 records

P0 = ((2.5, 1.75, 1.0), (-0.25, 0.1, -2.0), (0.3, 1.0, -0.2))                        # test_gpu_camera.POSES["oblique_rolled"]
Z = ((0.0, 0.0, 0.0),) + P0[1:]                                                       # ... with the eye at the origin
BIG = (tuple(float(np.float32(c) * np.float32(1e18)) for c in P0[0]),) + P0[1:]           # ... with the eye scaled by 1e18
INF, NAN = math.inf, math.nan

# the kinds of a squared length: +-0; subnormal; normal below 2^-96; finite from 2^-96; +inf; NaN
KINDS = ("zero", "sub", "low", "norm", "inf", "nan")


def kind_masks(a):
    """(n, len(KINDS)) bool: the kind of every one of the n values of a."""
    a = np.asarray(a, np.float32).reshape(-1)
    fin = np.isfinite(a)
    mag = np.abs(a)
    tiny, lo = np.float32(2.0 ** -126), np.float32(2.0 ** -96)
    return np.stack([a == 0, fin & (mag > 0) & (mag < tiny), fin & (mag >= tiny) & (mag < lo), fin & (mag >= lo), np.isinf(a),
                     np.isnan(a)], 1)


def kinds(a):
    """The count of every kind among the float32 values a, as a dict without the kinds that do not occur."""
    return {k: int(c) for k, c in zip(KINDS, kind_masks(a).sum(0)) if c}


def _cls(dot1, dot2, nan):
    return dict(dot1=dot1, dot2=dot2, nan=nan)


N = 192
_NORM = {"norm": N}

# the knob cases under a pose, with the class measured through the restatement at FRAME (the table of DESIGN.md 9.4)
POSED = [
    ("plain", {}, P0, _cls(_NORM, _NORM, 0)),
    ("tiny_view", dict(fov=1e-20, focal_length=1e-21, aperture=0.0, focus_distance=1.0), Z, _cls({"sub": N}, _NORM, 0)),
    ("tiny_view2", dict(fov=4e-19, focal_length=2e-20, aperture=1e-21, focus_distance=3e-20), Z,
     _cls({"sub": 43, "low": 149}, {"sub": N}, 0)),
    ("tiny_view3", dict(fov=1e-22, focal_length=1e-23, aperture=1e-23, focus_distance=1e-22), Z,
     _cls({"zero": 52, "sub": 140}, {"sub": 140, "nan": 52}, 52)),
    # both squared lengths straddle 2^-96, the lower edge of sqrt_rn's fast path, inside every wave: the view and the lens are of the
    # size of 2^-48
    ("fast_path_edge", dict(fov=3e-15, focal_length=3e-15, aperture=4e-15, focus_distance=3.4e-15), Z,
     _cls({"low": 114, "norm": 78}, {"low": 91, "norm": 101}, 0)),
    ("huge_focus", dict(focus_distance=1.8e19, aperture=2e18), P0, _cls(_NORM, {"norm": 167, "inf": 25}, 25)),
    ("huge_focal", dict(focal_length=1.8e19, fov=0.3), P0, _cls(_NORM, _NORM, 0)),
    # dot1 overflow: at this focal length the film terms are absorbed in focal_length w, so every record has the same dot1 and f32
    # has no value at which some records overflow and others do not — bisecting focal_length over (1.8e19, 2e19) the class flips
    # from all finite at 2^64 (1 - 2^-24) to all infinite at 2^64 exactly; both neighbours are kept
    ("dot1_top", dict(focal_length=1.8446742974197924e19, fov=0.3), P0, _cls(_NORM, _NORM, 0)),
    ("dot1_overflow", dict(focal_length=1.8446744073709552e19, fov=0.3), P0, _cls({"inf": N}, {"nan": N}, N)),
    ("big_eye", {}, BIG, _cls({"zero": N}, {"nan": N}, N)),
    ("big_eye_focus", dict(focus_distance=1e19, aperture=1e18, focal_length=1e18), BIG, _cls(_NORM, _NORM, 0)),
    ("tiny_eye", dict(aperture=0.4), ((1e-21, 2e-21, -3e-21), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), _cls(_NORM, _NORM, 0)),
    ("tiny_up", dict(aperture=0.4), ((0.0, 0.0, 0.0), (0.0, 0.2, -1.0), (1e-21, 3e-21, 0.0)), _cls(_NORM, _NORM, 0)),
    ("near_parallel_up", dict(aperture=0.4), ((0.0, 0.0, 0.0), (1e-4, 1.0, 0.0), (0.0, 1.0, 0.0)), _cls(_NORM, _NORM, 0)),
    ("focus_zero_ap0", dict(focus_distance=0.0, aperture=0.0), P0, _cls(_NORM, {"zero": N}, N)),
    ("focus_neg", dict(focus_distance=-2.0, aperture=0.3), P0, _cls(_NORM, _NORM, 0)),
    ("focus_inf", dict(focus_distance=INF, aperture=0.3), P0, _cls(_NORM, {"inf": N}, N)),
    ("ap_inf", dict(aperture=INF), P0, _cls(_NORM, {"nan": N}, N)),
    ("ap_nan", dict(aperture=NAN), P0, _cls(_NORM, {"nan": N}, N)),
    ("ap_neg", dict(aperture=-0.5), P0, _cls(_NORM, _NORM, 0)),
    ("fov_zero", dict(fov=0.0, aperture=0.3), P0, _cls(_NORM, _NORM, 0)),
    ("fov_pi", dict(fov=3.1415927, aperture=0.4), P0, _cls(_NORM, _NORM, 0)),
    ("focal_zero", dict(focal_length=0.0), P0, _cls(_NORM, _NORM, 0)),
    ("focal_neg", dict(focal_length=-1.0), P0, _cls(_NORM, _NORM, 0)),
    ("fov_nan", dict(fov=NAN), P0, _cls({"nan": N}, {"nan": N}, N)),
    ("H1", dict(height=1, divisions=1, division_no=0), P0, _cls({"inf": 48}, {"nan": 48}, 48)),
    ("W1", dict(width=1), P0, _cls({"inf": 8}, {"nan": 8}, 8)),
]

# every distinct knob set above under no pose: the reference camera through the same kernels (the oracle's camera_ray is a second
# reference there).  The class is the posed one except where listed.
_REF_CLASS = {
    "tiny_view3": _cls({"zero": 47, "sub": 145}, {"sub": 145, "nan": 47}, 47),
    "ap_inf": _cls(_NORM, {"inf": N}, N),
    "H1": _cls({"nan": 48}, {"nan": 48}, 48),
    "W1": _cls({"nan": 8}, {"nan": 8}, 8),
}
_seen = set()
REF = []
for _name, _knobs, _pose, _c in POSED:
    _key = repr(sorted(_knobs.items()))
    if _knobs and _key not in _seen:
        _seen.add(_key)
        REF.append((_name + "@ref", _knobs, None, _REF_CLASS.get(_name, _c)))
CASES = POSED + REF

# the cases whose class has two kinds, per stage the two kinds that must meet in one aligned run of 64 consecutive records (a wave).
# Of these, fast_path_edge and huge_focus pair a kind of sqrt_rn's fast path with one that leaves it: lanes on both sides of its
# ballot.  The pairs of the tiny views all leave it (the ballot is uniform; the lanes differ inside the compiler's sequence).
MIXED = {"tiny_view2": {"dot1": ("sub", "low")}, "tiny_view3": {"dot1": ("zero", "sub"), "dot2": ("sub", "nan")},
         "fast_path_edge": {"dot1": ("low", "norm"), "dot2": ("low", "norm")}, "huge_focus": {"dot2": ("norm", "inf")}}
MIXED.update({k + "@ref": v for k, v in list(MIXED.items())})


def request(knobs, **kw):
    return _abi.default_request(**{**FRAME, **knobs, **kw})


def restated(oracle, rq, pose, begin=0, end=None, _cache={}):
    """cnp.strip_rays(..., dots=True) of a request, cached by its bytes (the numpy restatement is slow; the arrays are shared:
    leave them unchanged)."""
    key = (bytes(rq), pose, begin, end)
    if key not in _cache:
        _cache[key] = cnp.strip_rays(oracle, rq, pose, begin, end, dots=True)
    return _cache[key]


# ----------------------------------------------------------------------------------------------- geometry and index cases
# (name, request knobs, sample range): pose P0, the default knobs.  `tall`: 2 x (2^30 - 1) in strips of one row at 4096 spp — stream
# indices (y W + x) S + s up to 2^43, camera rows up to 2^30 - 2 (above 2^24: (float) of the row rounds), u_den = 1.0; the seeds make
# the 64-bit stream arithmetic wrap.  `wide`: one row of 32768 records at the last row of a 32768 x 65535 film (W H = 2^31 - 32768).
# `n*`: record counts around the wave (64) and block (256) sizes.
TALL_H = 2 ** 30 - 1
_TALL = dict(width=2, height=TALL_H, divisions=TALL_H, spp=4096, seed=7)
GEOMETRY = [(f"tall_{tag}", dict(_TALL, division_no=k), (4090, 4096))
            for tag, k in (("first", 0), ("middle", 2 ** 29), ("last", 2 ** 30 - 2))]
GEOMETRY += [(f"tall_seed_{tag}", dict(_TALL, division_no=2 ** 29, seed=seed), (4090, 4096))
             for tag, seed in (("0", 0), ("max", 2 ** 64 - 1), ("max_m15", 2 ** 64 - 16))]
WIDE = ("wide_last_row", dict(width=32768, height=65535, divisions=65535, division_no=65534, spp=4096, seed=7), (4095, 4096))
COUNTS = [(f"n_w{w}_s{n}", dict(width=w, height=2, divisions=2, division_no=1, spp=5, seed=7), (1, 1 + n))
          for w in (1, 3, 63, 65, 257) for n in (1, 3)]
