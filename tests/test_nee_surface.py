"""The next-event-estimation integrator for caller rays, the part that needs no GPU: where rt_tile.h puts its section, the package's
names, every argument check of the contract refuses before any device work, and Scene.trace_nee checks its arguments before it
calls.  (The declarations of rt_scene_trace_nee / rt_scene_trace_nee_device, the binding's argument lists, rt_nee_request's layout,
RT_NEE_LIGHT_ONLY = 0 and RT_NEE_MIS = 1, the exports and the ABI version: tests/test_surface.py.  The limit of 2^23 emitters is the
plan's: tests/test_nee_host.py.)"""
import ctypes as C

import numpy as np
import pytest

from ray_tracer_s8_amd import _abi

from _surface import HEADER, check_abi_version_unchanged, check_exports


def test_header_declares_the_nee_entry_points():
    assert HEADER.index("RT_API int rt_scene_direct_device") < HEADER.index("typedef struct rt_nee_request") < HEADER.index("typedef struct rt_aov_planes")
    assert "additions only: next-event estimation" in HEADER


def test_libraries_export_the_nee_entry_points():
    check_exports(["rt_scene_trace_nee", "rt_scene_trace_nee_device"], exactly=True)


def test_abi_version_unchanged():
    check_abi_version_unchanged()


def test_package_exports_the_nee_names():
    import ray_tracer_s8_amd as rt
    assert rt.NeeRequest is _abi.NeeRequest and (rt.RT_NEE_LIGHT_ONLY, rt.RT_NEE_MIS) == (0, 1)
    assert hasattr(rt.Scene, "trace_nee") and hasattr(rt.Scene, "trace_nee_device")


def arg_error_calls(lib, scene):
    """Every argument error of the contract as (what, status, expected status) triples, for a scene handle (None: the NULL scene itself
    is the error, as on a machine without a device).  Shared with tests/test_gpu_nee.py, which passes a live scene."""
    n = 4
    rays = (_abi.Ray * n)()
    st = (C.c_uint64 * (4 * n))()
    rgb = (C.c_float * (3 * n))()
    segs, shadow = (C.c_uint32 * n)(), (C.c_uint32 * n)()
    BAD, LIMIT = _abi.RT_ERR_BAD_ARG, _abi.RT_ERR_LIMIT

    def rq(**kw):
        r = _abi.NeeRequest(1, 3, 7, 0, _abi.RT_TRACE_RAY_NEW, _abi.RT_NEE_MIS, 0)
        for k, v in kw.items():
            setattr(r, k, v)
        return C.byref(r)

    def host(req=None, scene_=scene, rays_=rays, n_=n, st_=st, rgb_=rgb, null_req=False):
        return lib.rt_scene_trace_nee(scene_, None if null_req else (req or rq()), rays_, n_, st_, rgb_, segs, shadow, None)

    v = lambda a: C.cast(a, C.c_void_p)

    def dev(req=None, scene_=scene, rays_=v(rays), n_=n, st_=v(st), rgb_=v(rgb), null_req=False):
        return lib.rt_scene_trace_nee_device(scene_, None if null_req else (req or rq()), rays_, n_, st_, rgb_, v(segs), v(shadow), None)

    out = []
    for name, f in (("host", host), ("device", dev)):
        out += [((name, "scene"), f(scene_=None), BAD), ((name, "request"), f(null_req=True), BAD), ((name, "rays"), f(rays_=None), BAD),
                ((name, "out_rgb"), f(rgb_=None), BAD), ((name, "n == 0"), f(n_=0), BAD), ((name, "spp == 0"), f(req=rq(spp=0)), BAD),
                ((name, "ray_form"), f(req=rq(ray_form=2)), BAD), ((name, "mode"), f(req=rq(mode=2)), BAD),
                ((name, "reserved"), f(req=rq(reserved=1)), BAD)]
        if scene is not None:
            out += [((name, "spp > RT_MAX_SPP"), f(req=rq(spp=_abi.RT_MAX_SPP + 1)), LIMIT),
                    ((name, "max_bounces > RT_MAX_BOUNCES"), f(req=rq(max_bounces=_abi.RT_MAX_BOUNCES + 1)), LIMIT)]
    assert not any(bytes(rgb)) and not any(bytes(st)) and not any(bytes(segs)) and not any(bytes(shadow))
    return out


def test_nee_entry_points_check_arguments_without_a_device():
    """Without a scene every call is refused for that alone.  With a scene pointer that is merely non-NULL (zeroed memory that is no
    scene: any use of it would need a device) every other case is still refused, so the checks come before any device work.  The same
    cases run on the GPU with a live scene (tests/test_gpu_nee.py, through arg_error_calls too)."""
    lib = _abi.load()
    for what, status, want in arg_error_calls(lib, None):
        assert status == want == _abi.RT_ERR_BAD_ARG, what
    dummy = (C.c_uint8 * 4096)()
    calls = arg_error_calls(lib, C.cast(dummy, C.c_void_p))
    assert {want for _, _, want in calls} == {_abi.RT_ERR_BAD_ARG, _abi.RT_ERR_LIMIT}
    for what, status, want in calls:
        assert status == want, what
        assert lib.rt_last_error(), what
    assert not any(bytes(dummy))


class _NoLibrary:
    """Stands in for the library behind a Scene: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


def test_python_argument_handling():
    """Scene.trace_nee refuses malformed arrays itself, before the library is called."""
    import ray_tracer_s8_amd as rt
    sc = object.__new__(rt.Scene)
    sc._lib, sc._h = _NoLibrary(), None
    o, d = np.zeros((5, 3), np.float32), np.ones((5, 3), np.float32)
    states = np.ones((5, 4), np.uint64)
    try:
        with pytest.raises(ValueError):
            sc.trace_nee(o, d[:4])
        with pytest.raises(ValueError):
            sc.trace_nee(o.reshape(3, 5), d.reshape(3, 5))
        with pytest.raises(ValueError):
            sc.trace_nee(o, d, rng_state=states[:-1])
        with pytest.raises(ValueError):
            sc.trace_nee(o, d, rng_state=states[:, :3])
        with pytest.raises(AssertionError):                                # well-formed arguments do reach the library
            sc.trace_nee(o, d, rng_state=states, mode=_abi.RT_NEE_LIGHT_ONLY)
    finally:
        sc._h = None                                                       # (nothing for close() to destroy)
