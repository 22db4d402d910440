"""Direct lighting of caller rays, the part that needs no GPU: where rt_tile.h puts its section, the package's names, every argument
check of the contract refuses before any device work, and Scene.direct checks its arguments before it calls.  (The declarations of
rt_scene_light_count / rt_scene_direct / rt_scene_direct_device, the binding's argument lists, the layouts of rt_direct_request and
rt_direct, the exports and the ABI version: tests/test_surface.py.  The limit of 2^23 emitters is the plan's:
tests/test_direct_host.py.)"""
import ctypes as C

import numpy as np
import pytest

from ray_tracer_s8_amd import _abi

from _surface import HEADER, check_abi_version_unchanged, check_exports


def test_header_declares_the_direct_entry_points():
    assert HEADER.index("RT_API int rt_scene_bounce_device") < HEADER.index("typedef struct rt_direct_request") < HEADER.index("typedef struct rt_aov_planes")
    assert "additions only: direct lighting" in HEADER


def test_libraries_export_the_direct_entry_points():
    check_exports(["rt_scene_light_count", "rt_scene_direct", "rt_scene_direct_device"], exactly=True)


def test_abi_version_unchanged():
    check_abi_version_unchanged()


def test_package_exports_the_direct_names():
    import ray_tracer_s8_amd as rt
    assert rt.DIRECT_DTYPE is _abi.DIRECT_DTYPE and rt.DirectRequest is _abi.DirectRequest
    assert hasattr(rt.Scene, "direct") and hasattr(rt.Scene, "direct_device") and isinstance(rt.Scene.n_lights, property)


def bad_arg_calls(lib, scene):
    """Every RT_ERR_BAD_ARG case of the contract as (what, status) pairs, for a scene handle (None: the NULL scene itself is the
    error, as on a machine without a device).  Shared with tests/test_gpu_direct.py, which passes a live scene."""
    n = 4
    hits = (_abi.Hit * n)()
    st = (C.c_uint64 * (4 * n))()
    out_ = (_abi.Direct * n)()
    cnt = C.c_uint32(7)
    act = (C.c_uint32 * n)(0, 1, 2, 3)
    bad = (C.c_uint32 * n)(0, 1, 2, n)

    def rq(**kw):
        r = _abi.DirectRequest(0, 0, 0.001, 1000.0)
        for k, v in kw.items():
            setattr(r, k, v)
        return C.byref(r)

    def host(req=None, scene_=scene, hits_=hits, n_=n, st_=st, act_=None, n_act=0, o_=out_, null_req=False):
        return lib.rt_scene_direct(scene_, None if null_req else (req or rq()), hits_, n_, st_, act_, n_act, o_, None)

    v = lambda a: C.cast(a if isinstance(a, C.Array) else C.pointer(a), C.c_void_p)

    def dev(req=None, scene_=scene, hits_=v(hits), n_=n, st_=v(st), act_=None, n_act=None, o_=v(out_), null_req=False):
        return lib.rt_scene_direct_device(scene_, None if null_req else (req or rq()), hits_, n_, st_, act_, n_act, o_, None)

    out = []
    for name, f in (("host", host), ("device", dev)):
        out += [((name, "scene"), f(scene_=None)), ((name, "request"), f(null_req=True)), ((name, "hits"), f(hits_=None)),
                ((name, "states"), f(st_=None)), ((name, "out"), f(o_=None)), ((name, "n == 0"), f(n_=0)),
                ((name, "reserved"), f(req=rq(reserved=1)))]
    out += [(("host", "index >= n"), host(act_=bad, n_act=n)), (("host", "n_active > n"), host(act_=act, n_act=n + 1)),
            (("host", "n_active without active"), host(n_act=2)),
            (("device", "active without n_active"), dev(act_=v(act))), (("device", "n_active without active"), dev(n_act=v(cnt)))]
    m = C.c_uint32(9)
    out += [(("count", "scene"), lib.rt_scene_light_count(None, C.byref(m))), (("count", "out"), lib.rt_scene_light_count(scene, None))]
    assert cnt.value == 7 and m.value == 9 and not any(bytes(out_)) and not any(bytes(st))
    return out


def test_direct_entry_points_check_arguments_without_a_device():
    """Without a scene every call is refused for that alone.  With a scene pointer that is merely non-NULL (zeroed memory that is
    no scene: any use of it would need a device) every other case is still refused, so the checks come before any device work.
    The same cases run on the GPU with a live scene (tests/test_gpu_direct.py, through bad_arg_calls too)."""
    lib = _abi.load()
    for what, status in bad_arg_calls(lib, None):
        assert status == _abi.RT_ERR_BAD_ARG, what
    dummy = (C.c_uint8 * 4096)()
    for what, status in bad_arg_calls(lib, C.cast(dummy, C.c_void_p)):
        assert status == _abi.RT_ERR_BAD_ARG, what
        assert lib.rt_last_error(), what
    assert not any(bytes(dummy))
    # the light count of a scene is a host-side value: zeroed memory has none
    m = C.c_uint32(9)
    assert lib.rt_scene_light_count(C.cast(dummy, C.c_void_p), C.byref(m)) == _abi.RT_OK and m.value == 0


class _NoLibrary:
    """Stands in for the library behind a Scene: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


def test_python_argument_handling():
    """Scene.direct refuses malformed arrays itself, before the library is called."""
    import ray_tracer_s8_amd as rt
    sc = object.__new__(rt.Scene)
    sc._lib, sc._h = _NoLibrary(), None
    hits = np.zeros(5, _abi.HIT_DTYPE)
    states = np.ones((5, 4), np.uint64)
    try:
        with pytest.raises(ValueError):
            sc.direct(hits.reshape(5, 1), states)
        with pytest.raises(ValueError):
            sc.direct(hits, None)
        with pytest.raises(ValueError):
            sc.direct(hits, states[:-1])
        with pytest.raises(ValueError):
            sc.direct(hits, states.reshape(4, 5))
        with pytest.raises(ValueError):
            sc.direct(hits, states[:, :3])
        with pytest.raises(AssertionError):                                # well-formed arguments do reach the library
            sc.direct(hits, states, active=[0, 2])
    finally:
        sc._h = None                                                       # (nothing for close() to destroy)
