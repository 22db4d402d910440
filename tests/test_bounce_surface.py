"""Path steps of caller rays, the part that needs no GPU: where rt_tile.h puts its section, the package's names, and every argument
check of the contract refuses before any device work.  (The declarations of rt_scene_bounce / rt_scene_bounce_device, the binding's
argument lists, the layouts of rt_bounce and rt_bounce_request, the exports and the ABI version: tests/test_surface.py.)"""
import ctypes as C

from ray_tracer_s8_amd import _abi

from _surface import HEADER, check_abi_version_unchanged, check_exports


def test_header_declares_the_bounce_entry_points():
    assert HEADER.index("RT_API int rt_scene_trace_device") < HEADER.index("typedef struct rt_bounce ") < HEADER.index("typedef struct rt_aov_planes")


def test_libraries_export_the_bounce_entry_points():
    check_exports(["rt_scene_bounce", "rt_scene_bounce_device"], exactly=True)


def test_abi_version_unchanged():
    check_abi_version_unchanged()


def test_package_exports_the_bounce_names():
    import ray_tracer_s8_amd as rt
    assert rt.BOUNCE_DTYPE is _abi.BOUNCE_DTYPE and rt.BounceRequest is _abi.BounceRequest and rt.RT_BOUNCE_MISSED == 2
    assert hasattr(rt.Scene, "bounce") and hasattr(rt.Scene, "bounce_device")


def bad_arg_calls(lib, scene):
    """Every RT_ERR_BAD_ARG case of the contract as (what, status) pairs, for a scene handle (None: the NULL scene itself is the
    error, as on a machine without a device).  Shared with tests/test_gpu_bounce.py, which passes a live scene."""
    n = 4
    rays = (_abi.Ray * n)()
    st = (C.c_uint64 * (4 * n))()
    bnc = (_abi.Bounce * n)()
    nxt = (C.c_uint32 * n)()
    cnt = C.c_uint32(7)
    act = (C.c_uint32 * n)(0, 1, 2, 3)
    bad = (C.c_uint32 * n)(0, 1, 2, n)

    def rq(**kw):
        r = _abi.BounceRequest(0, 0, 0, 0, 0)
        for k, v in kw.items():
            setattr(r, k, v)
        return C.byref(r)

    def host(req=None, scene_=scene, rays_=rays, n_=n, st_=st, act_=None, n_act=0, bnc_=bnc, nxt_=None, cnt_=None, null_req=False):
        return lib.rt_scene_bounce(scene_, None if null_req else (req or rq()), rays_, n_, st_, act_, n_act, bnc_, None, nxt_, cnt_, None)

    v = lambda a: C.cast(a if isinstance(a, C.Array) else C.pointer(a), C.c_void_p)

    def dev(req=None, scene_=scene, rays_=v(rays), n_=n, st_=v(st), act_=None, n_act=None, bnc_=v(bnc), nxt_=None, cnt_=None,
            null_req=False):
        return lib.rt_scene_bounce_device(scene_, None if null_req else (req or rq()), rays_, n_, st_, act_, n_act, bnc_, None, nxt_, cnt_,
                                          None)

    out = []
    for name, f in (("host", host), ("device", dev)):
        out += [((name, "scene"), f(scene_=None)), ((name, "request"), f(null_req=True)), ((name, "rays"), f(rays_=None)),
                ((name, "states"), f(st_=None)), ((name, "out_bounce"), f(bnc_=None)), ((name, "n == 0"), f(n_=0)),
                ((name, "ray_form"), f(req=rq(ray_form=2))), ((name, "reserved"), f(req=rq(reserved=1))),
                ((name, "seed_states"), f(req=rq(seed_states=2))),
                ((name, "next without n_next"), f(nxt_=nxt if name == "host" else v(nxt)))]
    out += [(("host", "index >= n"), host(act_=bad, n_act=n)), (("host", "n_active > n"), host(act_=act, n_act=n + 1)),
            (("device", "active without n_active"), dev(act_=v(act))), (("device", "n_active without active"), dev(n_act=v(cnt)))]
    assert cnt.value == 7 and not any(bytes(bnc)) and not any(bytes(nxt))
    return out


def test_bounce_entry_points_check_arguments_without_a_device():
    """Without a scene every call is refused for that alone.  With a scene pointer that is merely non-NULL (zeroed memory that is
    no scene: any use of it would need a device) every other case is still refused, so the checks come before any device work.
    The same cases run on the GPU with a live scene (tests/test_gpu_bounce.py, through bad_arg_calls too)."""
    lib = _abi.load()
    for what, status in bad_arg_calls(lib, None):
        assert status == _abi.RT_ERR_BAD_ARG, what
    dummy = (C.c_uint8 * 4096)()
    for what, status in bad_arg_calls(lib, C.cast(dummy, C.c_void_p)):
        assert status == _abi.RT_ERR_BAD_ARG, what
        assert lib.rt_last_error(), what
    assert not any(bytes(dummy))
