"""The next-event-estimation integrator for caller rays on the GPU (rt_scene_trace_nee, rt_scene_trace_nee_device):
1. RT_NEE_LIGHT_ONLY equals, bit for bit, the contract's forward fold over the EXISTING entry points — Scene.bounce per step, Scene.direct
   on the scattered hits whose primitive has roughness 0 — colours, segment and shadow-ray counts and final states, for max_bounces 0, 1
   and 3, with given states (spp = 1) and seeded (spp = 3, the per-sample states formed with the oracle's seeding);
2. both modes equal the CPU restatement tests/_lights_np.py `nee` (its arithmetic pinned by tests/test_nee_host.py, its bytes by
   tests/test_light_restatement.py) bit for bit on six scenes under four configurations, every ray in its own window, states included;
3. without emitters the segments and the written-back states are Scene.trace's;
4. batch sizes around the wave and workgroup sizes, the device form against the host form, two streams at once and repeated calls,
   spp = 4 against two calls of spp = 2, the scan engine on a tree deeper than the walk's stack; host-form calls of all five
   caller-ray kinds interleaved on one scene, whose staging buffer they share, against each call on a fresh scene;
5. both modes agree with rt_scene_trace within 5 sigma at 2^16 samples on a roughness-0 room, a room with glossy and mirror surfaces
   and that room inside an emissive sphere — where the composed recipe of examples/nee_rays.c (the control) does not;
6. both modes have the lower variance for a small bright light;
7. the argument errors with a live scene, and the plain-C client examples/nee_trace.c."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

import _bounce_np as B
import _direct_np as D
import _lights_np as LN
import _nee_np as N
from test_gpu_bounce import CONFIGS, FILL, SCAN, Dev, dev  # noqa: F401  (dev: a fixture of this module too)
from test_gpu_direct import SCENES, SIZES, _gap_and_bound, _room_rays, _scene
from test_nee_surface import arg_error_calls

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
R = B.R
F32 = np.float32
LIGHT_ONLY, MIS = N.LIGHT_ONLY, N.MIS
N_RAYS = 2000
REF = slice(None, None, 2)                       # the rays of the comparisons with the (per-ray Python) restatement: every other one
T_MIN, T_MAX = F32(0.001), F32(1000.0)

_CASES = {}


def _case(oracle, name):
    if name not in _CASES:
        sph, tri, wi, make = _scene(name)
        rays = np.ascontiguousarray(make(oracle, N_RAYS, 2700 + len(name)))
        _CASES[name] = dict(sph=sph, tri=tri, wi=wi, rays=rays, st0=R.states(len(rays), 2800 + len(name)))
    return _CASES[name]


def _nee(sc, rays, **kw):
    """Scene.trace_nee of rt_ray records as a dict."""
    o, d = R.od(rays)
    out = sc.trace_nee(o, d, rays["t_min"], rays["t_max"], **kw)
    res = dict(rgb=out[0], segments=out[1], shadow=out[2], stats=out[3])
    if len(out) > 4:
        res["states"] = out[4]
    return res


def _assert_rgb(got, want, what):
    ok = np.all(B.same_bits(got, want), 1)
    assert ok.all(), (what, np.nonzero(~ok)[0][:5], got[~ok][:3], want[~ok][:3])


# ---------------------------------------------------------------- 1. LIGHT_ONLY is the fold of the existing entry points
def _composed_sample(sc, lights, rays, states, max_bounces, flags, as_given, recipe="contract"):
    """One sample of every ray through Scene.bounce and Scene.direct, the forward fold in float32 numpy.  recipe "contract": the
    sampled rule and the samplable rule of rt_tile.h (RT_NEE_LIGHT_ONLY); "composed": the recipe of examples/nee_rays.c — a sample
    at every hit that scattered, every EMITTED after the first step dropped.  The rays share one window (one rt_direct_request).
    Returns (c (n, 3) float32, segments, shadow, states)."""
    n = len(rays)
    t_min, t_max = rays["t_min"][0], rays["t_max"][0]
    assert np.all(rays["t_min"] == t_min) and np.all(rays["t_max"] == t_max)
    T, c = np.ones((n, 3), F32), np.zeros((n, 3), F32)
    segs, shadow = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    sampled = np.zeros(n, bool)
    n_prev = np.zeros((n, 3), F32)
    cur_rays, cur_states = rays, np.array(states, np.uint64)
    act = np.arange(n)
    for k in range(max_bounces + 1):
        if not len(act):
            break
        d_in = np.stack([cur_rays["dx"], cur_rays["dy"], cur_rays["dz"]], 1).astype(F32)   # (read at k > 0 only: as given)
        s = sc.bounce(cur_rays, cur_states, active=act, as_given=as_given or k > 0, flags=flags, want_hits=True)
        cur_rays, cur_states = s["rays"], s["states"]
        segs[act] += 1
        status, rgb, hits = s["bounce"]["status"], B.rgb_of(s["bounce"]), s["hits"]
        emitted = act[status[act] == B.EMITTED]
        keep = np.ones(len(emitted), bool) if k == 0 else ~sampled[emitted]
        if recipe == "contract":                                           # an emitter the sample of the step before could not reach
            for q in np.nonzero(~keep)[0]:
                i = emitted[q]
                nh = D.v3(hits["nx"][i], hits["ny"][i], hits["nz"][i])
                keep[q] = not N.emitter_view(n_prev[i], d_in[i], nh, hits["distance"][i], bool(lights.sphere[hits["index"][i]]))[3]
        add = np.concatenate([act[status[act] == B.MISSED], emitted[keep]])
        with np.errstate(all="ignore"):
            c[add] = c[add] + T[add] * rgb[add]
            scat = act[status[act] == B.SCATTERED]
            T[scat] = T[scat] * rgb[scat]
        if k == max_bounces:
            break
        sampled[scat] = lights.M > 0 if recipe == "composed" else (lights.rough[hits["index"][scat]] == 0) & (lights.M > 0)
        n_prev[scat] = np.stack([hits["nx"][scat], hits["ny"][scat], hits["nz"][scat]], 1)
        lst = scat[sampled[scat]]
        dl = sc.direct(hits, cur_states, active=lst, t_min=float(t_min), t_max=float(t_max), flags=flags)
        cur_states = dl["states"]
        st = dl["direct"]["status"]
        shadow[lst] += np.isin(st[lst], (D.LIT, D.OCCLUDED)).astype(np.uint32)
        lit = lst[st[lst] == D.LIT]
        with np.errstate(all="ignore"):
            c[lit] = c[lit] + T[lit] * D.rgb_of(dl["direct"])[lit]
        act = scat
    return c, segs, shadow, cur_states


def _one_window(rays):
    r = rays.copy()
    r["t_min"], r["t_max"] = T_MIN, T_MAX
    return r


def _check_light_only(oracle, name, cfg, max_bounces):
    flags = CONFIGS[cfg][0]
    c = _case(oracle, name)
    rays = _one_window(c["rays"])
    n = len(rays)
    lights = LN.Table(c["sph"], c["tri"], c["wi"])
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        assert sc.n_lights == lights.M
        # spp = 1, given states
        want_c, want_segs, want_shadow, want_states = _composed_sample(sc, lights, rays, c["st0"], max_bounces, flags, False)
        got = _nee(sc, rays, spp=1, max_bounces=max_bounces, rng_state=c["st0"], mode=LIGHT_ONLY, flags=flags)
        _assert_rgb(got["rgb"], (np.zeros((n, 3), F32) + want_c).astype(F32), (name, cfg, max_bounces, "given states"))
        assert np.array_equal(got["segments"], want_segs) and np.array_equal(got["shadow"], want_shadow)
        assert np.array_equal(got["states"], want_states)
        st = got["stats"]
        assert st.n_launches == 1 and st.primary_rays == n and st.ray_segments == int(want_segs.sum()) + int(want_shadow.sum())
        if lights.M and max_bounces and name != "deep_tree":
            assert want_shadow.sum() > 0 and (want_c.sum(1) > 0).sum() > 100
        # spp = 3, seeded: the composition per sample, on the states the oracle's seeding gives sample s of ray i
        seed, spp, m = 90210 + max_bounces, 3, 600
        total, segs, shadow = np.zeros((m, 3), F32), np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        for s in range(spp):
            cs, sg, sh, _ = _composed_sample(sc, lights, rays[:m], N.sample_states(seed, m, spp, s), max_bounces, flags, False)
            with np.errstate(all="ignore"):
                total = total + cs
            segs += sg
            shadow += sh
        got = _nee(sc, rays[:m], spp=spp, max_bounces=max_bounces, seed=seed, mode=LIGHT_ONLY, flags=flags)
        _assert_rgb(got["rgb"], total, (name, cfg, max_bounces, "seeded"))
        assert np.array_equal(got["segments"], segs) and np.array_equal(got["shadow"], shadow)
        assert got["stats"].primary_rays == m * spp


@pytest.mark.parametrize("max_bounces", [0, 1, 3])
@pytest.mark.parametrize("name", SCENES)
def test_light_only_equals_the_existing_entry_points(ndev, oracle, name, max_bounces):
    _check_light_only(oracle, name, "default", max_bounces)


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c != "default"])
def test_light_only_equals_the_existing_entry_points_under_flags(ndev, oracle, cfg):
    _check_light_only(oracle, "mixed", cfg, 3)


# ---------------------------------------------------------------- 2. both modes against the restatement
_REF = {}


def _reference(oracle, name, backend):
    """The restatement on the REF rays of the case, 2 samples from given states, 3 bounces: once per (scene, backend)."""
    if (name, backend) not in _REF:
        c = _case(oracle, name)
        _REF[name, backend] = LN.nee(oracle, c["sph"], c["tri"], c["rays"][REF], 2, 3, backend, c["wi"], states=c["st0"][REF])
    return _REF[name, backend]


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", SCENES)
def test_both_modes_equal_the_restatement(ndev, oracle, name, cfg):
    flags, engine, backend = CONFIGS[cfg]
    c = _case(oracle, name)
    want = _reference(oracle, name, backend)
    rays, st0 = np.ascontiguousarray(c["rays"][REF]), np.ascontiguousarray(c["st0"][REF])
    if name == "deep_tree":
        engine = SCAN                                                      # deeper than the walk's stack: the scan
        assert R.tree_depth(c["sph"], c["tri"]) >= R.trav_stack()
    if name in B.SCENE_NAMES:
        assert len(np.unique(rays["t_max"])) > 10                          # the rays keep their own windows
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        for mode in (LIGHT_ONLY, MIS):
            got = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=mode, flags=flags)
            _assert_rgb(got["rgb"], want["rgb"][mode], (name, cfg, mode))
            assert np.array_equal(got["segments"], want["segments"]) and np.array_equal(got["shadow"], want["shadow"]), (name, cfg, mode)
            assert np.array_equal(got["states"], want["states"]), (name, cfg, mode)
            st = got["stats"]
            assert st.engine == engine and st.n_launches == 1 and st.primary_rays == 2 * len(rays)
            assert st.ray_segments == int(want["segments"].sum()) + int(want["shadow"].sum())
            if engine == SCAN:
                assert st.broad_candidates == st.ray_segments * (len(c["sph"]) + len(c["tri"]))
    if name == "no_lights":
        assert want["shadow"].sum() == 0
    elif name != "deep_tree":
        assert want["shadow"].sum() > 0
        assert not np.array_equal(want["rgb"][LIGHT_ONLY], want["rgb"][MIS])


# ---------------------------------------------------------------- 3. no emitters: the trace's segments and states
@pytest.mark.parametrize("mode", [LIGHT_ONLY, MIS])
def test_without_emitters_segments_and_states_are_the_trace(ndev, oracle, mode):
    c = _case(oracle, "no_lights")
    rays = c["rays"]
    o, d = R.od(rays)
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        assert sc.n_lights == 0
        for spp, mb in ((1, 3), (3, 5), (2, 0)):
            _, segs, _, states = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=spp, max_bounces=mb, rng_state=c["st0"])
            got = _nee(sc, rays, spp=spp, max_bounces=mb, rng_state=c["st0"], mode=mode)
            assert np.array_equal(got["segments"], segs) and np.array_equal(got["states"], states) and not got["shadow"].any()
        segs = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=2, max_bounces=4, seed=5)[1]
        assert np.array_equal(_nee(sc, rays, spp=2, max_bounces=4, seed=5, mode=mode)["segments"], segs)


# ---------------------------------------------------------------- 4. shapes and forms
def _device_nee(sc, dev, rays, states, **kw):
    n = len(rays)
    d_rays, d_state = dev.put(rays), dev.put(states)
    d_rgb, d_segs, d_shadow = dev.alloc(12 * n, FILL), dev.alloc(4 * n, FILL), dev.alloc(4 * n, FILL)
    sc.trace_nee_device(d_rays, n, d_rgb, d_segments=d_segs, d_shadow=d_shadow, d_rng_state=d_state, **kw)
    sc.collect()
    return dict(rgb=dev.get(d_rgb, np.float32, 3 * n).reshape(n, 3), segments=dev.get(d_segs, np.uint32, n),
                shadow=dev.get(d_shadow, np.uint32, n), states=dev.get(d_state, np.uint64, 4 * n).reshape(n, 4))


def _same(a, b):
    return (a["rgb"].tobytes() == b["rgb"].tobytes() and np.array_equal(a["segments"], b["segments"])
            and np.array_equal(a["shadow"], b["shadow"]) and np.array_equal(a["states"], b["states"]))


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes_and_the_device_form(ndev, oracle, dev, n):
    c = _case(oracle, "spheres")
    rays, st0 = c["rays"][:n], c["st0"][:n]
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        whole = {m: _nee(sc, c["rays"], spp=2, max_bounces=3, rng_state=c["st0"], mode=m) for m in (LIGHT_ONLY, MIS)}
        for mode in (LIGHT_ONLY, MIS):
            host = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=mode)
            assert _same(host, {k: v[:n] for k, v in whole[mode].items() if k != "stats"}), (n, mode, "a ray's result depends on the batch")
            assert _same(_device_nee(sc, dev, rays, st0, spp=2, max_bounces=3, mode=mode), host), (n, mode, "device form")


def test_two_streams_repeated_calls_and_split_samples(ndev, oracle, dev):
    c = _case(oracle, "mixed")
    rays, n = c["rays"], len(c["rays"])
    st_b = R.states(n, 78)
    runs = ((c["st0"], 0, LIGHT_ONLY), (st_b, _abi.RT_FLAG_EXACT_SCAN, MIS))
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        seq = [_nee(sc, rays, spp=2, max_bounces=3, rng_state=s, mode=m, flags=f) for s, f, m in runs]
        assert _same(_nee(sc, rays, spp=2, max_bounces=3, rng_state=c["st0"], mode=LIGHT_ONLY), seq[0])
        bufs = [(dev.put(rays), dev.put(s), dev.alloc(12 * n, FILL), dev.alloc(4 * n, FILL), dev.alloc(4 * n, FILL), dev.stream())
                for s, _, _ in runs]
        dev.sync()
        sc.collect()
        for (d_rays, d_state, d_rgb, d_segs, d_shadow, stream), (_, f, m) in zip(bufs, runs):
            sc.trace_nee_device(d_rays, n, d_rgb, d_segments=d_segs, d_shadow=d_shadow, d_rng_state=d_state, spp=2, max_bounces=3,
                                mode=m, flags=f, stream=stream)
        dev.sync()
        st = sc.collect()
        assert st.n_launches == 2 and st.ray_segments == sum(s["stats"].ray_segments for s in seq)
        for (d_rays, d_state, d_rgb, d_segs, d_shadow, _), want in zip(bufs, seq):
            got = dict(rgb=dev.get(d_rgb, np.float32, 3 * n).reshape(n, 3), segments=dev.get(d_segs, np.uint32, n),
                       shadow=dev.get(d_shadow, np.uint32, n), states=dev.get(d_state, np.uint64, 4 * n).reshape(n, 4))
            assert _same(got, want)
        # with given states, spp = 4 leaves the state that two calls of spp = 2 leave
        for mode in (LIGHT_ONLY, MIS):
            four = _nee(sc, rays, spp=4, max_bounces=3, rng_state=c["st0"], mode=mode)
            a = _nee(sc, rays, spp=2, max_bounces=3, rng_state=c["st0"], mode=mode)
            b = _nee(sc, rays, spp=2, max_bounces=3, rng_state=a["states"], mode=mode)
            assert np.array_equal(four["states"], b["states"])
            assert np.array_equal(four["segments"], a["segments"] + b["segments"]) and np.array_equal(four["shadow"], a["shadow"] + b["shadow"])


def _arrays(out):
    """The arrays of a host-form call's result (a tuple or a dict), the stats left out, as bytes."""
    vals = out.values() if isinstance(out, dict) else out
    return [np.ascontiguousarray(v).tobytes() for v in vals if isinstance(v, np.ndarray)]


def test_interleaved_host_forms_share_one_staging_buffer(ndev):
    """The host forms of all five caller-ray calls stage their arrays in ONE buffer of the scene, carved anew by every call.  Calls of
    all kinds interleaved on one scene, with batch sizes that grow and shrink and optional arrays that come and go, each give the
    bytes of the same call on a fresh scene of the same world: no stale offset, no missed upload, nothing left over from the call
    before."""
    sph, tri = D.lit_room()
    rays = D.camera_rays(64, 48, 0.3, -0.1)[:3000]
    n = len(rays)
    assert n == 3000
    o, d = R.od(rays)
    tm, tx = rays["t_min"], rays["t_max"]
    st = R.states(n, 2900)
    listed = np.random.default_rng(2901).permutation(n)[:2000].astype(np.uint32)
    step = {}                                          # the path step's results on the shared scene: the light sample's inputs

    def bounce(sc):
        out = sc.bounce(rays, st, active=listed, want_hits=True, want_next=True)
        step.setdefault("out", out)
        return out

    calls = [
        ("intersect 1000", lambda sc: sc.intersect(o[:1000], d[:1000], tm[:1000], tx[:1000])),
        ("trace_nee 64", lambda sc: sc.trace_nee(o[:64], d[:64], tm[:64], tx[:64], spp=2, max_bounces=3, rng_state=st[:64])),
        ("bounce 3000, listed", bounce),
        ("direct 3000 on its hits", lambda sc: sc.direct(step["out"]["hits"], step["out"]["states"], active=step["out"]["next"])),
        ("trace 257", lambda sc: sc.trace(o[:257], d[:257], tm[:257], tx[:257], spp=2, max_bounces=3, rng_state=st[:257])),
        ("intersect 1000 again", lambda sc: sc.intersect(o[:1000], d[:1000], tm[:1000], tx[:1000])),
        ("trace_nee 3000, seeded", lambda sc: sc.trace_nee(o, d, tm, tx, spp=1, max_bounces=2, seed=7, mode=LIGHT_ONLY)),
        ("bounce 65, all, seeded", lambda sc: sc.bounce(rays[:65], None, seed=11)),
        ("direct 700, all", lambda sc: sc.direct(step["out"]["hits"][:700], st[:700])),
        ("trace 3000, seeded", lambda sc: sc.trace(o, d, tm, tx, spp=1, max_bounces=2, seed=5)),
        ("any hit 63", lambda sc: sc.intersect(o[:63], d[:63], tm[:63], tx[:63], any_hit=True)),
    ]
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        assert sc.n_lights == 2
        shared = [_arrays(call(sc)) for _, call in calls]
    assert len(step["out"]["next"]) > 100 and len(shared[2]) == 5 and len(shared[3]) == 2
    for (what, call), got in zip(calls, shared):
        with rt.Scene(0, rt.World(sph, tri)) as fresh:
            assert got == _arrays(call(fresh)), what


def test_optional_outputs_and_as_given(ndev, oracle):
    """The counts are optional in the C form, and RT_TRACE_RAY_AS_GIVEN of normalised directions is RT_TRACE_RAY_NEW of the same."""
    import ctypes as C
    c = _case(oracle, "spheres")
    rays, n = _one_window(c["rays"][:300]), 300
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        want = _nee(sc, rays, spp=1, max_bounces=2, seed=3)
        rq = _abi.NeeRequest(1, 2, 3, 0, _abi.RT_TRACE_RAY_NEW, MIS, 0)
        rgb = np.zeros((n, 3), np.float32)
        _abi.check(sc._lib.rt_scene_trace_nee(sc._h, C.byref(rq), rays.ctypes.data_as(C.POINTER(_abi.Ray)), n, None,
                                              rgb.ctypes.data_as(C.POINTER(C.c_float)), None, None, None), "rt_scene_trace_nee")
        assert rgb.tobytes() == want["rgb"].tobytes()
        unit = rays.copy()
        dn = B.directions(rays, False)
        unit["dx"], unit["dy"], unit["dz"] = dn.T
        assert _same(_nee(sc, unit, spp=1, max_bounces=2, rng_state=c["st0"][:n], as_given=True),
                     _nee(sc, rays, spp=1, max_bounces=2, rng_state=c["st0"][:n]))


# ---------------------------------------------------------------- 5. unbiased where the composed recipe is not
def _rooms(which):
    """(spheres, triangles): `plain` the roughness-0 room of tests/_direct_np.py; `glossy` the same room with a ground of roughness
    0.5 and spheres of roughness 0, 0.5 and 1 under its sphere light and its triangle light; `enclosed` that room inside an emissive
    sphere of radius 300 that is only ever hit from inside, so no ray sees the sky."""
    sph, tri = D.lit_room()
    if which == "plain":
        return sph, tri
    sph["roughness"][:4] = [0.5, 0.0, 0.5, 1.0]
    if which == "glossy":
        return sph, tri
    env = np.zeros(1, _abi.SPHERE_DTYPE)
    env["cz"], env["radius"], env["emission"] = -3.0, 300.0, 0.6
    env["albedo_r"], env["albedo_g"], env["albedo_b"] = 0.9, 1.0, 1.0
    return np.concatenate([sph, env]), tri


_MAX_BOUNCES = 3


def _estimates(which, seed):
    """Per ray sample at 2^16 samples (2048 camera rays, 32 samples of each, every estimator in one launch of spp = 1 rays so that the
    samples themselves are at hand for the variances, as tests/test_gpu_direct.py takes them): rt_scene_trace, the two modes, and
    the control."""
    sph, tri = _rooms(which)
    rays = _one_window(_room_rays())
    n = len(rays)
    assert n == 1 << 16
    o, d = R.od(rays)
    lights = LN.Table(sph, tri)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        assert sc.n_lights == lights.M == (3 if which == "enclosed" else 2)
        A = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=_MAX_BOUNCES, rng_state=R.states(n, seed))[0]
        est = {"trace": A.astype(np.float64)}
        for k, mode in enumerate((LIGHT_ONLY, MIS)):
            got = _nee(sc, rays, spp=1, max_bounces=_MAX_BOUNCES, rng_state=R.states(n, seed + 1 + k), mode=mode)
            assert got["stats"].n_launches == 1
            est[mode] = got["rgb"].astype(np.float64)
        est["control"] = _composed_sample(sc, lights, rays, R.states(n, seed + 3), _MAX_BOUNCES, 0, False, recipe="composed")[0].astype(np.float64)
    return est


@pytest.mark.parametrize("which", ["plain", "glossy", "enclosed"])
def test_both_modes_are_unbiased_and_the_composed_recipe_is_not(ndev, which):
    """The bound is that of tests/test_gpu_direct.py: per channel |mean_x - mean_y| <= 5 sqrt(var_x / N + var_y / N) at N = 2^16, the
    variances from the samples themselves.  On the roughness-0 room the control (a sample at every scatter, every later EMITTED
    dropped) is the same estimator as RT_NEE_LIGHT_ONLY and must hold the bound too; with glossy surfaces, or inside an emitter that
    the light sample cannot reach, it must break it."""
    est = _estimates(which, 5100 + len(which))
    for mode in (LIGHT_ONLY, MIS):
        gap, bound = _gap_and_bound(est["trace"], est[mode])
        print(which, "mode", mode, "mean trace", est["trace"].mean(0), "mean", est[mode].mean(0), "gap", gap, "bound", bound)
        assert np.all(gap <= bound), (which, mode, gap, bound)
    gap, bound = _gap_and_bound(est["trace"], est["control"])
    print(which, "control: mean", est["control"].mean(0), "gap", gap, "bound", bound)
    if which == "plain":
        assert np.all(gap <= bound), (which, "control", gap, bound)
    else:
        assert not np.all(gap <= bound), (which, "control", gap, bound)    # (the bound asserted above, violated)


# ---------------------------------------------------------------- 6. variance
def _nee_rays_scene():
    """The scene and the camera of examples/nee_rays.c: a diffuse sphere on a diffuse floor triangle under a small bright light."""
    sph = np.zeros(2, _abi.SPHERE_DTYPE)
    sph["cx"], sph["cy"], sph["cz"], sph["radius"] = [0.0, 1.0], [0.0, 3.0], [-3.0, -2.0], [1.0, 0.3]
    sph["albedo_r"], sph["albedo_g"], sph["albedo_b"] = [0.8, 1.0], [0.3, 1.0], [0.3, 1.0]
    sph["emission"] = [0.0, 20.0]
    tri = np.zeros(1, _abi.TRIANGLE_DTYPE)
    tri["a"][0], tri["b"][0], tri["c"][0] = (-10, -1, 0), (10, -1, 0), (0, -1, -20)
    tri["albedo_r"], tri["albedo_g"], tri["albedo_b"] = 0.5, 0.5, 0.5
    eye, at = np.array([0, 1, 2.0]), np.array([0, 0, -3.0])
    f = (at - eye) / np.linalg.norm(at - eye)
    r = np.cross(f, [0, 1, 0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    half = np.tan(0.5235988)
    ys, xs = np.mgrid[0:32, 0:32]
    sx, sy = ((xs + 0.5) / 32 * 2 - 1) * half, (1 - (ys + 0.5) / 32 * 2) * half
    d = (f + sx[..., None] * r + sy[..., None] * u).reshape(-1, 3).astype(F32)
    return sph, tri, R.make_rays(np.tile(eye.astype(F32), (len(d), 1)), d)


def test_both_modes_have_the_lower_variance_for_a_small_light(ndev):
    sph, tri, rays = _nee_rays_scene()
    rays = np.tile(rays, 16)                                               # 16 384 samples of each estimator, as the example takes
    n = len(rays)
    o, d = R.od(rays)
    lum = lambda rgb: rgb.astype(np.float64).mean(1)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        a = lum(sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=3, rng_state=R.states(n, 6100))[0])
        for k, mode in enumerate((LIGHT_ONLY, MIS)):
            b = lum(_nee(sc, rays, spp=1, max_bounces=3, rng_state=R.states(n, 6101 + k), mode=mode)["rgb"])
            va, vb = a.var(ddof=1), b.var(ddof=1)
            print("mode", mode, "mean trace", a.mean(), "mean", b.mean(), "variance trace", va, "variance", vb, "ratio", va / vb)
            assert vb < va, (mode, va, vb)
            assert abs(a.mean() - b.mean()) <= 5 * np.sqrt(va / n + vb / n)


# ---------------------------------------------------------------- 7. errors and the plain-C client
def test_argument_errors_launch_nothing(ndev, oracle):
    lib = _abi.load()
    c = _case(oracle, "spheres")
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        sc.collect()
        calls = arg_error_calls(lib, sc._h)
        assert {want for _, _, want in calls} == {_abi.RT_ERR_BAD_ARG, _abi.RT_ERR_LIMIT}
        for what, status, want in calls:
            assert status == want, what
        st = sc.collect()
        assert st.n_launches == 0 and st.ray_segments == 0 and st.primary_rays == 0
        assert _nee(sc, c["rays"][:64], spp=1, max_bounces=2)["stats"].n_launches == 1     # the scene still works


def test_plain_c_nee_trace_client(ndev, tmp_path):
    """examples/nee_trace.c through the C-ABI only: the scene of examples/nee_rays.c through both modes and rt_scene_trace."""
    exe = tmp_path / "nee_trace"
    lib = _abi.lib_path().parent
    r = subprocess.run([shutil.which("gcc"), "-std=c99", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "nee_trace.c"),
                        f"-L{lib}", "-lrt_s8", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "NEE_TRACE_OK" in run.stdout, run.stdout + run.stderr
