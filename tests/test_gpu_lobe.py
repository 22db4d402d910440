"""Light samples at glossy hits on the GPU (rt_scene_set_glossy_sampling(RT_GLOSSY_MIS) for rt_scene_trace_nee* in mode RT_NEE_MIS):
1. the kernel against the CPU restatement tests/_lights_np.py with glossy=True (its lobe arithmetic pinned by tests/test_lobe_host.py,
   its bytes by tests/test_light_restatement.py), bit for bit: colours, segment and shadow counts and written-back states on the glossy room of tests/test_gpu_nee.py (a ground of roughness 0.5, spheres of roughness
   0, 0.5 and 1, one sphere light and one triangle light), 300 rays, 2 samples, 3 bounces, given states; with and without
   RT_FLAG_LIGHTS_BY_POWER, under RT_LIGHTS_AREA and RT_LIGHTS_CONE, the four flag sets of tests/test_gpu_bounce.py; host and device
   forms; batches of 1, 63, 64, 65 and 2000 (the first 300 against the restatement, the rest host == device); the seeded streams at
   spp = 3; max_bounces 0, 1 and 3; RT_TRACE_RAY_AS_GIVEN with non-unit directions; a scene of its own with hit records on the
   class boundaries (roughness 2^-24, 1 - 2^-24, 1, -0.5, NaN, and a back-face hit of a rough triangle);
2. invariants: RT_GLOSSY_BOUNCE after RT_GLOSSY_MIS restores the default bytes; RT_NEE_LIGHT_ONLY, Scene.direct, Scene.trace,
   Scene.bounce, Scene.intersect and a strip are byte-identical under both settings; the plain room (every roughness 0), a room with
   roughnesses 0 and 1 only, and M = 0 give RT_GLOSSY_BOUNCE's bytes; no output holds a NaN on the fuzz population of
   tests/_ray_cases.py;
3. statistics at 2^16 samples with the 5 sigma bound of tests/test_gpu_direct.py: under RT_GLOSSY_MIS the integrator agrees with
   rt_scene_trace per channel on the glossy room and on the enclosed room, under either light sampling and either pick; on the glossy
   room var(RT_GLOSSY_BOUNCE) / var(RT_GLOSSY_MIS) > 1 (only the direction is asserted);
4. the plain-C client examples/glossy_lights.c.
Without the feature every test here fails: the entry points do not exist.  No timing is asserted."""
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
import _lobe_np as L
from test_gpu_bounce import CONFIGS, FILL, Dev, dev  # noqa: F401  (dev: a fixture of this module too)
from test_gpu_direct import _gap_and_bound, _room_rays
from test_gpu_nee import _device_nee, _nee, _one_window, _rooms, _same

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
R = B.R
F32 = np.float32
AREA, CONE = _abi.RT_LIGHTS_AREA, _abi.RT_LIGHTS_CONE
BOUNCE, GLOSSY = _abi.RT_GLOSSY_BOUNCE, _abi.RT_GLOSSY_MIS
POWER = _abi.RT_FLAG_LIGHTS_BY_POWER
LIGHT_ONLY, MIS = LN.LIGHT_ONLY, LN.MIS
N_RAYS = 2000
N_NEE = 300                                      # the rays compared with the (per-ray Python) restatement
SIZES = [1, 63, 64, 65, 2000]

_CASE, _REF = {}, {}


def _scene(sph, tri, wi=None, glossy=GLOSSY, lights=AREA):
    sc = rt.Scene(0, rt.World(sph, tri, wi))
    sc.set_light_sampling(lights)
    sc.set_glossy_sampling(glossy)
    return sc


def _case(oracle):
    """The glossy room, camera rays onto it and the wild population of tests/_ray_cases.py mixed in every leading part of the batch,
    and states: made once."""
    if not _CASE:
        sph, tri = _rooms("glossy")
        rays = np.concatenate([D.camera_rays(40, 25, 0.6, -0.1), R.ray_population(oracle, np.random.default_rng(5300), sph, tri, N_RAYS - 1000)[0]])
        rays = np.ascontiguousarray(rays[np.random.default_rng(5200).permutation(N_RAYS)])
        _CASE.update(sph=sph, tri=tri, rays=rays, st0=R.states(N_RAYS, 5400))
    return _CASE


def _ref(oracle, backend, by_power, cone):
    """The restatement on the first N_NEE rays, 2 samples from given states, 3 bounces: once per (backend, pick, light sampling)."""
    key = (backend, by_power, cone)
    if key not in _REF:
        c = _case(oracle)
        _REF[key] = LN.nee(oracle, c["sph"], c["tri"], c["rays"][:N_NEE], 2, 3, backend, None, states=c["st0"][:N_NEE], by_power=by_power,
                          cone=cone, glossy=True)
    return _REF[key]


def _assert_mis(got, want, n, what):
    ok = np.all(B.same_bits(got["rgb"], want["rgb"][MIS][:n]), 1)
    assert ok.all(), (what, np.nonzero(~ok)[0][:5], got["rgb"][~ok][:3], want["rgb"][MIS][:n][~ok][:3])
    assert np.array_equal(got["segments"], want["segments"][:n]) and np.array_equal(got["shadow"], want["shadow"][:n]), what
    if want["states"] is not None:
        assert np.array_equal(got["states"], want["states"][:n]), what


# ---------------------------------------------------------------- 1. the kernel against the restatement
def test_setting_reads_back_and_refuses_other_values(ndev):
    sph, tri = _rooms("glossy")
    lib = _abi.load()
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.collect()
        assert sc.glossy_sampling == BOUNCE                                # the default
        sc.set_glossy_sampling(GLOSSY)
        assert sc.glossy_sampling == GLOSSY and sc.light_sampling == AREA
        assert lib.rt_scene_set_glossy_sampling(sc._h, 2) == _abi.RT_ERR_BAD_ARG and sc.glossy_sampling == GLOSSY
        with pytest.raises(rt.RtError):
            sc.set_glossy_sampling(7)
        sc.set_glossy_sampling(BOUNCE)
        assert sc.glossy_sampling == BOUNCE
        assert sc.collect().n_launches == 0                                # host only


@pytest.mark.parametrize("cone", [False, True], ids=["area", "cone"])
@pytest.mark.parametrize("by_power", [False, True], ids=["uniform", "by_power"])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_mis_is_bit_exact_on_the_glossy_room(ndev, oracle, dev, cfg, by_power, cone):
    flags, engine, backend = CONFIGS[cfg]
    bit = POWER if by_power else 0
    c = _case(oracle)
    want = _ref(oracle, backend, by_power, cone)
    cnt = want["counts"]
    assert cnt["lobe"] > 200 and cnt["diffuse"] > 10 and cnt["none"] > 10 and 0 < cnt["dropped"] < cnt["lobe"], cnt
    assert cnt["emitted_after_lobe"] > 0, cnt                              # (test_class_boundaries has many more of them)
    rays, st0 = c["rays"][:N_NEE], c["st0"][:N_NEE]
    kw = dict(spp=2, max_bounces=3, mode=MIS, flags=flags | bit)
    with _scene(c["sph"], c["tri"], lights=CONE if cone else AREA) as sc:
        assert sc.n_lights == 2
        got = _nee(sc, rays, rng_state=st0, **kw)
        _assert_mis(got, want, N_NEE, (cfg, by_power, cone, "host"))
        st = got["stats"]
        assert st.engine == engine and st.n_launches == 1 and st.primary_rays == 2 * N_NEE
        assert st.ray_segments == int(want["segments"].sum()) + int(want["shadow"].sum())
        assert _same(_device_nee(sc, dev, rays, st0, **kw), got), (cfg, by_power, cone, "device")
        sc.set_glossy_sampling(BOUNCE)                                     # ... and back: the default bytes
        off = _nee(sc, rays, rng_state=st0, **kw)
    with rt.Scene(0, rt.World(c["sph"], c["tri"])) as fresh:               # a scene that never saw the setting
        fresh.set_light_sampling(CONE if cone else AREA)
        base = _nee(fresh, rays, rng_state=st0, **kw)
    assert _same(off, base)
    # the setting is not a no-op: more shadow rays, other states and colours
    assert got["shadow"].sum() > off["shadow"].sum() and not np.array_equal(got["states"], off["states"])
    assert got["rgb"].tobytes() != off["rgb"].tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(ndev, oracle, dev, n):
    c = _case(oracle)
    want = _ref(oracle, 1, True, True)
    m = min(n, N_NEE)
    kw = dict(spp=2, max_bounces=3, mode=MIS, flags=POWER)
    with _scene(c["sph"], c["tri"], lights=CONE) as sc:
        host = _nee(sc, c["rays"][:n], rng_state=c["st0"][:n], **kw)
        _assert_mis({k: v[:m] for k, v in host.items() if k != "stats"}, want, m, ("host", n))
        assert _same(_device_nee(sc, dev, c["rays"][:n], c["st0"][:n], **kw), host), (n, "device")


@pytest.mark.parametrize("max_bounces", [0, 1, 3])
def test_seeded_streams_and_depths(ndev, oracle, max_bounces):
    c = _case(oracle)
    m = 120
    rays = c["rays"][:m]
    want = LN.nee(oracle, c["sph"], c["tri"], rays, 3, max_bounces, 1, None, seed=0x10BE + max_bounces, cone=False, glossy=True)
    given = LN.nee(oracle, c["sph"], c["tri"], rays, 1, max_bounces, 1, None, states=c["st0"][:m], cone=False, glossy=True)
    with _scene(c["sph"], c["tri"]) as sc:
        got = _nee(sc, rays, spp=3, max_bounces=max_bounces, seed=0x10BE + max_bounces, mode=MIS)
        _assert_mis(got, want, m, (max_bounces, "seeded"))
        got1 = _nee(sc, rays, spp=1, max_bounces=max_bounces, rng_state=c["st0"][:m], mode=MIS)
        _assert_mis(got1, given, m, (max_bounces, "given"))
    assert (want["shadow"].sum() > 0) == (max_bounces > 0) and (want["counts"].get("lobe", 0) > 0) == (max_bounces > 0)


def test_ray_as_given_with_non_unit_directions(ndev, oracle, dev):
    c = _case(oracle)
    m = 200
    rays = D.camera_rays(20, 10, 0.6, -0.1).copy()
    scale = np.exp2(np.random.default_rng(5500).integers(-6, 7, m)).astype(F32)
    for f in ("dx", "dy", "dz"):
        rays[f] = rays[f] * scale
    st0 = R.states(m, 5501)
    want = LN.nee(oracle, c["sph"], c["tri"], rays, 2, 3, 1, None, as_given=True, states=st0, cone=True, glossy=True)
    unit = LN.nee(oracle, c["sph"], c["tri"], rays, 2, 3, 1, None, as_given=False, states=st0, cone=True, glossy=True)
    assert want["counts"]["lobe"] > 100 and want["rgb"][MIS].tobytes() != unit["rgb"][MIS].tobytes()
    with _scene(c["sph"], c["tri"], lights=CONE) as sc:
        got = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=MIS, as_given=True)
        _assert_mis(got, want, m, "as given")
        assert _same(_device_nee(sc, dev, rays, st0, spp=2, max_bounces=3, mode=MIS, as_given=True), got)


@pytest.mark.parametrize("cone", [False, True], ids=["area", "cone"])
def test_class_boundaries(ndev, oracle, cone):
    """tests/_lobe_np.py boundary_scene: spheres of roughness 2^-24, 0.5, 1 - 2^-24, 1, -0.5, NaN and 0, and a rough triangle hit on
    both faces; the first step's hits are checked to land on every one of them."""
    sph, tri = L.boundary_scene()
    rays = L.boundary_rays()
    n = len(rays)
    st0 = R.states(n, 5600)
    first = B.step(oracle, sph, tri, rays, st0, 1)
    idx = first["hits"]["index"]
    for k in range(len(L.BOUNDARY_RHOS)):
        assert (idx == k).sum() >= 20, (k, int((idx == k).sum()))
    on_tri = idx == len(sph)
    nd = B._dot(np.stack([first["hits"]["nx"], first["hits"]["ny"], first["hits"]["nz"]], 1), B.directions(rays, False))
    assert (on_tri & (nd > 0)).sum() >= 20 and (on_tri & (nd < 0)).sum() >= 20          # its back and its front
    want = LN.nee(oracle, sph, tri, rays, 2, 3, 1, None, states=st0, cone=cone, glossy=True)
    assert min(want["counts"][k] for k in ("none", "diffuse", "lobe")) > 50, want["counts"]
    assert want["counts"]["emitted_after_lobe"] > 50, want["counts"]
    with _scene(sph, tri, lights=CONE if cone else AREA) as sc:
        got = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=MIS)
        _assert_mis(got, want, n, "boundaries")
        assert not np.isnan(got["rgb"]).any()


# ---------------------------------------------------------------- 2. invariants
def test_other_modes_and_entry_points_ignore_the_setting(ndev, oracle):
    c = _case(oracle)
    rays, st0 = c["rays"][:500], c["st0"][:500]
    o, d = R.od(rays)
    out = []
    with _scene(c["sph"], c["tri"], glossy=BOUNCE) as sc:
        for s in (BOUNCE, GLOSSY, BOUNCE):
            sc.set_glossy_sampling(s)
            rq = _abi.default_request(width=64, height=32, divisions=4, division_no=1, spp=2, max_bounces=3, seed=0x11)
            rgb, f32, st = sc.render_tile(rq, want_f32=True)
            tr = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=2, max_bounces=3, rng_state=st0)
            bn = sc.bounce(rays, st0, want_hits=True, want_next=True)
            dl = sc.direct(bn["hits"], bn["states"], flags=POWER)
            hit = sc.intersect(o, d, rays["t_min"], rays["t_max"])[0]
            lo = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=LIGHT_ONLY)
            mis = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=MIS)
            out.append(((rgb.tobytes(), f32.tobytes(), st.ray_segments, tr[0].tobytes(), tr[1].tobytes(), bn["rays"].tobytes(), bn["states"].tobytes(),
                         bn["bounce"].tobytes(), bn["hits"].tobytes(), bn["next"].tobytes(), dl["direct"].tobytes(), dl["states"].tobytes(),
                         hit.tobytes(), lo["rgb"].tobytes(), lo["segments"].tobytes(), lo["shadow"].tobytes(), lo["states"].tobytes()),
                        (mis["rgb"].tobytes(), mis["states"].tobytes())))
    assert out[0][0] == out[1][0] == out[2][0] and any(out[0][0][0])
    assert out[0][1] == out[2][1] != out[1][1]                             # RT_NEE_MIS alone reads it, and BOUNCE restores its bytes


def _room_without_lobes(which):
    if which == "plain":
        return _rooms("plain")
    sph, tri = _rooms("glossy")
    if which == "rho_0_and_1":
        sph["roughness"][:4] = [1.0, 0.0, 1.0, 0.0]
    else:                                                                  # no_lights: the glossy room with M = 0
        sph["emission"] = 0
        tri["emission"] = 0
    return sph, tri


@pytest.mark.parametrize("which", ["plain", "rho_0_and_1", "no_lights"])
def test_without_lobe_sampled_hits_the_setting_changes_no_byte(ndev, oracle, which):
    sph, tri = _room_without_lobes(which)
    c = _case(oracle)
    rays, st0 = c["rays"], c["st0"]
    out = {}
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        assert sc.n_lights == (0 if which == "no_lights" else 2)
        for s in (BOUNCE, GLOSSY):
            sc.set_glossy_sampling(s)
            out[s] = [_nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=MIS, flags=f) for f in (0, POWER)]
            sc.set_light_sampling(CONE)
            out[s].append(_nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=MIS))
            sc.set_light_sampling(AREA)
    for a, b in zip(out[BOUNCE], out[GLOSSY]):
        assert _same(a, b), which
    assert (out[GLOSSY][0]["shadow"].sum() > 100) == (which != "no_lights")


def test_no_nan_on_the_fuzz_population(ndev, oracle):
    sph, tri, wi, rays, st0 = B.population(oracle, "mixed", N_RAYS, 5700)
    assert {0.0, 1.0} < set(np.concatenate([sph["roughness"], tri["roughness"]]).tolist())   # rough primitives among them
    with _scene(sph, tri, wi) as sc:
        assert sc.n_lights > 2
        for lights in (AREA, CONE):
            sc.set_light_sampling(lights)
            for flags in (0, POWER):
                got = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=MIS, flags=flags)
                assert not np.isnan(got["rgb"]).any() and got["shadow"].sum() > 100, (lights, flags)
        sc.set_glossy_sampling(BOUNCE)
        off = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=MIS, flags=POWER)
    assert got["shadow"].sum() > off["shadow"].sum()


# ---------------------------------------------------------------- 3. statistics
@pytest.mark.parametrize("by_power", [False, True], ids=["uniform", "by_power"])
@pytest.mark.parametrize("lights", [AREA, CONE], ids=["area", "cone"])
@pytest.mark.parametrize("which", ["glossy", "enclosed"])
def test_mis_is_unbiased_under_glossy_mis(ndev, which, lights, by_power):
    """The bound is that of tests/test_gpu_direct.py: per channel |mean_x - mean_y| <= 5 sqrt(var_x / N + var_y / N) at N = 2^16, the
    variances from the samples themselves."""
    sph, tri = _rooms(which)
    rays = _one_window(_room_rays())
    n = len(rays)
    assert n == 1 << 16
    o, d = R.od(rays)
    seed = 8100 + len(which)
    with _scene(sph, tri, lights=lights) as sc:
        trace = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=3, rng_state=R.states(n, seed))[0].astype(np.float64)
        got = _nee(sc, rays, spp=1, max_bounces=3, rng_state=R.states(n, seed + 1), mode=MIS, flags=POWER if by_power else 0)
        sc.set_glossy_sampling(BOUNCE)
        off = _nee(sc, rays, spp=1, max_bounces=3, rng_state=R.states(n, seed + 1), mode=MIS, flags=POWER if by_power else 0)
    est = got["rgb"].astype(np.float64)
    gap, bound = _gap_and_bound(trace, est)
    print(which, "lights", lights, "by_power", by_power, "mean trace", trace.mean(0), "mean", est.mean(0), "gap", gap, "bound", bound,
          "shadow rays", int(got["shadow"].sum()), "without the setting", int(off["shadow"].sum()))
    assert got["shadow"].sum() > 1000 and got["shadow"].sum() > 2 * off["shadow"].sum()    # most of these rooms' hits are glossy
    assert np.all(gap <= bound), (which, lights, by_power, gap, bound)


def test_glossy_mis_has_the_lower_variance_on_the_glossy_room(ndev):
    """2^16 ray samples, max_bounces 3, the same states under either setting: only the direction of var(RT_GLOSSY_BOUNCE) /
    var(RT_GLOSSY_MIS) is asserted; the figures are printed."""
    sph, tri = _rooms("glossy")
    rays = _one_window(_room_rays())
    n = len(rays)
    o, d = R.od(rays)
    lum = lambda rgb: rgb.astype(np.float64).mean(1)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        tr = lum(sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=3, rng_state=R.states(n, 8200))[0])
        var = {}
        for lights in (AREA, CONE):
            sc.set_light_sampling(lights)
            for s in (BOUNCE, GLOSSY):
                sc.set_glossy_sampling(s)
                got = _nee(sc, rays, spp=1, max_bounces=3, rng_state=R.states(n, 8201), mode=MIS)
                x = lum(got["rgb"])
                var[lights, s] = x.var(ddof=1)
                print("lights", lights, "glossy", s, "mean trace", tr.mean(), "mean", x.mean(), "variance trace", tr.var(ddof=1), "variance",
                      var[lights, s], "largest sample", x.max(), "shadow rays", int(got["shadow"].sum()), "kernel ms", got["stats"].kernel_ms)
    for lights in (AREA, CONE):
        print("lights", lights, "var(BOUNCE) / var(GLOSSY_MIS)", var[lights, BOUNCE] / var[lights, GLOSSY])
        assert var[lights, BOUNCE] / var[lights, GLOSSY] > 1, (lights, var)


# ---------------------------------------------------------------- 4. the plain-C client
def test_plain_c_glossy_lights_client(ndev, tmp_path):
    """examples/glossy_lights.c through rt_tile.h and the C-ABI only: the glossy room under both settings next to rt_scene_trace."""
    exe = tmp_path / "glossy_lights"
    lib = _abi.lib_path().parent
    r = subprocess.run([shutil.which("gcc"), "-std=c99", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "glossy_lights.c"),
                        f"-L{lib}", "-lrt_s8", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and "GLOSSY_LIGHTS_OK" in run.stdout, run.stdout + run.stderr
