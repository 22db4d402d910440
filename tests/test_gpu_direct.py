"""Direct lighting of caller rays on the GPU (rt_scene_direct, rt_scene_direct_device):
1. parity, bit for bit, with the CPU restatement tests/_lights_np.py `direct` (its arithmetic pinned by tests/test_direct_host.py, its
   bytes by tests/test_light_restatement.py): every field of rt_direct
   and the states, host form and device form, under four configurations, on one diffuse sphere under one emissive sphere (M = 1), the
   sphere, triangle and mixed (permuted world) scenes of tests/_bounce_np.py, a scene without emitters (M = 0) and a tree deeper than
   the walk's stack (the scan fallback); batch sizes around the wave and workgroup sizes;
2. active lists: sentinel-filled outputs and states keep every byte outside the list, a listed miss is SKIPPED with its state
   unchanged, an index >= n in the device list touches nothing, the next list of a real bounce step goes straight in;
3. composition through public entry points only: rt_scene_intersect of (P, L - P) hits `light` exactly when the status is LIT;
4. the K-step integrator (bounce + direct per step) against the restatement's fold, bit for bit;
5. two streams at once and repeated calls give the same bits;
6. the estimator is unbiased against rt_scene_trace within 5 sigma (and is not without the factor M), and has the lower variance
   for a small light;
7. the argument errors with a live scene, and the plain-C client examples/nee_rays.c."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes

import _bounce_np as B
import _direct_np as D
import _lights_np as LN
from test_direct_surface import bad_arg_calls
from test_gpu_bounce import CONFIGS, FILL, SCAN, SENTINEL_U32, WALK, Dev, dev  # noqa: F401  (dev: a fixture of this module too)

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
R = B.R
N_RAYS = 2000
SIZES = [1, 63, 64, 65, 257, 2000]
SCENES = ("two_spheres", "spheres", "triangles", "mixed", "no_lights", "deep_tree")


def _scene(name):
    """(spheres, triangles, world_index or None, a function (oracle, n, seed) -> rays)."""
    pop = lambda sph, tri, wi: (lambda oracle, n, seed: R.ray_population(oracle, np.random.default_rng(seed), sph, tri, n, wi)[0])
    if name == "two_spheres":
        sph, tri, wi = D.two_spheres()
        return sph, tri, wi, lambda oracle, n, seed: D.camera_rays(50, 40)[:n]
    if name in B.SCENE_NAMES:
        sph, tri, wi = B.scene(name)
        return sph, tri, wi, pop(sph, tri, wi)
    if name == "no_lights":
        sph = scenes.cornell16().copy()
        sph["emission"] = 0.0
        return sph, B.NO_TRI, None, pop(sph, B.NO_TRI, None)
    if name == "deep_tree":
        sph = R.chain_world(70)
        sph["emission"][::9] = 2.5
        return sph, B.NO_TRI, None, lambda oracle, n, seed: R.chain_rays(np.random.default_rng(seed), sph, n)
    raise KeyError(name)


_CASES, _REF = {}, {}


def _case(oracle, name, flags=0):
    """The scene, its rays and states, and — once per (scene, flags) — the hits and advanced states of one bounce step of them (the
    records a caller passes on), made by the library's own step (tests/test_gpu_bounce.py holds it to the CPU reference)."""
    if name not in _CASES:
        sph, tri, wi, make = _scene(name)
        rays = np.ascontiguousarray(make(oracle, N_RAYS, 1700 + len(name)))
        _CASES[name] = dict(sph=sph, tri=tri, wi=wi, rays=rays, st0=R.states(len(rays), 1800 + len(name)), steps={})
    c = _CASES[name]
    if flags not in c["steps"]:
        with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
            c["steps"][flags] = sc.bounce(c["rays"], c["st0"], flags=flags, want_hits=True, want_next=True)
    return c, c["steps"][flags]


def _reference(oracle, name, cfg):
    """The restatement's samples of every record of the case's step: computed once per (scene, configuration), never modified."""
    flags, _, backend = CONFIGS[cfg]
    if (name, cfg) not in _REF:
        c, step = _case(oracle, name, flags)
        _REF[name, cfg] = LN.direct(oracle, c["sph"], c["tri"], step["hits"], step["states"], backend, c["wi"])
    return _REF[name, cfg]


def _assert_equal(got_direct, got_states, want, idx, what):
    ok = D.records_equal(got_direct[idx], want["direct"][idx])
    assert ok.all(), (what, np.asarray(idx)[~ok][:5], got_direct[idx][~ok][:3], want["direct"][idx][~ok][:3])
    assert np.array_equal(got_states[idx], want["states"][idx]), (what, "states")


def _device_direct(sc, dev, hits, states, n, **kw):
    """The device form on fresh buffers, the output sentinel-filled.  Returns (samples, states)."""
    d_hits, d_state, d_out = dev.put(hits), dev.put(states), dev.alloc(32 * n, FILL)
    sc.direct_device(d_hits, n, d_state, d_out, **kw)
    sc.collect()
    return dev.get(d_out, _abi.DIRECT_DTYPE, n), dev.get(d_state, np.uint64, 4 * n).reshape(n, 4)


# ---------------------------------------------------------------- 1. parity with the restatement
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", SCENES)
def test_samples_are_bit_exact(ndev, oracle, dev, name, cfg):
    flags, engine, backend = CONFIGS[cfg]
    c, step = _case(oracle, name, flags)
    want = _reference(oracle, name, cfg)
    n = len(c["rays"])
    every = np.arange(n)
    status = want["direct"]["status"]
    M = len(D.emitters(c["sph"], c["tri"], c["wi"]))
    if name == "deep_tree":
        engine = SCAN                                                      # deeper than the walk's stack: the scan
        assert R.tree_depth(c["sph"], c["tri"]) >= R.trav_stack()
    if name == "no_lights":
        assert M == 0 and set(status.tolist()) == {D.NO_LIGHTS, D.SKIPPED}
    elif name == "two_spheres":
        assert M == 1 and {D.LIT, D.FACING_AWAY, D.SKIPPED} <= set(status.tolist())
    elif name != "deep_tree":
        assert M >= 1 and {D.LIT, D.OCCLUDED, D.FACING_AWAY, D.SKIPPED} <= set(status.tolist()), (name, set(status.tolist()))
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        assert sc.n_lights == M
        got = sc.direct(step["hits"], step["states"], flags=flags)
        _assert_equal(got["direct"], got["states"], want, every, (name, cfg, "host"))
        st = got["stats"]
        assert st.n_launches == 1 and st.primary_rays == 0 and st.ray_segments == int(want["shadow"].sum())
        if M:
            assert st.engine == engine
        if engine == SCAN:
            assert st.broad_candidates == st.ray_segments * (len(c["sph"]) + len(c["tri"]))
        drew = ~np.isin(status, (D.SKIPPED, D.NO_LIGHTS))
        assert np.array_equal(got["states"][~drew], step["states"][~drew])
        assert np.all(np.any(got["states"][drew] != step["states"][drew], 1))
        lit = status == D.LIT
        assert np.all(D.rgb_of(got["direct"])[~lit] == 0)
        d_direct, d_states = _device_direct(sc, dev, step["hits"], step["states"], n, flags=flags)
        assert d_direct.tobytes() == got["direct"].tobytes() and np.array_equal(d_states, got["states"]), (name, cfg, "device")


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(ndev, oracle, dev, n):
    c, step = _case(oracle, "spheres")
    want = _reference(oracle, "spheres", "default")
    hits, states = step["hits"][:n], step["states"][:n]
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        got = sc.direct(hits, states)
        _assert_equal(got["direct"], got["states"], want, np.arange(n), ("host", n))
        d_direct, d_states = _device_direct(sc, dev, hits, states, n)
        _assert_equal(d_direct, d_states, want, np.arange(n), ("device", n))


# ---------------------------------------------------------------- 2. active lists
@pytest.mark.parametrize("n", [65, 2000])
def test_active_lists(ndev, oracle, dev, n):
    c, step = _case(oracle, "spheres")
    want = _reference(oracle, "spheres", "default")
    hits, states = step["hits"][:n], step["states"][:n]
    missed = np.nonzero(hits["index"] == _abi.RT_HIT_NONE)[0]
    assert len(missed)
    g = np.random.default_rng(n)
    listed = np.concatenate([missed[:3], g.permutation(np.setdiff1d(np.arange(0, n, 3), missed[:3]))]).astype(np.uint32)   # misses first
    rest = np.setdiff1d(np.arange(n), listed)
    junk = np.full((n, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
    mixed_states = np.where(np.isin(np.arange(n), listed)[:, None], states, junk)      # sentinel states outside the list
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        # (a) the device form: a list longer than its device-side length, with indices >= n among the entries taken
        wild = np.concatenate([listed[:5], [n, n + 7, 0xFFFFFFFF], listed[5:]]).astype(np.uint32)
        used = len(wild) - len(listed) // 4
        stepped = np.sort(wild[:used][wild[:used] < n]).astype(np.int64)
        untouched = np.setdiff1d(np.arange(n), stepped)
        d_list, d_len = dev.put(wild), dev.put(np.array([used], np.uint32))
        got, got_states = _device_direct(sc, dev, hits, mixed_states, n, d_active=d_list, d_n_active=d_len)
        _assert_equal(got, got_states, want, stepped, ("device list", n))
        assert set(got[untouched].tobytes()) <= {FILL} and np.array_equal(got_states[untouched], mixed_states[untouched])
        skipped = np.intersect1d(stepped, missed)
        assert len(skipped) and np.all(got["status"][skipped] == D.SKIPPED) and np.all(got["light"][skipped] == _abi.RT_HIT_NONE)
        assert not any(D.rgb_of(got)[skipped].tobytes()) and np.array_equal(got_states[skipped], states[skipped])
        # (b) a device-side length of 0 touches nothing
        got, got_states = _device_direct(sc, dev, hits, mixed_states, n, d_active=d_list, d_n_active=dev.put(np.array([0], np.uint32)))
        assert set(got.tobytes()) <= {FILL} and np.array_equal(got_states, mixed_states)
        # (c) the host form: records outside the list come back as they went in
        h = sc.direct(hits, mixed_states, active=listed)
        _assert_equal(h["direct"], h["states"], want, np.sort(listed).astype(np.int64), ("host list", n))
        assert not any(h["direct"][rest].tobytes()) and np.array_equal(h["states"][rest], junk[rest])
        assert h["stats"].ray_segments == int(want["shadow"][listed].sum())
        h = sc.direct(hits, states, active=[])
        assert not any(h["direct"].tobytes()) and np.array_equal(h["states"], states) and h["stats"].ray_segments == 0


def test_next_list_of_a_bounce_step_goes_straight_in(ndev, oracle, dev):
    """rt_scene_bounce_device then rt_scene_direct_device on one stream, the step's d_next_active / d_n_next as the active list, no
    host synchronisation in between: the samples of exactly the rays that scattered."""
    c, step = _case(oracle, "mixed")
    want = _reference(oracle, "mixed", "default")
    n = len(c["rays"])
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        d_rays, d_state = dev.put(c["rays"]), dev.put(c["st0"])
        d_bnc, d_hits, d_next, d_n_next = dev.alloc(16 * n, FILL), dev.alloc(32 * n, FILL), dev.alloc(4 * n, FILL), dev.put(np.array([99], np.uint32))
        d_out = dev.alloc(32 * n, FILL)
        sc.collect()
        sc.bounce_device(d_rays, n, d_state, d_bnc, d_hits=d_hits, d_next_active=d_next, d_n_next=d_n_next)
        sc.direct_device(d_hits, n, d_state, d_out, d_active=d_next, d_n_active=d_n_next)
        st = sc.collect()
        got, got_states = dev.get(d_out, _abi.DIRECT_DTYPE, n), dev.get(d_state, np.uint64, 4 * n).reshape(n, 4)
        scat = step["next"].astype(np.int64)
        rest = np.setdiff1d(np.arange(n), scat)
        assert 0 < len(scat) < n and st.n_launches == 2
        _assert_equal(got, got_states, want, scat, "after a bounce step")
        assert set(got[rest].tobytes()) <= {FILL} and np.array_equal(got_states[rest], step["states"][rest])
        assert st.ray_segments == n + int(want["shadow"][scat].sum())


# ---------------------------------------------------------------- 3. composition through public entry points
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", ["spheres", "mixed"])
def test_lit_exactly_when_the_public_query_hits_the_light(ndev, oracle, name, cfg):
    flags = CONFIGS[cfg][0]
    c, step = _case(oracle, name, flags)
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        d = sc.direct(step["hits"], step["states"], flags=flags, t_min=0.002, t_max=500.0)["direct"]
        traced = np.isin(d["status"], (D.LIT, D.OCCLUDED))
        assert (d["status"] == D.LIT).sum() > 10 and (d["status"] == D.OCCLUDED).sum() > 10
        h = step["hits"][traced]
        P = np.stack([h["px"], h["py"], h["pz"]], 1).astype(np.float32)
        L = np.stack([d["lx"], d["ly"], d["lz"]], 1).astype(np.float32)[traced]
        q, _ = sc.intersect(P, L - P, 0.002, 500.0, flags=flags)
        assert np.array_equal(q["index"] == d["light"][traced], d["status"][traced] == D.LIT)


# ---------------------------------------------------------------- 4. the K-step integrator
@pytest.mark.parametrize("cfg", ["default", "no_bvh_cull"])
def test_k_step_integrator_equals_the_restatement(ndev, oracle, cfg):
    flags, _, backend = CONFIGS[cfg]
    c, _ = _case(oracle, "spheres", flags)
    rays, st0 = c["rays"][:500], c["st0"][:500]
    sph, tri, wi = c["sph"], c["tri"], c["wi"]
    want_rgb, want_states = D.integrate(
        lambda r, s, act, given: B.step(oracle, sph, tri, r, s, backend, wi, as_given=given, active=act),
        lambda h, s, act: LN.direct(oracle, sph, tri, h, s, backend, wi, active=act), rays, st0, 3)
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        got_rgb, got_states = D.integrate(
            lambda r, s, act, given: sc.bounce(r, s, active=act, as_given=given, flags=flags, want_hits=True),
            lambda h, s, act: sc.direct(h, s, active=act, flags=flags), rays, st0, 3)
    ok = np.all(B.same_bits(got_rgb, want_rgb), 1)
    assert ok.all(), (cfg, np.nonzero(~ok)[0][:5], got_rgb[~ok][:3], want_rgb[~ok][:3])
    assert np.array_equal(got_states, want_states)
    assert (want_rgb.sum(1) > 0).sum() > 100


# ---------------------------------------------------------------- 5. overlap and repetition
def test_two_streams_and_repeated_calls(ndev, oracle, dev):
    c, step = _case(oracle, "mixed")
    n = len(c["rays"])
    st_b = R.states(n, 77)
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        seq = [sc.direct(step["hits"], s, flags=f) for s, f in ((step["states"], 0), (st_b, _abi.RT_FLAG_EXACT_SCAN))]
        again = sc.direct(step["hits"], step["states"])
        assert again["direct"].tobytes() == seq[0]["direct"].tobytes() and np.array_equal(again["states"], seq[0]["states"])
        runs = [(dev.put(step["hits"]), dev.put(s), dev.alloc(32 * n, FILL), dev.stream(), f)
                for s, f in ((step["states"], 0), (st_b, _abi.RT_FLAG_EXACT_SCAN))]
        dev.sync()
        sc.collect()
        for d_hits, d_state, d_out, stream, f in runs:
            sc.direct_device(d_hits, n, d_state, d_out, flags=f, stream=stream)
        dev.sync()
        st = sc.collect()
        assert st.n_launches == 2 and st.ray_segments == sum(s["stats"].ray_segments for s in seq)
        for (d_hits, d_state, d_out, _, _), want in zip(runs, seq):
            assert dev.get(d_out, _abi.DIRECT_DTYPE, n).tobytes() == want["direct"].tobytes()
            assert np.array_equal(dev.get(d_state, np.uint64, 4 * n).reshape(n, 4), want["states"])


# ---------------------------------------------------------------- 6. unbiasedness and benefit
def _estimators(sc, rays, seed, M):
    """Per ray sample: A = rt_scene_trace with max_bounces = 1; B = step, direct x albedo, then a second step counted only when it
    MISSED (the first step's EMITTED and MISSED terms as they are); B_noM = B with the sample's factor M taken out again."""
    n = len(rays)
    o, d = R.od(rays)
    A = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=1, rng_state=R.states(n, seed))[0].astype(np.float64)
    s1 = sc.bounce(rays, R.states(n, seed + 1), want_hits=True, want_next=True)
    nxt = s1["next"]
    dl = sc.direct(s1["hits"], s1["states"], active=nxt)
    s2 = sc.bounce(s1["rays"], dl["states"], active=nxt, as_given=True)
    a1 = B.rgb_of(s1["bounce"]).astype(np.float64)
    sky2 = np.where((s2["bounce"]["status"] == B.MISSED)[:, None], B.rgb_of(s2["bounce"]), 0).astype(np.float64)
    direct = D.rgb_of(dl["direct"]).astype(np.float64)
    scat = (s1["bounce"]["status"] == B.SCATTERED)[:, None]
    Bv = np.where(scat, a1 * (direct + sky2), a1)
    B_noM = np.where(scat, a1 * (direct / M + sky2), a1)
    return A, Bv, B_noM


def _gap_and_bound(x, y):
    """Per channel: |mean_x - mean_y| and 5 sqrt(var_x / N_x + var_y / N_y), the variances from the samples themselves."""
    return np.abs(x.mean(0) - y.mean(0)), 5 * np.sqrt(x.var(0, ddof=1) / len(x) + y.var(0, ddof=1) / len(y))


def _room_rays():
    """2^16 ray samples of 2 048 fixed camera rays.  The view is narrow and pitched down onto the three spheres and the ground around
    them, within about 2 units of the emissive sphere, so that direct light is a large part of what every ray sees: the negative
    control needs that.  Without the factor M = 2 estimator B loses half its direct light, about 0.15 a (a the albedo: irradiance
    Le r^2 / d^2 = 6 * 0.25 / 4 under the light, less around it, halved), against a bound of 5 sqrt(var_A / N) of about 0.03 a
    (A finds the light with probability p of about 0.05 and then returns Le: variance p Le^2 a^2 = 1.8 a^2, N = 2^16).  A view that is
    mostly sky and far ground has no such power: there the direct light is a few per cent of the mean."""
    return np.tile(D.camera_rays(64, 32, 0.3, -0.1), 32)


def test_estimate_is_unbiased(ndev):
    sph, tri = D.lit_room()
    assert np.all(sph["roughness"] == 0) and np.all(tri["roughness"] == 0)
    rays = _room_rays()
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        M = sc.n_lights
        assert M == 2
        A, Bv, B_noM = _estimators(sc, rays, 4100, M)
    gap, bound = _gap_and_bound(A, Bv)
    print("unbiasedness: mean A", A.mean(0), "mean B", Bv.mean(0), "gap", gap, "bound", bound)
    assert np.all(gap <= bound), (gap, bound)
    gap0, bound0 = _gap_and_bound(A, B_noM)                                # the negative control: without the factor M
    print("without the factor M: gap", gap0, "bound", bound0)
    assert not np.all(gap0 <= bound0), (gap0, bound0)                     # (the bound asserted above, violated)


def test_small_light_has_the_lower_variance(ndev):
    sph, tri = D.lit_room(light_radius=0.1)
    rays = _room_rays()
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        A, Bv, _ = _estimators(sc, rays, 4200, sc.n_lights)
    va, vb = A.var(0, ddof=1), Bv.var(0, ddof=1)
    print("variance A", va, "variance B", vb, "ratio", va / vb)
    # (for the record, not asserted: the variance WITHIN a camera ray's 32 samples, which leaves the image's own variance out)
    wa, wb = (x.reshape(32, -1, 3).var(0, ddof=1).mean(0) for x in (A, Bv))
    print("within-ray variance A", wa, "B", wb, "ratio", wa / wb)
    assert np.all(vb < va), (va, vb)


# ---------------------------------------------------------------- 7. errors and the plain-C client
def test_argument_errors_launch_nothing(ndev, oracle):
    lib = _abi.load()
    c, step = _case(oracle, "spheres")
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        sc.collect()
        for what, status in bad_arg_calls(lib, sc._h):
            assert status == _abi.RT_ERR_BAD_ARG, what
        st = sc.collect()
        assert st.n_launches == 0 and st.ray_segments == 0
        with pytest.raises(_abi.RtError):
            sc.direct(step["hits"], step["states"], active=[len(step["hits"])])
        assert sc.direct(step["hits"], step["states"])["stats"].n_launches == 1    # the scene still works


def test_plain_c_nee_client(ndev, tmp_path):
    """examples/nee_rays.c through the C-ABI only: K host-form steps with a direct-light call after each, folded, its mean next to
    rt_scene_trace of the same rays."""
    exe = tmp_path / "nee_rays"
    lib = _abi.lib_path().parent
    r = subprocess.run([shutil.which("gcc"), "-std=c99", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "nee_rays.c"),
                        f"-L{lib}", "-lrt_s8", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "NEE_OK" in run.stdout, run.stdout + run.stderr
