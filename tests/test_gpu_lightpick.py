"""Light selection by power on the GPU (RT_FLAG_LIGHTS_BY_POWER in rt_scene_direct*, rt_scene_trace_nee*; rt_scene_light_table):
1. both kernels against the CPU restatement tests/_lights_np.py with by_power=True (its table, pick and weights pinned by
   tests/test_lightpick_host.py, its bytes by tests/test_light_restatement.py), bit for bit: every rt_direct field and the states, the NEE colours of both modes, segment and shadow counts and states; M = 2 (one sphere, one triangle light) and
   M = 33 (mixed kinds, an emitter of albedo 0, one of radius 0, emissions over six decades, a permuted world_index); the four flag sets
   of tests/test_gpu_direct.py each with the bit; host and device forms; batches of 1, 63, 64, 65 and 2000 records; active lists; the
   next list of a bounce step passed straight in.  Without the feature the flag changes nothing and these fail;
2. M = 1 and the degenerate tables: the flag's output is the flag-off output, bit for bit;
3. RT_NEE_LIGHT_ONLY with the flag is the fold of Scene.bounce and Scene.direct with the flag (the fold of tests/test_gpu_nee.py);
4. rt_scene_light_table equals the restatement, refuses a small capacity, and the `light` field of 2^16 independent samples is
   distributed as p;
5. unbiased against rt_scene_trace on a room with one lamp and 32 dim emitters (5 sigma at 2^16 samples), where forgetting the pmf is
   not; and there the variance is lower with the flag than without, for direct and for both NEE modes;
6. a tile entry point ignores the bit; the plain-C client examples/many_lights.c."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes

import _bounce_np as B
import _direct_np as D
import _lightpick_np as LP
import _lights_np as LN
from test_gpu_bounce import CONFIGS, FILL, Dev, dev  # noqa: F401  (dev: a fixture of this module too)
from test_gpu_direct import _assert_equal as _assert_direct, _device_direct, _gap_and_bound, _room_rays
from test_gpu_nee import _composed_sample, _device_nee, _nee, _one_window, _same

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
R = B.R
F32 = np.float32
BIT = _abi.RT_FLAG_LIGHTS_BY_POWER
LIGHT_ONLY, MIS = LN.LIGHT_ONLY, LN.MIS
N_RAYS = 2000
N_NEE = 600                                      # the rays of the NEE comparisons with the (per-ray Python) restatement
SIZES = [1, 63, 64, 65, 2000]
SCENES = {"two_lights": LP.two_lights, "many_lights": LP.many_lights}

_CASES, _REF = {}, {}


def _case(oracle, name, flags=0):
    """The scene, its rays (camera rays onto the room and the wild population of tests/_ray_cases.py, each in its own window) and
    states, and — once per (scene, flags) — the hits and advanced states of one bounce step of them, by the library's own step."""
    if name not in _CASES:
        sph, tri, wi = SCENES[name]()
        rays = np.concatenate([D.camera_rays(40, 25, 0.6, -0.1),
                               R.ray_population(oracle, np.random.default_rng(3300 + len(name)), sph, tri, N_RAYS - 1000, wi)[0]])
        rays = rays[np.random.default_rng(3200).permutation(N_RAYS)]       # both kinds in every leading part of the batch
        _CASES[name] = dict(sph=sph, tri=tri, wi=wi, rays=np.ascontiguousarray(rays), st0=R.states(N_RAYS, 3400 + len(name)), steps={})
    c = _CASES[name]
    if flags not in c["steps"]:
        with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
            c["steps"][flags] = sc.bounce(c["rays"], c["st0"], flags=flags, want_hits=True, want_next=True)
    return c, c["steps"][flags]


def _ref_direct(oracle, name, cfg):
    """The restatement's samples of every record of the case's step: once per (scene, configuration), never modified."""
    flags, _, backend = CONFIGS[cfg]
    if ("direct", name, cfg) not in _REF:
        c, step = _case(oracle, name, flags)
        _REF["direct", name, cfg] = LN.direct(oracle, c["sph"], c["tri"], step["hits"], step["states"], backend, c["wi"],
                                               by_power=True)
    return _REF["direct", name, cfg]


def _ref_nee(oracle, name, backend):
    """The restatement on the first N_NEE rays of the case, 2 samples from given states, 3 bounces: once per (scene, backend)."""
    if ("nee", name, backend) not in _REF:
        c, _ = _case(oracle, name)
        _REF["nee", name, backend] = LN.nee(oracle, c["sph"], c["tri"], c["rays"][:N_NEE], 2, 3, backend, c["wi"], states=c["st0"][:N_NEE],
                                             by_power=True)
    return _REF["nee", name, backend]


def _assert_nee(got, want, mode, n, what):
    ok = np.all(B.same_bits(got["rgb"], want["rgb"][mode][:n]), 1)
    assert ok.all(), (what, np.nonzero(~ok)[0][:5], got["rgb"][~ok][:3], want["rgb"][mode][:n][~ok][:3])
    assert np.array_equal(got["segments"], want["segments"][:n]) and np.array_equal(got["shadow"], want["shadow"][:n]), what
    assert np.array_equal(got["states"], want["states"][:n]), what


# ---------------------------------------------------------------- 1. both kernels against the restatement
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", SCENES)
def test_direct_is_bit_exact(ndev, oracle, dev, name, cfg):
    flags, engine, _ = CONFIGS[cfg]
    c, step = _case(oracle, name, flags)
    want = _ref_direct(oracle, name, cfg)
    n = len(c["rays"])
    status = want["direct"]["status"]
    assert {D.LIT, D.OCCLUDED, D.FACING_AWAY, D.SKIPPED} <= set(status.tolist()), (name, set(status.tolist()))
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        assert sc.n_lights == (2 if name == "two_lights" else 33)
        got = sc.direct(step["hits"], step["states"], flags=flags | BIT)
        _assert_direct(got["direct"], got["states"], want, np.arange(n), (name, cfg, "host"))
        st = got["stats"]
        assert st.n_launches == 1 and st.engine == engine and st.ray_segments == int(want["shadow"].sum())
        d_direct, d_states = _device_direct(sc, dev, step["hits"], step["states"], n, flags=flags | BIT)
        assert d_direct.tobytes() == got["direct"].tobytes() and np.array_equal(d_states, got["states"]), (name, cfg, "device")
        # the flag is not a no-op: the uniform pick names other lights, and where it names the same one the weight differs
        off = sc.direct(step["hits"], step["states"], flags=flags)["direct"]
        drew = ~np.isin(status, (D.SKIPPED, D.NO_LIGHTS))
        assert (off["light"][drew] != got["direct"]["light"][drew]).mean() > 0.2
        lit = (off["status"] == D.LIT) & (status == D.LIT) & (off["light"] == got["direct"]["light"])
        assert lit.sum() > 10 and np.all(D.rgb_of(off)[lit] != D.rgb_of(got["direct"])[lit])
    if name == "many_lights":                                              # every emitter is picked, those without power too
        assert len(np.unique(want["direct"]["light"][drew])) == 33


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", SCENES)
def test_nee_is_bit_exact_in_both_modes(ndev, oracle, dev, name, cfg):
    flags, engine, backend = CONFIGS[cfg]
    c, _ = _case(oracle, name)
    want = _ref_nee(oracle, name, backend)
    rays, st0 = c["rays"][:N_NEE], c["st0"][:N_NEE]
    assert len(np.unique(rays["t_max"])) > 10                              # the rays keep their own windows
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        for mode in (LIGHT_ONLY, MIS):
            got = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=mode, flags=flags | BIT)
            _assert_nee(got, want, mode, N_NEE, (name, cfg, mode, "host"))
            st = got["stats"]
            assert st.engine == engine and st.n_launches == 1 and st.primary_rays == 2 * N_NEE
            assert st.ray_segments == int(want["segments"].sum()) + int(want["shadow"].sum())
            assert _same(_device_nee(sc, dev, rays, st0, spp=2, max_bounces=3, mode=mode, flags=flags | BIT), got), (name, cfg, mode, "device")
            off = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=mode, flags=flags)
            assert off["rgb"].tobytes() != got["rgb"].tobytes()            # the flag is not a no-op
    assert want["shadow"].sum() > 100 and not np.array_equal(want["rgb"][LIGHT_ONLY], want["rgb"][MIS])


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(ndev, oracle, dev, n):
    c, step = _case(oracle, "many_lights")
    want = _ref_direct(oracle, "many_lights", "default")
    hits, states = step["hits"][:n], step["states"][:n]
    m = min(n, N_NEE)
    want_nee = _ref_nee(oracle, "many_lights", 1)
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        got = sc.direct(hits, states, flags=BIT)
        _assert_direct(got["direct"], got["states"], want, np.arange(n), ("host", n))
        d_direct, d_states = _device_direct(sc, dev, hits, states, n, flags=BIT)
        _assert_direct(d_direct, d_states, want, np.arange(n), ("device", n))
        rays, st0 = c["rays"][:m], c["st0"][:m]
        for mode in (LIGHT_ONLY, MIS):
            host = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=mode, flags=BIT)
            _assert_nee(host, want_nee, mode, m, ("nee host", n, mode))
            assert _same(_device_nee(sc, dev, rays, st0, spp=2, max_bounces=3, mode=mode, flags=BIT), host), (n, mode, "nee device")
        if n == 2000:                                                      # a ray's result does not depend on the batch
            whole = _nee(sc, c["rays"], spp=2, max_bounces=3, rng_state=c["st0"], mode=MIS, flags=BIT)
            assert _same({k: v[:m] for k, v in whole.items() if k != "stats"}, host)


@pytest.mark.parametrize("n", [65, 2000])
def test_active_lists(ndev, oracle, dev, n):
    c, step = _case(oracle, "many_lights")
    want = _ref_direct(oracle, "many_lights", "default")
    hits, states = step["hits"][:n], step["states"][:n]
    g = np.random.default_rng(n)
    listed = g.permutation(np.arange(0, n, 3)).astype(np.uint32)
    rest = np.setdiff1d(np.arange(n), listed)
    junk = np.full((n, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
    mixed = np.where(np.isin(np.arange(n), listed)[:, None], states, junk)
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        # the device form: a list longer than its device-side length, with indices >= n among the entries taken
        wild = np.concatenate([listed[:5], [n, n + 7, 0xFFFFFFFF], listed[5:]]).astype(np.uint32)
        used = len(wild) - len(listed) // 4
        stepped = np.sort(wild[:used][wild[:used] < n]).astype(np.int64)
        untouched = np.setdiff1d(np.arange(n), stepped)
        got, got_states = _device_direct(sc, dev, hits, mixed, n, d_active=dev.put(wild), d_n_active=dev.put(np.array([used], np.uint32)),
                                         flags=BIT)
        _assert_direct(got, got_states, want, stepped, ("device list", n))
        assert set(got[untouched].tobytes()) <= {FILL} and np.array_equal(got_states[untouched], mixed[untouched])
        # the host form: records outside the list come back as they went in
        h = sc.direct(hits, mixed, active=listed, flags=BIT)
        _assert_direct(h["direct"], h["states"], want, np.sort(listed).astype(np.int64), ("host list", n))
        assert not any(h["direct"][rest].tobytes()) and np.array_equal(h["states"][rest], junk[rest])
        assert h["stats"].ray_segments == int(want["shadow"][listed].sum())


def test_next_list_of_a_bounce_step_goes_straight_in(ndev, oracle, dev):
    c, step = _case(oracle, "many_lights")
    want = _ref_direct(oracle, "many_lights", "default")
    n = len(c["rays"])
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        d_rays, d_state = dev.put(c["rays"]), dev.put(c["st0"])
        d_bnc, d_hits, d_next, d_n_next = dev.alloc(16 * n, FILL), dev.alloc(32 * n, FILL), dev.alloc(4 * n, FILL), dev.put(np.array([99], np.uint32))
        d_out = dev.alloc(32 * n, FILL)
        sc.collect()
        sc.bounce_device(d_rays, n, d_state, d_bnc, d_hits=d_hits, d_next_active=d_next, d_n_next=d_n_next, flags=BIT)   # (ignored there)
        sc.direct_device(d_hits, n, d_state, d_out, d_active=d_next, d_n_active=d_n_next, flags=BIT)
        st = sc.collect()
        got, got_states = dev.get(d_out, _abi.DIRECT_DTYPE, n), dev.get(d_state, np.uint64, 4 * n).reshape(n, 4)
        scat = step["next"].astype(np.int64)
        rest = np.setdiff1d(np.arange(n), scat)
        assert 0 < len(scat) < n and st.n_launches == 2
        _assert_direct(got, got_states, want, scat, "after a bounce step")
        assert set(got[rest].tobytes()) <= {FILL} and np.array_equal(got_states[rest], step["states"][rest])


# ---------------------------------------------------------------- 2. where the flag changes nothing
def _degenerate_scene(kind):
    """LP.many_lights with a table that is degenerate: every emitter's albedo 0, a running sum that overflows, one infinite power."""
    sph, tri, wi = LP.many_lights()
    em = sph["emission"] > 0
    if kind == "zero":
        for a in (sph, tri):
            a["albedo_r"][a["emission"] > 0], a["albedo_g"][a["emission"] > 0], a["albedo_b"][a["emission"] > 0] = 0, 0, 0
    elif kind == "overflow":
        sph["emission"][em] = 2e37
        sph["radius"][em] = 0.2
        sph["albedo_r"][em], sph["albedo_g"][em], sph["albedo_b"][em] = 0.9, 0.9, 0.9
    else:
        sph["emission"][np.nonzero(em)[0][0]] = np.inf
    return sph, tri, wi


@pytest.mark.parametrize("which", ["two_spheres", "cornell16", "zero", "overflow", "inf"])
def test_flag_changes_no_bit_with_one_emitter_or_a_degenerate_table(ndev, oracle, which):
    if which == "two_spheres":
        sph, tri, wi = D.two_spheres()
        rays = D.camera_rays(50, 40)[:N_RAYS]
    elif which == "cornell16":
        sph, tri, wi = scenes.cornell16(), B.NO_TRI, None
        rays = R.ray_population(oracle, np.random.default_rng(77), sph, tri, N_RAYS, wi)[0]
    else:
        sph, tri, wi = _degenerate_scene(which)
        rays = _case(oracle, "many_lights")[0]["rays"]
        t = LN.Table(sph, tri, wi)
        assert t.degenerate and t.M == 33 and np.all(t.ip == F32(33))
        if which == "overflow":
            assert np.all(np.isfinite(t.q))
    rays = np.ascontiguousarray(rays)
    n = len(rays)
    st0 = R.states(n, 3500)
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        if which in ("two_spheres", "cornell16"):
            assert sc.n_lights == 1
        step = sc.bounce(rays, st0, want_hits=True)
        a, b = (sc.direct(step["hits"], step["states"], flags=f) for f in (0, BIT))
        assert a["direct"].tobytes() == b["direct"].tobytes() and np.array_equal(a["states"], b["states"])
        assert (a["direct"]["status"] == D.LIT).sum() > 10
        for mode in (LIGHT_ONLY, MIS):
            x, y = (_nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=mode, flags=f) for f in (0, BIT))
            assert _same(x, y), (which, mode)
            assert x["shadow"].sum() > 10
        wi_t, p = sc.light_table(BIT)
        assert np.all(p == F32(1) / F32(sc.n_lights)) and p.tobytes() == sc.light_table(0)[1].tobytes()


# ---------------------------------------------------------------- 3. LIGHT_ONLY is the fold of the entry points, with the flag
@pytest.mark.parametrize("cfg", ["default", "no_bvh_cull"])
def test_light_only_is_the_fold_of_bounce_and_direct_with_the_flag(ndev, oracle, cfg):
    flags = CONFIGS[cfg][0] | BIT
    c, _ = _case(oracle, "many_lights")
    rays = _one_window(c["rays"])
    n = len(rays)
    lights = LN.Table(c["sph"], c["tri"], c["wi"])
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as sc:
        for max_bounces in (1, 3):
            want_c, want_segs, want_shadow, want_states = _composed_sample(sc, lights, rays, c["st0"], max_bounces, flags, False)
            got = _nee(sc, rays, spp=1, max_bounces=max_bounces, rng_state=c["st0"], mode=LIGHT_ONLY, flags=flags)
            want_rgb = (np.zeros((n, 3), F32) + want_c).astype(F32)
            ok = np.all(B.same_bits(got["rgb"], want_rgb), 1)
            assert ok.all(), (cfg, max_bounces, np.nonzero(~ok)[0][:5], got["rgb"][~ok][:3], want_rgb[~ok][:3])
            assert np.array_equal(got["segments"], want_segs) and np.array_equal(got["shadow"], want_shadow)
            assert np.array_equal(got["states"], want_states)
            assert want_shadow.sum() > 100 and (want_c.sum(1) > 0).sum() > 100
        # (the same fold without the flag gives other colours: the comparison above is not vacuous)
        off = _nee(sc, rays, spp=1, max_bounces=3, rng_state=c["st0"], mode=LIGHT_ONLY, flags=flags & ~BIT)
        assert off["rgb"].tobytes() != got["rgb"].tobytes()


# ---------------------------------------------------------------- 4. the table, and the lights drawn
@pytest.mark.parametrize("name", SCENES)
def test_light_table_equals_the_restatement(ndev, name):
    sph, tri, wi = SCENES[name]()
    t = LN.Table(sph, tri, wi)
    lib = _abi.load()
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        sc.collect()
        got_wi, got_p = sc.light_table(BIT)
        assert np.array_equal(got_wi, t.world_index) and B.same_bits(got_p, t.p).all()
        off_wi, off_p = sc.light_table(0)
        assert np.array_equal(off_wi, t.world_index) and np.all(off_p == F32(1) / F32(t.M))
        M = t.M
        buf_wi, buf_p = np.full(M + 1, 7, np.uint32), np.full(M + 1, 7, F32)
        u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        assert lib.rt_scene_light_table(sc._h, BIT, buf_wi.ctypes.data_as(u32p), buf_p.ctypes.data_as(f32p), M - 1) == _abi.RT_ERR_BAD_ARG
        assert np.all(buf_wi == 7) and np.all(buf_p == 7)
        assert lib.rt_scene_light_table(sc._h, BIT, None, buf_p.ctypes.data_as(f32p), M + 1) == _abi.RT_OK     # either output alone
        assert lib.rt_scene_light_table(sc._h, BIT, buf_wi.ctypes.data_as(u32p), None, M) == _abi.RT_OK
        assert np.array_equal(buf_wi[:M], t.world_index) and buf_wi[M] == 7 and B.same_bits(buf_p[:M], t.p).all() and buf_p[M] == 7
        assert sc.collect().n_launches == 0                                # host only


def test_lights_are_drawn_with_the_tables_probability(ndev):
    """2^16 independent samples at one hit record: the count of emitter k is binomial (N, p_k), so |count - N p_k| <=
    5 sqrt(N p_k (1 - p_k)) + 1 for every k (5 sigma, and 1 for the discreteness of a count whose sigma is small)."""
    sph, tri, wi = LP.many_lights()
    n = 1 << 16
    hits = np.zeros(n, _abi.HIT_DTYPE)
    hits["px"], hits["py"], hits["pz"], hits["ny"], hits["distance"], hits["index"] = 0.0, 0.6, -3.0, 1.0, 3.0, 0
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        world, p = sc.light_table(BIT)
        d = sc.direct(hits, R.states(n, 3600), flags=BIT)["direct"]
        u = sc.direct(hits, R.states(n, 3600), flags=0)["direct"]
    p = p.astype(np.float64)
    for got, prob in ((d, p), (u, np.full(len(p), 1 / len(p)))):
        counts = np.array([(got["light"] == w).sum() for w in world], np.float64)
        assert counts.sum() == n
        dev_ = np.abs(counts - n * prob)
        print("largest deviation in sigma", (dev_ / np.sqrt(n * prob * (1 - prob))).max())
        assert np.all(dev_ <= 5 * np.sqrt(n * prob * (1 - prob)) + 1), (counts, n * prob)
    assert p.max() / p.min() > 10                                          # (a table that is far from uniform)


# ---------------------------------------------------------------- 5. unbiased, and the lower variance
_EST = {}


def _estimates():
    """On the lamp room (M = 33: one lamp, 32 dim spheres), per ray sample at 2^16 samples, once for the tests of this section:
    trace1 / trace3 = rt_scene_trace with max_bounces 1 / 3;
    direct[f] = the host forms folded right to left as tests/_direct_np.py integrate folds them, over the two steps trace1 has: the
      step, its light sample times the albedo, and a second step that counts only when it MISSED (its EMITTED stood in the sample);
    forgot = direct[BIT] with every sample rescaled by M p_k, i.e. weighted as if the pick had been uniform (the pmf forgotten);
    nee[f, mode] = rt_scene_trace_nee, max_bounces 3."""
    if _EST:
        return _EST
    sph, tri = LP.lamp_room()
    rays = _one_window(_room_rays())
    n = len(rays)
    assert n == 1 << 16 and np.all(sph["roughness"] == 0)
    o, d = R.od(rays)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        M = sc.n_lights
        assert M == 33
        world, p = sc.light_table(BIT)
        p_at = dict(zip(world.tolist(), p.astype(np.float64).tolist()))
        _EST["p"] = p
        _EST["trace1"] = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=1, rng_state=R.states(n, 3700))[0].astype(np.float64)
        _EST["trace3"] = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=3, rng_state=R.states(n, 3701))[0].astype(np.float64)
        for f in (0, BIT):
            s1 = sc.bounce(rays, R.states(n, 3702), want_hits=True, want_next=True)
            nxt = s1["next"]
            dl = sc.direct(s1["hits"], s1["states"], active=nxt, flags=f)
            s2 = sc.bounce(s1["rays"], dl["states"], active=nxt, as_given=True)
            a1 = B.rgb_of(s1["bounce"]).astype(np.float64)
            sky2 = np.where((s2["bounce"]["status"] == B.MISSED)[:, None], B.rgb_of(s2["bounce"]), 0).astype(np.float64)
            direct = D.rgb_of(dl["direct"]).astype(np.float64)
            scat = (s1["bounce"]["status"] == B.SCATTERED)[:, None]
            _EST["direct", f] = np.where(scat, a1 * (direct + sky2), a1)
            if f == BIT:
                scale = np.array([M * p_at.get(int(w), 0.0) for w in dl["direct"]["light"]])[:, None]
                _EST["forgot"] = np.where(scat, a1 * (direct * scale + sky2), a1)
            for k, mode in enumerate((LIGHT_ONLY, MIS)):
                _EST["nee", f, mode] = _nee(sc, rays, spp=1, max_bounces=3, rng_state=R.states(n, 3710 + k), mode=mode,
                                            flags=f)["rgb"].astype(np.float64)
    return _EST


def test_estimates_are_unbiased_with_the_flag(ndev):
    est = _estimates()
    assert est["p"].max() > 0.5 and est["p"].min() < 0.02                  # the lamp, and a dim sphere
    pairs = [("direct", est["trace1"], est["direct", BIT]), ("nee light only", est["trace3"], est["nee", BIT, LIGHT_ONLY]),
             ("nee mis", est["trace3"], est["nee", BIT, MIS])]
    for what, a, b in pairs:
        gap, bound = _gap_and_bound(a, b)
        print(what, "mean trace", a.mean(0), "mean", b.mean(0), "gap", gap, "bound", bound)
        assert np.all(gap <= bound), (what, gap, bound)
    gap0, bound0 = _gap_and_bound(est["trace1"], est["forgot"])            # the negative control: the pmf forgotten
    print("pmf forgotten: mean", est["forgot"].mean(0), "gap", gap0, "bound", bound0)
    assert not np.all(gap0 <= bound0), (gap0, bound0)                      # (the bound asserted above, violated)


def test_variance_is_lower_with_the_flag(ndev):
    est = _estimates()
    lum = lambda x: x.mean(1)
    for what, key in (("direct", ("direct",)), ("nee light only", ("nee", LIGHT_ONLY)), ("nee mis", ("nee", MIS))):
        off, on = (lum(est[(key[0], f) + key[1:]]).var(ddof=1) for f in (0, BIT))
        print(what, "luminance variance without the flag", off, "with", on, "ratio", off / on)
        assert on < off, (what, off, on)


# ---------------------------------------------------------------- 6. the tile path ignores the bit; the plain-C client
def test_a_tile_entry_point_ignores_the_bit(ndev):
    sph, tri, wi = LP.many_lights()
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        out = []
        for f in (0, BIT):
            rq = _abi.default_request(width=64, height=32, divisions=4, division_no=1, spp=2, max_bounces=3, seed=0x11, flags=f)
            rgb, f32, st = sc.render_tile(rq, want_f32=True)
            out.append((rgb.tobytes(), f32.tobytes(), st.engine, st.ray_segments))
        assert out[0] == out[1] and any(out[0][0])


def test_plain_c_many_lights_client(ndev, tmp_path):
    """examples/many_lights.c through rt_tile.h and the C-ABI only: mean and variance of rt_scene_trace_nee with and without the flag
    on a 33-emitter scene."""
    exe = tmp_path / "many_lights"
    lib = _abi.lib_path().parent
    r = subprocess.run([shutil.which("gcc"), "-std=c99", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "many_lights.c"),
                        f"-L{lib}", "-lrt_s8", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "MANY_LIGHTS_OK" in run.stdout, run.stdout + run.stderr
