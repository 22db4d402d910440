"""Cone sampling of sphere lights on the GPU (rt_scene_set_light_sampling(RT_LIGHTS_CONE) for rt_scene_direct*, rt_scene_trace_nee*):
1. both kernels against the CPU restatement tests/_lights_np.py with cone=True (its cone arithmetic pinned by tests/test_cone_host.py,
   its bytes by tests/test_light_restatement.py), bit for bit: every rt_direct field and the states, the NEE colours of both modes, segment and shadow counts and states; on two_lights (M = 2, one sphere and one triangle
   light), many_lights (M = 33, the radius-0 emitter among them, a permuted world_index), the lamp room and the "regimes" scene (hit
   points inside an emissive sphere, on either side of q = 2^-10, under a light that nearly touches the surface); the four flag sets of
   tests/test_gpu_direct.py each with and without RT_FLAG_LIGHTS_BY_POWER; host and device forms; batches of 1, 63, 64, 65 and 2000;
   active lists with wild indices; the next list of a bounce step passed straight in; max_bounces 0, 1 and 3; given states, and the
   seeded streams at spp = 3; hit records placed on the regime's threshold to the ulp.  Without the feature these fail;
2. invariants: RT_LIGHTS_AREA after RT_LIGHTS_CONE restores the default bytes; the states of direct and the segments and states of NEE
   do not depend on the setting; records whose emitter is a triangle are RT_LIGHTS_AREA's byte for byte; a scene without sphere
   emitters, and M = 0, give RT_LIGHTS_AREA's bytes; RT_NEE_LIGHT_ONLY under RT_LIGHTS_CONE is the fold of Scene.bounce and
   Scene.direct under it; a strip, Scene.trace, bounce and intersect ignore the setting;
3. statistics at 2^16 samples with the 5 sigma bound of tests/test_gpu_direct.py: both modes under RT_LIGHTS_CONE agree with
   rt_scene_trace on the roughness-0 room, the glossy room and the room inside an emissive sphere; on c2's camera rays
   var(AREA) / var(CONE) > 1 in both modes (only the direction is asserted);
4. the plain-C client examples/cone_lights.c.
No timing is asserted."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes

import _bounce_np as B
import _cone_np as CN
import _direct_np as D
import _lightpick_np as LP
import _lights_np as LN
import _nee_np as N
from test_gpu_bounce import CONFIGS, FILL, Dev, dev  # noqa: F401  (dev: a fixture of this module too)
from test_gpu_direct import _device_direct, _gap_and_bound, _room_rays
from test_gpu_lightpick import _assert_direct, _assert_nee
from test_gpu_nee import _device_nee, _nee, _one_window, _rooms, _same

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
R = B.R
F32 = np.float32
AREA, CONE = _abi.RT_LIGHTS_AREA, _abi.RT_LIGHTS_CONE
POWER = _abi.RT_FLAG_LIGHTS_BY_POWER
LIGHT_ONLY, MIS = LN.LIGHT_ONLY, LN.MIS
N_RAYS = 2000
N_NEE = 300                                      # the rays of the NEE comparisons with the (per-ray Python) restatement
SIZES = [1, 63, 64, 65, 2000]


def _regimes():
    sph, tri = CN.regimes_scene()
    return sph, tri, None


def _lamps():
    sph, tri = LP.lamp_room()
    return sph, tri, None


SCENES = {"two_lights": LP.two_lights, "many_lights": LP.many_lights, "lamp_room": _lamps, "regimes": _regimes}
N_LIGHTS = {"two_lights": 2, "many_lights": 33, "lamp_room": 33, "regimes": 4}

_CASES, _REF = {}, {}


def _scene(c, sampling=CONE):
    sc = rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"]))
    sc.set_light_sampling(sampling)
    return sc


def _case(oracle, name, flags=0):
    """The scene, its rays (camera rays onto the room and the wild population of tests/_ray_cases.py, each in its own window; for
    `regimes` the rays of tests/_cone_np.py straight down onto its ground) and states, and — once per (scene, flags) — the hits and
    advanced states of one bounce step of them, by the library's own step."""
    if name not in _CASES:
        sph, tri, wi = SCENES[name]()
        if name == "regimes":
            rays = CN.regimes_rays(N_RAYS)
        else:
            rays = np.concatenate([D.camera_rays(40, 25, 0.6, -0.1),
                                   R.ray_population(oracle, np.random.default_rng(4300 + len(name)), sph, tri, N_RAYS - 1000, wi)[0]])
        rays = rays[np.random.default_rng(4200).permutation(N_RAYS)]       # every kind in every leading part of the batch
        _CASES[name] = dict(sph=sph, tri=tri, wi=wi, rays=np.ascontiguousarray(rays), st0=R.states(N_RAYS, 4400 + len(name)), steps={})
    c = _CASES[name]
    if flags not in c["steps"]:
        with _scene(c, AREA) as sc:
            c["steps"][flags] = sc.bounce(c["rays"], c["st0"], flags=flags, want_hits=True, want_next=True)
    return c, c["steps"][flags]


def _ref_direct(oracle, name, cfg, by_power, cone=True):
    """The restatement's samples of every record of the case's step: once per (scene, configuration, pick, setting), never modified."""
    flags, _, backend = CONFIGS[cfg]
    key = ("direct", name, cfg, by_power, cone)
    if key not in _REF:
        c, step = _case(oracle, name, flags)
        _REF[key] = LN.direct(oracle, c["sph"], c["tri"], step["hits"], step["states"], backend, c["wi"], by_power=by_power, cone=cone)
    return _REF[key]


def _ref_nee(oracle, name, backend, by_power, cone=True):
    """The restatement on the first N_NEE rays of the case, 2 samples from given states, 3 bounces."""
    key = ("nee", name, backend, by_power, cone)
    if key not in _REF:
        c, _ = _case(oracle, name)
        _REF[key] = LN.nee(oracle, c["sph"], c["tri"], c["rays"][:N_NEE], 2, 3, backend, c["wi"], states=c["st0"][:N_NEE],
                           by_power=by_power, cone=cone)
    return _REF[key]


# ---------------------------------------------------------------- 1. both kernels against the restatement
def test_setting_reads_back_and_refuses_other_values(ndev):
    sph, tri, wi = LP.two_lights()
    lib = _abi.load()
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        sc.collect()
        assert sc.light_sampling == AREA                                   # the default
        sc.set_light_sampling(CONE)
        assert sc.light_sampling == CONE
        assert lib.rt_scene_set_light_sampling(sc._h, 2) == _abi.RT_ERR_BAD_ARG and sc.light_sampling == CONE
        with pytest.raises(rt.RtError):
            sc.set_light_sampling(7)
        sc.set_light_sampling(AREA)
        assert sc.light_sampling == AREA
        assert sc.collect().n_launches == 0                                # host only


@pytest.mark.parametrize("by_power", [False, True], ids=["uniform", "by_power"])
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", SCENES)
def test_direct_is_bit_exact(ndev, oracle, dev, name, cfg, by_power):
    flags, engine, _ = CONFIGS[cfg]
    bit = POWER if by_power else 0
    c, step = _case(oracle, name, flags)
    want = _ref_direct(oracle, name, cfg, by_power)
    n = len(c["rays"])
    status = want["direct"]["status"]
    assert {D.LIT, D.OCCLUDED, D.FACING_AWAY} <= set(status.tolist()), (name, set(status.tolist()))
    assert want["in_cone"].sum() > 50, (name, int(want["in_cone"].sum()))
    if name in ("regimes", "many_lights"):                                 # sphere lights outside the regime too
        sphere_prims = LN.Table(c["sph"], c["tri"], c["wi"]).list
        is_sphere = {pos for pos, kind, _ in sphere_prims if kind == "sphere"}
        drew_sphere = np.isin(want["direct"]["light"], list(is_sphere)) & ~np.isin(status, (D.SKIPPED, D.NO_LIGHTS))
        assert (drew_sphere & ~want["in_cone"]).sum() > 20, name
    with _scene(c) as sc:
        assert sc.n_lights == N_LIGHTS[name]
        got = sc.direct(step["hits"], step["states"], flags=flags | bit)
        _assert_direct(got["direct"], got["states"], want, np.arange(n), (name, cfg, by_power, "host"))
        st = got["stats"]
        assert st.n_launches == 1 and st.engine == engine and st.ray_segments == int(want["shadow"].sum())
        d_direct, d_states = _device_direct(sc, dev, step["hits"], step["states"], n, flags=flags | bit)
        assert d_direct.tobytes() == got["direct"].tobytes() and np.array_equal(d_states, got["states"]), (name, cfg, "device")
        # the setting is not a no-op, touches no state and no record outside the regime; AREA afterwards restores the default bytes
        sc.set_light_sampling(AREA)
        off = sc.direct(step["hits"], step["states"], flags=flags | bit)
        assert np.array_equal(off["states"], got["states"])
        rest = ~want["in_cone"]
        assert off["direct"][rest].tobytes() == got["direct"][rest].tobytes()
        assert not D.records_equal(off["direct"][want["in_cone"]], got["direct"][want["in_cone"]]).any()
        lit = got["direct"][want["in_cone"] & (status == D.LIT)]
        ip_max = 1.0 / LN.Table(c["sph"], c["tri"], c["wi"], by_power).p.min()
    with rt.Scene(0, rt.World(c["sph"], c["tri"], c["wi"])) as fresh:      # a scene that never saw the setting
        base = fresh.direct(step["hits"], step["states"], flags=flags | bit)
    assert base["direct"].tobytes() == off["direct"].tobytes() and np.array_equal(base["states"], off["states"])
    # W <= 2 ip: the estimate is bounded by 2 ip (albedo emission) per channel
    e_max = max(float((a["emission"] * np.maximum.reduce([a["albedo_r"], a["albedo_g"], a["albedo_b"]])).max()) for a in (c["sph"], c["tri"]) if len(a))
    assert len(lit) > 20 and D.rgb_of(lit).max() <= 2 * ip_max * e_max * (1 + 1e-6)


def test_direct_on_the_regimes_threshold(ndev, oracle):
    """Hit records placed by hand around regimes_scene's far light (radius 0.25 = 2^-2, so r2 = 2^-4 exactly): along eight directions
    at the distances whose f32 dc2 are 64 (q = 2^-10 exactly) and its neighbours, and under the near light a few ulps outside it
    (q just below 1) and just inside it; every one compared with the restatement, and both sides of both ends occur."""
    sph, tri, _ = _regimes()
    g = np.random.default_rng(4500)
    c_far, c_near = np.array([0.0, 3.0, -6.0]), np.array([0.0, 0.5 + 1.0 / 64, 0.0])
    P, nrm = [], []
    for k in range(8):
        w = g.normal(size=3)
        w /= np.linalg.norm(w)
        for j in range(-6, 7):
            P.append(c_far - w * 8.0 * (1 + j * 2.0 ** -23))
            nrm.append(w)
            P.append(c_near - w * 0.5 * (1 + j * 2.0 ** -22))
            nrm.append(w)
    m = 24                                                                 # samples per placed point, each from its own state
    P, nrm = np.repeat(np.array(P, F32), m, 0), np.repeat(np.array(nrm, F32), m, 0)
    n = len(P)
    hits = np.zeros(n, _abi.HIT_DTYPE)
    hits["px"], hits["py"], hits["pz"], hits["nx"], hits["ny"], hits["nz"] = *P.T, *nrm.T
    hits["distance"], hits["index"] = 1.0, 0
    st = R.states(n, 4501)
    want = LN.direct(oracle, sph, tri, hits, st, 1, None, cone=True)
    q_far = CN.cone_axis(P.T.copy(), np.array(c_far, F32)[:, None], F32(0.25))[3]
    q_near = CN.cone_axis(P.T.copy(), np.array(c_near, F32)[:, None], F32(0.5))[3]
    far_pts, near_pts = np.arange(n) // m % 2 == 0, np.arange(n) // m % 2 == 1
    assert (q_far[far_pts] == F32(2.0 ** -10)).any() and (q_far[far_pts] < F32(2.0 ** -10)).any() and (q_far[far_pts] > F32(2.0 ** -10)).any()
    assert (q_near[near_pts] < 1).any() and (q_near[near_pts] >= 1).any()
    far_l, near_l = want["direct"]["light"] == 3, want["direct"]["light"] == 2
    for pts, lgt in ((far_pts, far_l), (near_pts, near_l)):
        assert (want["in_cone"] & pts & lgt).sum() > 50 and (~want["in_cone"] & pts & lgt).sum() > 50
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_light_sampling(CONE)
        got = sc.direct(hits, st)
        _assert_direct(got["direct"], got["states"], want, np.arange(n), "threshold")


@pytest.mark.parametrize("by_power", [False, True], ids=["uniform", "by_power"])
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", SCENES)
def test_nee_is_bit_exact_in_both_modes(ndev, oracle, dev, name, cfg, by_power):
    flags, engine, backend = CONFIGS[cfg]
    bit = POWER if by_power else 0
    c, _ = _case(oracle, name)
    want = _ref_nee(oracle, name, backend, by_power)
    area = _ref_nee(oracle, name, backend, by_power, cone=False)
    rays, st0 = c["rays"][:N_NEE], c["st0"][:N_NEE]
    assert np.array_equal(want["segments"], area["segments"]) and np.array_equal(want["states"], area["states"])
    with _scene(c) as sc:
        for mode in (LIGHT_ONLY, MIS):
            got = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=mode, flags=flags | bit)
            _assert_nee(got, want, mode, N_NEE, (name, cfg, by_power, mode, "host"))
            st = got["stats"]
            assert st.engine == engine and st.n_launches == 1 and st.primary_rays == 2 * N_NEE
            assert st.ray_segments == int(want["segments"].sum()) + int(want["shadow"].sum())
            assert _same(_device_nee(sc, dev, rays, st0, spp=2, max_bounces=3, mode=mode, flags=flags | bit), got), (name, cfg, mode, "device")
        sc.set_light_sampling(AREA)                                        # ... and back: the default bytes, the same paths
        for mode in (LIGHT_ONLY, MIS):
            off = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=mode, flags=flags | bit)
            _assert_nee(off, area, mode, N_NEE, (name, cfg, by_power, mode, "area again"))
            assert off["rgb"].tobytes() != want["rgb"][mode].tobytes()     # the setting is not a no-op
    assert want["shadow"].sum() > 50 and not np.array_equal(want["rgb"][LIGHT_ONLY], want["rgb"][MIS])
    assert want["shadow"].sum() > area["shadow"].sum()                     # fewer samples face away


@pytest.mark.parametrize("max_bounces", [0, 1, 3])
def test_nee_seeded_streams_and_depths(ndev, oracle, max_bounces):
    c, _ = _case(oracle, "two_lights")
    m = 120
    rays = c["rays"][:m]
    want = LN.nee(oracle, c["sph"], c["tri"], rays, 3, max_bounces, 1, c["wi"], seed=0xC0DE + max_bounces, cone=True)
    given = LN.nee(oracle, c["sph"], c["tri"], rays, 1, max_bounces, 1, c["wi"], states=c["st0"][:m], cone=True)
    with _scene(c) as sc:
        for mode in (LIGHT_ONLY, MIS):
            got = _nee(sc, rays, spp=3, max_bounces=max_bounces, seed=0xC0DE + max_bounces, mode=mode)
            ok = np.all(B.same_bits(got["rgb"], want["rgb"][mode]), 1)
            assert ok.all(), (max_bounces, mode, np.nonzero(~ok)[0][:5])
            assert np.array_equal(got["segments"], want["segments"]) and np.array_equal(got["shadow"], want["shadow"])
            got1 = _nee(sc, rays, spp=1, max_bounces=max_bounces, rng_state=c["st0"][:m], mode=mode)
            _assert_nee(got1, given, mode, m, (max_bounces, mode, "given"))
    assert (want["shadow"].sum() > 0) == (max_bounces > 0)


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(ndev, oracle, dev, n):
    c, step = _case(oracle, "many_lights")
    want = _ref_direct(oracle, "many_lights", "default", True)
    hits, states = step["hits"][:n], step["states"][:n]
    m = min(n, N_NEE)
    want_nee = _ref_nee(oracle, "many_lights", 1, True)
    with _scene(c) as sc:
        got = sc.direct(hits, states, flags=POWER)
        _assert_direct(got["direct"], got["states"], want, np.arange(n), ("host", n))
        d_direct, d_states = _device_direct(sc, dev, hits, states, n, flags=POWER)
        _assert_direct(d_direct, d_states, want, np.arange(n), ("device", n))
        rays, st0 = c["rays"][:m], c["st0"][:m]
        for mode in (LIGHT_ONLY, MIS):
            host = _nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=mode, flags=POWER)
            _assert_nee(host, want_nee, mode, m, ("nee host", n, mode))
            assert _same(_device_nee(sc, dev, rays, st0, spp=2, max_bounces=3, mode=mode, flags=POWER), host), (n, mode, "nee device")
        if n == 2000:                                                      # a ray's result does not depend on the batch
            whole = _nee(sc, c["rays"], spp=2, max_bounces=3, rng_state=c["st0"], mode=MIS, flags=POWER)
            assert _same({k: v[:m] for k, v in whole.items() if k != "stats"}, host)


@pytest.mark.parametrize("n", [65, 2000])
def test_active_lists(ndev, oracle, dev, n):
    c, step = _case(oracle, "regimes")
    want = _ref_direct(oracle, "regimes", "default", False)
    hits, states = step["hits"][:n], step["states"][:n]
    g = np.random.default_rng(n)
    listed = g.permutation(np.arange(0, n, 3)).astype(np.uint32)
    rest = np.setdiff1d(np.arange(n), listed)
    junk = np.full((n, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
    mixed = np.where(np.isin(np.arange(n), listed)[:, None], states, junk)
    with _scene(c) as sc:
        # the device form: a list longer than its device-side length, with indices >= n among the entries taken
        wild = np.concatenate([listed[:5], [n, n + 7, 0xFFFFFFFF], listed[5:]]).astype(np.uint32)
        used = len(wild) - len(listed) // 4
        stepped = np.sort(wild[:used][wild[:used] < n]).astype(np.int64)
        untouched = np.setdiff1d(np.arange(n), stepped)
        got, got_states = _device_direct(sc, dev, hits, mixed, n, d_active=dev.put(wild), d_n_active=dev.put(np.array([used], np.uint32)))
        _assert_direct(got, got_states, want, stepped, ("device list", n))
        assert set(got[untouched].tobytes()) <= {FILL} and np.array_equal(got_states[untouched], mixed[untouched])
        # the host form: records outside the list come back as they went in
        h = sc.direct(hits, mixed, active=listed)
        _assert_direct(h["direct"], h["states"], want, np.sort(listed).astype(np.int64), ("host list", n))
        assert not any(h["direct"][rest].tobytes()) and np.array_equal(h["states"][rest], junk[rest])
        assert h["stats"].ray_segments == int(want["shadow"][listed].sum())


def test_next_list_of_a_bounce_step_goes_straight_in(ndev, oracle, dev):
    c, step = _case(oracle, "lamp_room")
    want = _ref_direct(oracle, "lamp_room", "default", False)
    n = len(c["rays"])
    with _scene(c) as sc:
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
        _assert_direct(got, got_states, want, scat, "after a bounce step")
        assert set(got[rest].tobytes()) <= {FILL} and np.array_equal(got_states[rest], step["states"][rest])


# ---------------------------------------------------------------- 2. invariants
def test_triangle_records_are_the_area_bytes(ndev, oracle):
    c, step = _case(oracle, "many_lights")
    tri_pos = {pos for pos, kind, _ in LN.Table(c["sph"], c["tri"], c["wi"]).list if kind == "triangle"}
    with _scene(c) as sc:
        on = sc.direct(step["hits"], step["states"])["direct"]
        sc.set_light_sampling(AREA)
        off = sc.direct(step["hits"], step["states"])["direct"]
    is_tri = np.isin(on["light"], list(tri_pos))
    assert is_tri.sum() > 100 and np.array_equal(on["light"], off["light"])
    assert on[is_tri].tobytes() == off[is_tri].tobytes() and on.tobytes() != off.tobytes()


def _no_sphere_emitters(which):
    sph, tri, wi = LP.many_lights()
    sph["emission"] = 0
    if which == "no_lights":
        tri["emission"] = 0
    return sph, tri, wi


@pytest.mark.parametrize("which", ["triangle_lights_only", "no_lights"])
def test_without_sphere_emitters_the_setting_changes_no_byte(ndev, oracle, which):
    sph, tri, wi = _no_sphere_emitters(which)
    rays, st0 = _case(oracle, "many_lights")[0]["rays"], R.states(N_RAYS, 4600)
    out = {}
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        assert sc.n_lights == (9 if which == "triangle_lights_only" else 0)
        step = sc.bounce(rays, st0, want_hits=True)
        for s in (AREA, CONE):
            sc.set_light_sampling(s)
            d = sc.direct(step["hits"], step["states"], flags=POWER)
            nee = [_nee(sc, rays, spp=2, max_bounces=3, rng_state=st0, mode=mode, flags=POWER) for mode in (LIGHT_ONLY, MIS)]
            out[s] = (d, nee)
    assert out[AREA][0]["direct"].tobytes() == out[CONE][0]["direct"].tobytes() and np.array_equal(out[AREA][0]["states"], out[CONE][0]["states"])
    want_status = D.LIT if which == "triangle_lights_only" else D.NO_LIGHTS
    assert (out[CONE][0]["direct"]["status"] == want_status).sum() > 10
    for a, b in zip(out[AREA][1], out[CONE][1]):
        assert _same(a, b), which


def _cone_fold(sc, lights, rays, states, max_bounces, flags):
    """One sample of every ray through Scene.bounce and Scene.direct under the scene's setting RT_LIGHTS_CONE, the forward fold of
    tests/test_gpu_nee.py _composed_sample in float32 numpy with the contract's sampled rule and, for an emitter the bounce reached,
    the cone view from the segment's origin where the emitter is a sphere in the regime (the area view otherwise).  The rays share
    one window.  Returns (c (n, 3) float32, segments, shadow, states)."""
    n = len(rays)
    t_min, t_max = rays["t_min"][0], rays["t_max"][0]
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
        o_in = np.stack([cur_rays["ox"], cur_rays["oy"], cur_rays["oz"]], 1).astype(F32)
        s = sc.bounce(cur_rays, cur_states, active=act, as_given=k > 0, flags=flags, want_hits=True)
        cur_rays, cur_states = s["rays"], s["states"]
        segs[act] += 1
        status, rgb, hits = s["bounce"]["status"], B.rgb_of(s["bounce"]), s["hits"]
        emitted = act[status[act] == B.EMITTED]
        keep = np.ones(len(emitted), bool) if k == 0 else ~sampled[emitted]
        for q in np.nonzero(~keep)[0]:
            i = emitted[q]
            j = int(hits["index"][i])
            sphere = bool(lights.sphere[j])
            in_regime = False
            if sphere:
                rec = lights.rec[j]
                _, _, in_regime, samplable = CN.emitter_view_cone(o_in[i], n_prev[i], d_in[i], D.v3(rec["cx"], rec["cy"], rec["cz"]), rec["radius"])
            if not in_regime:
                nh = D.v3(hits["nx"][i], hits["ny"][i], hits["nz"][i])
                samplable = N.emitter_view(n_prev[i], d_in[i], nh, hits["distance"][i], sphere)[3]
            keep[q] = not samplable
        add = np.concatenate([act[status[act] == B.MISSED], emitted[keep]])
        with np.errstate(all="ignore"):
            c[add] = c[add] + T[add] * rgb[add]
            scat = act[status[act] == B.SCATTERED]
            T[scat] = T[scat] * rgb[scat]
        if k == max_bounces:
            break
        sampled[scat] = (lights.rough[hits["index"][scat]] == 0) & (lights.M > 0)
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


@pytest.mark.parametrize("name,cfg,by_power", [("two_lights", "default", False), ("regimes", "no_bvh_cull", True)])
def test_light_only_is_the_fold_of_bounce_and_direct_under_cone(ndev, oracle, name, cfg, by_power):
    flags = CONFIGS[cfg][0] | (POWER if by_power else 0)
    c, _ = _case(oracle, name)
    rays = _one_window(c["rays"])
    n = len(rays)
    lights = LN.Table(c["sph"], c["tri"], c["wi"])
    with _scene(c) as sc:
        for max_bounces in (1, 3):
            want_c, want_segs, want_shadow, want_states = _cone_fold(sc, lights, rays, c["st0"], max_bounces, flags)
            got = _nee(sc, rays, spp=1, max_bounces=max_bounces, rng_state=c["st0"], mode=LIGHT_ONLY, flags=flags)
            want_rgb = (np.zeros((n, 3), F32) + want_c).astype(F32)
            ok = np.all(B.same_bits(got["rgb"], want_rgb), 1)
            assert ok.all(), (name, max_bounces, np.nonzero(~ok)[0][:5], got["rgb"][~ok][:3], want_rgb[~ok][:3])
            assert np.array_equal(got["segments"], want_segs) and np.array_equal(got["shadow"], want_shadow)
            assert np.array_equal(got["states"], want_states)
            assert want_shadow.sum() > 100 and (want_c.sum(1) > 0).sum() > 100
        sc.set_light_sampling(AREA)                                        # (the same call under AREA gives other colours)
        off = _nee(sc, rays, spp=1, max_bounces=3, rng_state=c["st0"], mode=LIGHT_ONLY, flags=flags)
        assert off["rgb"].tobytes() != got["rgb"].tobytes() and np.array_equal(off["segments"], got["segments"])
        assert np.array_equal(off["states"], got["states"])


def test_other_entry_points_ignore_the_setting(ndev, oracle):
    c, _ = _case(oracle, "many_lights")
    rays, st0 = c["rays"][:500], c["st0"][:500]
    o, d = R.od(rays)
    out = []
    with _scene(c, AREA) as sc:
        for s in (AREA, CONE):
            sc.set_light_sampling(s)
            rq = _abi.default_request(width=64, height=32, divisions=4, division_no=1, spp=2, max_bounces=3, seed=0x11)
            rgb, f32, st = sc.render_tile(rq, want_f32=True)
            tr = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=2, max_bounces=3, rng_state=st0)
            bn = sc.bounce(rays, st0, want_hits=True, want_next=True)
            hit = sc.intersect(o, d, rays["t_min"], rays["t_max"])[0]
            cam = sc.camera_rays(rq)
            out.append((rgb.tobytes(), f32.tobytes(), st.ray_segments, tr[0].tobytes(), tr[1].tobytes(), bn["rays"].tobytes(), bn["states"].tobytes(),
                        bn["bounce"].tobytes(), bn["hits"].tobytes(), bn["next"].tobytes(), hit.tobytes(), cam[0].tobytes(), cam[1].tobytes(),
                        sc.light_table(POWER)[1].tobytes()))
    assert out[0] == out[1] and any(out[0][0])


# ---------------------------------------------------------------- 3. statistics
@pytest.mark.parametrize("which", ["plain", "glossy", "enclosed"])
def test_both_modes_are_unbiased_under_cone(ndev, which):
    """The bound is that of tests/test_gpu_direct.py: per channel |mean_x - mean_y| <= 5 sqrt(var_x / N + var_y / N) at N = 2^16, the
    variances from the samples themselves."""
    sph, tri = _rooms(which)
    rays = _one_window(_room_rays())
    n = len(rays)
    assert n == 1 << 16
    o, d = R.od(rays)
    seed = 7100 + len(which)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_light_sampling(CONE)
        trace = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=3, rng_state=R.states(n, seed))[0].astype(np.float64)
        for k, mode in enumerate((LIGHT_ONLY, MIS)):
            got = _nee(sc, rays, spp=1, max_bounces=3, rng_state=R.states(n, seed + 1 + k), mode=mode)
            est = got["rgb"].astype(np.float64)
            gap, bound = _gap_and_bound(trace, est)
            print(which, "mode", mode, "mean trace", trace.mean(0), "mean", est.mean(0), "gap", gap, "bound", bound)
            assert got["shadow"].sum() > 1000
            assert np.all(gap <= bound), (which, mode, gap, bound)


def test_cone_has_the_lower_variance_on_c2(ndev):
    """c2's camera rays, 2^16 ray samples, max_bounces 3, the same states under either setting: only the direction of var(AREA) /
    var(CONE) is asserted; the figures are printed."""
    sph, rq = scenes.config("c2")
    rq.width, rq.height, rq.divisions, rq.division_no, rq.spp = 128, 64, 1, 0, 8
    lum = lambda rgb: rgb.astype(np.float64).mean(1)
    with rt.Scene(0, rt.World(sph)) as sc:
        rays, _, _ = sc.camera_rays(rq)
        n = len(rays)
        assert n == 1 << 16 and sc.n_lights == 1
        o, d = R.od(rays)
        tr = lum(sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=3, rng_state=R.states(n, 7200), as_given=True)[0])
        var = {}
        for s in (AREA, CONE):
            sc.set_light_sampling(s)
            for k, mode in enumerate((LIGHT_ONLY, MIS)):
                got = _nee(sc, rays, spp=1, max_bounces=3, rng_state=R.states(n, 7201 + k), as_given=True, mode=mode)
                x = lum(got["rgb"])
                var[s, mode] = x.var(ddof=1)
                print("setting", s, "mode", mode, "mean trace", tr.mean(), "mean", x.mean(), "variance trace", tr.var(ddof=1), "variance", var[s, mode],
                      "trace / mode", tr.var(ddof=1) / var[s, mode], "largest sample", x.max(), "shadow rays", int(got["shadow"].sum()))
                if s == CONE:
                    assert abs(tr.mean() - x.mean()) <= 5 * np.sqrt(tr.var(ddof=1) / n + var[s, mode] / n)
    for mode in (LIGHT_ONLY, MIS):
        print("mode", mode, "var(AREA) / var(CONE)", var[AREA, mode] / var[CONE, mode])
        assert var[AREA, mode] / var[CONE, mode] > 1, (mode, var)


# ---------------------------------------------------------------- 4. the plain-C client
def test_plain_c_cone_lights_client(ndev, tmp_path):
    """examples/cone_lights.c through rt_tile.h and the C-ABI only: c2 under both settings and both modes next to rt_scene_trace."""
    exe = tmp_path / "cone_lights"
    lib = _abi.lib_path().parent
    r = subprocess.run([shutil.which("gcc"), "-std=c99", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "cone_lights.c"),
                        f"-L{lib}", "-lrt_s8", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and "CONE_LIGHTS_OK" in run.stdout, run.stdout + run.stderr
