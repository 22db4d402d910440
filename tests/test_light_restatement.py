"""The one CPU restatement of direct lighting and NEE (tests/_lights_np.py) against what the five per-feature drivers it replaced
computed, bit for bit, on the CPU.

tests/golden/light_restatements.npz was recorded at commit cf0d93f ("Add light samples at glossy hits to RT_NEE_MIS"), the last one with
a driver per feature: `direct` and `nee` of tests/_direct_np.py / _nee_np.py (the uniform pick, the M-form weights, the oracle's own
UnitSphere draw), of _lightpick_np.py (by_power), of _cone_np.py (by_power x cone) and `nee(glossy=True)` of _lobe_np.py.  The recording
script ran `run` below with `call` set to that entry point, so the inputs are those of CASES here; it is not kept, since it imports what
that commit's successor deleted.  A key reads fn/origin/scene/p<by_power>c<cone>g<glossy>[/variant]:

  origin       entry point at cf0d93f, called as                                                   scenes
  _direct_np   D.direct(oracle, sph, tri, hits, states, backend, wi, active=)                      two_spheres, lit_room
  _nee_np      N.nee(oracle, sph, tri, rays, spp, max_bounces, backend, wi, as_given, states, seed) two_spheres, lit_room
  _lightpick_np  LP.direct / LP.nee(the same, by_power=)                                            two_lights, many_lights, regimes
  _cone_np     CN.direct / CN.nee(the same, by_power=, cone=)                                       two_lights, regimes; nee also on
                                                                                                    glossy and rough01 (cone only)
  _lobe_np     L.nee(the same, by_power=, cone=, glossy=True), its counts as well                   glossy, boundary, rough01

and the variants, once each on two_lights from _cone_np with by_power and cone set: `seeded` (states=None, spp=3, seed 0x5EED),
`as_given`, `bounces0` (max_bounces=0), `active` (direct, every third record from the second) and `backend0` (the BVH-semantics
backend of tests/test_gpu_bounce.py CONFIGS "no_bvh_cull").  Everything else runs backend 1, NEE with 2 samples from given states and 3
bounces.  The scenes, rays and states are those of tests/test_cone_host.py (f) and tests/test_lobe_host.py (d) — `scene` below.  A
`direct` case samples at the bounce step of all 160 rays, a `nee` case traces the first 60; on the three scenes of NEE_STRIDE, every
second or seventh ray, which keeps the file below 64 KB: a ray's result does not depend on the batch, so test_lobe_host.py compares
those entries of its full batch with `recorded`.

The uniform cases are the reduction no test asserted before: the driver with a uniform table, ip = (float)M and the UnitSphere pair
drawn by _cone_np.draw_pair is _direct_np.direct and _nee_np.nee."""
from pathlib import Path

import numpy as np
import pytest

import _bounce_np as B
import _cone_np as CN
import _direct_np as D
import _lightpick_np as LP
import _lights_np as LN
import _lobe_np as L

R = B.R
FIXTURE = Path(__file__).resolve().parent / "golden" / "light_restatements.npz"
NEE_STRIDE = {"boundary": 7, "glossy": 2, "rough01": 2}
OPTS = dict(spp=2, max_bounces=3, backend=1, as_given=False, seed=None, active=False)
COUNTS = ("none", "diffuse", "lobe", "dropped", "emitted_after_lobe", "emitted_outside_lobe")


def _cases():
    out = []

    def add(fn, origin, name, by_power=False, cone=False, glossy=False, variant=None, **opts):
        key = f"{fn}/{origin}/{name}/p{int(by_power)}c{int(cone)}g{int(glossy)}" + (f"/{variant}" if variant else "")
        out.append(dict(key=key, fn=fn, origin=origin, scene=name, flags=dict(by_power=by_power, cone=cone, glossy=glossy), opts=opts))

    both = [(p, c) for p in (False, True) for c in (False, True)]
    for fn in ("direct", "nee"):
        for name in ("two_spheres", "lit_room"):
            add(fn, "_direct_np" if fn == "direct" else "_nee_np", name)
        for name in ("two_lights", "many_lights", "regimes"):
            for p in (False, True):
                add(fn, "_lightpick_np", name, p)
        for name in ("two_lights", "regimes"):
            for p, c in both:
                add(fn, "_cone_np", name, p, c)
        add(fn, "_cone_np", "two_lights", True, True, variant="backend0", backend=0)
    add("direct", "_cone_np", "two_lights", True, True, variant="active", active=True)
    add("nee", "_cone_np", "two_lights", True, True, variant="seeded", spp=3, seed=0x5EED)
    add("nee", "_cone_np", "two_lights", True, True, variant="as_given", as_given=True)
    add("nee", "_cone_np", "two_lights", True, True, variant="bounces0", max_bounces=0)
    for c in (False, True):
        add("nee", "_cone_np", "glossy", False, c)
    add("nee", "_cone_np", "rough01")
    for name in ("glossy", "boundary"):
        for p, c in both:
            add("nee", "_lobe_np", name, p, c, True)
    add("nee", "_lobe_np", "rough01", glossy=True)
    return out


CASES = _cases()
_SCENES, _STEPS, _RECORDED = {}, {}, {}


def scene(name):
    """dict: sph, tri, wi, rays, st (a state per ray), nee (the indices of the rays a `nee` case takes)."""
    if name not in _SCENES:
        wi = None
        if name in ("two_spheres", "two_lights", "many_lights"):
            sph, tri, wi = {"two_spheres": D.two_spheres, "two_lights": LP.two_lights, "many_lights": LP.many_lights}[name]()
        elif name == "lit_room":
            sph, tri = D.lit_room()
        elif name == "regimes":
            sph, tri = CN.regimes_scene()
        elif name == "boundary":
            sph, tri = L.boundary_scene()
        else:
            from test_gpu_nee import _rooms
            sph, tri = _rooms("glossy")
            if name == "rough01":                                          # roughnesses 0 and 1 only: no hit is lobe-sampled
                sph["roughness"][:4] = [1.0, 0.0, 1.0, 0.0]
        if name == "regimes":
            rays = CN.regimes_rays(160)
        elif name == "boundary":
            rays = L.boundary_rays()
        else:
            rays = D.camera_rays(12, 8, 0.6, -0.1) if name in ("glossy", "rough01") else D.camera_rays(16, 10, 0.6, -0.1)
        n = len(rays)
        nee = np.arange(0, n, NEE_STRIDE[name]) if name in NEE_STRIDE else np.arange(60)
        _SCENES[name] = dict(sph=sph, tri=tri, wi=wi, rays=rays, st=R.states(n, 1800 if name in NEE_STRIDE else 4100), nee=nee)
    return _SCENES[name]


def step(oracle, name, backend=1):
    """The bounce step of every ray of the scene: the records a `direct` case samples at."""
    if (name, backend) not in _STEPS:
        s = scene(name)
        _STEPS[name, backend] = B.step(oracle, s["sph"], s["tri"], s["rays"], s["st"], backend, s["wi"])
    return _STEPS[name, backend]


def run(oracle, case, call=None):
    """The case through the one driver with its flags (or through call(case, *args, **kwargs), the flags left to it)."""
    s, o = scene(case["scene"]), dict(OPTS, **case["opts"])
    if call is None:
        call = lambda case, *a, **kw: getattr(LN, case["fn"])(*a, **kw, **{k: v for k, v in case["flags"].items()
                                                                             if k != "glossy" or case["fn"] == "nee"})
    if case["fn"] == "direct":
        st = step(oracle, case["scene"], o["backend"])
        return call(case, oracle, s["sph"], s["tri"], st["hits"], st["states"], o["backend"], s["wi"],
                    active=np.arange(1, len(st["hits"]), 3) if o["active"] else None)
    rays, states = np.ascontiguousarray(s["rays"][s["nee"]]), s["st"][s["nee"]]
    return call(case, oracle, s["sph"], s["tri"], rays, o["spp"], o["max_bounces"], o["backend"], s["wi"], as_given=o["as_given"],
                states=None if o["seed"] is not None else states, seed=o["seed"] or 0)


def recorded(key):
    """What the fixture holds of one case, in the driver's own layout: direct, states, shadow, in_cone; or rgb ({mode: the uint32 bit
    patterns}), segments, shadow, states (None when seeded), counts (None unless glossy)."""
    if not _RECORDED:
        z = dict(np.load(FIXTURE, allow_pickle=False))                     # per field, the cases' entries one after the other
        at = dict.fromkeys(z, 0)

        def take(field, m):
            at[field] += m
            return z[field][at[field] - m:at[field]]

        for k, n in zip(z["direct_keys"].tolist(), z["direct_n"].tolist()):
            _RECORDED[k] = dict(direct=take("direct_records", n), states=take("direct_states", n),
                                shadow=take("direct_shadow", n), in_cone=take("direct_in_cone", n))
        for k, n, given, modes in zip(z["nee_keys"].tolist(), z["nee_n"].tolist(), z["nee_given"].tolist(), z["nee_modes"].tolist()):
            rgb = {LN.MIS: take("nee_rgb_mis", n)}
            if modes == 2:
                rgb[LN.LIGHT_ONLY] = take("nee_rgb_light", n)
            _RECORDED[k] = dict(rgb=rgb, segments=take("nee_segments", n), shadow=take("nee_shadow", n),
                                states=take("nee_states", n) if given else None,
                                counts=dict(zip(COUNTS, take("nee_counts", 1)[0].tolist())) if modes == 1 else None)
    return _RECORDED[key]


def assert_recorded(got, key, idx=None):
    """`got` (of LN.direct or LN.nee) is what the fixture holds under `key`; idx: the entries of a larger batch that the fixture
    holds (its counts, which are the batch's, are then not compared)."""
    want = recorded(key)
    at = (lambda a: a) if idx is None else (lambda a: a[idx])
    if "direct" in want:
        assert at(got["direct"]).tobytes() == want["direct"].tobytes(), key
        assert np.array_equal(at(got["in_cone"]), want["in_cone"]), key
    else:
        assert set(got["rgb"]) == set(want["rgb"]), key
        for mode, bits in want["rgb"].items():
            assert np.array_equal(at(got["rgb"][mode]).view(np.uint32), bits), (key, mode)
        assert np.array_equal(at(got["segments"]), want["segments"]), key
        if want["counts"] is not None and idx is None:
            assert got["counts"] == want["counts"], key
    assert np.array_equal(at(got["shadow"]), want["shadow"]), key
    assert (got["states"] is None) == (want["states"] is None), key
    if want["states"] is not None:
        assert np.array_equal(at(got["states"]), want["states"]), key


def test_the_fixture_holds_every_case_and_is_not_vacuous():
    z = np.load(FIXTURE, allow_pickle=False)
    assert sorted(z["direct_keys"].tolist() + z["nee_keys"].tolist()) == sorted(c["key"] for c in CASES)
    assert FIXTURE.stat().st_size < 64 * 1024
    for c in CASES:
        r, f = recorded(c["key"]), c["flags"]
        if c["fn"] == "direct":
            status = r["direct"]["status"]
            if c["scene"] != "two_spheres":                                # (one light straight above one sphere: nothing occludes)
                assert {D.LIT, D.OCCLUDED, D.FACING_AWAY} <= set(status.tolist()), c["key"]
            assert r["in_cone"].any() == f["cone"], c["key"]
        else:
            assert r["segments"].sum() > len(r["segments"]) and all(v.any() for v in r["rgb"].values()), c["key"]
            if f["glossy"] and c["scene"] != "rough01":
                assert r["counts"]["lobe"] > 20 and 0 < r["counts"]["dropped"] < r["counts"]["lobe"], c["key"]
                assert r["counts"]["emitted_after_lobe"] > 0, c["key"]
            if len(r["rgb"]) == 2 and c["opts"].get("max_bounces", 3):
                assert r["shadow"].sum() > 0 and not np.array_equal(r["rgb"][LN.MIS], r["rgb"][LN.LIGHT_ONLY]), c["key"]


@pytest.mark.parametrize("case", CASES, ids=[c["key"] for c in CASES])
def test_the_one_driver_computes_what_the_replaced_drivers_did(oracle, case):
    assert_recorded(run(oracle, case), case["key"])
