"""The CPU reference of one path step (tests/_bounce_np.py) pinned on the CPU: K steps composed with the active list carried along and
folded right to left are oracle.trace_batch(states=..., spp=1, max_bounces=K - 1) bit for bit — the colours and the final states —
and step as many rays as the trace counts segments.  Both backends, K in {1, 2, 4}, a sphere scene, a triangle scene and the mixed
scene with a permuted world; the seeded states; the exceptional arms of the scatter.  A wrong reference cannot go unnoticed."""
import numpy as np
import pytest

import _bounce_np as B

N_RAYS = {"spheres": 300, "triangles": 300, "mixed": 200}


@pytest.fixture(scope="module")
def cases(oracle):
    return {name: B.population(oracle, name, N_RAYS[name], 500 + k) for k, name in enumerate(B.SCENE_NAMES)}


@pytest.mark.parametrize("backend", [0, 1])
@pytest.mark.parametrize("name", B.SCENE_NAMES)
def test_steps_compose_to_trace_batch(oracle, cases, name, backend):
    sph, tri, wi, rays, st0 = cases[name]
    seen = set()
    for K in (1, 2, 4):
        want_rgb, want_segs, want_st = oracle.trace_batch(sph, tri, rays, spp=1, max_bounces=K - 1, backend=backend, world_index=wi,
                                                          states=st0)
        rgb, st, stepped = B.compose(oracle, sph, tri, rays, st0, K, backend, wi)
        ok = np.all(B.same_bits(rgb, want_rgb), 1)
        assert ok.all(), (name, backend, K, np.nonzero(~ok)[0][:5], rgb[~ok][:3], want_rgb[~ok][:3])
        assert np.array_equal(st, want_st), (name, backend, K)
        assert stepped == int(want_segs.sum()), (name, backend, K)
    first = B.step(oracle, sph, tri, rays, st0, backend, wi)
    seen = set(first["bounce"]["status"].tolist())
    assert seen == {B.SCATTERED, B.EMITTED, B.MISSED}, (name, seen)      # every status occurs in every scene
    assert int(want_segs.max()) == 4                                       # some path is alive after four steps


def test_ray_forms_and_seeded_states(oracle, cases):
    sph, tri, wi, rays, st0 = cases["mixed"]
    seed = 0xC0FFEE1234
    want = oracle.trace_batch(sph, tri, rays, spp=1, max_bounces=3, backend=1, world_index=wi, seed=seed)
    rgb, _, stepped = B.compose(oracle, sph, tri, rays, np.zeros_like(st0), 4, 1, wi, seed=seed)
    assert B.same_bits(rgb, want[0]).all() and stepped == int(want[1].sum())
    want = oracle.trace_batch(sph, tri, rays, spp=1, max_bounces=3, backend=1, world_index=wi, states=st0, ray_as_given=True)
    rgb, st, _ = B.compose(oracle, sph, tri, rays, st0, 4, 1, wi, as_given=True)
    assert B.same_bits(rgb, want[0]).all() and np.array_equal(st, want[2])


def test_a_step_touches_only_its_active_rays(oracle, cases):
    sph, tri, wi, rays, st0 = cases["spheres"]
    act = np.arange(0, len(rays), 3)
    s = B.step(oracle, sph, tri, rays, st0, 1, wi, active=act)
    full = B.step(oracle, sph, tri, rays, st0, 1, wi)
    rest = np.setdiff1d(np.arange(len(rays)), act)
    assert s["rays"][rest].tobytes() == rays[rest].tobytes() and np.array_equal(s["states"][rest], st0[rest])
    assert not s["bounce"][rest].tobytes().strip(b"\0") and not s["hits"][rest].tobytes().strip(b"\0")
    for k in ("rays", "bounce", "hits"):
        assert s[k][act].tobytes() == full[k][act].tobytes(), k
    still = full["bounce"]["status"] != B.SCATTERED
    assert full["rays"][still].tobytes() == rays[still].tobytes() and np.array_equal(full["states"][still], st0[still])
    moved = ~still
    assert moved.any() and np.all(np.any(full["states"][moved] != st0[moved], 1))


def test_exceptional_arms_of_the_scatter(oracle):
    sph, tri, rays = B.exceptional_case()
    st0 = B.R.states(len(rays), 5)
    m = len(rays) // 3
    for backend in (0, 1):
        s = B.step(oracle, sph, tri, rays, st0, backend)
        status, hits, out = s["bounce"]["status"], s["hits"], s["rays"]
        zero_n = (hits["nx"] == 0) & (hits["ny"] == 0) & (hits["nz"] == 0)
        a, b, c = slice(0, m), slice(m, 2 * m), slice(2 * m, 3 * m)
        # (a) the zero normal is the fallback: Ray::new of the zero vector is NaN
        assert np.all(status[a] == B.SCATTERED) and np.all(hits["index"][a] == 1) and zero_n[a].all()
        assert np.isnan(out["dx"][a]).all() and np.isnan(out["dy"][a]).all() and np.isnan(out["dz"][a]).all()
        # (c) the zero normal with roughness 0: a unit direction, the UnitSphere draw
        assert np.all(status[b] == B.SCATTERED) and np.all(hits["index"][b] == 2) and zero_n[b].all()
        assert np.all(np.isfinite(out["dx"][b]))
        # (b) the mirror: the reflected direction up to rounding
        assert np.all(status[c] == B.SCATTERED) and np.all(hits["index"][c] == 0)
        d = B.directions(rays[c], False).astype(np.float64)
        nn = np.stack([hits["nx"][c], hits["ny"][c], hits["nz"][c]], 1).astype(np.float64)
        refl = d - 2 * np.sum(d * nn, 1, keepdims=True) * nn
        got = np.stack([out["dx"][c], out["dy"][c], out["dz"][c]], 1)
        assert np.allclose(got, refl, atol=1e-5)
        # the NaN rays miss at the next step and the trace agrees: two steps fold to trace_batch
        want = oracle.trace_batch(sph, tri, rays, spp=1, max_bounces=1, backend=backend, states=st0)
        rgb, st, _ = B.compose(oracle, sph, tri, rays, st0, 2, backend)
        assert B.same_bits(rgb, want[0]).all() and np.array_equal(st, want[2])
