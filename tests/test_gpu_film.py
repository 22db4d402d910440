"""The device-resident film on the GPU (ray_tracer_s8_amd/film.py), bytes compared throughout:
1. integrator="path" equals the tile path: accum is the stacked accum of Scene.render_tile_pass and preview() its preview, on cornell16
   under a placed camera, on quad_room (triangles) and under RT_FLAG_NO_BVH_CULL, with k = 1 and k = spp records per pixel in flight;
2. integrator="nee" equals the host composition, per strip the numpy fold of Scene.trace_nee over Scene.camera_rays, for both modes,
   both picks, both light samplings and RT_GLOSSY_MIS, on the glossy room of tests/test_gpu_nee.py; three cuts into passes and two
   values of max_records give identical bytes;
3. the anchor: the same sum from tests/_camera_np.py's rays and tests/_lights_np.py's colours, the per-ray CPU restatements;
4. features() equals Scene.render_aov per strip and resolve() equals Scene.denoise on the downloaded accum and planes;
5. discipline: refused calls leave samples and accum untouched, reset() reproduces the bytes, collect() counts the records, and the
   film collects by itself before the library's limit on uncollected launches;
6. examples/film_nee.py writes the film's resolve.
Every body that touches torch runs in a child process that imports torch first (two HIP runtimes, _abi.check_single_hip_runtime).
Without the feature every test here fails: there is no ray_tracer_s8_amd.film.  No timing is asserted."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from ray_tracer_s8_amd import _abi

import _camera_np as cnp
import _direct_np as D
import _lights_np as LN

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

_PRELUDE = r"""
import sys
import numpy as np
import torch                                                      # first: the library then binds to torch's HIP runtime
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes

def host(film, t):
    film.sync()                                                   # (.cpu() copies on torch's current stream, not the film's)
    return t.cpu().numpy()

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).tobytes() if a.dtype == np.float32 else a.tobytes()

def fold(per):
    tot = np.zeros((per.shape[0], per.shape[2]), np.float32)
    with np.errstate(all="ignore"):
        for s in range(per.shape[1]):
            tot = (tot + per[:, s]).astype(np.float32)
    return tot

def refused(call, *a, **kw):
    try:
        call(*a, **kw)
    except ValueError:
        return True
    return False
"""


def _child(body, *args, timeout=600):
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body, *map(str, args)], capture_output=True, text=True, cwd=ROOT,
                       timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    return r.stdout


def _glossy_room():
    """The glossy room of tests/test_gpu_nee.py: a ground of roughness 0.5, spheres of roughness 0, 0.5 and 1, a sphere light and a
    triangle light, in front of the reference camera."""
    sph, tri = D.lit_room()
    sph["roughness"][:4] = [0.5, 0.0, 0.5, 1.0]
    return sph, tri


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    path = tmp_path_factory.mktemp("film") / "room.npz"
    sph, tri = _glossy_room()
    np.savez(path, sph=sph, tri=tri)
    return path


# ------------------------------------------------------------------------------------------- 1. the path integrator is the tile path

_PATH_CHILD = r"""
name = sys.argv[1]
W, H, DIV, SPP = 48, 27, 3, 5
flags = _abi.RT_FLAG_NO_BVH_CULL if name == "cornell16_no_bvh_cull" else 0
sph, tri = scenes.quad_room() if name == "quad_room" else (scenes.cornell16(), None)
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=6, seed=0xC0FFEE, flags=flags)
       for k in range(DIV)]
pixels = (H // DIV) * W
with rt.Scene(0, rt.World(sph, tri)) as sc:
    if name == "cornell16":
        sc.set_camera(_abi.Camera.look_at((2.5, 1.75, 1.0), (-0.25, 0.1, -2.0), (0.3, 1.0, -0.2)))
    passes = [sc.render_tile_pass(r, 0, SPP, want_f32=True) for r in rqs]
    want_rgb = np.concatenate([p[0] for p in passes])
    want_f32 = np.concatenate([p[1] for p in passes])
    want_acc = np.concatenate([p[2] for p in passes])
    assert want_acc.shape == (H, W, 3) and want_rgb.std() > 1.0
    for max_records, k in ((pixels, 1), (pixels * SPP + pixels - 1, SPP)):
        with rt.Film(sc, rqs, integrator="path", flags=flags, max_records=max_records) as film:
            assert film.k == k and film.samples == 0 and tuple(film.accum.shape) == (H, W, 3)
            film.render_pass(0, 2)
            film.render_pass(2, SPP)
            assert film.samples == SPP
            acc = host(film, film.accum)
            assert bits(acc) == bits(want_acc), (name, k, np.argwhere(acc.view(np.uint32) != want_acc.view(np.uint32))[:5])
            out = film.preview(("rgb", "f32"))
            assert host(film, out["rgb"]).tobytes() == want_rgb.tobytes(), (name, k)
            assert bits(host(film, out["f32"]).reshape(-1)) == bits(want_f32), (name, k)
            st = film.collect()
            # every record is one camera ray made and one ray traced; a launch each per strip and sub-range, and the preview's two
            assert st.primary_rays == 2 * H * W * SPP, st.primary_rays
            assert st.n_launches == 2 * DIV * (SPP if k == 1 else 2) + 2, st.n_launches
print("ok")
"""


@pytest.mark.parametrize("name", ["cornell16", "quad_room", "cornell16_no_bvh_cull"])
def test_path_integrator_equals_the_tile_path(ndev, name):
    _child(_PATH_CHILD, name)


# ------------------------------------------------------------------------------------------- 2. NEE equals the host composition

_NEE_CHILD = r"""
room = np.load(sys.argv[1])
W, H, DIV, SPP, MB = 32, 16, 2, 4, 3
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=MB, seed=0xF11A) for k in range(DIV)]
pixels = (H // DIV) * W
POWER = _abi.RT_FLAG_LIGHTS_BY_POWER
AREA, CONE, BOUNCE, GLOSSY = _abi.RT_LIGHTS_AREA, _abi.RT_LIGHTS_CONE, _abi.RT_GLOSSY_BOUNCE, _abi.RT_GLOSSY_MIS
LIGHT_ONLY, MIS = _abi.RT_NEE_LIGHT_ONLY, _abi.RT_NEE_MIS
combos = [(mode, flags, lights, BOUNCE) for lights in (AREA, CONE) for flags in (0, POWER) for mode in (LIGHT_ONLY, MIS)]
combos += [(MIS, flags, lights, GLOSSY) for lights in (AREA, CONE) for flags in (0, POWER)]
seen = set()
with rt.Scene(0, rt.World(room["sph"], room["tri"])) as sc:
    assert sc.n_lights == 2
    for mode, flags, lights, glossy in combos:
        sc.set_light_sampling(lights)
        sc.set_glossy_sampling(glossy)
        want = []
        for rq in rqs:
            rays, states, _ = sc.camera_rays(rq, 0, SPP)
            o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)
            d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)
            rgb = sc.trace_nee(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=MB, rng_state=states, as_given=True, mode=mode,
                               flags=flags)[0]
            want.append(fold(rgb.reshape(pixels, SPP, 3)).reshape(H // DIV, W, 3))
        want = np.concatenate(want)
        assert np.isfinite(want).all() and want.std() > 0.05
        seen.add(bits(want))
        # three cuts, two values of max_records (k = 1 and k = spp): the same bytes
        for cuts in ([(0, 4)], [(0, 1), (1, 4)], [(0, 2), (2, 3), (3, 4)]):
            for max_records in (pixels, 1 << 22):
                with rt.Film(sc, rqs, integrator="nee", mode=mode, flags=flags, max_records=max_records) as film:
                    for b, e in cuts:
                        film.render_pass(b, e)
                    acc = host(film, film.accum)
                    assert bits(acc) == bits(want), (mode, flags, lights, glossy, cuts, max_records,
                                                     np.argwhere(acc.view(np.uint32) != want.view(np.uint32))[:5])
    # the settings a pass is enqueued under are the scene's at that moment: a change between two passes reaches the second
    sc.set_light_sampling(AREA)
    sc.set_glossy_sampling(BOUNCE)
    with rt.Film(sc, rqs[0], integrator="nee") as film:
        film.render_pass(0, 2)
        sc.set_light_sampling(CONE)
        film.render_pass(2, 4)
        mixed = host(film, film.accum)
    per = {}
    for lights in (AREA, CONE):
        sc.set_light_sampling(lights)
        rays, states, _ = sc.camera_rays(rqs[0], 0, SPP)
        o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)
        d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)
        per[lights] = sc.trace_nee(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=MB, rng_state=states, as_given=True)[0].reshape(pixels, SPP, 3)
    assert bits(mixed.reshape(pixels, 3)) == bits(fold(np.concatenate([per[AREA][:, :2], per[CONE][:, 2:]], 1)))
# every combination is an estimator of its own (the kernel instances are told apart)
assert len(seen) == len(combos), (len(seen), len(combos))
print("ok")
"""


def test_nee_equals_the_host_composition_however_it_is_cut(ndev, room):
    _child(_NEE_CHILD, room)


# ------------------------------------------------------------------------------------------- 3. the anchor on the CPU restatement

_ANCHOR_CHILD = r"""
room, want = np.load(sys.argv[1]), np.load(sys.argv[2])
W, H, DIV, SPP, MB = 12, 8, 2, 3, 3
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=MB, seed=0xA9C0) for k in range(DIV)]
with rt.Scene(0, rt.World(room["sph"], room["tri"])) as sc:
    for mode in (_abi.RT_NEE_LIGHT_ONLY, _abi.RT_NEE_MIS):
        with rt.Film(sc, rqs, integrator="nee", mode=mode) as film:
            film.render_pass(0, 1)
            film.render_pass(1, SPP)
            acc = host(film, film.accum)
        exp = want[f"mode{mode}"]
        assert exp.std() > 0.05
        assert bits(acc) == bits(exp), (mode, np.argwhere(acc.view(np.uint32) != exp.view(np.uint32))[:5])
print("ok")
"""


def test_nee_film_equals_the_cpu_restatements(ndev, oracle, room, tmp_path):
    """12 x 8, 2 divisions, 3 samples: 144 records a strip, because the restatement is per-ray Python.  Rays and states from
    _camera_np.strip_rays, colours from _lights_np.nee one sample per record, the numpy fold."""
    w, h, div, spp, mb = 12, 8, 2, 3, 3
    sph, tri = _glossy_room()
    want = {m: [] for m in LN.MODES}
    for k in range(div):
        rq = _abi.default_request(width=w, height=h, divisions=div, division_no=k, spp=spp, max_bounces=mb, seed=0xA9C0)
        rays, states = cnp.strip_rays(oracle, rq)
        got = LN.nee(oracle, sph, tri, rays, 1, mb, 1, None, as_given=True, states=states)
        for m in LN.MODES:
            per = got["rgb"][m].astype(np.float32).reshape(-1, spp, 3)
            tot = np.zeros((per.shape[0], 3), np.float32)
            with np.errstate(all="ignore"):
                for s in range(spp):
                    tot = (tot + per[:, s]).astype(np.float32)
            want[m].append(tot.reshape(h // div, w, 3))
    assert (LN.LIGHT_ONLY, LN.MIS) == (_abi.RT_NEE_LIGHT_ONLY, _abi.RT_NEE_MIS)
    path = tmp_path / "want.npz"
    np.savez(path, **{f"mode{m}": np.concatenate(want[m]) for m in LN.MODES})
    _child(_ANCHOR_CHILD, room, path)


# ------------------------------------------------------------------------------------------- 4. features and the denoiser

_DENOISE_CHILD = r"""
W, H, DIV, SPP = 48, 27, 3, 5
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=6, seed=0xC0FFEE) for k in range(DIV)]
hs = H // DIV
with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
    sc.set_camera(_abi.Camera.look_at((2.5, 1.75, 1.0), (-0.25, 0.1, -2.0), (0.3, 1.0, -0.2)))
    with rt.Film(sc, rqs, integrator="path") as film:
        film.render_pass(0, SPP)
        planes = film.features(2)
        assert sorted(planes) == ["albedo", "depth", "hits", "normal"] and film.aov_samples == 2
        got = {n: host(film, t) for n, t in planes.items()}
        acc = host(film, film.accum)
        want = [sc.render_aov(r, 0, 2, planes=("albedo", "normal", "depth", "hits"))[0] for r in rqs]
        for n in got:
            stacked = np.concatenate([w[n] for w in want])
            assert got[n].shape == stacked.shape and got[n].tobytes() == stacked.tobytes(), n
        assert got["hits"].max() == 2
        dq = _abi.DenoiseRequest.defaults()
        names = ("rgb", "f32", "linear")
        out = film.resolve(dq, planes, outputs=names)
        res = {o: host(film, out[o]) for o in names}
        strips = [{n: got[n][i * hs:(i + 1) * hs].view(np.uint32 if n == "hits" else got[n].dtype) for n in got} for i in range(DIV)]
        ref, _ = sc.denoise(rqs, [acc[i * hs:(i + 1) * hs] for i in range(DIV)], strips, SPP, 2, dreq=dq, outputs=names)
        for o in names:
            stacked = np.concatenate([r[o] for r in ref])
            assert res[o].shape == stacked.shape and bits(res[o]) == bits(stacked), o
        # it did something: the denoised frame is not the preview, and the request's own sample counts were ignored
        assert res["rgb"].tobytes() != host(film, film.preview()["rgb"]).tobytes()
        assert dq.color_samples == _abi.DenoiseRequest.defaults().color_samples
        # the plain colour a-trous, and a part of the planes
        for part in (None, {n: planes[n] for n in ("normal", "depth", "hits")}):
            out = film.resolve(planes=part, outputs=("f32",))
            ref, _ = sc.denoise(rqs, [acc[i * hs:(i + 1) * hs] for i in range(DIV)],
                                [{n: s[n] for n in (part or {})} for s in strips], SPP, 2, outputs=("f32",))
            assert bits(host(film, out["f32"])) == bits(np.concatenate([r["f32"] for r in ref])), part
        assert refused(film.resolve, planes={"normal": planes["normal"][:hs]})
        assert refused(film.resolve, planes={"colour": planes["normal"]})
print("ok")
"""


def test_features_and_resolve_equal_the_host_forms(ndev):
    _child(_DENOISE_CHILD)


# ------------------------------------------------------------------------------------------- 5. discipline

_DISCIPLINE_CHILD = r"""
room = np.load(sys.argv[1])
W, H, DIV, SPP = 16, 8, 2, 20
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=3, seed=0xD15C) for k in range(DIV)]
with rt.Scene(0, rt.World(room["sph"], room["tri"])) as sc:
    # a stream whose handle is 0 is the scene's own to the library and the default stream to torch
    null = [s for s in (torch.cuda.default_stream(0), torch.cuda.ExternalStream(0, device=0)) if s.cuda_stream == 0]
    assert null, "no stream with handle 0 to refuse"
    for s in null:
        assert refused(rt.Film, sc, rqs, stream=s), s
    assert sc.collect().n_launches == 0
    mine = torch.cuda.Stream(device=0)
    with rt.Film(sc, rqs, stream=mine) as film:
        assert film.stream is mine and mine.cuda_stream != 0
        film.render_pass(0, 2)
        a2 = bits(host(film, film.accum))
    with rt.Film(sc, rqs, _collect_at=6) as film:
        assert film.stream.cuda_stream != 0 and film.samples == 0
        assert refused(film.resolve) and refused(film.preview)             # no samples yet
        film.render_pass(0, 2)
        assert bits(host(film, film.accum)) == a2
        for b, e in ((0, 1), (0, 2), (1, 3), (3, 4), (2, 2), (2, 1), (2, SPP + 1)):
            assert refused(film.render_pass, b, e), (b, e)
            assert film.samples == 2 and bits(host(film, film.accum)) == a2, (b, e)
        assert refused(film.features, 0) and refused(film.features, SPP + 1) and refused(film.features, 1, ("colour",))
        assert refused(film.resolve, outputs=()) and refused(film.resolve, outputs=("png",))
        assert refused(lambda: next(film.render_progressive(0)))
        assert film.samples == 2 and bits(host(film, film.accum)) == a2
        film.render_pass(2, 5)
        a5 = bits(host(film, film.accum))
        assert a5 != a2
        film.reset()
        assert film.samples == 0 and not host(film, film.accum).any()
        film.render_pass(0, 2)
        film.render_pass(2, 5)
        assert bits(host(film, film.accum)) == a5
        film.collect()
        # 20 one-sample passes: 80 launches against a threshold of 6, so the film collects by itself on the way
        film.reset()
        for s in range(SPP):
            film.render_pass(s, s + 1)
        assert film._uncollected <= 6 and film._stats.n_launches >= 74
        one_by_one = bits(host(film, film.accum))
        st = film.collect()
        assert st.n_launches == 2 * DIV * SPP and st.primary_rays == 2 * W * H * SPP, (st.n_launches, st.primary_rays)
        assert st.ray_segments > W * H * SPP and st.kernel_ms > 0
        assert film.collect().n_launches == 0
        film.reset()
        assert list(film.render_progressive(3)) == [3, 6, 9, 12, 15, 18, 20]
        assert bits(host(film, film.accum)) == one_by_one
        assert list(film.render_progressive(3)) == []
    assert film.accum is None and refused(film.render_pass, 0, 1)        # closed
    film.close()
print("ok")
"""


def test_refused_calls_reset_collect_and_the_self_collect(ndev, room):
    _child(_DISCIPLINE_CHILD, room)


# ------------------------------------------------------------------------------------------- 6. the example

_EXAMPLE_CHILD = r"""
import runpy
prefix, example = sys.argv[1], sys.argv[2]
args = ["--frames", "2", "--width", "64", "--height", "36", "--divisions", "2", "--spp", "4", "--pass-spp", "3", "--out", prefix]
sys.argv = [example] + args
mod = runpy.run_path(example, run_name="__main__")
frames = [np.load(f"{prefix}_{i:03d}.npy") for i in range(2)]
assert all(f.shape == (36, 64, 3) and f.dtype == np.uint8 for f in frames) and frames[0].tobytes() != frames[1].tobytes()
sph, rq = scenes.config("c2")
rqs = [_abi.default_request(width=64, height=36, divisions=2, division_no=k, spp=4, max_bounces=rq.max_bounces, seed=rq.seed) for k in range(2)]
with rt.Scene(0, rt.World(sph)) as sc:
    sc.set_light_sampling(_abi.RT_LIGHTS_CONE)
    sc.set_glossy_sampling(_abi.RT_GLOSSY_MIS)
    with rt.Film(sc, rqs, integrator="nee") as film:
        for i in range(2):
            sc.set_camera(mod["orbit_camera"](i, 2))
            film.reset()
            film.render_pass(0, 4)
            out = film.resolve(planes=film.features(1))
            assert host(film, out["rgb"]).tobytes() == frames[i].tobytes(), i
print("ok")
"""


def test_example_film_nee(ndev, tmp_path):
    _child(_EXAMPLE_CHILD, tmp_path / "orbit", ROOT / "examples" / "film_nee.py")
