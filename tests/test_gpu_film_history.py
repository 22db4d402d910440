"""The film history on the GPU (ray_tracer_s8_amd/film_history.py, history_csrc/), bytes compared wherever the
contract is exact:
1. the kernel on the seeded synthetic frames of tests/_history_np.py, uploaded as a film's accum, moments and planes, 1 x 1, 70 x 9
   (whole and as a band) and 130 x 70, with and without normals, over four frames so that both state sets are read and written:
   accum, moments and length equal the numpy restatement;
2. end to end on cornell16 and the quad room, "nee" and "path", three strips (and strips 1 ... 2 of 3), three frames of an orbit with a
   seed per frame: the history's tensors after each frame equal the restatement applied to the downloaded film buffers and planes;
3. the resolves: preview() with alpha = 1 is the film's preview; resolve_guided, variance and resolve equal tests/_film_np.py and
   Scene.denoise on the downloaded history tensors; the film's own resolves return what they returned before;
4. refusals leave the history unchanged; reset() and close();
5. it works: under a still camera eight frames of eight samples have at most a quarter of one frame's squared error against a
   512-sample film; along the orbit the history's error at the last pose is below the single frame's (the ratio is printed);
6. examples/film_temporal.py writes the single-frame and the history resolve of its last frame.
Every body runs in a child process that imports torch first.  Without the feature every test here fails: there is no rt.FilmHistory.
No timing is asserted."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

_PRELUDE = r"""
import math
import sys
import numpy as np
import torch                                                      # first: the libraries then bind to torch's HIP runtime
sys.path.insert(0, "tests")
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, _history_lib, film as film_mod, scenes
import _film_np as fnp
import _history_np as hnp

f32 = np.float32
PLANES = ("normal", "depth", "hits", "index")               # (features() leaves index out unless asked)

def host(film, t):
    film.sync()                                                   # (.cpu() copies on torch's current stream, not the film's)
    return t.cpu().numpy()

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).tobytes() if a.dtype == np.float32 else a.tobytes()

def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if bits(got) != bits(want):
        g, w = (got, want) if got.dtype == np.uint8 else (got.view(np.uint32), want.view(np.uint32))
        bad = np.argwhere(g != w)
        raise AssertionError((what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))

def refused(call, *a, **kw):
    try:
        call(*a, **kw)
    except ValueError:
        return True
    return False

def pose_of(camera):
    return None if camera is None else (tuple(camera.origin), tuple(camera.target), tuple(camera.up))

def orbit_camera(i, n):
    # examples/film_nee.py's
    a = 2.0 * math.pi * i / n
    return rt.Camera.look_at((1.2 * math.sin(a), 0.3 + 0.4 * math.cos(a), 0.2), (0.0, -0.8, -4.0))

def world_of(name):
    if name == "cornell16":
        return rt.World(scenes.cornell16())
    return rt.World(*scenes.quad_room())

def frame_of(film, planes):
    # the downloaded film buffers and planes, as tests/_history_np.py takes a frame
    d = {n: host(film, t) for n, t in planes.items()}
    return dict(C=host(film, film.accum), M=host(film, film.moments), depth=d["depth"], hits=d["hits"].view(np.uint32),
                index=d["index"].view(np.uint32), normal=d.get("normal"))

def check_state(film, history, want, what):
    same(host(film, history.accum), want["accum"], (what, "accum"))
    same(host(film, history.moments), want["moments"], (what, "moments"))
    same(host(film, history.length), want["length"], (what, "length"))
"""


def _child(body, *args, timeout=600):
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body, *map(str, args)], capture_output=True, text=True, cwd=ROOT,
                       timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    return r.stdout


# ------------------------------------------------------------------------------------------- 1. the kernel on synthetic frames

_SYNTH_CHILD = r"""
W, H, DIV, FIRST, N = (int(a) for a in sys.argv[1:6])
E = 4
LOOK = lambda o, t=None: rt.Camera.look_at(o, t if t is not None else (o[0], o[1], o[2] - 1.0))
PATHS = [[None, LOOK((0.02, 0.013, 0.0)), LOOK((0.3, 0.1, 0.0)), LOOK((0.3, 0.1, 0.0))],
         [LOOK((0.4, 0.2, 0.5), (0.0, 0.0, -5.0)), None, LOOK((0, 0, 0), (0.2, 0.05, -1.0)), LOOK((4.0, -2.5, 0.0))],
         [LOOK((0.0, 0.0, -9.0)), None, None, LOOK((0.0, 0.35, 0.0))]]
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=FIRST + k, spp=E, max_bounces=2, seed=1) for k in range(N)]
R = (H // DIV) * N
with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
    with rt.Film(sc, rqs, integrator="path", moments=True) as film:
        dev = film.device
        film.samples = E
        blended = 0
        for p, cams in enumerate(PATHS):
            for consts in ((0.4, 3.0, 0.05, 0.9), (0.05, 8.0, 0.1, None)):
                rng = np.random.default_rng(1000 * W + 10 * p + FIRST)
                with rt.FilmHistory(film, *consts) as history:
                    prev, last = None, None
                    for i, camera in enumerate(cams):
                        fr = hnp.synthetic_frame(rng, rqs[0], pose_of(camera), R, consts[2], consts[3])
                        with torch.cuda.stream(film.stream):
                            film.accum.copy_(torch.from_numpy(fr["C"]).to(dev))
                            film.moments.copy_(torch.from_numpy(fr["M"]).to(dev))
                            planes = dict(depth=torch.from_numpy(fr["depth"]).to(dev), hits=torch.from_numpy(fr["hits"].view(np.int32)).to(dev),
                                          index=torch.from_numpy(fr["index"].view(np.int32)).to(dev), normal=torch.from_numpy(fr["normal"]).to(dev))
                        out = history.accumulate(camera, planes)
                        assert sorted(out) == ["accum", "length", "moments"] and out["length"] is history.length
                        cam = hnp.cameras(rqs[0], pose_of(camera), rqs[0] if last is not None else None, last[0] if last else None)
                        prev = hnp.accumulate(cam, fr, prev, *consts)
                        check_state(film, history, prev, (p, consts, i))
                        last = (pose_of(camera),)
                        blended += int((prev["length"] > 1).sum())
                    assert history.frames == len(cams)
        assert blended > 0 or W * R < 4
print("ok")
"""


@pytest.mark.parametrize("W,H,DIV,FIRST,N", [(1, 1, 1, 0, 1), (70, 9, 3, 0, 3), (70, 9, 3, 1, 2), (130, 70, 5, 0, 5)])
def test_kernel_on_synthetic_frames_equals_the_restatement(ndev, W, H, DIV, FIRST, N):
    _child(_SYNTH_CHILD, W, H, DIV, FIRST, N)


# ------------------------------------------------------------------------------------------- 2. end to end

_E2E_CHILD = r"""
scene, integrator, FIRST, N = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
W, H, DIV, SPP, MB = 96, 54, 3, 4, 3
mine = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=FIRST + k, spp=SPP, max_bounces=MB, seed=0xF11A) for k in range(N)]
consts = (0.2, 8.0, 0.1, 0.9)
with rt.Scene(0, world_of(scene)) as sc:
    sc.set_light_sampling(_abi.RT_LIGHTS_CONE)
    sc.set_glossy_sampling(_abi.RT_GLOSSY_MIS)
    with rt.Film(sc, mine, integrator=integrator, moments=True) as film, rt.FilmHistory(film, *consts) as history:
        prev, last, firsts = None, None, []
        for i in range(3):
            camera = orbit_camera(i, 48) if i else None           # the first frame under the reference camera
            sc.set_camera(camera)
            film.reset(seed=0xF11A + i)
            assert [r.seed for r in film.reqs] == [0xF11A + i] * N and [r.seed for r in mine] == [0xF11A] * N
            film.render_pass(0, SPP)
            planes = film.features(1, PLANES)
            fr = frame_of(film, planes)
            firsts.append(bits(fr["C"]))
            history.accumulate(camera, planes)
            cam = hnp.cameras(film.reqs[0], pose_of(camera), film.reqs[0] if last is not None else None, last[0] if last else None)
            prev = hnp.accumulate(cam, fr, prev, *consts)
            check_state(film, history, prev, (scene, integrator, i))
            last = (pose_of(camera),)
            if i == 0:
                same(host(film, history.accum), fr["C"], "a first frame is the film's")
        assert len(set(firsts)) == 3                               # a seed per frame: three different frames
        took = prev["length"] > 1
        print("pixels with history after three frames:", float(took.mean()))
        assert took.any() and (prev["length"] == 1).any()
        assert bits(prev["accum"][took]) != bits(fr["C"][took])
print("ok")
"""


@pytest.mark.parametrize("scene,integrator", [("cornell16", "nee"), ("cornell16", "path"), ("quad_room", "nee"), ("quad_room", "path")])
def test_three_frames_of_an_orbit_equal_the_restatement(ndev, scene, integrator):
    _child(_E2E_CHILD, scene, integrator, 0, 3)


def test_a_band_of_the_frame_equals_the_restatement(ndev):
    _child(_E2E_CHILD, "cornell16", "nee", 1, 2)


# ------------------------------------------------------------------------------------------- 3. the resolves

_RESOLVE_CHILD = r"""
W, H, DIV, SPP, MB = 96, 54, 3, 4, 3
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=MB, seed=0xF11A) for k in range(DIV)]
hs = H // DIV
OUTPUTS = ("rgb", "linear", "f32", "variance")
DEFAULTS = dict(sigma_l=f32(film_mod.SIGMA_L), var_eps=f32(film_mod.VAR_EPS), k_normal=f32(1.0), k_depth=f32(4.0))

def frame(sc, film, i):
    camera = orbit_camera(i, 48)
    sc.set_camera(camera)
    film.reset(seed=0xABC + i)
    film.render_pass(0, SPP)
    return camera, film.features(1, PLANES)

with rt.Scene(0, world_of("cornell16")) as sc:
    with rt.Film(sc, rqs, integrator="nee", moments=True) as film:
        # alpha = 1: the history is the current frame, and its preview the film's
        with rt.FilmHistory(film, alpha=1.0) as h1:
            assert refused(h1.preview) and refused(h1.resolve_guided) and refused(h1.variance) and refused(lambda: h1.length)
            for i in range(2):
                camera, planes = frame(sc, film, i)
                h1.accumulate(camera, planes)
                want = {o: host(film, t).copy() for o, t in film.preview(("rgb", "f32")).items()}
                got = {o: host(film, t).copy() for o, t in h1.preview(("rgb", "f32")).items()}
                same(got["rgb"], want["rgb"], ("preview rgb", i))
                same(got["f32"], want["f32"], ("preview f32", i))
        with rt.FilmHistory(film, alpha=0.2, n_max=8) as history:
            for i in range(3):
                camera, planes = frame(sc, film, i)
                history.accumulate(camera, planes)
            guide = {n: planes[n] for n in ("normal", "depth", "hits")}
            got = {n: host(film, t) for n, t in guide.items()}
            np_guide = dict(N=got["normal"], D=got["depth"], hits=got["hits"].view(np.uint32))
            # what the film's own resolves return now
            mine = {o: host(film, t).copy() for o, t in film.resolve_guided(guide, OUTPUTS).items()}
            mine["resolve"] = host(film, film.resolve(planes=guide, outputs=("f32",))["f32"]).copy()
            acc, mom = host(film, history.accum), host(film, history.moments)
            assert bits(acc) != bits(host(film, film.accum))
            for it in (0, 3, 5):
                out = history.resolve_guided(guide, OUTPUTS, iterations=it)
                want = fnp.resolve(acc, mom, SPP, iterations=it, **DEFAULTS, **np_guide)
                for o in OUTPUTS:
                    same(host(film, out[o]), want[o], ("resolve_guided", it, o))
            same(host(film, history.variance()), fnp.entry_variance(mom, SPP), "variance()")
            same(host(film, history.preview(("f32",))["f32"]), np.sqrt(acc / f32(SPP)), "preview")
            # resolve: Scene.denoise on the downloaded history sums
            names = ("rgb", "f32", "linear")
            out = history.resolve(None, guide, names)
            res = {o: host(film, out[o]).copy() for o in names}
            strips = [{n: got[n][i * hs:(i + 1) * hs].view(np.uint32 if n == "hits" else got[n].dtype) for n in got} for i in range(DIV)]
            ref, _ = sc.denoise(film.reqs, [acc[i * hs:(i + 1) * hs] for i in range(DIV)], strips, SPP, 1, outputs=names)
            for o in names:
                same(res[o], np.concatenate([r[o] for r in ref]), ("resolve", o))
            # ... and the film's own resolves still return what they returned
            again = {o: host(film, t).copy() for o, t in film.resolve_guided(guide, OUTPUTS).items()}
            for o in OUTPUTS:
                same(again[o], mine[o], ("the film's resolve_guided", o))
            same(host(film, film.resolve(planes=guide, outputs=("f32",))["f32"]), mine["resolve"], "the film's resolve")
            assert bits(mine["linear"]) != bits(fnp.resolve(acc, mom, SPP, iterations=5, **DEFAULTS, **np_guide)["linear"])
print("ok")
"""


def test_the_films_resolves_on_the_history(ndev):
    _child(_RESOLVE_CHILD)


# ------------------------------------------------------------------------------------------- 4. refusals and state

_DISCIPLINE_CHILD = r"""
W, H, DIV, SPP = 32, 18, 2, 4
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=3, seed=0xD15C) for k in range(DIV)]
with rt.Scene(0, world_of("cornell16")) as sc:
    with rt.Film(sc, rqs) as plain:
        assert refused(rt.FilmHistory, plain)                                       # a film without moments
    with rt.Film(sc, rqs, moments=True) as film:
        for kw in (dict(alpha=0.0), dict(alpha=2.0), dict(n_max=0), dict(k_depth=-1.0), dict(k_normal=float("nan"))):
            assert refused(rt.FilmHistory, film, **kw), kw
        with rt.FilmHistory(film, alpha=0.3, n_max=4, k_normal=0.9) as history:
            assert refused(history.accumulate, None, {})                            # no samples yet
            film.render_pass(0, 2)
            planes = film.features(1, PLANES)
            assert refused(lambda: history.accum) and history.frames == 0
            history.accumulate(None, planes)
            film.reset(seed=5)
            film.render_pass(0, 2)
            planes = film.features(1, PLANES)
            history.accumulate(None, planes)
            state = lambda: (history.frames, bits(host(film, history.accum)), bits(host(film, history.moments)),
                             bits(host(film, history.length)), history._cur)
            s2 = state()
            assert host(film, history.length).max() == 2.0
            bad = [dict(planes={}), dict(planes=None), dict(planes={n: planes[n] for n in ("depth", "hits")}),
                   dict(planes={n: planes[n] for n in ("depth", "hits", "index")}),               # k_normal: the normal is needed
                   dict(planes=dict(planes, depth=planes["depth"][:4])), dict(planes=dict(planes, hits=planes["depth"])),
                   dict(planes=dict(planes, index=planes["index"].cpu())), dict(planes=dict(planes, normal=planes["normal"].double())),
                   dict(camera="front")]
            for kw in bad:
                args = dict(camera=None, planes=planes)
                args.update(kw)
                assert refused(history.accumulate, **args), kw
                assert state() == s2, kw
            # a pose the library refuses: its status, and nothing changed
            try:
                history.accumulate(rt.Camera.look_at((0, 0, 0), (0, 0, 0)), planes)
                raise AssertionError("a degenerate pose was accepted")
            except _history_lib.RthError as e:
                assert e.status == 1
            assert state() == s2
            # a frame whose sample count differs from the last
            film.render_pass(2, 3)
            assert refused(history.accumulate, None, planes) and state() == s2
            # reset(): the next frame is a first frame, at any sample count
            history.reset()
            assert history.frames == 0 and refused(lambda: history.length)
            history.accumulate(None, planes)
            assert (host(film, history.length) == 1).all() and bits(host(film, history.accum)) == bits(host(film, film.accum))
            # the state is allocated once: the tensors alternate between two sets
            a0 = history.accum
            film.reset(seed=6)
            film.render_pass(0, 3)
            history.accumulate(None, film.features(1, PLANES))
            a1 = history.accum
            film.reset(seed=7)
            film.render_pass(0, 3)
            history.accumulate(None, film.features(1, PLANES))
            assert history.accum is a0 and a1 is not a0 and host(film, history.length).max() == 3.0
        assert refused(history.accumulate, None, planes) and refused(history.reset) and refused(lambda: history.accum)      # closed
        history.close()
    h = rt.FilmHistory.__new__(rt.FilmHistory)
    h.close()                                                                        # never constructed: nothing to do
print("ok")
"""


def test_refusals_reset_and_close(ndev):
    _child(_DISCIPLINE_CHILD)


# ------------------------------------------------------------------------------------------- 5. it works

_WORKS_CHILD = r"""
moving = sys.argv[1] == "moving"
W, H, DIV, SPP, MB, FRAMES, REF = 96, 54, 3, 8, 4, 8, 512
def strips(spp, seed):
    return [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=spp, max_bounces=MB, seed=seed) for k in range(DIV)]
with rt.Scene(0, world_of("cornell16")) as sc:
    sc.set_light_sampling(_abi.RT_LIGHTS_CONE)
    sc.set_glossy_sampling(_abi.RT_GLOSSY_MIS)
    # still: alpha below 1 / FRAMES, the history is the plain mean of its frames; moving: the defaults
    kw = dict(alpha=0.05, n_max=32) if not moving else {}
    with rt.Film(sc, strips(SPP, 100), integrator="nee", moments=True) as film, rt.FilmHistory(film, **kw) as history:
        for i in range(FRAMES):
            camera = orbit_camera(i, 96) if moving else None
            sc.set_camera(camera)
            film.reset(seed=100 + i)
            film.render_pass(0, SPP)
            history.accumulate(camera, film.features(1, ("depth", "hits", "index")))
        single = host(film, film.accum) / f32(SPP)
        mean = host(film, history.accum) / f32(SPP)
        length = host(film, history.length)
    with rt.Film(sc, strips(REF, 0xBEEF), integrator="nee") as ref_film:              # the same camera: the last pose
        ref_film.render_pass(0, REF)
        ref = host(ref_film, ref_film.accum) / f32(REF)
err = lambda img, m: float((((img - ref) ** 2).sum(-1))[m].mean())
if moving:
    took = length >= 2.0
    ratio = err(mean, took) / err(single, took)
    print(f"moving camera: {took.mean():.3f} of the pixels have length >= 2, mean length {length[took].mean():.2f}, "
          f"squared error of the history / of the last frame = {ratio:.3f}")
    assert took.mean() > 0.5
    assert ratio < 1.0, ratio
else:
    # "reached 8": a pixel reprojects onto itself up to the roundings of its ray and projection, some 16 ulps of a coordinate below
    # 128, 1.2e-4 of a pixel in x and in y; that sliver of weight goes to a neighbour whose history may be as short as 1, which costs
    # at most 2.4e-4 x 7 of length a frame, 0.012 over 7 frames: 7.98 and up is a history of all 8 frames
    full = length >= 7.98
    left_out = 1.0 - full.mean()
    ratio = err(mean, full) / err(single, full)
    print(f"still camera: {left_out:.3f} of the pixels left out (length below 8), "
          f"squared error of the history / of the last frame = {ratio:.3f}")
    assert left_out <= 0.25, left_out
    assert ratio <= 0.25, ratio
print("ok")
"""


def test_it_works_under_a_still_camera(ndev):
    """Independent frames give 1/8 of a frame's squared error; the reference's own noise (8 / 512 of a frame's) brings the expected
    ratio to about 0.14; 0.25 leaves under a factor of two for that and for the bilinear weight that is not exactly 1 on the pixel
    itself.  At most a quarter of the pixels may fall out because their length stayed below 8 (primitive edges, where sample 0's
    jitter picks another primitive from frame to frame)."""
    print(_child(_WORKS_CHILD, "still"))


def test_it_works_along_the_orbit(ndev):
    """At the last pose of eight, with FilmHistory's defaults, over the pixels with length >= 2: the history's error is below the
    single frame's.  The ratio is measured, not fixed."""
    print(_child(_WORKS_CHILD, "moving"))


# ------------------------------------------------------------------------------------------- 6. the example

_EXAMPLE_CHILD = r"""
import runpy
out_dir, example = sys.argv[1], sys.argv[2]
sys.argv = [example, "--out", out_dir + "/t", "--width", "64", "--height", "36", "--divisions", "2", "--spp", "4", "--frames", "3"]
runpy.run_path(example, run_name="__main__")
got = {n: np.load(f"{out_dir}/t_{n}.npy") for n in ("single", "history")}
assert got["single"].shape == got["history"].shape == (36, 64, 3) and got["single"].dtype == got["history"].dtype == np.uint8
assert got["single"].tobytes() != got["history"].tobytes() and got["history"].std() > 1.0
print("ok")
"""


def test_example_film_temporal(ndev, tmp_path):
    _child(_EXAMPLE_CHILD, tmp_path, ROOT / "examples" / "film_temporal.py")
