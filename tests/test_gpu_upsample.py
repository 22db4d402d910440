"""The film upsampler on the GPU (ray_tracer_s8_amd/film_upsampler.py, upsample_csrc/), bytes compared throughout:
1. rtu_upsample on the uploaded synthetic pairs of tests/_upsample_np.py with no scene: low films of 1 x 1, 5 x 3, 33 x 7 (partial
   workgroups in both directions) and 64 x 9, at s = 2, 3, 4, every plane set a call may have (albedo on and off among them), strip
   offsets above zero, outputs into sentinel-filled tensors: all four outputs equal the restatement's, and an output not asked for
   keeps its sentinel (one form of the kernel exists, the direct one);
2. on the glossy room of tests/test_gpu_film.py, a film of the three strips of a 24 x 14 frame (4 rows each) at 4 samples, "nee" MIS,
   upsampled to the 48 x 28 and the 72 x 42 frame: upsample() on the film's resolve and resolve(source=...) for the three sources
   equal the restatement run on the tensors read back; the film's accum, moments and samples are untouched;
3. refused calls change nothing: aliasing, a plane of the wrong shape, a closed film, a stream-0 film;
4. examples/film_upsample.py writes its three files.
Every body runs in a child process that imports torch first.  Without the feature every test here fails: there is no
rt.FilmUpsampler.  No timing is asserted."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _direct_np as D

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

_PRELUDE = r"""
import sys
import numpy as np
import torch                                                      # first: the libraries then bind to torch's HIP runtime
sys.path.insert(0, "tests")
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, _upsample_lib as ul, film_upsampler as fu, scenes
import _upsample_np as unp

f32 = np.float32

def host(film, t):
    film.sync()                                                   # (.cpu() copies on torch's current stream, not the film's)
    return t.cpu().numpy()

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).tobytes() if a.dtype == np.float32 else a.tobytes()

def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if bits(got) != bits(want):
        g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
        bad = np.argwhere(g != w)
        raise AssertionError((what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))

def refused(call, *a, **kw):
    try:
        call(*a, **kw)
    except ValueError:
        return True
    return False

OUTS = ("linear", "f32", "rgb", "class")
NP_OUT = dict(linear="linear", f32="f32", rgb="rgb", cls="class")
"""


def _child(body, *args, timeout=600):
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body, *map(str, args)], capture_output=True, text=True, cwd=ROOT,
                       timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    """The glossy room of tests/test_gpu_film.py."""
    path = tmp_path_factory.mktemp("film_upsample") / "room.npz"
    sph, tri = D.lit_room()
    sph["roughness"][:4] = [0.5, 0.0, 0.5, 1.0]
    np.savez(path, sph=sph, tri=tri)
    return path


# ------------------------------------------------------------------------------------------- 1. the kernel, no scene

_SYNTHETIC_CHILD = r"""
WL, RL, ABOVE, BELOW = (int(v) for v in sys.argv[1:5])
lib = ul.load()
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
SENTINEL = 0x5A

def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)

calls = 0
for s in unp.SCALES:
    L, lo, hi, geom, kl, kh, _ = unp.pair(unp.seed_of(WL, RL, s), WL, RL, s, ABOVE, BELOW)
    Rh, Wh = geom["Rh"], geom["Wh"]
    assert (geom["y0l"] > 0) == (ABOVE > 0) and geom["y0h"] == s * geom["y0l"]
    with torch.cuda.stream(stream):
        d_L, d_lo, d_hi = up(L), {n: up(a) for n, a in lo.items()}, {n: up(a) for n, a in hi.items()}
    for i, names in enumerate(unp.plane_subsets()):
        want = unp.upsample(L, unp.take(lo, names), unp.take(hi, names), geom, unp.K_DEPTH, unp.K_NORMAL, unp.EPS, kl, kh)
        for asked in (OUTS, (OUTS[i % 4],)):
            with torch.cuda.stream(stream):
                out = dict(linear=torch.full((Rh, Wh, 3), 7.0, dtype=torch.float32, device=dev),
                           f32=torch.full((Rh, Wh, 3), 7.0, dtype=torch.float32, device=dev),
                           rgb=torch.full((Rh, Wh, 3), SENTINEL, dtype=torch.uint8, device=dev),
                           cls=torch.full((Rh, Wh), SENTINEL, dtype=torch.uint8, device=dev))
                side = lambda d, k: ul.Planes(**{n: d[n].data_ptr() for n in names}, samples=k)
                ptr = lambda o, key: out[key].data_ptr() if o in asked else None
                a = ul.UpsampleArgs(Wl=WL, Rl=RL, Hl=geom["Hl"], y0l=geom["y0l"], Wh=Wh, Rh=Rh, Hh=geom["Hh"], y0h=geom["y0h"], scale=s,
                                    k_depth=float(unp.K_DEPTH), k_normal=float(unp.K_NORMAL), eps=float(unp.EPS), linear=d_L.data_ptr(),
                                    lo=side(d_lo, kl), hi=side(d_hi, kh), out_linear=ptr("linear", "linear"), out_f32=ptr("f32", "f32"),
                                    out_rgb=ptr("rgb", "rgb"), out_class=ptr("class", "cls"))
                ul.check("rtu_upsample", lib.rtu_upsample(a, stream.cuda_stream))
            stream.synchronize()
            calls += 1
            for key, o in NP_OUT.items():
                got = out[key].cpu().numpy()
                if o in asked:
                    same(got, want[key], (s, names, asked, o))
                elif got.dtype == np.uint8:
                    assert (got == SENTINEL).all(), (s, names, asked, o, "the sentinel")
                else:
                    assert (got == 7.0).all(), (s, names, asked, o, "the sentinel")
        if WL * RL > 15 and names == unp.PLANES:
            c = want["counts"]
            assert c["class0"] >= 0.05 * Rh * Wh and c["class1"] >= 0.05 * Rh * Wh, c        # both classes, as on the CPU
    # the inputs are read only
    same(d_L.cpu().numpy(), L, "linear")
    for n in unp.PLANES:
        assert bits(d_lo[n].cpu().numpy()) == bits(lo[n]) and bits(d_hi[n].cpu().numpy()) == bits(hi[n]), n
assert calls == 3 * 24 * 2
print("ok")
"""


@pytest.mark.parametrize("Wl,Rl,above,below", [(1, 1, 0, 0), (5, 3, 1, 1), (33, 7, 2, 0), (64, 9, 1, 1)])
def test_the_kernel_on_synthetic_pairs(ndev, Wl, Rl, above, below):
    _child(_SYNTHETIC_CHILD, Wl, Rl, above, below)


# ------------------------------------------------------------------------------------------- 2. the glossy room

_SCENE = r"""
room = np.load(sys.argv[1])
W, H, DIV, SPP, MB = 24, 14, 3, 4, 3
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=MB, seed=0x5A3F) for k in range(DIV)]
ROWS = (H // DIV) * DIV                                            # 12: the film's rows; the frame's last two belong to no strip

def strips_hi(s):
    # the s W x s H frame in 7 divisions of 2 s rows: the first 6 are the film's 12 rows times s
    return [_abi.default_request(width=s * W, height=s * H, divisions=7, division_no=k, spp=SPP, max_bounces=MB, seed=0x5A3F)
            for k in range(6)]

def scene():
    sc = rt.Scene(0, rt.World(room["sph"], room["tri"]))
    sc.set_light_sampling(_abi.RT_LIGHTS_CONE)
    sc.set_glossy_sampling(_abi.RT_GLOSSY_MIS)
    return sc

def np_planes(film, planes, names):
    out = {}
    for n in names:
        a = host(film, planes[n])
        out[n] = a.view(np.uint32) if a.dtype == np.int32 else a
    return out

def restated(film, up, linear, names, kl, kh):
    geom = dict(Hl=H, y0l=0, Hh=up.scale * H, y0h=0, Rh=up.rows, Wh=up.width)
    return unp.upsample(host(film, linear), np_planes(film, film.planes, names), np_planes(film, up.planes_hi, names), geom,
                        f32(up.k_depth), f32(up.k_normal), f32(up.eps), kl, kh)

def check(film, out, want, what):
    for key, o in NP_OUT.items():
        if o in out:
            same(host(film, out[o]), want[key], (what, o))
"""

_ROOM_CHILD = _SCENE + r"""
with scene() as sc:
    with rt.Film(sc, rqs, integrator="nee", mode=_abi.RT_NEE_MIS, moments=True) as film:
        assert film.rows == ROWS
        film.render_pass(0, SPP)
        film.features(2, fu.PLANES)
        state = lambda: (film.samples, bits(host(film, film.accum)), bits(host(film, film.moments)))
        s0 = state()
        guide = {n: film.planes[n] for n in ("normal", "depth", "hits")}
        for s in (2, 3):
            with rt.FilmUpsampler(film, strips_hi(s)) as up:
                assert (up.scale, up.width, up.rows) == (s, s * W, s * ROWS)
                hi = up.features(1)
                assert sorted(hi) == sorted(fu.PLANES) and up.aov_samples_hi == 1 and tuple(hi["albedo"].shape) == (s * ROWS, s * W, 3)
                idx = host(film, hi["index"]).view(np.uint32)
                assert len(np.unique(idx)) > 2                                 # a condition of the test: several primitives in view
                linear = film.resolve(outputs=("linear",))["linear"]
                for names, kw in ((fu.PLANES, {}), (("normal", "depth", "hits", "index"), dict(albedo=False)), ((), dict(planes_lo={}, planes_hi={}))):
                    out = up.upsample(linear, outputs=OUTS, **kw)
                    want = restated(film, up, linear, names, 2, 1)
                    check(film, out, want, ("upsample", s, names))
                    n = want["cls"].size
                    if names == fu.PLANES:
                        assert want["counts"]["class0"] > 0 and sum(want["counts"][t] for t in unp.TESTS) > 0, want["counts"]
                    if not names:
                        assert want["counts"]["class1"] == 0
                # without the index planes
                with rt.FilmUpsampler(film, strips_hi(s), use_index=False, k_depth=0.05, k_normal=0.95, eps=0.01) as up2:
                    up2.features(1, ("albedo", "normal", "depth", "hits"))
                    out = up2.upsample(linear, outputs=("linear", "class"))
                    want = restated(film, up2, linear, ("albedo", "normal", "depth", "hits"), 2, 1)
                    check(film, out, want, ("use_index=False", s))
                # the three sources: the film's own linear image of that resolve, upsampled
                for source, kw, again in (("resolve", dict(planes=guide), lambda: film.resolve(planes=guide, outputs=("linear",))),
                                          ("resolve", {}, lambda: film.resolve(outputs=("linear",))),
                                          ("guided", dict(planes=guide, iterations=2), lambda: film.resolve_guided(guide, ("linear",), 2)),
                                          ("preview", {}, lambda: film.preview(("linear",)))):
                    out = up.resolve(source, outputs=OUTS, **kw)
                    got = {o: host(film, t).copy() for o, t in out.items()}
                    want = restated(film, up, again()["linear"], fu.PLANES, 2, 1)
                    for key, o in NP_OUT.items():
                        same(got[o], want[key], ("resolve", source, s, o))
                assert state() == s0, "the film's accum, moments and samples are untouched"
        assert film.collect().n_launches > 0
print("ok")
"""


def test_the_room_upsampled_equals_the_restatement(ndev, room):
    _child(_ROOM_CHILD, room)


# ------------------------------------------------------------------------------------------- 3. discipline

_DISCIPLINE_CHILD = _SCENE + r"""
with scene() as sc:
    with rt.Film(sc, rqs, integrator="nee", mode=_abi.RT_NEE_MIS) as film:
        film.render_pass(0, 2)
        film.features(1, fu.PLANES)
        for bad in (rqs, strips_hi(5), strips_hi(2)[:5], strips_hi(2)[1:]):
            assert refused(rt.FilmUpsampler, film, bad)
        for kw in (dict(k_depth=-1.0), dict(k_normal=float("nan")), dict(eps=0.0), dict(eps=float("inf"))):
            assert refused(rt.FilmUpsampler, film, strips_hi(2), **kw), kw
        up = rt.FilmUpsampler(film, strips_hi(2))
        linear = film.preview(("linear",))["linear"]
        assert refused(up.upsample, linear)                                   # the film has planes, the upsampler none yet
        hi = up.features(1)
        out = up.upsample(linear, outputs=OUTS)
        state = lambda: tuple(bits(host(film, out[o])) for o in OUTS) + (bits(host(film, film.accum)), film.samples)
        s0 = state()
        # a plane of the wrong shape, dtype or side; a linear image of the wrong shape; outputs and sources that do not exist
        wrong = dict(hi, depth=hi["depth"][:-1])
        assert refused(up.upsample, linear, planes_hi=wrong)
        assert refused(up.upsample, linear, planes_hi=dict(hi, hits=hi["depth"]))
        assert refused(up.upsample, linear, planes_lo=dict(film.planes, normal=hi["normal"]))
        assert refused(up.upsample, linear, planes_hi={n: hi[n] for n in ("albedo", "normal")})      # planes on one side only
        assert refused(up.upsample, linear, planes_lo={"depth": film.planes["depth"]}, planes_hi={"depth": hi["depth"]})
        assert refused(up.upsample, linear[:-1]) and refused(up.upsample, hi["albedo"]) and refused(up.upsample, None)
        assert refused(up.upsample, linear, outputs=()) and refused(up.upsample, linear, outputs=("variance",))
        assert refused(up.resolve, "temporal") and refused(up.resolve, "preview", iterations=1)
        assert refused(up.resolve, "guided")                                  # the film keeps no moments
        assert refused(up.features, 0) and refused(up.features, 1, ("colour",)) and refused(up.features, 1, ())
        assert state() == s0
        # aliasing, at the library: an output that is an input of the call is refused with a status and nothing is written
        lib = ul.load()
        R2, W2 = up.rows, up.width
        a = ul.UpsampleArgs(Wl=W, Rl=ROWS, Hl=H, y0l=0, Wh=W2, Rh=R2, Hh=2 * H, y0h=0, scale=2, k_depth=0.1, k_normal=0.9, eps=0.01,
                            linear=linear.data_ptr(), lo=ul.Planes(albedo=film.planes["albedo"].data_ptr(), samples=1),
                            hi=ul.Planes(albedo=hi["albedo"].data_ptr(), samples=1), out_linear=hi["albedo"].data_ptr())
        before = bits(host(film, hi["albedo"]))
        assert lib.rtu_upsample(a, film.stream.cuda_stream) == 1
        a.out_linear, a.out_f32 = out["linear"].data_ptr(), out["linear"].data_ptr() + 12
        assert lib.rtu_upsample(a, film.stream.cuda_stream) == 1
        a.out_f32, a.out_class = None, linear.data_ptr()
        assert lib.rtu_upsample(a, film.stream.cuda_stream) == 1
        try:
            ul.check("rtu_upsample", lib.rtu_upsample(a, film.stream.cuda_stream))
            raise SystemExit("an aliasing call was not refused")
        except ul.RtuError as e:
            assert e.status == 1
        assert bits(host(film, hi["albedo"])) == before and state() == s0
        # a stream-0 film: to the library 0 is the scene's own stream, to torch the default one
        own = film.stream
        film.stream = torch.cuda.default_stream(film.device)
        assert film.stream.cuda_stream == 0
        assert refused(rt.FilmUpsampler, film, strips_hi(2)) and refused(up.upsample, linear) and refused(up.features, 1)
        film.stream = own
        assert state() == s0
        up.close()
        up.close()
        assert refused(up.upsample, linear) and refused(up.features, 1) and refused(up.resolve, "preview")
        assert film.accum is not None
        with rt.FilmUpsampler(film, strips_hi(3)) as up3:
            up3.features(1)
            assert tuple(up3.resolve("preview", outputs=("class",))["class"].shape) == (3 * ROWS, 3 * W)
        assert up3._out is None
        up = rt.FilmUpsampler(film, strips_hi(2))
        up.features(1)
    assert refused(up.upsample, linear) and refused(up.features, 1) and refused(rt.FilmUpsampler, film, strips_hi(2))      # a closed film
    up.close()
print("ok")
"""


def test_refused_calls_change_nothing(ndev, room):
    _child(_DISCIPLINE_CHILD, room)


# ------------------------------------------------------------------------------------------- 4. the example

_EXAMPLE_CHILD = r"""
import runpy
out_dir, example = sys.argv[1], sys.argv[2]
sys.argv = [example, out_dir, "--width", "64", "--height", "36", "--divisions", "2", "--spp", "4"]
runpy.run_path(example, run_name="__main__")
got = {n: np.load(f"{out_dir}/{n}.npy") for n in ("upsampled", "bilinear", "class")}
assert got["upsampled"].shape == got["bilinear"].shape == (72, 128, 3) and got["upsampled"].dtype == got["bilinear"].dtype == np.uint8
assert got["class"].shape == (72, 128) and got["class"].dtype == np.uint8 and set(np.unique(got["class"])) <= {0, 1}
assert got["upsampled"].std() > 1 and (got["upsampled"] != got["bilinear"]).any() and (got["class"] == 0).any()
sph, rq = scenes.config("c2")
strips = lambda s: [_abi.default_request(width=64 * s, height=36 * s, divisions=2, division_no=k, spp=4, max_bounces=rq.max_bounces,
                                         seed=rq.seed) for k in range(2)]
with rt.Scene(0, rt.World(sph)) as sc:
    sc.set_light_sampling(_abi.RT_LIGHTS_CONE)
    sc.set_glossy_sampling(_abi.RT_GLOSSY_MIS)
    with rt.Film(sc, strips(1), integrator="nee") as film, rt.FilmUpsampler(film, strips(2)) as up:
        film.render_pass(0, 4)
        planes = film.features(1, fu.PLANES)
        up.features(1)
        guide = {n: planes[n] for n in ("albedo", "normal", "depth", "hits")}
        out = up.resolve("resolve", outputs=("rgb", "class"), planes=guide)
        same(host(film, out["rgb"]), got["upsampled"], "upsampled.npy")
        same(host(film, out["class"]), got["class"], "class.npy")
        linear = film.resolve(planes=guide, outputs=("linear",))["linear"]
        same(host(film, up.upsample(linear, planes_lo={}, planes_hi={})["rgb"]), got["bilinear"], "bilinear.npy")
print("ok")
"""


def test_example_film_upsample(ndev, tmp_path):
    _child(_EXAMPLE_CHILD, tmp_path, ROOT / "examples" / "film_upsample.py")
