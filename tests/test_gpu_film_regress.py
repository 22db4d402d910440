"""The film's regression resolve on the GPU (ray_tracer_s8_amd/film.py, film_csrc/), bytes compared throughout with the
numpy restatement of film_csrc/rt_film.h (tests/_film_regress_np.py):
1. synthetic accum and planes uploaded at 1 x 1, 16 x 16, 17 x 16, 33 x 47, 70 x 9 and 130 x 70 (a lone pixel, exactly one cell, one
   pixel past a cell, ragged edges in both axes, more nodes than one wave of workgroups), the five plane subsets, two ridges:
   regression_model and every output equal the restatement; and the awkward windows of tests/test_film_regress_host.py;
2. on the glossy room of tests/test_gpu_film.py, three strips at 48 x 27: the result equals the restatement on the downloaded accum
   and features(); one sample; moments=False; _state; a refused call changes no tensor; a second call overwrites the first's tensors;
   reset() reproduces the bytes;
3. the planes of tests/_extreme_planes.py (subnormal, huge, infinite, NaN) in the discipline of tests/test_gpu_film_extremes.py:
   bytes are equal wherever the restatement is not a NaN, and a NaN where it is; the inputs are read only;
4. examples/film_regress.py writes its three files.
Every body runs in a child process that imports torch first.  Without the feature every test here fails: Film has no
resolve_regression.  No timing is asserted."""
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
from ray_tracer_s8_amd import _abi, _film_lib, film as film_mod, scenes
import _extreme_planes as xp
import _film_regress_np as rnp

f32 = np.float32
np.seterr(all="ignore")
OUTPUTS = ("rgb", "linear", "f32")
EPS = f32(_abi.DenoiseRequest.defaults().albedo_eps)

def host(film, t):
    film.sync()                                                   # (.cpu() copies on torch's current stream, not the film's)
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a

def up(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).tobytes() if a.dtype == np.float32 else a.tobytes()

def refused(call, *a, **kw):
    try:
        call(*a, **kw)
    except ValueError:
        return True
    return False

def upload(film, s, e, k):
    # a synthetic image as the film's accum and planes
    dev = film.device
    with torch.cuda.stream(film.stream):
        film.accum.copy_(up(s["C"], dev))
        planes = dict(albedo=up(s["A"], dev), normal=up(s["N"], dev), depth=up(s["D"], dev), hits=up(s["hits"], dev))
    film.samples, film.aov_samples = e, k
    return planes

def check(film, planes, s, names, e, k, ridge, what):
    out = film.resolve_regression({n: planes[n] for n in names}, OUTPUTS, ridge=float(ridge))
    assert sorted(out) == sorted(OUTPUTS)
    want = rnp.resolve(s["C"], e, k=k, albedo_eps=EPS, ridge=f32(ridge), **rnp.np_planes(s, names))
    xp.same(host(film, film.regression_model), want["model"], (what, names, float(ridge), "model"))
    for o in OUTPUTS:
        xp.same(host(film, out[o]), want[o], (what, names, float(ridge), o))
    return want
"""


def _child(body, *args, timeout=600):
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body, *map(str, args)], capture_output=True, text=True, cwd=ROOT,
                       timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), f"child exit {r.returncode}\n" + r.stdout[-6000:] + r.stderr[-6000:]
    return r.stdout


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    """The glossy room of tests/test_gpu_film.py."""
    path = tmp_path_factory.mktemp("film_regress") / "room.npz"
    sph, tri = D.lit_room()
    sph["roughness"][:4] = [0.5, 0.0, 0.5, 1.0]
    np.savez(path, sph=sph, tri=tri)
    return path


# ------------------------------------------------------------------------------------------- 1. synthetic images

_SYNTH_CHILD = r"""
import test_film_regress_host as th
E, K = 8, 4
solved = fallback = 0
with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
    for W, R in [(1, 1), (16, 16), (17, 16), (33, 47), (70, 9), (130, 70)]:
        s = rnp.synthetic(np.random.default_rng(R * 1000 + W), R, W, E, K)
        rq = _abi.default_request(width=W, height=R, divisions=1, division_no=0, spp=E, max_bounces=2, seed=1)
        with rt.Film(sc, rq, integrator="path") as film:
            planes = upload(film, s, E, K)
            assert film_mod.regression_nodes(W, R) == rnp.nodes(W, R)
            for names in rnp.SUBSETS:
                for ridge in (film_mod.RIDGE, 1e-1):
                    want = check(film, planes, s, names, E, K, ridge, (W, R))
                    assert tuple(film.regression_model.shape) == want["model"].shape
                    solved += int((want["model"][..., 27] == 1).sum())
            xp.identical(host(film, film.accum), s["C"], "accum")
            for n, k in rnp.KEYS.items():
                xp.identical(host(film, planes[n]), s[k], n)
    # the awkward windows, and a pivot lost to rounding
    rq = _abi.default_request(width=70, height=9, divisions=1, division_no=0, spp=E, max_bounces=2, seed=1)
    with rt.Film(sc, rq, integrator="path") as film:
        for kind in th.KINDS:
            s = th.special(kind)
            want = check(film, upload(film, s, E, K), s, rnp.SUBSETS[-1], E, K, film_mod.RIDGE, kind)
            fallback += int(((want["model"][..., 27] == 0) & (want["model"][..., 26] > 0)).sum())
        s = th.special("flat wall")
        want = check(film, upload(film, s, E, K), s, ("normal", "hits"), E, K, 1e-12, "rounding")
        fallback += int(((want["model"][..., 27] == 0) & (want["model"][..., 26] > 0)).sum())
assert solved > 300 and fallback > 4, (solved, fallback)
print(solved, "fits,", fallback, "fallbacks")
print("ok")
"""


def test_synthetic_images_equal_the_restatement(ndev):
    print(_child(_SYNTH_CHILD))


# ------------------------------------------------------------------------------------------- 2. the glossy room

_ROOM_CHILD = r"""
room = np.load(sys.argv[1])
W, H, DIV, SPP, MB = 48, 27, 3, 5, 3
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=MB, seed=0xF11A) for k in range(DIV)]
ALL = ("albedo", "normal", "depth", "hits")

def np_kw(got, names):
    return {rnp.KEYS[n]: ((got[n].view(np.uint32) if n == "hits" else got[n]) if n in names else None) for n in rnp.KEYS}

with rt.Scene(0, rt.World(room["sph"], room["tri"])) as sc:
    sc.set_light_sampling(_abi.RT_LIGHTS_CONE)
    sc.set_glossy_sampling(_abi.RT_GLOSSY_MIS)
    with rt.Film(sc, rqs, integrator="nee", moments=True) as film:
        assert refused(film.resolve_regression)                                  # no samples yet
        assert film.regression_model is None
        film.render_pass(0, 1)
        planes = film.features(2)
        got = {n: host(film, t) for n, t in planes.items()}
        assert (got["hits"] == 0).any() and (got["hits"] > 0).any()
        # one sample
        acc1 = host(film, film.accum).copy()
        out = film.resolve_regression({n: planes[n] for n in ALL}, OUTPUTS)
        want = rnp.resolve(acc1, 1, k=2, albedo_eps=EPS, ridge=f32(film_mod.RIDGE), **np_kw(got, ALL))
        xp.same(host(film, film.regression_model), want["model"], "one sample, model")
        for o in OUTPUTS:
            xp.same(host(film, out[o]), want[o], ("one sample", o))
        film.render_pass(1, SPP)
        acc, mom = host(film, film.accum).copy(), host(film, film.moments).copy()
        state = lambda: (film.samples, bits(host(film, film.accum)), bits(host(film, film.moments)),
                         *(bits(host(film, planes[n])) for n in ALL))
        s5 = state()
        seen = set()
        for names in rnp.SUBSETS:
            out = film.resolve_regression({n: planes[n] for n in names}, OUTPUTS)
            want = rnp.resolve(acc, SPP, k=2, albedo_eps=EPS, ridge=f32(film_mod.RIDGE), **np_kw(got, names))
            assert tuple(film.regression_model.shape) == (3, 4, 32) and (want["model"][..., 27] == 1).any()
            xp.same(host(film, film.regression_model), want["model"], (names, "model"))
            for o in OUTPUTS:
                xp.same(host(film, out[o]), want[o], (names, o))
            seen.add(bits(want["linear"]))
        assert len(seen) == len(rnp.SUBSETS)                                    # every subset is a fit of its own
        # index is ignored, ridge and albedo_eps reach the kernels, one output alone is written
        out = film.resolve_regression(dict(planes, index=None), ("linear",), ridge=0.05, albedo_eps=0.125)
        want = rnp.resolve(acc, SPP, k=2, albedo_eps=f32(0.125), ridge=f32(0.05), **np_kw(got, ALL))
        assert list(out) == ["linear"]
        xp.same(host(film, out["linear"]), want["linear"], "constants")
        # a refused call changes no tensor
        full = {n: planes[n] for n in ALL}
        first = film.resolve_regression(full, OUTPUTS)
        kept = {o: bits(host(film, t)) for o, t in first.items()}
        kept_model = bits(host(film, film.regression_model))
        bad = [dict(outputs=()), dict(outputs=("variance",)), dict(outputs=("rgb", "rgb")), dict(planes={"depth": planes["depth"]}),
               dict(planes={"colour": planes["normal"]}), dict(ridge=0.0), dict(ridge=-1.0), dict(ridge=float("nan")),
               dict(ridge=float("inf")), dict(ridge=1e-60), dict(albedo_eps=0.0), dict(albedo_eps=float("nan")),
               dict(planes={"normal": planes["normal"][:4]}), dict(planes={"normal": planes["normal"].double()}),
               dict(planes={"normal": planes["normal"].cpu()}), dict(planes={"hits": planes["depth"]})]
        for kw in bad:
            assert refused(film.resolve_regression, **kw), kw
            assert state() == s5 and bits(host(film, film.regression_model)) == kept_model, kw
            assert {o: bits(host(film, t)) for o, t in first.items()} == kept, kw
        # a second call overwrites the first's tensors
        model = film.regression_model
        second = film.resolve_regression(None, OUTPUTS)
        assert all(second[o] is first[o] for o in OUTPUTS) and film.regression_model is model
        assert all(bits(host(film, first[o])) != kept[o] for o in OUTPUTS) and bits(host(film, model)) != kept_model
        assert state() == s5
        # _state: other sums of the film's shape in the place of the film's own
        other = (film.accum * 0.5 + 0.25).contiguous()
        film.sync()
        out = film.resolve_regression(full, ("linear",), _state=(other, None))
        want = rnp.resolve(host(film, other), SPP, k=2, albedo_eps=EPS, ridge=f32(film_mod.RIDGE), **np_kw(got, ALL))
        xp.same(host(film, out["linear"]), want["linear"], "_state")
        assert state() == s5
        # the film library's launches are not the scene's
        film.collect()
        film.resolve_regression(full)
        assert film.collect().n_launches == 0
        # reset() and the same passes reproduce the bytes
        film.reset()
        film.render_pass(0, 1)
        film.render_pass(1, SPP)
        assert state() == s5
        again = film.resolve_regression(full, OUTPUTS)
        assert {o: bits(host(film, t)) for o, t in again.items()} == kept and bits(host(film, film.regression_model)) == kept_model
    assert film.regression_model is None and refused(film.resolve_regression)    # closed
    # a film without moments loads the film library on first use, and has the same bytes
    with rt.Film(sc, rqs, integrator="nee") as plain:
        assert plain.moments is None and plain._film_lib is None
        plain.render_pass(0, SPP)
        pl = plain.features(2)
        out = plain.resolve_regression({n: pl[n] for n in ALL}, OUTPUTS)
        assert plain._film_lib is not None
        assert {o: bits(host(plain, t)) for o, t in out.items()} == kept and bits(host(plain, plain.regression_model)) == kept_model
        assert refused(plain.resolve_guided)                                     # (still no moments)
print("ok")
"""


def test_the_glossy_room(ndev, room):
    _child(_ROOM_CHILD, room)


# ------------------------------------------------------------------------------------------- 3. extreme planes

_EXTREME_CHILD = r"""
E, K = xp.E, xp.K
calls = nans = fallback = 0
with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
    for tier in xp.TIERS:
        R, W = xp.FILTER_SIZES[tier]
        rq = _abi.default_request(width=W, height=R, divisions=1, division_no=0, spp=E, max_bounces=2, seed=1)
        with rt.Film(sc, rq, integrator="path") as film:
            for name, names, s in rnp.extreme_cases(tier, EPS):
                planes = upload(film, s, E, K)
                for ridge in (film_mod.RIDGE, 1e-1):
                    want = check(film, planes, s, names, E, K, ridge, (tier, name))
                    calls += 1
                    nans += int(np.isnan(want["linear"]).sum()) + int(np.isnan(want["model"]).sum())
                    fallback += int(((want["model"][..., 27] == 0) & (want["model"][..., 26] > 0)).sum())
                # the inputs are read only
                xp.identical(host(film, film.accum), s["C"], (tier, name, "accum"))
                for n, k in rnp.KEYS.items():
                    xp.identical(host(film, planes[n]), s[k], (tier, name, n))
assert calls >= 30 and nans > 0 and fallback > 0, (calls, nans, fallback)
print(calls, "calls,", nans, "NaNs in the restatement,", fallback, "fallbacks")
print("ok")
"""


def test_the_regression_resolve_on_extreme_planes(ndev):
    print(_child(_EXTREME_CHILD))


# ------------------------------------------------------------------------------------------- 4. the example

_EXAMPLE_CHILD = r"""
import runpy
out_dir, example = sys.argv[1], sys.argv[2]
sys.argv = [example, out_dir, "--width", "64", "--height", "36", "--divisions", "2", "--spp", "4"]
runpy.run_path(example, run_name="__main__")
got = {n: np.load(f"{out_dir}/{n}.npy") for n in ("resolve", "resolve_guided", "resolve_regression")}
assert all(g.shape == (36, 64, 3) and g.dtype == np.uint8 for g in got.values())
assert len({g.tobytes() for g in got.values()}) == 3
sph, rq = scenes.config("c2")
rqs = [_abi.default_request(width=64, height=36, divisions=2, division_no=k, spp=4, max_bounces=rq.max_bounces, seed=rq.seed) for k in range(2)]
with rt.Scene(0, rt.World(sph)) as sc:
    sc.set_light_sampling(_abi.RT_LIGHTS_CONE)
    sc.set_glossy_sampling(_abi.RT_GLOSSY_MIS)
    with rt.Film(sc, rqs, integrator="nee", moments=True) as film:
        film.render_pass(0, 4)
        planes = film.features(1)
        out = film.resolve_regression({n: planes[n] for n in ("albedo", "normal", "depth", "hits")}, ("rgb",))
        xp.same(host(film, out["rgb"]), got["resolve_regression"], "resolve_regression.npy")
print("ok")
"""


def test_example_film_regress(ndev, tmp_path):
    _child(_EXAMPLE_CHILD, tmp_path, ROOT / "examples" / "film_regress.py")
