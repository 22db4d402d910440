"""The film-stage kernels on extreme planes: the corpus of tests/_extreme_planes.py, the very cases
tests/test_extreme_planes_host.py holds to its input conditions on the CPU, through the device kernels of the four libraries, against
the numpy restatements.  The rule is the CPU test's: a float is NaN in one exactly where it is NaN in the other, every other float is
bit-equal (signed zeros and infinities too), uint8 and integer planes are equal; a NaN's payload and sign are not compared.
1. the denoiser (rt_scene_denoise): 70 x 9 salted with small values, 70 x 22 with sparse huge and non-finite ones; no planes, the
   albedo alone, all planes; 0, 1 and 3 iterations; the product library as it plans, and the test library with every step loading
   directly (RT_DENOISE_LDS_STEP 0) and with every step staged in LDS (4); as one strip and as three strips of a call (no three
   equal strips make 22 rows: the three-strip call is the image's first 21 rows, restated as such);
2. the guided resolve (Film.resolve_guided on uploaded accum, moments and planes): the same two sizes, the six plane subsets, 0, 1
   and 3 iterations, every step loading directly and the plan's choice of LDS windows, all four outputs;
3. the history (FilmHistory.accumulate on uploaded frames): 70 x 9 in three strips, a still camera and the half-a-pixel step, three
   frames each, so that the extreme values come back as previous state, with and without normals; the whole state is compared;
4. its clip: the same sequences, both radii, both forms of the kernel (the window staged in LDS, and read directly), gamma 0.5 and
   3; the state and the clip amount;
5. the upsampler (rtu_upsample): a low film of 33 x 7, strip 2 of 3, at s = 2 and 3; every plane, none, and depth with hits; all
   four outputs, and an output not asked for keeps its sentinel.
In every child the inputs are read back after the calls and hold the bytes that were uploaded, NaN payloads included.  On a
mismatch the child names the first differing pixel, both values with their bits, and the inputs of that pixel's footprint.  Every
body runs in a child process that imports torch first.  No address of any of these kernels depends on a plane's value but the
history's reprojected tap position, which is tested against the film's bounds before it is converted to an integer (DESIGN.md 4.28
has the reading).  No timing is asserted."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

_PRELUDE = r"""
import sys
import numpy as np
import torch                                                      # first: the libraries then bind to torch's HIP runtime
sys.path.insert(0, "tests")
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes
import _extreme_planes as xp

f32 = np.float32
np.seterr(all="ignore")

def host(film, t):
    film.sync()                                                   # (.cpu() copies on torch's current stream, not the film's)
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a

def up(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)

def around(planes, y, x, r=1):
    # the values of every plane in the (2 r + 1)^2 pixels around (y, x): what a mismatch is printed with
    return {n: a[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].tolist() for n, a in planes.items() if a is not None}
"""


def _child(body, *args, timeout=600):
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body, *map(str, args)], capture_output=True, text=True, cwd=ROOT,
                       timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), f"child exit {r.returncode}\n" + r.stdout[-6000:] + r.stderr[-6000:]
    return r.stdout


# ------------------------------------------------------------------------------------------- 1. the denoiser

_DENOISE_CHILD = r"""
import _denoise_np as dn

OUTS = ("rgb", "linear", "f32")
NAMES = dict(A="albedo", N="normal", D="depth", hits="hits")

def frame(W, R, n):
    return [_abi.default_request(width=W, height=R, divisions=n, division_no=i, spp=16, seed=3) for i in range(n)]

wants = {}

def wanted(key, planes, names, rows, it, consts):
    if key not in wants:
        kc, kn, kd = consts
        wants[key] = dn.denoise(planes["C"][:rows], xp.E, k=xp.K, iterations=it, k_color=f32(kc), k_normal=f32(kn), k_depth=f32(kd),
                                **{k: (planes[k][:rows] if k in names else None) for k in NAMES})
    return wants[key]

def run_all(sc, label):
    calls = 0
    for tier in xp.TIERS:
        for c, (name, names, planes) in enumerate(xp.denoise_cases(tier)):
            keep = {k: v.copy() for k, v in planes.items()}
            R, W = planes["C"].shape[:2]
            for consts in xp.denoise_consts(tier):
                for it in xp.SPARSE_ITERATIONS:
                    dq = _abi.DenoiseRequest.defaults(iterations=it, k_color=consts[0], k_normal=consts[1], k_depth=consts[2])
                    for n, rows in ((1, R), (3, R - R % 3)):
                        want = wanted((tier, c, consts, it, rows), planes, names, rows, it, consts)
                        cut = lambda a: np.split(np.ascontiguousarray(a[:rows]), n, 0)
                        got, _ = sc.denoise(frame(W, rows, n), cut(planes["C"]),
                                            [{NAMES[k]: cut(planes[k])[i] for k in names} for i in range(n)], xp.E, xp.K, dq, outputs=OUTS)
                        for o in OUTS:
                            xp.same(np.concatenate([g[o] for g in got], 0), want[o], (label, tier, name, names, consts, it, n, o),
                                    lambda p: around({k: planes[k] for k in ("C",) + tuple(names)}, p[0], p[1], 2))
                        calls += 1
            for k in planes:
                xp.identical(planes[k], keep[k], (tier, name, k))
    return calls

rt.init()
with rt.Scene(0, rt.World(scenes.single_sphere())) as sc:
    calls = run_all(sc, "the product library")
with _abi.debug_library():
    rt.init()
    with rt.Scene(0, rt.World(scenes.single_sphere())) as sc:
        for step in (0, 4):                                       # every step through L2; steps 1, 2 and 4 staged in LDS
            prev = _abi.debug_set("RT_DENOISE_LDS_STEP", step)
            try:
                calls += run_all(sc, f"the test library, RT_DENOISE_LDS_STEP {step}")
            finally:
                _abi.debug_set("RT_DENOISE_LDS_STEP", prev)
assert calls % 3 == 0 and calls >= 3 * 100 and len(wants) >= 100, (calls, len(wants))
print(calls, "calls")
print("ok")
"""


def test_the_denoiser_on_extreme_planes(ndev):
    print(_child(_DENOISE_CHILD))


# ------------------------------------------------------------------------------------------- 2. the guided resolve

_GUIDED_CHILD = r"""
from ray_tracer_s8_amd import _film_lib
import _film_np as fnp

OUTPUTS = ("rgb", "linear", "f32", "variance")

def np_planes(planes, normal, depth):
    return dict(N=planes["N"] if normal else None, D=planes["D"] if depth == "depth" else None, hits=planes["hits"] if depth else None)

calls = 0
with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
    for tier in xp.TIERS:
        R, W = xp.FILTER_SIZES[tier]
        rq = _abi.default_request(width=W, height=R, divisions=1, division_no=0, spp=xp.E, max_bounces=2, seed=1)
        with rt.Film(sc, rq, integrator="path", moments=True) as film:
            dev = film.device
            film.samples, film.aov_samples = xp.E, xp.K
            for name, (normal, depth), planes in xp.film_cases(tier):
                with torch.cuda.stream(film.stream):
                    film.accum.copy_(up(planes["C"], dev))
                    film.moments.copy_(up(planes["M"], dev))
                    d = dict(normal=up(planes["N"], dev), depth=up(planes["D"], dev), hits=up(planes["hits"], dev))
                names = (["normal"] if normal else []) + {"": [], "hits": ["hits"], "depth": ["depth", "hits"]}[depth]
                guide = {n: d[n] for n in names}
                for sl, ve, kn, kd in xp.film_consts(tier):
                    for it in xp.SPARSE_ITERATIONS:
                        want = fnp.resolve(planes["C"], planes["M"], xp.E, iterations=it, sigma_l=f32(sl), var_eps=f32(ve), k_normal=f32(kn),
                                           k_depth=f32(kd), **np_planes(planes, normal, depth))
                        for lds in (0, _film_lib.LDS_PLAN):
                            out = film.resolve_guided(guide, OUTPUTS, iterations=it, sigma_l=sl, var_eps=ve, k_normal=kn, k_depth=kd,
                                                      _lds_max_step=lds)
                            for o in OUTPUTS:
                                xp.same(host(film, out[o]), want[o], (tier, name, normal, depth, sl, it, lds, o),
                                        lambda p: around(dict(C=planes["C"], M=planes["M"], **{k: v for k, v in
                                                         np_planes(planes, normal, depth).items()}), p[0], p[1], 2))
                            calls += 1
                # the inputs are read only
                xp.identical(host(film, film.accum), planes["C"], (tier, name, "accum"))
                xp.identical(host(film, film.moments), planes["M"], (tier, name, "moments"))
                for n, k in (("normal", "N"), ("depth", "D"), ("hits", "hits")):
                    xp.identical(host(film, d[n]), planes[k], (tier, name, n))
assert calls >= 300, calls
print(calls, "calls")
print("ok")
"""


def test_the_guided_resolve_on_extreme_planes(ndev):
    print(_child(_GUIDED_CHILD))


# ------------------------------------------------------------------------------------------- 3, 4. the history and its clip

_HISTORY_PRELUDE = r"""
from ray_tracer_s8_amd import _history_lib
import _history_clip_np as cnp
import _history_np as hnp

W, H, DIV = xp.HISTORY_FILM
E = xp.HISTORY_SAMPLES
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=E, max_bounces=2, seed=1) for k in range(DIV)]
INPUTS = ("depth", "hits", "index", "normal")

def upload(film, fr):
    dev = film.device
    with torch.cuda.stream(film.stream):
        film.accum.copy_(up(fr["C"], dev))
        film.moments.copy_(up(fr["M"], dev))
        return {n: up(fr[n], dev) for n in INPUTS}

def check_inputs(film, planes, fr, what):
    xp.identical(host(film, film.accum), fr["C"], (what, "accum"))
    xp.identical(host(film, film.moments), fr["M"], (what, "moments"))
    for n in INPUTS:
        xp.identical(host(film, planes[n]), fr[n], (what, n))

def check_state(film, history, want, fr, what):
    got = history._sets[history._cur]
    for n in hnp.STATE:
        if want[n] is not None:
            xp.same(host(film, got[n]), want[n], (what, n),
                    lambda p: dict(frame=around({k: fr[k] for k in ("C", "M") + INPUTS}, p[0], p[1], 0), want=around(want, p[0], p[1], 0)))

def camera_of(pose):
    return None if pose is None else rt.Camera.look_at(*pose)
"""

_HISTORY_CHILD = _HISTORY_PRELUDE + r"""
frames_run = blended = 0
with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
    with rt.Film(sc, rqs, integrator="path", moments=True) as film:
        film.samples = E
        for tier in xp.TIERS:
            for name, path, consts, frames in xp.history_cases(tier, rqs[0]):
                with rt.FilmHistory(film, *consts) as history:
                    prev, last = None, None
                    for i, (pose, fr) in enumerate(frames):
                        planes = upload(film, fr)
                        history.accumulate(camera_of(pose), planes)
                        cam = hnp.cameras(rqs[0], pose, rqs[0] if i else None, last)
                        prev = hnp.accumulate(cam, fr, prev, *consts)
                        check_state(film, history, prev, fr, (tier, name, path, consts, i))
                        check_inputs(film, planes, fr, (tier, name, path, i))
                        last = pose
                        frames_run += 1
                        blended += int((prev["length"] > 1).sum())
assert frames_run >= 100 and blended > 1000, (frames_run, blended)
print(frames_run, "frames,", blended, "pixels blended")
print("ok")
"""


def test_the_history_on_extreme_planes(ndev):
    print(_child(_HISTORY_CHILD))


_CLIP_CHILD = _HISTORY_PRELUDE + r"""
FORMS = (_history_lib.CLIP_FORM_STAGED, _history_lib.CLIP_FORM_DIRECT)
frames_run = touched = 0
with rt.Scene(0, rt.World(scenes.cornell16())) as sc:
    with rt.Film(sc, rqs, integrator="path", moments=True) as film:
        film.samples = E
        for tier in xp.TIERS:
            for name, path, consts, frames in xp.history_cases(tier, rqs[0]):
                for radius in (1, 2):
                    for gamma in (0.5, 3.0):
                        want, prev, last = [], None, None
                        for i, (pose, fr) in enumerate(frames):
                            cam = hnp.cameras(rqs[0], pose, rqs[0] if i else None, last)
                            prev = cnp.accumulate(cam, fr, prev, *consts, clip=gamma, clip_radius=radius, samples=E)
                            want.append(prev)
                            last = pose
                            touched += int((prev["clip"] != 0).sum())
                        for form in FORMS:
                            with rt.FilmHistory(film, *consts, clip=gamma, clip_radius=radius) as history:
                                history._clip_form = form
                                for i, (pose, fr) in enumerate(frames):
                                    planes = upload(film, fr)
                                    history.accumulate(camera_of(pose), planes)
                                    what = (tier, name, path, consts, radius, gamma, form, i)
                                    check_state(film, history, want[i], fr, what)
                                    xp.same(host(film, history.clip_amount), want[i]["clip"], (what, "clip"),
                                            lambda p: around(dict(C=fr["C"]), p[0], p[1], radius))
                                    check_inputs(film, planes, fr, what)
                                    frames_run += 1
assert frames_run >= 800 and touched > 1000, (frames_run, touched)
print(frames_run, "frames,", touched, "clip amounts that are not zero")
print("ok")
"""


def test_the_historys_clip_on_extreme_planes(ndev):
    print(_child(_CLIP_CHILD))


# ------------------------------------------------------------------------------------------- 5. the upsampler

_UPSAMPLE_CHILD = r"""
from ray_tracer_s8_amd import _upsample_lib as ul
import _upsample_np as unp

lib = ul.load()
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
SENTINEL = 0x5A
OUTS = ("linear", "f32", "rgb", "class")
NP_OUT = dict(linear="linear", f32="f32", rgb="rgb", cls="class")
WL, RL, ABOVE, BELOW = xp.UPSAMPLE_LOW

calls = 0
for tier in xp.TIERS:
    for s in xp.UPSAMPLE_SCALES:
        for name, L, lo, hi, geom, kl, kh in xp.upsample_cases(tier, s):
            Rh, Wh = geom["Rh"], geom["Wh"]
            assert geom["y0l"] > 0 and geom["y0h"] == s * geom["y0l"]
            with torch.cuda.stream(stream):
                d_L, d_lo, d_hi = up(L, dev), {n: up(a, dev) for n, a in lo.items()}, {n: up(a, dev) for n, a in hi.items()}
            for i, names in enumerate(xp.UPSAMPLE_SETS):
                if name not in names + ("every plane", "colour"):
                    continue                                       # (the case's special plane is not among the call's)
                want = unp.upsample(L, unp.take(lo, names), unp.take(hi, names), geom, unp.K_DEPTH, unp.K_NORMAL, unp.EPS, kl, kh)
                for asked in (OUTS, (OUTS[(i + calls) % 4],)):
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
                            xp.same(got, want[key], (tier, s, name, names, asked, o),
                                    lambda p: dict(hi=around({n: hi[n] for n in names}, p[0], p[1], 0),
                                                   lo=around(dict(L=L, **{n: lo[n] for n in names}), p[0] // s, p[1] // s, 1)))
                        elif got.dtype == np.uint8:
                            assert (got == SENTINEL).all(), (tier, s, name, names, asked, o, "the sentinel")
                        else:
                            assert (got == 7.0).all(), (tier, s, name, names, asked, o, "the sentinel")
            # the inputs are read only
            xp.identical(d_L.cpu().numpy(), L, (tier, s, name, "linear"))
            for n in unp.PLANES:
                xp.identical(d_lo[n].cpu().numpy().view(lo[n].dtype), lo[n], (tier, s, name, "lo", n))
                xp.identical(d_hi[n].cpu().numpy().view(hi[n].dtype), hi[n], (tier, s, name, "hi", n))
assert calls >= 80, calls
print(calls, "calls")
print("ok")
"""


def test_the_upsampler_on_extreme_planes(ndev):
    print(_child(_UPSAMPLE_CHILD))
