#!/usr/bin/env python3
"""The film upsampler (ray_tracer_s8_amd.FilmUpsampler) measured next to the full-resolution film, per config (default
c2 and c3), the config's own divisions, bounces and seed, a --width x --height frame reconstructed from films of 1 / s of it in both
directions for s in --scales (default 2 and 3: 1920 x 1080 from 960 x 540 and from 640 x 360):

  full        the full-resolution film over a ladder of sample counts: the time of a frame (the passes, one sample of the feature
              buffers and the resolve; host clock around a synchronised frame, the median of --runs) and the squared error,
              mean((x - ref)^2), of the `linear` output of resolve (the a-trous with albedo, normal, depth and hits) and of
              resolve_guided (normal, depth and hits) against accum / n of a --reference-spp film under another seed.
  upsampled   per scale and per traced samples m of the ladder, the low-resolution film at s^2 m samples a pixel, which is m traced
              samples per output pixel: the kernel's time (events around the one launch, median), the time of a whole frame (the
              low-resolution passes, both feature sets, the resolve and the upsampling), the share of class-1 pixels, and the error
              of the upsampled `linear` for the film's resolve and resolve_guided as the source, each with no planes (plain
              bilinear), with the planes but no albedo, and with the planes and the albedo.  Beside every error the full-resolution
              film's, through the same resolve, at equal traced samples (m) and at equal time (interpolated log-log along the
              ladder, clamped at its ends), and the ratios (below 1: the upsampled frame's error is the smaller).

    python tools/film_upsample_bench.py [--configs c2 c3] [--width 1920 --height 1080] [--scales 2 3] [--ladder 2 4 8 16] [--runs 3]
                                        [--aperture 0]
Prints one JSON line.  torch is imported first: the libraries then bind to torch's HIP runtime."""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import _abi, film_upsampler as fu, scenes  # noqa: E402

GUIDE = ("normal", "depth", "hits")
DENOISE = ("albedo", "normal", "depth", "hits")
VARIANTS = {"no_planes": dict(planes_lo={}, planes_hi={}), "planes": dict(albedo=False), "planes_albedo": dict(albedo=True)}


APERTURE = None                                   # --aperture: the lens of every frame of a run; None: default_request's (0.1)


def _requests(rq, width, height, spp, seed, divisions=None):
    d = divisions or rq.divisions
    kw = {} if APERTURE is None else {"aperture": APERTURE}
    return [_abi.default_request(width=width, height=height, divisions=d, division_no=k, spp=spp, max_bounces=rq.max_bounces, seed=seed,
                                 **kw) for k in range(d)]


def _mse(x, ref):
    return float(((x - ref) ** 2).mean())


def _timed_wall(film, work, runs):
    """The median host time, in ms, of work() followed by a synchronise of the film's stream (the first run is a warm-up)."""
    t = []
    for _ in range(runs + 1):
        film.sync()
        t0 = time.perf_counter()
        work()
        film.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t[1:])


def _timed_events(film, work, runs):
    """The median time, in ms, between events on the film's stream around work(), which enqueues one launch."""
    t = []
    for _ in range(runs + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(film.stream)
        work()
        b.record(film.stream)
        film.sync()
        t.append(a.elapsed_time(b))
    return statistics.median(t[2:])


def _interp(xs, ys, x):
    """y at x along the ladder, log-log, clamped at the ends."""
    if x <= xs[0]:
        return ys[0]
    for (x0, y0), (x1, y1) in zip(zip(xs, ys), zip(xs[1:], ys[1:])):
        if x <= x1:
            w = (math.log(x) - math.log(x0)) / (math.log(x1) - math.log(x0))
            return math.exp(math.log(y0) + w * (math.log(y1) - math.log(y0)))
    return ys[-1]


def _linear(film, source, planes):
    if source == "resolve":
        return film.resolve(planes={n: planes[n] for n in DENOISE}, outputs=("linear",))["linear"]
    return film.resolve_guided({n: planes[n] for n in GUIDE}, ("linear",))["linear"]


def full_ladder(sc, rq, a, ref):
    out = []
    with rt.Film(sc, _requests(rq, a.width, a.height, max(a.ladder), rq.seed), integrator="nee", moments=True) as film:
        for n in a.ladder:
            entry = {"samples": n}
            for source in ("resolve", "guided"):
                def frame(source=source, n=n):
                    film.reset()
                    film.render_pass(0, n)
                    return _linear(film, source, film.features(1))
                entry[source] = {"ms": _timed_wall(film, frame, a.runs)}
                x = frame()
                film.sync()
                entry[source]["mse"] = _mse(x, ref)
            out.append(entry)
    return out


def upsampled(sc, rq, a, ref, s, ladder):
    out = []
    wl, hl = a.width // s, a.height // s
    spp = s * s * max(a.ladder)
    d = max(k for k in range(1, rq.divisions + 1) if hl % k == 0)       # the config's divisions, or the most below that cover the film
    with rt.Film(sc, _requests(rq, wl, hl, spp, rq.seed, d), integrator="nee", moments=True) as film, \
            rt.FilmUpsampler(film, _requests(rq, a.width, a.height, spp, rq.seed, d)) as up:
        for m in a.ladder:
            entry = {"traced_samples": m, "film_samples": s * s * m, "divisions": d}
            for source in ("resolve", "guided"):
                def frame(source=source, m=m, **kw):
                    film.reset()
                    film.render_pass(0, s * s * m)
                    planes = film.features(1, fu.PLANES)
                    up.features(1)
                    return up.upsample(_linear(film, source, planes), outputs=("linear", "class"), **kw)
                e = entry[source] = {"frame_ms": _timed_wall(film, frame, a.runs)}
                for name, kw in VARIANTS.items():
                    got = frame(**kw)
                    film.sync()
                    e[name] = {"mse": _mse(got["linear"], ref), "class1": float(got["class"].float().mean())}
                    sq, one = ((got["linear"] - ref) ** 2).mean(dim=2), got["class"] == 1
                    e[name]["mse_class0"] = float(sq[~one].mean()) if bool((~one).any()) else None
                    e[name]["mse_class1"] = float(sq[one].mean()) if bool(one.any()) else None
                    linear = _linear(film, source, film.planes)
                    e[name]["kernel_ms"] = _timed_events(film, lambda: up.upsample(linear, outputs=("linear", "class"), **kw), a.runs)
                    at_samples = next(l[source]["mse"] for l in ladder if l["samples"] == m)
                    at_time = _interp([l[source]["ms"] for l in ladder], [l[source]["mse"] for l in ladder], e["frame_ms"])
                    e[name].update(full_at_equal_samples=at_samples, ratio_at_equal_samples=e[name]["mse"] / at_samples,
                                   full_at_equal_time=at_time, ratio_at_equal_time=e[name]["mse"] / at_time)
            out.append(entry)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scales", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--ladder", type=int, nargs="+", default=[2, 4, 8, 16], help="traced samples per output pixel, ascending, from 2")
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--aperture", type=float, default=None, help="the lens of every frame, the reference's too (default: 0.1; 0: a pinhole)")
    a = ap.parse_args()
    global APERTURE
    APERTURE = a.aperture
    if any(a.width % s or a.height % s or not fu.MIN_SCALE <= s <= fu.MAX_SCALE for s in a.scales) or min(a.ladder) < 2:
        ap.error("--scales divide the frame and lie in 2 ... 4; the ladder starts at 2 samples (resolve_guided needs a variance)")
    rt.init()
    result = {"tool": "film_upsample_bench", "width": a.width, "height": a.height, "scales": a.scales, "ladder": a.ladder,
              "reference_spp": a.reference_spp, "runs": a.runs, "k_depth": fu.K_DEPTH, "k_normal": fu.K_NORMAL, "aperture": a.aperture, "configs": {}}
    for name in a.configs:
        sph, rq = scenes.config(name)
        with rt.Scene(0, rt.World(sph)) as sc:
            sc.set_light_sampling(rt.RT_LIGHTS_CONE)
            sc.set_glossy_sampling(rt.RT_GLOSSY_MIS)
            with rt.Film(sc, _requests(rq, a.width, a.height, a.reference_spp, rq.seed + 1), integrator="nee") as ref_film:
                for _ in ref_film.render_progressive(32):
                    pass
                ref_film.sync()
                ref = (ref_film.accum / float(a.reference_spp)).clone()
            ladder = full_ladder(sc, rq, a, ref)
            result["configs"][name] = {"divisions": rq.divisions, "full": ladder,
                                       "upsampled": {str(s): upsampled(sc, rq, a, ref, s, ladder) for s in a.scales}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
