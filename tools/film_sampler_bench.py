#!/usr/bin/env python3
"""The film sampler (ray_tracer_s8_amd.FilmSampler) measured next to the uniform film, per config (default c2 and c3),
the config's own divisions, bounces and seed, at --width x --height, a floor of --floor samples and rounds of --round sample indices up
to --spp a pixel:

  round_ms    the first round after the floor at --threshold, phase by phase: select (with the round's one host wait), and summed over
              the strips the whole-strip ray generation, the gather, the trace of the compact batch and the fold; beside it a uniform
              Film.render_pass of the same sample indices.  Events on the film's stream around each phase (a phase is enqueued alone, so
              the sum of the phases is the round without overlap between them), --runs after --warmup warm-ups, the median.
  quality     against accum / n of a --reference-spp uniform film under another seed: the squared error, mean((x - ref)^2) and
              mean((x - ref)^2 / (ref^2 + 0.01)), of the `linear` output of preview and of resolve_guided (5 iterations, normal, depth
              and hits), for uniform films over a ladder of sample counts and for the sampler over the threshold grid, each with its
              traced samples per pixel and its time (host clock around a synchronised render, the median of --runs; for the
              uniform film in one pass, and where the count allows also as the floor and passes of --round, which is how the sampler
              renders).  For every sampler point the uniform film's error at the same traced samples and at the same time,
              interpolated log-log along the ladder, and the ratios (below 1: the sampler's error is the smaller).

    python tools/film_sampler_bench.py [--configs c2 c3] [--width 1920 --height 1080] [--floor 4 --round 4 --spp 32] [--runs 3]
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
from ray_tracer_s8_amd import _abi, _sampler_lib, scenes  # noqa: E402
from ray_tracer_s8_amd import film_sampler as fs  # noqa: E402
from ray_tracer_s8_amd.film import sample_chunks  # noqa: E402

THRESHOLD_GRID = (0.05, 0.1, 0.2, 0.4, 0.8)
LADDER = (4, 6, 8, 12, 16, 24, 32)
GUIDE = ("normal", "depth", "hits")
PHASES = ("select", "rays", "gather", "trace", "fold")


def _requests(rq, width, height, spp, seed):
    return [_abi.default_request(width=width, height=height, divisions=rq.divisions, division_no=k, spp=spp,
                                 max_bounces=rq.max_bounces, seed=seed) for k in range(rq.divisions)]


def _film(sc, rq, a, spp, seed):
    return rt.Film(sc, _requests(rq, a.width, a.height, spp, seed), integrator="nee", moments=True)


class _Clock:
    """Event pairs on one stream, summed per name after a synchronise."""

    def __init__(self, stream):
        self.stream, self.pairs = stream, []

    def __call__(self, name, work):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        out = work()
        b.record(self.stream)
        self.pairs.append((name, a, b))
        return out

    def totals(self):
        self.stream.synchronize()
        out = {}
        for name, a, b in self.pairs:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        return out


def _round_by_phase(sampler, n):
    """FilmSampler.render_pass(n) with an event pair around every phase: the same calls in the same order."""
    film = sampler.film
    lib, handle = sampler._lib, film.stream.cuda_stream
    clock = _Clock(film.stream)
    begin, end = sampler.samples, min(sampler.samples + n, film.spp)
    pixels = film.hs * film.width
    with torch.cuda.stream(film.stream):
        counts = clock("select", sampler._select)
        for i, rq in enumerate(film.reqs):
            na = counts[i]
            if na == 0:
                continue
            active = sampler.active[i * pixels:].data_ptr()
            acc, mom, cnt = (film._strip(t, i).data_ptr() for t in (sampler.accum, sampler.moments, sampler.counts))
            for b, e in sample_chunks(pixels, begin, end, film.max_records):
                k = e - b
                film._reserve(2)
                clock("rays", lambda: film.scene.camera_rays_device(rq, b, e, film._rays.data_ptr(), film._states.data_ptr(), stream=handle))
                g = _sampler_lib.GatherArgs(n_active=na, k=k, pixels=pixels, active=active, rays=film._rays.data_ptr(),
                                            states=film._states.data_ptr(), out_rays=sampler._rays.data_ptr(),
                                            out_states=sampler._states.data_ptr())
                clock("gather", lambda: _sampler_lib.check("rts_gather", lib.rts_gather(g, handle)))
                clock("trace", lambda: film._trace(na * k, rq.max_bounces, handle, sampler._rays, sampler._states))
                f = _sampler_lib.FoldArgs(n_active=na, k=k, pixels=pixels, active=active, rgb=film._rgb.data_ptr(), accum=acc,
                                          moments=mom, counts=cnt)
                clock("fold", lambda: _sampler_lib.check("rts_fold", lib.rts_fold(f, handle)))
    t = clock.totals()
    sampler.samples = end
    return {p: t.get(p, 0.0) for p in PHASES}, sum(counts)


def round_times(sc, rq, a):
    with _film(sc, rq, a, a.spp, rq.seed) as film, _film(sc, rq, a, a.spp, rq.seed) as uni, \
            rt.FilmSampler(film, threshold=a.threshold) as sampler:
        film.render_pass(0, a.floor)
        runs, uniform, whole, active = [], [], [], 0
        for r in range(a.warmup + a.runs):
            sampler.begin()
            t, active = _round_by_phase(sampler, a.round)
            sampler.begin()
            film.sync()
            t0 = time.perf_counter()
            sampler.render_pass(a.round)
            film.sync()
            w = (time.perf_counter() - t0) * 1e3
            uni.reset()
            uni.render_pass(0, a.floor)
            clock = _Clock(uni.stream)
            with torch.cuda.stream(uni.stream):
                clock("uniform", lambda: uni.render_pass(a.floor, min(a.floor + a.round, a.spp)))
            u = clock.totals()["uniform"]
            if r >= a.warmup:
                runs.append(t)
                uniform.append(u)
                whole.append(w)
        out = {p: statistics.median(t[p] for t in runs) for p in PHASES}
        out["phases_sum"] = statistics.median(sum(t.values()) for t in runs)
        out["render_pass_wall"] = statistics.median(whole)
        out["uniform_render_pass"] = statistics.median(uniform)
        out["active_fraction"] = active / float(film.rows * film.width)
        out["threshold"] = a.threshold
        return out


def _errors(x, ref):
    d = (x - ref) ** 2
    return {"mse": float(d.mean()), "rel_mse": float((d / (ref * ref + 0.01)).mean())}


def _timed_wall(film, work, runs):
    """The median host time, in ms, of work() followed by a synchronise of the film's stream; work() starts from its own reset."""
    t = []
    for _ in range(runs + 1):                                  # the first is a warm-up
        film.sync()
        t0 = time.perf_counter()
        work()
        film.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t[1:])


def _interp(xs, ys, x):
    """y at x along the ladder, log-log, clamped at the ends."""
    if x <= xs[0]:
        return ys[0]
    for (x0, y0), (x1, y1) in zip(zip(xs, ys), zip(xs[1:], ys[1:])):
        if x <= x1:
            w = (math.log(x) - math.log(x0)) / (math.log(x1) - math.log(x0))
            return math.exp(math.log(y0) + w * (math.log(y1) - math.log(y0)))
    return ys[-1]


def quality(sc, rq, a):
    with _film(sc, rq, a, a.reference_spp, rq.seed + 1) as ref_film:
        for _ in ref_film.render_progressive(32):
            pass
        ref_film.sync()
        ref = (ref_film.accum / float(a.reference_spp)).clone()
    with _film(sc, rq, a, a.spp, rq.seed) as film:
        planes = film.features(1)
        guide = {n: planes[n] for n in GUIDE}

        def outputs(owner):
            prev = owner.preview(("linear",))["linear"]
            guided = owner.resolve_guided(guide, ("linear",))["linear"]
            film.sync()                                        # the errors are computed on torch's current stream
            return {"preview": _errors(prev, ref), "resolve_guided": _errors(guided, ref)}

        ladder = []
        for n in [s for s in LADDER if s <= a.spp]:
            def work(n=n):
                film.reset()
                film.render_pass(0, n)

            def in_rounds(n=n):
                film.reset()
                film.render_pass(0, min(a.floor, n))
                while film.samples < n:
                    film.render_pass(film.samples, min(film.samples + a.round, n))
            ms_rounds = _timed_wall(film, in_rounds, a.runs) if (n - a.floor) % a.round == 0 else None
            ms = _timed_wall(film, work, a.runs)
            ladder.append(dict(samples=float(n), ms=ms, ms_in_rounds=ms_rounds, **outputs(film)))
        points = []
        for eps in a.eps_grid:
            for thr in THRESHOLD_GRID:
                with rt.FilmSampler(film, threshold=thr, eps=eps) as sampler:
                    def work():
                        film.reset()
                        film.render_pass(0, a.floor)
                        sampler.begin()
                        sampler.render(a.round)
                    ms = _timed_wall(film, work, a.runs)
                    samples = float(sampler.counts.sum().item()) / (film.rows * film.width)
                    p = dict(threshold=thr, eps=eps, samples=samples, ms=ms, rounds=sampler.rounds, **outputs(sampler))
                    for out in ("preview", "resolve_guided"):
                        for key, axis in (("uniform_at_equal_samples", "samples"), ("uniform_at_equal_time", "ms")):
                            u = _interp([l[axis] for l in ladder], [l[out]["mse"] for l in ladder], p[axis])
                            p[out][key] = u
                            p[out][key.replace("uniform_at", "ratio_at")] = p[out]["mse"] / u
                        stepped = [l for l in ladder if l["ms_in_rounds"] is not None]
                        u = _interp([l["ms_in_rounds"] for l in stepped], [l[out]["mse"] for l in stepped], ms)
                        p[out]["ratio_at_equal_time_in_rounds"] = p[out]["mse"] / u
                    points.append(p)
        return {"uniform": ladder, "adaptive": points}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--floor", type=int, default=4)
    ap.add_argument("--round", type=int, default=4)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=fs.THRESHOLD)
    ap.add_argument("--eps-grid", type=float, nargs="+", default=[fs.EPS])
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-quality", action="store_true")
    a = ap.parse_args()
    rt.init()
    result = {"tool": "film_sampler_bench", "width": a.width, "height": a.height, "floor": a.floor, "round": a.round, "spp": a.spp,
              "reference_spp": a.reference_spp, "runs": a.runs, "configs": {}}
    for name in a.configs:
        sph, rq = scenes.config(name)
        with rt.Scene(0, rt.World(sph)) as sc:
            sc.set_light_sampling(rt.RT_LIGHTS_CONE)
            sc.set_glossy_sampling(rt.RT_GLOSSY_MIS)
            entry = {"divisions": rq.divisions, "round_ms": round_times(sc, rq, a)}
            if not a.skip_quality:
                entry["quality"] = quality(sc, rq, a)
            result["configs"][name] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
