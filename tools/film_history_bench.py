#!/usr/bin/env python3
"""The film history (ray_tracer_s8_amd.FilmHistory) measured next to the frame it follows, per config (default c2 and
c3), the config's own divisions, bounces and seed, along the orbit of examples/film_temporal.py with a seed per frame:

  frame_ms    at --width x --height and --spp samples: one pass of all strips, the feature buffers (one sample), accumulate() without
              and with normals, and resolve_guided on the history at 5 iterations.  Events on the film's stream, --runs after
              --warmup warm-ups, the calls alternating within every run, --calls accumulate / resolve calls per timed window.
              median, best and worst;
  quality     at --quality-width x --quality-height (480 x 280, which every config's divisions divide): --frames poses of the orbit; per pose the squared error against accum / n of a
              --reference-spp film at that pose (its own seed), mean((x - ref)^2) and mean((x - ref)^2 / (ref^2 + 0.01)), averaged over
              the poses after the first, and that of the last pose alone: of the single frame's mean and of the history's mean for
              alpha x n_max; of the `linear` output of resolve_guided on the single frame and on the history for sigma_l x alpha x
              n_max; and of the history's mean over a small grid of k_depth x k_normal.  The share of pixels with history and their
              mean length at the last pose go with each history.

  --clip      the clip of the history to the frame's colour box beside all that, from the same run: in frame_ms,
              accumulate() with the clip at gamma = 1 and a radius of 1 and of 2, in both forms of the kernel (the window staged in
              LDS, and `_direct`), alternating with the calls without it, and whether the two forms' bytes are equal; in quality,
              the history's mean and resolve_guided for gamma x radius x alpha at n_max = 32 (CLIP_GAMMAS, CLIP_RADII, CLIP_ALPHAS),
              and the share of the pixels with history that the last pose's clip moved.

    python tools/film_history_bench.py [--configs c2 c3] [--width 1920 --height 1080 --spp 8] [--runs 7 --warmup 2] [--aperture 0]
                                       [--clip]
Prints one JSON line.  torch is imported first: the libraries then bind to torch's HIP runtime."""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import _abi, _history_lib, scenes  # noqa: E402
from ray_tracer_s8_amd import film_history as fh  # noqa: E402

ALPHA_GRID = (0.05, 0.1, 0.2, 0.5)
N_MAX_GRID = (8, 32)
SIGMA_GRID = (4.0, 8.0, 16.0)
GATE_GRID = ((0.02, None), (0.1, None), (0.5, None), (0.02, 0.9), (0.1, 0.9), (0.5, 0.9), (0.1, 0.99))     # (k_depth, k_normal)
CLIP_GAMMAS = (0.5, 1.0, 1.5, 2.0, 3.0)
CLIP_RADII = (1, 2)
CLIP_ALPHAS = (0.05, 0.2, 0.5)
CLIP_N_MAX = 32
PLANES = ("normal", "depth", "hits", "index")
GUIDE = ("normal", "depth", "hits")


def orbit_camera(i, n):
    a = 2.0 * math.pi * i / max(n, 1)
    return rt.Camera.look_at((1.2 * math.sin(a), 0.3 + 0.4 * math.cos(a), 0.2), (0.0, -0.8, -4.0))


def _spread(t):
    return {"median": statistics.median(t), "best": min(t), "worst": max(t), "runs": len(t)}


def _timed(stream, work):
    """Milliseconds between two events on `stream` around what work() enqueues there."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    work()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


LENS = {}                                    # --aperture: the request's aperture in the place of the reference's 0.1


def _requests(rq, width, height, spp, seed):
    return [_abi.default_request(width=width, height=height, divisions=rq.divisions, division_no=k, spp=spp,
                                 max_bounces=rq.max_bounces, seed=seed, **LENS) for k in range(rq.divisions)]


def _frame(sc, film, rq, i, a):
    camera = orbit_camera(i, a.orbit)
    sc.set_camera(camera)
    film.reset(seed=rq.seed + i)
    film.render_pass(0, a.spp)
    return camera, film.features(1, PLANES)


def frame_times(sc, rq, a, variants=None):
    """variants: {name: FilmHistory-like factory(film)} timed next to the two of the product (tools of an experiment add theirs)."""
    with rt.Film(sc, _requests(rq, a.width, a.height, a.spp, rq.seed), integrator="nee", moments=True) as film:
        make = {"accumulate": lambda f: rt.FilmHistory(f), "accumulate_normals": lambda f: rt.FilmHistory(f, k_normal=0.9)}
        if a.clip:
            def clipped(radius, form):
                def make_one(f):
                    h = rt.FilmHistory(f, clip=1.0, clip_radius=radius)
                    h._clip_form = form
                    return h
                return make_one
            for r in CLIP_RADII:
                make[f"accumulate_clip_radius_{r}"] = clipped(r, _history_lib.CLIP_FORM_STAGED)
                make[f"accumulate_clip_radius_{r}_direct"] = clipped(r, _history_lib.CLIP_FORM_DIRECT)
        make.update(variants or {})
        hist = {k: m(film) for k, m in make.items()}
        t = {k: [] for k in ("pass", "features", "resolve_guided", *hist)}
        for run in range(a.warmup + a.runs):
            camera = orbit_camera(run, a.orbit)
            sc.set_camera(camera)
            film.reset(seed=rq.seed + run)
            got = {"pass": _timed(film.stream, lambda: film.render_pass(0, a.spp))}
            planes = {}
            got["features"] = _timed(film.stream, lambda: planes.update(film.features(1, PLANES)))
            for k, h in hist.items():
                got[k] = _timed(film.stream, lambda: [h.accumulate(camera, planes) for _ in range(a.calls)]) / a.calls
            guide = {n: planes[n] for n in GUIDE}
            h = hist["accumulate"]
            got["resolve_guided"] = _timed(film.stream, lambda: [h.resolve_guided(guide, ("linear",)) for _ in range(a.calls)]) / a.calls
            film.collect()
            if run >= a.warmup:
                for k, ms in got.items():
                    t[k].append(ms)
        film.sync()
        twin = lambda k: hist["accumulate_normals" if k.endswith("_normals") else "accumulate"]
        equal = {k: bool(torch.equal(h.accum.view(torch.int32), twin(k).accum.view(torch.int32)))
                 for k, h in hist.items() if k in (variants or {})}
        equal.update({k: bool(torch.equal(h.accum.view(torch.int32), hist[k[:-len("_direct")]].accum.view(torch.int32)))
                      for k, h in hist.items() if k.endswith("_direct")})
        for h in hist.values():
            h.close()
    out = {"width": a.width, "height": a.height, "spp": a.spp, "calls_per_window": a.calls, "ms": {k: _spread(v) for k, v in t.items()}}
    if equal:
        out["equal_to_accumulate"] = equal
    return out


def _errors(x, ref):
    d = x.to(torch.float64) - ref
    return {"mse": float((d * d).mean().item()), "rel_mse": float((d * d / (ref * ref + 0.01)).mean().item())}


class _Mean:
    """The errors of one row over the poses: their mean after the first pose, and the last pose's."""

    def __init__(self):
        self.rows = []

    def add(self, e):
        self.rows.append(e)

    def result(self):
        rest = self.rows[1:] or self.rows
        return {"mean": {k: sum(r[k] for r in rest) / len(rest) for k in rest[0]}, "last": self.rows[-1]}


def quality(sc, rq, a):
    W, H = a.quality_width, a.quality_height
    rows = {}

    def row(name):
        return rows.setdefault(name, _Mean())

    with rt.Film(sc, _requests(rq, W, H, a.spp, rq.seed), integrator="nee", moments=True) as film, \
            rt.Film(sc, _requests(rq, W, H, a.reference_spp, rq.seed ^ 0x5EED), integrator="nee") as big:
        grid = {(al, nm): rt.FilmHistory(film, alpha=al, n_max=nm) for al in ALPHA_GRID for nm in N_MAX_GRID}
        gates = {g: rt.FilmHistory(film, k_depth=g[0], k_normal=g[1]) for g in GATE_GRID}
        clips = {(g, r, al): rt.FilmHistory(film, alpha=al, n_max=CLIP_N_MAX, clip=g, clip_radius=r)
                 for g in CLIP_GAMMAS for r in CLIP_RADII for al in CLIP_ALPHAS} if a.clip else {}
        stats = {}
        for i in range(a.frames):
            camera, planes = _frame(sc, film, rq, i, a)
            guide = {n: planes[n] for n in GUIDE}
            big.reset()
            big.render_pass(0, a.reference_spp)
            big.sync()
            big.collect()
            ref = big.accum.to(torch.float64) / a.reference_spp

            def err(t, scale=1.0):
                film.sync()
                return _errors(t.to(torch.float64) / scale, ref)

            row("single mean").add(err(film.accum, a.spp))
            for s in SIGMA_GRID:
                row(f"single resolve_guided sigma_l={s:g}").add(err(film.resolve_guided(guide, ("linear",), sigma_l=s)["linear"]))
            for (al, nm), h in grid.items():
                h.accumulate(camera, planes)
                row(f"history mean alpha={al:g} n_max={nm}").add(err(h.accum, a.spp))
                for s in SIGMA_GRID:
                    row(f"history resolve_guided sigma_l={s:g} alpha={al:g} n_max={nm}").add(
                        err(h.resolve_guided(guide, ("linear",), sigma_l=s)["linear"]))
            for g, h in gates.items():
                h.accumulate(camera, planes)
                row(f"history mean k_depth={g[0]:g} k_normal={g[1]}").add(err(h.accum, a.spp))
            for (g, r, al), h in clips.items():
                h.accumulate(camera, planes)
                row(f"clip mean gamma={g:g} radius={r} alpha={al:g} n_max={CLIP_N_MAX}").add(err(h.accum, a.spp))
                for s in SIGMA_GRID:
                    row(f"clip resolve_guided sigma_l={s:g} gamma={g:g} radius={r} alpha={al:g} n_max={CLIP_N_MAX}").add(
                        err(h.resolve_guided(guide, ("linear",), sigma_l=s)["linear"]))
            film.collect()
        film.sync()
        clipped = {}
        for (g, r, al), h in clips.items():
            has = h.length > 1
            clipped[f"gamma={g:g} radius={r} alpha={al:g}"] = float(((h.clip_amount > 0) & has).double().sum().item()
                                                                    / max(int(has.sum().item()), 1))
            h.close()
        for name, h in [(f"alpha={al:g} n_max={nm}", h) for (al, nm), h in grid.items()] + \
                       [(f"k_depth={g[0]:g} k_normal={g[1]}", h) for g, h in gates.items()]:
            n = h.length.to(torch.float64)
            stats[name] = {"with_history": float((n > 1).double().mean().item()), "mean_length": float(n.mean().item())}
            h.close()
    return {"width": W, "height": H, "spp": a.spp, "frames": a.frames, "orbit": a.orbit, "reference_spp": a.reference_spp,
            "errors": {k: v.result() for k, v in rows.items()}, "history_at_the_last_pose": stats,
            **({"clipped_of_the_pixels_with_history_at_the_last_pose": clipped} if a.clip else {}),
            "defaults": {"alpha": fh.ALPHA, "n_max": fh.N_MAX, "k_depth": fh.K_DEPTH}}


def bench(name, a, variants=None):
    sph, tri, rq = scenes.config_world(name)
    out = {"divisions": rq.divisions, "max_bounces": rq.max_bounces}
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_light_sampling(rt.RT_LIGHTS_CONE)
        sc.set_glossy_sampling(rt.RT_GLOSSY_MIS)
        out["frame"] = frame_times(sc, rq, a, variants)
        if a.frames:
            out["quality"] = quality(sc, rq, a)
    return out


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--quality-width", type=int, default=480)
    ap.add_argument("--quality-height", type=int, default=280)
    ap.add_argument("--frames", type=int, default=8, help="poses of the quality orbit; 0: timing only")
    ap.add_argument("--orbit", type=int, default=96, help="viewpoints of the whole circle")
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--aperture", type=float, default=None, help="0: pinhole rays (default: the reference's 0.1, focused at 1)")
    ap.add_argument("--clip", action="store_true", help="also time and grade the clip of the history (DESIGN.md 4.26)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10, help="accumulate / resolve calls per timed window")
    return ap


def main():
    a = parser().parse_args()
    if a.aperture is not None:
        LENS["aperture"] = a.aperture
    rt.init()
    print(json.dumps({name: bench(name, a) for name in a.configs}))


if __name__ == "__main__":
    main()
