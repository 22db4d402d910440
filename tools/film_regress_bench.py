#!/usr/bin/env python3
"""The film's regression resolve (ray_tracer_s8_amd.Film.resolve_regression) measured next to the two a-trous
resolves, per config (default c2 and c3) at 1920 x 1080 and 2, 8 and 32 samples per pixel, the config's own divisions, bounces and
seed, on the "nee" (RT_NEE_MIS) film:

  mse         the mean squared error of the `linear` output against accum / n of a --reference-spp film of another seed, and the same
              error relative to the reference, mean((x - ref)^2 / (ref^2 + 0.01)): for preview(), resolve() and resolve_guided() with
              the normal, depth and hits planes at their defaults, and for resolve_regression over a grid of ridge, with the albedo
              plane (the colour is fitted demodulated), without it and without any plane, and at the default ridge with the hits
              plane alone, the normal alone, depth and hits, and the albedo alone;
  resolve_ms  each resolve at its defaults on the film's stream, timed with events, --calls calls per timed window, --runs windows
              after --warmup warm-ups, the variants alternating within every run: median, best and worst.  A regression call is its
              two kernels, the fit and the apply, back to back on the stream: what is timed is the two together.

    python tools/film_regress_bench.py [--configs c2 c3] [--width 1920 --height 1080] [--spp 2 8 32] [--runs 7 --warmup 2]
Prints one JSON line.  torch is imported first: the libraries then bind to torch's HIP runtime."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import _abi, scenes  # noqa: E402
from ray_tracer_s8_amd import film as film_mod  # noqa: E402

RIDGE_GRID = (1e-5, 1e-4, 1e-3, 1e-2, 1e-1)
GUIDE = ("normal", "depth", "hits")
ALL = ("albedo",) + GUIDE


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


def _requests(rq, a, spp, seed):
    return [_abi.default_request(width=a.width, height=a.height, divisions=rq.divisions, division_no=k, spp=spp,
                                 max_bounces=rq.max_bounces, seed=seed) for k in range(rq.divisions)]


def _errors(x, ref):
    d = x.to(torch.float64) - ref
    return {"mse": float((d * d).mean().item()), "rel_mse": float((d * d / (ref * ref + 0.01)).mean().item())}


def _resolves(sc, rq, a, ref, spp, timed):
    out = {}
    with rt.Film(sc, _requests(rq, a, max(spp, 2), rq.seed), integrator="nee", moments=True) as film:
        film.render_pass(0, spp)
        planes = film.features(1)
        guide = {n: planes[n] for n in GUIDE}
        full = {n: planes[n] for n in ALL}

        def err(res):
            film.sync()
            return _errors(res["linear"], ref)

        mse = {"preview": err(film.preview(("linear",))), "resolve": err(film.resolve(planes=guide, outputs=("linear",)))}
        if spp >= 2:
            mse["resolve_guided"] = err(film.resolve_guided(guide, ("linear",)))
        mse["regression_albedo"] = {f"{r:g}": err(film.resolve_regression(full, ("linear",), ridge=r)) for r in RIDGE_GRID}
        mse["regression_no_albedo"] = {f"{r:g}": err(film.resolve_regression(guide, ("linear",), ridge=r)) for r in RIDGE_GRID}
        mse["regression_no_planes"] = {f"{r:g}": err(film.resolve_regression(None, ("linear",), ridge=r)) for r in RIDGE_GRID}
        # which planes the error comes with: each subset at the default ridge
        mse["regression_subsets"] = {"+".join(names): err(film.resolve_regression({n: planes[n] for n in names}, ("linear",)))
                                     for names in (("hits",), ("normal",), ("depth", "hits"), ("albedo",))}
        film.resolve_regression(full, ("linear",))
        film.sync()
        m = film.regression_model                          # (of the default call with every plane)
        out["mse"] = mse
        out["nodes"] = {"total": int(m.shape[0] * m.shape[1]), "solved": int(m[..., 27].sum().item()),
                        "empty": int((m[..., 26] == 0).sum().item())}
        if timed:
            calls = {"resolve": lambda: film.resolve(planes=guide, outputs=("linear",)),
                     "resolve_guided": lambda: film.resolve_guided(guide, ("linear",)),
                     "resolve_regression": lambda: film.resolve_regression(full, ("linear",)),
                     "resolve_regression_no_albedo": lambda: film.resolve_regression(guide, ("linear",)),
                     "resolve_regression_rgb": lambda: film.resolve_regression(full, ("rgb",))}
            t = {k: [] for k in calls}
            for run in range(a.warmup + a.runs):
                for k, call in calls.items():
                    ms = _timed(film.stream, lambda: [call() for _ in range(a.calls)]) / a.calls
                    if run >= a.warmup:
                        t[k].append(ms)
                film.collect()
            out["resolve_ms"] = {k: _spread(v) for k, v in t.items()}
            out["calls_per_window"] = a.calls
    return out


def bench(name, a):
    sph, tri, rq = scenes.config_world(name)
    out = {"width": a.width, "height": a.height, "divisions": rq.divisions, "max_bounces": rq.max_bounces,
           "reference_spp": a.reference_spp, "ridge_default": film_mod.RIDGE}
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        sc.set_light_sampling(_abi.RT_LIGHTS_CONE)
        sc.set_glossy_sampling(_abi.RT_GLOSSY_MIS)
        with rt.Film(sc, _requests(rq, a, a.reference_spp, rq.seed ^ 0x5EED), integrator="nee") as big:
            big.render_pass(0, a.reference_spp)
            big.sync()
            ref = (big.accum.to(torch.float64) / a.reference_spp).clone()
            big.collect()
        out["reference_luminance"] = float(ref.sum(-1).mean().item())
        for spp in a.spp:
            out[f"spp{spp}"] = _resolves(sc, rq, a, ref, spp, timed=spp == a.time_spp)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, nargs="+", default=[2, 8, 32])
    ap.add_argument("--time-spp", type=int, default=8, help="the sample count whose resolves are timed")
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10, help="resolve calls per timed window")
    a = ap.parse_args()
    rt.init()
    print(json.dumps({name: bench(name, a) for name in a.configs}))


if __name__ == "__main__":
    main()
