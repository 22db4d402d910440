#!/usr/bin/env python3
"""The film's moments fold and variance-guided resolve (ray_tracer_s8_amd.Film(moments=True)) measured next to what
they replace, per config (default c2 and c3) at 1920 x 1080 and 8 samples per pixel, the config's own divisions, bounces and seed:

  pass_ms     one pass of all strips, samples [0, spp), timed with events on the film's stream, --runs after --warmup warm-ups, the
              variants alternating within every run, for the "path" and the "nee" (RT_NEE_MIS) film: `torch` is the film without
              moments (k strided add_ launches a strip), `kernel` the film with moments (one rtf_fold_moments launch a strip),
              `none` the pass without any fold.  median, best and worst, and each fold's share of its pass,
              1 - median(none) / median(with): DESIGN.md 4.22's "fold share" rows, re-measured in the same run;
  resolve_ms  Film.resolve (the a-trous of 4.14, its defaults, the normal, depth and hits planes) and Film.resolve_guided (the same
              planes, the default constants) at 5 iterations on the same 8-sample NEE frame, --calls calls per timed window;
  mse         the mean squared error of the `linear` output against accum / n of a --reference-spp film of the same integrator (its own
              seed), and the same error relative to the reference, mean((x - ref)^2 / (ref^2 + 0.01)): for preview(), resolve() and
              resolve_guided over a grid of sigma_l x var_eps with the planes, and of sigma_l at the default var_eps without them.

    python tools/film_guided_bench.py [--configs c2 c3] [--width 1920 --height 1080 --spp 8] [--runs 7 --warmup 2]
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

SIGMA_GRID = (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0)
EPS_GRID = (2.0 ** -12, 2.0 ** -10, 2.0 ** -8, 2.0 ** -6, 2.0 ** -4)
GUIDE = ("normal", "depth", "hits")


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


def _no_fold(*a):
    pass


def _requests(rq, a, spp, seed):
    return [_abi.default_request(width=a.width, height=a.height, divisions=rq.divisions, division_no=k, spp=spp,
                                 max_bounces=rq.max_bounces, seed=seed) for k in range(rq.divisions)]


def _pass_times(sc, rqs, a):
    out = {}
    for integrator in ("path", "nee"):
        plain = rt.Film(sc, rqs, integrator=integrator)
        mom = rt.Film(sc, rqs, integrator=integrator, moments=True)

        def one(f):
            f.reset()
            f.render_pass(0, a.spp)

        t = {k: [] for k in ("torch", "kernel", "none")}
        for run in range(a.warmup + a.runs):
            got = {"torch": _timed(plain.stream, lambda: one(plain)), "kernel": _timed(mom.stream, lambda: one(mom))}
            plain._fold = _no_fold
            got["none"] = _timed(plain.stream, lambda: one(plain))
            del plain._fold
            plain.collect()
            mom.collect()
            if run >= a.warmup:
                for k, ms in got.items():
                    t[k].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        # the two films hold the same accum at the size timed
        one(plain)
        one(mom)
        plain.sync()
        mom.sync()
        same = bool(torch.equal(plain.accum.view(torch.int32), mom.accum.view(torch.int32)))
        out[integrator] = {"pass_ms": {k: _spread(v) for k, v in t.items()},
                           "fold_share": {k: 1.0 - med["none"] / med[k] for k in ("torch", "kernel")},
                           "fold_ms": {k: med[k] - med["none"] for k in ("torch", "kernel")},
                           "accum_equal": same}
        plain.close()
        mom.close()
    return out


def _errors(x, ref):
    d = x.to(torch.float64) - ref
    return {"mse": float((d * d).mean().item()), "rel_mse": float((d * d / (ref * ref + 0.01)).mean().item())}


def _resolve(sc, rq, a):
    rqs = _requests(rq, a, a.spp, rq.seed)
    out = {}
    with rt.Film(sc, _requests(rq, a, a.reference_spp, rq.seed ^ 0x5EED), integrator="nee") as big:
        big.render_pass(0, a.reference_spp)
        big.sync()
        ref = (big.accum.to(torch.float64) / a.reference_spp).clone()
        big.collect()
    with rt.Film(sc, rqs, integrator="nee", moments=True) as film:
        film.render_pass(0, a.spp)
        planes = film.features(1)
        guide = {n: planes[n] for n in GUIDE}
        calls = {"resolve": lambda: film.resolve(planes=guide, outputs=("linear",)),
                 "resolve_guided": lambda: film.resolve_guided(guide, ("linear",)),
                 "resolve_guided_direct": lambda: film.resolve_guided(guide, ("linear",), _lds_max_step=0),
                 "resolve_no_planes": lambda: film.resolve(outputs=("linear",)),
                 "resolve_guided_no_planes": lambda: film.resolve_guided(None, ("linear",))}
        t = {k: [] for k in calls}
        for run in range(a.warmup + a.runs):
            for k, call in calls.items():
                ms = _timed(film.stream, lambda: [call() for _ in range(a.calls)]) / a.calls
                if run >= a.warmup:
                    t[k].append(ms)
            film.collect()
        out["resolve_ms"] = {k: _spread(v) for k, v in t.items()}
        out["calls_per_window"] = a.calls

        def err(res):
            film.sync()
            return _errors(res["linear"], ref)

        mse = {"preview": err(film.preview(("linear",))), "resolve": err(calls["resolve"]()),
               "resolve_no_planes": err(calls["resolve_no_planes"]())}
        mse["guided"] = {str(s): {f"{e:.3g}": err(film.resolve_guided(guide, ("linear",), sigma_l=s, var_eps=e)) for e in EPS_GRID}
                         for s in SIGMA_GRID}
        mse["guided_no_planes"] = {str(s): err(film.resolve_guided(None, ("linear",), sigma_l=s)) for s in SIGMA_GRID}
        out["mse"] = mse
        out["defaults"] = {"sigma_l": film_mod.SIGMA_L, "var_eps": film_mod.VAR_EPS}
        v0 = film.variance()
        film.sync()                                        # (.to() below runs on torch's current stream, not the film's)
        v0 = v0.to(torch.float64)
        out["v0"] = {"mean": float(v0.mean().item()), "median": float(v0.median().item()), "max": float(v0.max().item()),
                     "zero_share": float((v0 == 0).double().mean().item())}
        out["reference_luminance"] = float(ref.sum(-1).mean().item())
    return out


def bench(name, a):
    sph, tri, rq = scenes.config_world(name)
    out = {"width": a.width, "height": a.height, "spp": a.spp, "divisions": rq.divisions, "max_bounces": rq.max_bounces,
           "reference_spp": a.reference_spp}
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        out["fold"] = _pass_times(sc, _requests(rq, a, a.spp, rq.seed), a)
        out.update(_resolve(sc, rq, a))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10, help="resolve calls per timed window")
    a = ap.parse_args()
    rt.init()
    print(json.dumps({name: bench(name, a) for name in a.configs}))


if __name__ == "__main__":
    main()
