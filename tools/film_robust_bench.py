#!/usr/bin/env python3
"""The robust film (ray_tracer_s8_amd.FilmRobust) measured next to the film it taps, per config (default c2 and c3), the
config's own divisions, bounces and seed, at --width x --height:

  time        one pass of --time-spp samples (default 8 and 32) between events on the film's stream, with no tap and with a robust tap
              of --buckets buckets, the variants alternating, median / best / worst of --runs after --warmup warm-ups; the tap's
              share of a pass; estimate() and state() per call (where the pass holds a sample for every bucket).  With
              --parent-film FILE (the film.py of another commit, e.g. `git show HEAD~1:ray_tracer_s8_amd/film.py > FILE`) that
              commit's Film takes turns with them: its pass is the margin the untapped pass is held against (the only change on that
              path is an empty loop over the taps).  "nee" RT_NEE_MIS, moments=True.
  error       against accum / n of a --reference-spp film of the same integrator under another seed: mean((x - ref)^2) and
              mean((x - ref)^2 / (ref^2 + 0.01)) of the `linear` output of preview and of resolve_guided (5 iterations, normal, depth
              and hits), for the film's mean and, for K in --error-buckets, the robust film under "gini", the median (c = 0) and
              c = h, at --error-spp samples (default 16, 32, 64; one film carries a tap per K and stops at each count), under "path",
              "nee" RT_NEE_LIGHT_ONLY and "nee" RT_NEE_MIS with the scene's default light and glossy sampling.
  energy      the image mean of each preview over the reference's: below 1, the estimate is biased low.

    python tools/film_robust_bench.py [--configs c2 c3] [--width 1920 --height 1080] [--parts time error] [--parent-film FILE]
Prints one JSON line.  torch is imported first: the libraries then bind to torch's HIP runtime."""
import argparse
import importlib.util
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import _abi, scenes  # noqa: E402

GUIDE = ("normal", "depth", "hits")
INTEGRATORS = {"path": ("path", _abi.RT_NEE_MIS), "nee_light_only": ("nee", _abi.RT_NEE_LIGHT_ONLY), "nee_mis": ("nee", _abi.RT_NEE_MIS)}


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


def _parent_film(path):
    """The Film of another commit's film.py, loaded as a module of this package (its relative imports are this tree's)."""
    spec = importlib.util.spec_from_file_location("ray_tracer_s8_amd._parent_film", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.Film


def _times(sc, rq, a):
    out = {}
    for spp in a.time_spp:
        rqs = _requests(rq, a, spp, rq.seed)
        films = {"untapped": rt.Film(sc, rqs, integrator="nee", moments=True), "tapped": rt.Film(sc, rqs, integrator="nee", moments=True)}
        if a.parent_film:
            films["parent"] = _parent_film(a.parent_film)(sc, rqs, integrator="nee", moments=True)
        robust = rt.FilmRobust(films["tapped"], buckets=a.buckets)

        def one(f):
            f.reset()
            f.render_pass(0, spp)

        t = {k: [] for k in films}
        for run in range(a.warmup + a.runs):
            for k, f in films.items():
                ms = _timed(f.stream, lambda: one(f))
                f.collect()
                if run >= a.warmup:
                    t[k].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        res = {"pass_ms": {k: _spread(v) for k, v in t.items()}, "tap_ms": med["tapped"] - med["untapped"],
               "tap_share": 1.0 - med["untapped"] / med["tapped"]}
        if a.parent_film:
            p = res["pass_ms"]["parent"]
            res["untapped_within_parent_spread"] = bool(p["best"] <= med["untapped"] <= p["worst"])
            res["untapped_over_parent"] = med["untapped"] / med["parent"]
        films["untapped"].sync()
        films["tapped"].sync()
        res["accum_equal"] = bool(torch.equal(films["untapped"].accum.view(torch.int32), films["tapped"].accum.view(torch.int32)))
        calls = {"estimate": lambda: robust.estimate(("linear", "gini", "kept", "variance")), "estimate_linear": robust.estimate,
                 "state": robust.state}
        tc = {k: [] for k in calls}
        for run in range(a.warmup + a.runs if spp >= a.buckets else 0):       # (an estimate needs a sample in every bucket)
            for k, call in calls.items():
                ms = _timed(robust.film.stream, lambda: [call() for _ in range(a.calls)]) / a.calls
                if run >= a.warmup:
                    tc[k].append(ms)
        res["call_ms"] = {k: _spread(v) for k, v in tc.items() if v}
        res["bucket_bytes"] = robust.buckets.numel() * 4
        robust.close()
        for f in films.values():
            f.close()
        out[str(spp)] = res
    return out


def _errors(x, ref):
    d = x.to(torch.float64) - ref
    return {"mse": float((d * d).mean().item()), "rel_mse": float((d * d / (ref * ref + 0.01)).mean().item())}


def _quality(sc, rq, a):
    out = {}
    top = max(a.error_spp)
    for name, (integrator, mode) in INTEGRATORS.items():
        if name not in a.integrators:
            continue
        with rt.Film(sc, _requests(rq, a, a.reference_spp, rq.seed ^ 0x5EED), integrator=integrator, mode=mode) as big:
            big.render_pass(0, a.reference_spp)
            big.sync()
            ref = (big.accum.to(torch.float64) / a.reference_spp).clone()
            big.collect()
        ref_mean = float(ref.mean().item())
        res = {"reference_mean": ref_mean}
        with rt.Film(sc, _requests(rq, a, top, rq.seed), integrator=integrator, mode=mode, moments=True) as film:
            taps = {K: rt.FilmRobust(film, buckets=K) for K in a.error_buckets}
            planes = film.features(1)
            guide = {n: planes[n] for n in GUIDE}

            def row(src):
                film.sync()
                p = src.preview(("linear",))["linear"]
                film.sync()
                r = {"preview": _errors(p, ref), "energy": float(p.to(torch.float64).mean().item()) / ref_mean}
                g = src.resolve_guided(guide, ("linear",))["linear"]
                film.sync()
                r["guided"] = _errors(g, ref)
                return r

            for spp in sorted(a.error_spp):
                film.render_pass(film.samples, spp)
                at = {"mean": row(film)}
                for K, tap in taps.items():
                    h = (K - 1) // 2
                    # (one tap per K serves the three widths: the mode and the width are read at every resolve)
                    for label, m, c in (("gini", "gini", 0), ("median", "trim", 0), ("all", "trim", h)):
                        tap.mode, tap.c = m, c
                        at[f"K{K}_{label}"] = row(tap)
                        if label == "gini":
                            kept = tap.estimate(("kept",))["kept"]
                            film.sync()
                            at[f"K{K}_{label}"]["kept_mean"] = float(kept.double().mean().item())
                res[str(spp)] = at
                film.collect()
            for tap in taps.values():
                tap.close()
        out[name] = res
    return out


def bench(name, a):
    sph, tri, rq = scenes.config_world(name)
    out = {"width": a.width, "height": a.height, "divisions": rq.divisions, "max_bounces": rq.max_bounces, "buckets": a.buckets,
           "reference_spp": a.reference_spp}
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        if "time" in a.parts:
            out["time"] = _times(sc, rq, a)
        if "error" in a.parts:
            out["error"] = _quality(sc, rq, a)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--parts", nargs="+", default=["time", "error"], choices=("time", "error"))
    ap.add_argument("--integrators", nargs="+", default=list(INTEGRATORS), choices=tuple(INTEGRATORS))
    ap.add_argument("--buckets", type=int, default=9, help="the tap's buckets in the time part")
    ap.add_argument("--time-spp", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--error-spp", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--error-buckets", type=int, nargs="+", default=[5, 9, 15])
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--parent-film", type=Path, default=None, help="the film.py of another commit, timed beside this one's")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10, help="estimate / state calls per timed window")
    a = ap.parse_args()
    rt.init()
    print(json.dumps({name: bench(name, a) for name in a.configs}))


if __name__ == "__main__":
    main()
