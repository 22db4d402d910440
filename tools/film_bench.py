#!/usr/bin/env python3
"""The device-resident film (ray_tracer_s8_amd.Film) next to the tile path, per config (default c2 and c3) at
1920 x 1080 and 8 samples per pixel, the config's own divisions, bounces and seed:

  frame_ms   one frame of all strips, samples [0, spp), timed with events on one stream around the enqueued work, --runs after
             --warmup warm-ups, the variants alternating within every run: `tile` is rt_scene_render_tiles_pass_device (the
             progressive strip kernels), `path` the film with rt_scene_trace_device, `nee_light_only` and `nee_mis` the film with
             rt_scene_trace_nee_device in either mode.  median, best and worst;
  fold       the film's pass with and without the fold on the same buffers (the same Film, its _fold replaced by a no-op), per
             integrator: the share of the pass the torch adds take, 1 - median(without) / median(with);
  per_ray    film `path` over `tile`: how much slower the caller-ray kernels are per ray than the tile engines (the same rays);
  variance   the variance of a pixel's own samples (luminance, ddof 1) averaged over the frame, from one-sample passes, and the ratio
             nee / path at that equal sample count (below 1: NEE is the less noisy).

    python tools/film_bench.py [--configs c2 c3] [--width 1920 --height 1080 --spp 8] [--runs 7 --warmup 2]
Prints one JSON line.  torch is imported first: the library then binds to torch's HIP runtime."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import _abi, scenes  # noqa: E402

VARIANTS = {"path": ("path", _abi.RT_NEE_MIS), "nee_light_only": ("nee", _abi.RT_NEE_LIGHT_ONLY), "nee_mis": ("nee", _abi.RT_NEE_MIS)}


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


def _no_fold(accum, records):
    pass


def _sample_variance(film):
    """The mean over the frame of the variance of a pixel's own samples' luminance, from one-sample passes (float64 on the device)."""
    film.reset()
    with torch.cuda.stream(film.stream):
        prev = torch.zeros_like(film.accum, dtype=torch.float64)
        s1 = torch.zeros(film.accum.shape[:2], dtype=torch.float64, device=film.accum.device)
        s2 = torch.zeros_like(s1)
    for s in range(film.spp):
        film.render_pass(s, s + 1)
        with torch.cuda.stream(film.stream):
            cur = film.accum.to(torch.float64)
            lum = (cur - prev).mean(-1)
            s1 += lum
            s2 += lum * lum
            prev = cur
    film.sync()
    n = film.spp
    var = (s2 - s1 * s1 / n) / (n - 1)
    return float(var.mean().item()), float((s1 / n).mean().item())


def bench(name, a):
    sph, tri, rq = scenes.config_world(name)
    rqs = [_abi.default_request(width=a.width, height=a.height, divisions=rq.divisions, division_no=k, spp=a.spp,
                                max_bounces=rq.max_bounces, seed=rq.seed) for k in range(rq.divisions)]
    out = {"width": a.width, "height": a.height, "spp": a.spp, "divisions": rq.divisions, "max_bounces": rq.max_bounces}
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        out["lights"] = sc.n_lights
        films = {v: rt.Film(sc, rqs, integrator=i, mode=m) for v, (i, m) in VARIANTS.items()}
        stream = films["path"].stream
        out["records_in_flight"] = films["path"].hs * a.width * films["path"].k
        nb = films["path"].hs * a.width * 3
        with torch.cuda.stream(stream):
            acc = torch.zeros((a.height, a.width, 3), dtype=torch.float32, device=films["path"].device)
            rgb = torch.zeros((a.height, a.width, 3), dtype=torch.uint8, device=films["path"].device)
        hs = films["path"].hs
        accs = [acc[i * hs:(i + 1) * hs].data_ptr() for i in range(len(rqs))]
        outs = [rgb[i * hs:(i + 1) * hs].data_ptr() for i in range(len(rqs))]

        def tile():
            sc.render_tiles_pass_device(rqs, 0, a.spp, accs, outs, nb, stream=stream.cuda_stream)

        def film_pass(f):
            f.reset()
            f.render_pass(0, a.spp)

        t = {k: [] for k in ("tile", *VARIANTS, *(v + "_no_fold" for v in VARIANTS))}
        for run in range(a.warmup + a.runs):
            got = {"tile": _timed(stream, tile)}
            for v, f in films.items():
                got[v] = _timed(f.stream, lambda: film_pass(f))
                f._fold = _no_fold
                got[v + "_no_fold"] = _timed(f.stream, lambda: film_pass(f))
                del f._fold
            sc.collect()
            for f in films.values():
                f.collect()
            if run >= a.warmup:
                for k, ms in got.items():
                    t[k].append(ms)
        out["frame_ms"] = {k: _spread(v) for k, v in t.items()}
        med = {k: statistics.median(v) for k, v in t.items()}
        out["fold_share"] = {v: 1.0 - med[v + "_no_fold"] / med[v] for v in VARIANTS}
        out["per_ray_path_over_tile"] = med["path"] / med["tile"]
        out["frame_over_tile"] = {v: med[v] / med["tile"] for v in VARIANTS}
        # the path film against the tile path, byte for byte, at the size timed
        film_pass(films["path"])
        films["path"].sync()
        out["path_equals_tile"] = bool(torch.equal(films["path"].accum.view(torch.int32), acc.view(torch.int32)))
        var = {v: _sample_variance(f) for v, f in films.items()}
        out["variance"] = {v: {"within_pixel_variance": x[0], "mean_luminance": x[1]} for v, x in var.items()}
        out["variance_ratio_over_path"] = {v: var[v][0] / var["path"][0] for v in VARIANTS if v != "path"}
        for f in films.values():
            f.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    rt.init()
    print(json.dumps({name: bench(name, a) for name in a.configs}))


if __name__ == "__main__":
    main()
