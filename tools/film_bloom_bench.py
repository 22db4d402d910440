#!/usr/bin/env python3
"""The bloom (ray_tracer_s8_amd.FilmBloom) measured on a seeded HDR image (log-uniform colours over 2^-8 ... 2^4 with
a few lamps of 2^10) at each size (default 1920 x 1080 and 3840 x 2160) and each level count (default 4 ... 8), in both forms:

  apply_ms     FilmBloom.apply between events on the film's stream: median / best / worst of --runs windows of --calls calls after
               --warmup warm-ups.  The two forms and the torch chain alternate inside a run, so that a drift of the machine meets all
               three.  apply() allocates its output at every call, as a frame loop's call does.
  launches     the kernels a call launches; tail_from, the first level of the tail ("none": no level fits).
  bytes        what the form moves through memory at the least: the image read twice and written once, and every level of the pyramid
               written and read as the form implies (a level above the tail: written by its down step and by its up step, read by the
               next down step, by its up step and by the level above it, five passes; the tail's first level: written once, read
               once; the deeper levels of the tail: none).  rate_TBps = bytes / median time, and hbm_share is that rate over
               6.29 TB/s, the float4 copy rate measured on this chip; it is a whole-call figure, launch gaps included.
  torch_ms     a chain of the same structure written in torch on a (1, 3, R, W) tensor: replicate padding and a 4 x 4 binomial
               conv2d of stride 2 a level down, a bilinear interpolate and an add a level up, the mix at the end.  Its bytes are
               not the bloom's: only its time is compared.
  tail_gain    levels' median over tail's, beside spread, the worst over the best window of "levels" itself: the tail pays only where
               the gain is above the spread.

    python tools/film_bloom_bench.py [--sizes 1920x1080 3840x2160] [--levels 4 5 6 7 8]
Prints one JSON line.  torch is imported first: the libraries then bind to torch's HIP runtime."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import _abi, film_bloom, scenes  # noqa: E402

HBM_COPY_TBPS = 6.29
LDS_BUDGET = 160 * 1024


def tail_from(shape, levels):
    sizes = [r * w * 12 for r, w in film_bloom.level_shapes(shape, levels)]
    fits = [k for k in range(1, levels + 1) if sum(sizes[k:]) <= LDS_BUDGET]
    return min(fits) if fits else levels + 1


def plan(shape, levels, form):
    """(launches, bytes, tail_from or None) of a call."""
    sizes = [r * w * 12 for r, w in film_bloom.level_shapes(shape, levels)]
    tf = tail_from(shape, levels) if form == "tail" else levels + 1
    if tf > levels:
        passes = [5] * (levels - 1) + [2]
        return 2 * levels, 3 * sizes[0] + sum(p * s for p, s in zip(passes, sizes[1:])), None
    passes = [5] * (tf - 1) + [2] + [0] * (levels - tf)
    return 2 * tf, 3 * sizes[0] + sum(p * s for p, s in zip(passes, sizes[1:])), tf


def torch_chain(levels, spread, strength):
    """The same structure in torch, on (1, 3, R, W)."""
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0])
    kernel = (k1[:, None] * k1[None, :] / 64.0).expand(3, 1, 4, 4).contiguous()
    total = sum(spread ** k for k in range(levels))

    def run(x):
        w = kernel.to(x.device)
        D, s = [], x.clamp(0.0, 65536.0)
        for _ in range(levels):
            ph, pw = s.shape[2] % 2, s.shape[3] % 2
            s = F.conv2d(F.pad(s, (1, 1 + pw, 1, 1 + ph), mode="replicate"), w, stride=2, groups=3)
            D.append(s)
        u = D[-1]
        for d in reversed(D[:-1]):
            u = d + spread * F.interpolate(u, size=d.shape[2:], mode="bilinear", align_corners=False)
        b = F.interpolate(u, size=x.shape[2:], mode="bilinear", align_corners=False) / total
        return (1.0 - strength) * x.clamp_min(0.0) + strength * b

    return run


def _spread(t):
    return {"median": statistics.median(t), "best": min(t), "worst": max(t), "runs": len(t)}


def measure(stream, works, a):
    """Every work of `works` timed in every run, one after the other: {name: spread of ms a call}."""
    t = {name: [] for name in works}
    for run in range(a.warmup + a.runs):
        for name, work in works.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.calls):
                work()
            e1.record(stream)
            e1.synchronize()
            if run >= a.warmup:
                t[name].append(e0.elapsed_time(e1) / a.calls)
    return {name: _spread(v) for name, v in t.items()}


def image(shape, device, seed=7):
    g = torch.Generator().manual_seed(seed)
    x = torch.exp2(torch.rand((*shape, 3), generator=g) * 12.0 - 8.0)
    lamps = torch.rand(shape, generator=g) < 1e-4
    x[lamps] = 1024.0
    return x.to(device)


def bench(film, shape, levels, a):
    row = {"rows": shape[0], "columns": shape[1], "level_count": levels}
    with torch.cuda.stream(film.stream):
        img = image(shape, film.device)
        nchw = img.permute(2, 0, 1)[None].contiguous()
    blooms = {form: rt.FilmBloom(film, levels=levels, shape=shape) for form in ("levels", "tail")}
    for form, b in blooms.items():
        b.form = form
    chain = torch_chain(levels, 0.7, 0.05)

    def torch_work():
        with torch.cuda.stream(film.stream):
            chain(nchw)

    works = {form: (lambda b=b: b.apply(img)) for form, b in blooms.items()}
    works["torch"] = torch_work
    with torch.cuda.stream(film.stream):
        same = torch.equal(blooms["levels"].apply(img)["linear"], blooms["tail"].apply(img)["linear"])
    t = measure(film.stream, works, a)
    for form in ("levels", "tail"):
        launches, nbytes, tf = plan(shape, levels, form)
        rate = nbytes / (t[form]["median"] * 1e-3) / 1e12
        row[form] = {"apply_ms": t[form], "launches": launches, "tail_from": tf if tf is not None else "none", "bytes": nbytes,
                     "rate_TBps": rate, "hbm_share": rate / HBM_COPY_TBPS}
    row["torch_ms"] = t["torch"]
    row["same_bytes"] = same
    row["tail_gain"] = t["levels"]["median"] / t["tail"]["median"]
    row["spread"] = t["levels"]["worst"] / t["levels"]["best"]
    for b in blooms.values():
        b.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
    ap.add_argument("--levels", nargs="+", type=int, default=[4, 5, 6, 7, 8])
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window")
    a = ap.parse_args()
    rt.init()
    sph, rq = scenes.config("c2")
    strips = [_abi.default_request(width=64, height=36, divisions=1, division_no=0, spp=1, max_bounces=rq.max_bounces, seed=rq.seed)]
    res = {"default_form": film_bloom.FORM, "rows": []}
    with rt.Scene(0, rt.World(sph)) as sc:
        with rt.Film(sc, strips) as film:                                 # (the film gives the device and the stream; it renders nothing)
            for size in a.sizes:
                W, H = (int(v) for v in size.split("x"))
                for levels in a.levels:
                    res["rows"].append(bench(film, (H, W), levels, a))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
