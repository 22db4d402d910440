#!/usr/bin/env python3
"""The display (ray_tracer_s8_amd.FilmDisplay) measured on the film's stream at --width x --height, per config (default c2
and c3; the config's own divisions, bounces and seed, "nee" RT_NEE_MIS, --spp samples), median / best / worst of --runs windows of
--calls calls after --warmup warm-ups, between events on the film's stream:

  stages      rtd_meter, rtd_expose and rtd_apply alone (rgb only, and rgb with f32), FilmDisplay.display(), beside Film.preview() on
              the same film and beside a torch restatement of the same chain (luminance, bit-shift bins, bincount, the percentiles on
              the host, the filmic curve, the quantisation), which pays several launches and a host round trip.
  forms       rtd_meter under both histogram forms on three inputs: the config's preview (a few bins full), a constant image (one bin)
              and log-uniform noise (every bin); milliseconds and the bytes per second of the 12 bytes a pixel it reads.
  clipping    the share of the rgb bytes at code 255 and at codes 0 ... 2 under the film's plain rgb and under display() with the
              defaults, and the record display() left.
  orbit       (c2) the scale and the target of display() at rate --rate along --orbit-frames poses of the whole circle of
              examples/film_temporal.py, one pass of --spp samples each.

    python tools/film_display_bench.py [--configs c2 c3] [--width 1920 --height 1080] [--parts stages forms clipping orbit]
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
from ray_tracer_s8_amd import _abi, _display_lib as dl, film_display as fd, scenes  # noqa: E402

PARTS = ("stages", "forms", "clipping", "orbit")


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


def _per_call(stream, call, a):
    """The spread of one call's milliseconds: windows of a.calls calls."""
    t = []
    for run in range(a.warmup + a.runs):
        ms = _timed(stream, lambda: [call() for _ in range(a.calls)]) / a.calls
        if run >= a.warmup:
            t.append(ms)
    return _spread(t)


def _requests(rq, a, seed):
    return [_abi.default_request(width=a.width, height=a.height, divisions=rq.divisions, division_no=k, spp=a.spp,
                                 max_bounces=rq.max_bounces, seed=seed) for k in range(rq.divisions)]


def _rep(b):
    return torch.tensor([((b + 888) << 20) | 0x80000], dtype=torch.int32).view(torch.float32).item()


def _torch_chain(linear, s):
    """The chain in torch: what a user writes today.  The percentiles come to the host."""
    y = (linear[..., 0] + linear[..., 1]) + linear[..., 2]
    q = ((y.view(torch.int32) >> 20) - 888).clamp(0, 255)
    H = torch.bincount(q[y > 0].flatten(), minlength=256)
    cum = torch.cumsum(H, 0).cpu()
    N = int(cum[-1])
    bins = [int((cum > ((N * q16) >> 16)).nonzero()[0]) for q16 in (s.key_q16, s.white_q16)] if N else [120, 120]
    scale = min(max(s.key / _rep(bins[0]), s.scale_min), s.scale_max)
    x = (linear * scale).clamp_min(0)
    t = ((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)).clamp_max(1)
    return (t.sqrt() * 255.999).clamp(0, 255).to(torch.uint8)


def _stages(film, disp, linear, a):
    lib, stream = disp._lib, film.stream
    R, W = disp.settings.shape
    s = disp.settings
    out_rgb = torch.empty((R, W, 3), dtype=torch.uint8, device=film.device)
    out_f32 = torch.empty((R, W, 3), dtype=torch.float32, device=film.device)
    meter = dl.MeterArgs(W=W, R=R, form=dl.FORMS[disp.form], linear=linear.data_ptr(), hist=disp._hist.data_ptr())
    expose = dl.ExposeArgs(mode=0, key=s.key, key_q16=s.key_q16, white_q16=s.white_q16, rate=s.rate, scale_min=s.scale_min,
                           scale_max=s.scale_max, hist=disp._hist.data_ptr(), record=disp._record.data_ptr())
    apply = lambda f32: dl.ApplyArgs(W=W, R=R, curve=dl.CURVES[s.curve], dither=int(s.dither), linear=linear.data_ptr(),
                                     record=disp._record.data_ptr(), out_rgb=out_rgb.data_ptr(), out_f32=out_f32.data_ptr() if f32 else None)
    rgb, both = apply(False), apply(True)
    h = stream.cuda_stream

    def chain():
        with torch.cuda.stream(stream):
            return _torch_chain(linear, s)

    calls = {
        "meter": lambda: dl.check("rtd_meter", lib.rtd_meter(meter, h)),
        "expose": lambda: dl.check("rtd_expose", lib.rtd_expose(expose, h)),
        "apply_rgb": lambda: dl.check("rtd_apply", lib.rtd_apply(rgb, h)),
        "apply_rgb_f32": lambda: dl.check("rtd_apply", lib.rtd_apply(both, h)),
        "display": lambda: disp.display(linear),
        "film_preview": lambda: film.preview(("rgb",)),
        "torch_chain": chain,
    }
    res = {k: _per_call(stream, c, a) for k, c in calls.items()}
    pixels = R * W
    gbs = lambda ms, bytes_: bytes_ / (ms * 1e-3) / 1e9
    res["meter_GBps"] = gbs(res["meter"]["median"], 12 * pixels)
    res["apply_rgb_GBps"] = gbs(res["apply_rgb"]["median"], 15 * pixels)          # 12 read, 3 written
    res["apply_rgb_f32_GBps"] = gbs(res["apply_rgb_f32"]["median"], 27 * pixels)
    # the two chains show the same image up to the roundings torch orders differently
    disp.reset()
    mine = disp.display(linear)["rgb"]
    theirs = chain()
    film.sync()
    res["torch_chain_max_code_difference"] = int((mine.to(torch.int16) - theirs.to(torch.int16)).abs().max().item())
    return res


def _forms(film, disp, linear, a):
    lib, stream = disp._lib, film.stream
    R, W = disp.settings.shape
    with torch.cuda.stream(stream):
        g = torch.Generator(device=film.device).manual_seed(4300)
        inputs = {"preview": linear, "constant": torch.full((R, W, 3), 0.18, dtype=torch.float32, device=film.device),
                  "noise": torch.exp2(torch.rand((R, W, 3), generator=g, device=film.device) * 40.0 - 20.0)}
    out = {}
    for name, img in inputs.items():
        row = {}
        for form, code in dl.FORMS.items():
            args = dl.MeterArgs(W=W, R=R, form=code, linear=img.data_ptr(), hist=disp._hist.data_ptr())
            t = _per_call(stream, lambda: dl.check("rtd_meter", lib.rtd_meter(args, stream.cuda_stream)), a)
            t["GBps"] = 12 * R * W / (t["median"] * 1e-3) / 1e9
            film.sync()
            t["bins_filled"] = int((disp._hist[:256] > 0).sum().item())
            row[form] = t
        out[name] = row
    return out


def _shares(rgb):
    n = rgb.numel()
    return {"at_255": float((rgb == 255).sum().item()) / n, "at_0_to_2": float((rgb <= 2).sum().item()) / n}


def _clipping(film, disp, linear):
    disp.reset()
    shown = disp.display(linear)["rgb"]
    plain = film.preview(("rgb",))["rgb"]
    film.sync()
    return {"plain": _shares(plain), "display": _shares(shown), "record": disp.exposure()}


def orbit_camera(i: int, n: int) -> rt.Camera:
    a = 2.0 * math.pi * i / max(n, 1)
    return rt.Camera.look_at((1.2 * math.sin(a), 0.3 + 0.4 * math.cos(a), 0.2), (0.0, -0.8, -4.0))


def _orbit(sc, film, rq, a):
    rows = []
    with rt.FilmDisplay(film, rate=a.rate) as disp:
        for i in range(a.orbit_frames):
            sc.set_camera(orbit_camera(i, a.orbit_frames))
            film.reset(seed=rq.seed + i)
            film.render_pass(0, a.spp)
            rgb = disp.display(film.preview(("linear",))["linear"])["rgb"]
            e = disp.exposure()
            rows.append({"scale": e["scale"], "target": e["target"], "white": e["white"], "bin_key": e["bin_key"], "bin_white": e["bin_white"],
                         **_shares(rgb)})
            film.collect()
    return {"rate": a.rate, "frames": rows, "scale_range": [min(r["scale"] for r in rows), max(r["scale"] for r in rows)],
            "target_range": [min(r["target"] for r in rows), max(r["target"] for r in rows)]}


def bench(name, a):
    sph, tri, rq = scenes.config_world(name)
    out = {"width": a.width, "height": a.height, "spp": a.spp, "form": fd.HISTOGRAM_FORM}
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        with rt.Film(sc, _requests(rq, a, rq.seed), integrator="nee", mode=_abi.RT_NEE_MIS) as film, rt.FilmDisplay(film) as disp:
            film.render_pass(0, a.spp)
            with torch.cuda.stream(film.stream):             # (the clone on the film's stream: it reads what the preview enqueued there)
                linear = film.preview(("linear",))["linear"].clone()
            film.collect()
            if "stages" in a.parts:
                out["stages"] = _stages(film, disp, linear, a)
            if "forms" in a.parts:
                out["forms"] = _forms(film, disp, linear, a)
            if "clipping" in a.parts:
                out["clipping"] = _clipping(film, disp, linear)
            if "orbit" in a.parts and name == "c2":
                out["orbit"] = _orbit(sc, film, rq, a)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--parts", nargs="+", default=list(PARTS), choices=PARTS)
    ap.add_argument("--rate", type=float, default=0.25, help="the adaptation rate along the orbit")
    ap.add_argument("--orbit-frames", type=int, default=12)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    a = ap.parse_args()
    rt.init()
    print(json.dumps({name: bench(name, a) for name in a.configs}))


if __name__ == "__main__":
    main()
