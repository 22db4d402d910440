#!/usr/bin/env python3
"""The frame encoder (ray_tracer_s8_amd.FrameEncoder) measured on a displayed frame of each config (default c2 and c3;
the config's own divisions, bounces and seed, "nee" RT_NEE_MIS, --spp samples, FilmDisplay's defaults) at each size (default 1920 x 1080
and 3840 x 2160), for restart intervals of a row of MCUs, 64 and 16:

  kernels_ms   rtj_encode between events on the film's stream: median / best / worst of --runs windows of --calls calls after --warmup
               warm-ups.
  encode_ms    FrameEncoder.encode(): wall time of the launches, the read of the record and the copy of the file, the stream idle
               before; median / best / worst of --runs calls.
  file_bytes   what crosses to the host, beside raw_bytes, the frame.
  host         what the controller does today: the raw copy of the frame (rgb.cpu()) and Pillow's encoder on one thread at the same
               quality with subsampling=0 and the same restart interval, wall time each; and controller_shim.encode_jpeg as it is
               (Pillow's default subsampling).  same_file says whether Pillow's file and the device's hold the same entropy data.

    python tools/jpeg_bench.py [--configs c2 c3] [--sizes 1920x1080 3840x2160] [--quality 90]
Prints one JSON line.  torch is imported first: the libraries then bind to torch's HIP runtime."""
import argparse
import io
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import _abi, controller_shim, scenes  # noqa: E402


def _spread(t):
    return {"median": statistics.median(t), "best": min(t), "worst": max(t), "runs": len(t)}


def _events(stream, work, a):
    t = []
    for run in range(a.warmup + a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            work()
        e1.record(stream)
        e1.synchronize()
        if run >= a.warmup:
            t.append(e0.elapsed_time(e1) / a.calls)
    return _spread(t)


def _wall(stream, work, a):
    t = []
    for run in range(a.warmup + a.runs):
        stream.synchronize()
        t0 = time.perf_counter()
        work()
        t1 = time.perf_counter()
        if run >= a.warmup:
            t.append((t1 - t0) * 1e3)
    return _spread(t)


def _entropy(data):
    at = data.index(b"\xff\xda")
    return data[at + 2 + ((data[at + 2] << 8) | data[at + 3]):]


def bench(name, W, H, a):
    from PIL import Image
    sph, tri, rq = scenes.config_world(name)
    strips = [_abi.default_request(width=W, height=H, divisions=rq.divisions, division_no=k, spp=a.spp, max_bounces=rq.max_bounces,
                                   seed=rq.seed) for k in range(rq.divisions)]
    out = {"width": W, "height": H, "quality": a.quality, "raw_bytes": W * H * 3, "intervals": {}}
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        with rt.Film(sc, strips, integrator="nee", mode=_abi.RT_NEE_MIS) as film, rt.FilmDisplay(film) as disp:
            film.render_pass(0, a.spp)
            with torch.cuda.stream(film.stream):
                rgb = disp.display(film.preview(("linear",))["linear"])["rgb"].clone()
            film.sync()
            for label, interval in (("row", (W + 7) // 8), ("64", 64), ("16", 16)):
                with rt.FrameEncoder(film, quality=a.quality, interval=interval) as enc:
                    data = enc.encode(rgb)
                    row = {"interval": interval, "file_bytes": len(data), "record": enc.record(),
                           "kernels_ms": _events(film.stream, lambda: enc.encode_device(rgb), a),
                           "encode_ms": _wall(film.stream, lambda: enc.encode(rgb), a)}
                    frame = rgb.cpu().numpy()

                    def pillow():
                        b = io.BytesIO()
                        Image.fromarray(frame, "RGB").save(b, format="JPEG", quality=a.quality, subsampling=0, restart_marker_blocks=interval)
                        return b.getvalue()

                    theirs = pillow()
                    row["host"] = {"raw_copy_ms": _wall(film.stream, lambda: rgb.cpu(), a), "pillow_444_ms": _wall(film.stream, pillow, a),
                                   "pillow_444_bytes": len(theirs), "same_file": _entropy(theirs) == _entropy(data),
                                   "encode_jpeg_ms": _wall(film.stream, lambda: controller_shim.encode_jpeg(frame, a.quality), a)}
                    out["intervals"][label] = row
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window of the kernels")
    a = ap.parse_args()
    rt.init()
    res = {}
    for name in a.configs:
        for size in a.sizes:
            W, H = (int(v) for v in size.split("x"))
            res[f"{name} {size}"] = bench(name, W, H, a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
