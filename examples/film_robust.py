#!/usr/bin/env python3
"""Render the c2 box (scenes.cornell16) by plain path tracing, which finds the lamp by chance, on a film with a robust tap
(ray_tracer_s8_amd.FilmRobust): every pixel's samples go to K bucket sums as well, and the robust film estimates the pixel from the
central bucket means (median of means, the width of the centre from the Gini coefficient of the bucket means).  Writes the film's
preview, with its fireflies, the robust preview without them, and the Gini and kept-buckets planes that say where the two differ.

    python examples/film_robust.py OUT_DIR [--width 480 --height 270 --divisions 5] [--spp 32] [--buckets 9]
                                           [--mode gini | --mode trim --c 0]

Writes OUT_DIR/preview.npy and OUT_DIR/robust.npy, (height, width, 3) uint8 RGB, top row first, OUT_DIR/gini.npy, (height, width)
float32, and OUT_DIR/kept.npy, (height, width) int32 (numpy.load reads them)."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch  # noqa: F401  (before the library: it then binds to torch's HIP runtime)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import film_robust, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out_dir", type=Path)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--divisions", type=int, default=5)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--buckets", type=int, default=film_robust.BUCKETS)
    ap.add_argument("--mode", choices=film_robust.MODES, default="gini")
    ap.add_argument("--c", type=int, default=None, help='under --mode trim: the half-width of the kept centre, 0 the median bucket')
    a = ap.parse_args()
    a.out_dir.mkdir(parents=True, exist_ok=True)
    sph, rq = scenes.config("c2")
    strips = [rt.default_request(width=a.width, height=a.height, divisions=a.divisions, division_no=k, spp=a.spp,
                                 max_bounces=rq.max_bounces, seed=rq.seed) for k in range(a.divisions)]
    with rt.Scene(0, rt.World(sph)) as scene:
        with rt.Film(scene, strips, integrator="path") as film, \
                rt.FilmRobust(film, buckets=a.buckets, mode=a.mode, c=a.c) as robust:
            film.render_pass(0, a.spp)
            with torch.cuda.stream(film.stream):           # (the robust preview below writes the film's output tensor again)
                plain = film.preview()["rgb"].clone()
            out = robust.preview()["rgb"]
            planes = robust.estimate(("gini", "kept"))
            film.sync()                                    # the film's stream: .cpu() below copies on torch's current one
            kept = planes["kept"].cpu().numpy()
            np.save(a.out_dir / "preview.npy", plain.cpu().numpy())
            np.save(a.out_dir / "robust.npy", out.cpu().numpy())
            np.save(a.out_dir / "gini.npy", planes["gini"].cpu().numpy())
            np.save(a.out_dir / "kept.npy", kept)
            print(f"{a.out_dir}: preview.npy, robust.npy, gini.npy, kept.npy after {film.samples} samples in {a.buckets} buckets: "
                  f"{kept.mean():.2f} buckets kept a pixel, {(kept < a.buckets).mean() * 100:.1f} % of the pixels trimmed")


if __name__ == "__main__":
    main()
