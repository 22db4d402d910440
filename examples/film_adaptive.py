#!/usr/bin/env python3
"""Render the c2 box (scenes.cornell16) with next-event estimation on a film that keeps per-pixel sample moments: a floor of uniform
samples for every pixel, then adaptive rounds (ray_tracer_s8_amd.FilmSampler) that give further samples only to the pixels whose
moments say they are still noisy.  Writes the variance-guided resolve of the sampler's sums, the number of samples every pixel got
and the error plane the last round decided from.

    python examples/film_adaptive.py OUT_DIR [--width 480 --height 270 --divisions 5] [--spp 32 --floor 4 --round 4]
                                             [--threshold T --dilate 1]

Writes OUT_DIR/resolve.npy, (height, width, 3) uint8 RGB, top row first, OUT_DIR/counts.npy, (height, width) int32, and
OUT_DIR/err.npy, (height, width) float32 (numpy.load reads them)."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch  # noqa: F401  (before the library: it then binds to torch's HIP runtime)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import film_sampler, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out_dir", type=Path)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--divisions", type=int, default=5)
    ap.add_argument("--spp", type=int, default=32, help="the most samples a pixel can get")
    ap.add_argument("--floor", type=int, default=4, help="the uniform samples every pixel gets first (at least 2)")
    ap.add_argument("--round", type=int, default=4, help="the sample indices of an adaptive round")
    ap.add_argument("--threshold", type=float, default=film_sampler.THRESHOLD)
    ap.add_argument("--dilate", type=int, default=film_sampler.DILATE)
    a = ap.parse_args()
    a.out_dir.mkdir(parents=True, exist_ok=True)
    sph, rq = scenes.config("c2")
    strips = [rt.default_request(width=a.width, height=a.height, divisions=a.divisions, division_no=k, spp=a.spp,
                                 max_bounces=rq.max_bounces, seed=rq.seed) for k in range(a.divisions)]
    with rt.Scene(0, rt.World(sph)) as scene:
        scene.set_light_sampling(rt.RT_LIGHTS_CONE)
        scene.set_glossy_sampling(rt.RT_GLOSSY_MIS)
        with rt.Film(scene, strips, integrator="nee", mode=rt.RT_NEE_MIS, moments=True) as film, \
                rt.FilmSampler(film, threshold=a.threshold, dilate=a.dilate) as sampler:
            film.render_pass(0, min(a.floor, a.spp))
            sampler.begin()
            rounds = sampler.render(a.round)
            planes = film.features(1)
            guide = {n: planes[n] for n in ("normal", "depth", "hits")}        # (the guided filter takes no albedo)
            out = sampler.resolve_guided(guide, outputs=("rgb",))
            film.sync()                                    # the film's stream: .cpu() below copies on torch's current one
            counts = sampler.counts.cpu().numpy()
            np.save(a.out_dir / "resolve.npy", out["rgb"].cpu().numpy())
            np.save(a.out_dir / "counts.npy", counts)
            np.save(a.out_dir / "err.npy", sampler.error.cpu().numpy())
            print(f"{a.out_dir}: resolve.npy, counts.npy, err.npy after a floor of {film.samples} samples and {rounds} rounds: "
                  f"{counts.mean():.2f} samples a pixel, {counts.min()} to {counts.max()}")


if __name__ == "__main__":
    main()
