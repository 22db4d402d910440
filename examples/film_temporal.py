#!/usr/bin/env python3
"""Orbit the c2 box (scenes.cornell16) as examples/film_nee.py does, and carry a history from frame to frame
(ray_tracer_s8_amd.FilmHistory): every frame's colour sums and moments are blended with the last frame's, reprojected
by the frame's depth and the two camera poses, before the variance-guided resolve.

Every frame gets a seed of its own (film.reset(seed=...)).  A sample's stream depends on (seed, pixel, sample) only, so without it a
camera that stands still would render the same bytes again and a history of identical frames would gain nothing.

    python examples/film_temporal.py [--frames 8] [--width 480 --height 270 --divisions 5] [--spp 8] [--out film_temporal]
                                     [--clip G [--clip-radius 1] [--alpha A]]

--clip G clips the reprojected history of every pixel to mean +- G standard deviations of the frame's colours around it before the
blend, which lets a longer memory (--alpha below the default) keep less of what the frame no longer shows.

Writes OUT_single.npy and OUT_history.npy: the last frame resolved from its own samples alone and from the history, (height, width, 3)
uint8 RGB, top row first (numpy.load reads them)."""
import argparse
import math
import sys
from pathlib import Path

import numpy as np
import torch  # noqa: F401  (before the library: it then binds to torch's HIP runtime)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import scenes  # noqa: E402


def orbit_camera(i: int, n: int) -> rt.Camera:
    """Viewpoint i of n: the eye on a circle in front of the box's open side, looking at the spheres on its floor."""
    a = 2.0 * math.pi * i / max(n, 1)
    return rt.Camera.look_at((1.2 * math.sin(a), 0.3 + 0.4 * math.cos(a), 0.2), (0.0, -0.8, -4.0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--orbit", type=int, default=96, help="viewpoints of the whole circle; the frames are its first ones")
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--divisions", type=int, default=5)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--out", default="film_temporal")
    ap.add_argument("--clip", type=float, default=None, metavar="G", help="clip the history to the frame's colour box of G deviations")
    ap.add_argument("--clip-radius", type=int, default=1, choices=(1, 2), help="the radius of the box's window, with --clip")
    ap.add_argument("--alpha", type=float, default=None, help="the history's alpha (default: FilmHistory's)")
    a = ap.parse_args()
    sph, rq = scenes.config("c2")
    strips = [rt.default_request(width=a.width, height=a.height, divisions=a.divisions, division_no=k, spp=a.spp,
                                 max_bounces=rq.max_bounces, seed=rq.seed) for k in range(a.divisions)]
    with rt.Scene(0, rt.World(sph)) as scene:
        scene.set_light_sampling(rt.RT_LIGHTS_CONE)
        scene.set_glossy_sampling(rt.RT_GLOSSY_MIS)
        options = {} if a.alpha is None else {"alpha": a.alpha}
        if a.clip is not None:
            options.update(clip=a.clip, clip_radius=a.clip_radius)
        with rt.Film(scene, strips, integrator="nee", mode=rt.RT_NEE_MIS, moments=True) as film, \
                rt.FilmHistory(film, **options) as history:
            for i in range(a.frames):
                camera = orbit_camera(i, a.orbit)
                scene.set_camera(camera)
                film.reset(seed=rq.seed + i)                 # a seed per frame
                film.render_pass(0, a.spp)
                planes = film.features(1, ("normal", "depth", "hits", "index"))
                history.accumulate(camera, planes)
            guide = {n: planes[n] for n in ("normal", "depth", "hits")}
            with torch.cuda.stream(film.stream):             # (the two resolves share the film's output tensor)
                single = film.resolve_guided(guide)["rgb"].clone()
            resolved = history.resolve_guided(guide)["rgb"]
            film.sync()                                      # the film's stream: .cpu() below copies on torch's current one
            length = history.length.cpu().numpy()
            clipped = "" if a.clip is None else f", {100.0 * (history.clip_amount.cpu().numpy() > 0).mean():.1f} % clipped in the last frame"
            np.save(f"{a.out}_single.npy", single.cpu().numpy())
            np.save(f"{a.out}_history.npy", resolved.cpu().numpy())
            print(f"{a.out}_single.npy, {a.out}_history.npy: frame {a.frames - 1} of {a.frames} at {a.spp} samples each, "
                  f"mean history length {length.mean():.2f}, {100.0 * (length > 1).mean():.1f} % of the pixels with history{clipped}")


if __name__ == "__main__":
    main()
