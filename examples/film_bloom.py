#!/usr/bin/env python3
"""Orbit the c2 box (scenes.cornell16) as examples/film_display.py does, and show every frame through a display with and without a
bloom in front of it (ray_tracer_s8_amd.FilmBloom): the frame's variance-guided resolve, as a linear image, goes
through the pyramid bloom, and both the plain and the bloomed image are metered and tone-mapped by a display of their own.  The lamp
is the only thing above white in the box: with the bloom it has a glow on the ceiling around it.

    python examples/film_bloom.py [--frames 8] [--width 480 --height 270 --divisions 5] [--spp 8] [--strength 0.1] [--spread 0.7]
                                  [--mode mix] [--threshold 0] [--out film_bloom]

Writes OUT_bloom.npy and OUT_plain.npy, (frames, height, width, 3) uint8 RGB, top row first: every frame as the display shows it with
and without the bloom (numpy.load reads them)."""
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
    ap.add_argument("--orbit", type=int, default=24, help="viewpoints of the whole circle; the frames are its first ones")
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--divisions", type=int, default=5)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--strength", type=float, default=0.1)
    ap.add_argument("--spread", type=float, default=0.7)
    ap.add_argument("--mode", default="mix", choices=("mix", "add"))
    ap.add_argument("--threshold", type=float, default=0.0)
    ap.add_argument("--out", default="film_bloom")
    a = ap.parse_args()
    sph, rq = scenes.config("c2")
    strips = [rt.default_request(width=a.width, height=a.height, divisions=a.divisions, division_no=k, spp=a.spp,
                                 max_bounces=rq.max_bounces, seed=rq.seed) for k in range(a.divisions)]
    bloomed, plain = [], []
    with rt.Scene(0, rt.World(sph)) as scene:
        scene.set_light_sampling(rt.RT_LIGHTS_CONE)
        scene.set_glossy_sampling(rt.RT_GLOSSY_MIS)
        with rt.Film(scene, strips, integrator="nee", mode=rt.RT_NEE_MIS, moments=True) as film, \
                rt.FilmBloom(film, spread=a.spread, strength=a.strength, mode=a.mode, threshold=a.threshold) as bloom, \
                rt.FilmDisplay(film, rate=0.25) as with_bloom, rt.FilmDisplay(film, rate=0.25) as without:
            for i in range(a.frames):
                scene.set_camera(orbit_camera(i, a.orbit))
                film.reset(seed=rq.seed + i)                 # a seed per frame
                film.render_pass(0, a.spp)
                planes = film.features(1, ("normal", "depth", "hits"))
                linear = film.resolve_guided(planes, ("linear",))["linear"]
                glow = with_bloom.display(bloom.apply(linear)["linear"])["rgb"]
                flat = without.display(linear)["rgb"]
                film.sync()                                  # (the copies below are then safe)
                bloomed.append(glow.cpu().numpy())
                plain.append(flat.cpu().numpy())
    np.save(f"{a.out}_bloom.npy", np.stack(bloomed))
    np.save(f"{a.out}_plain.npy", np.stack(plain))
    white = lambda frames: 100.0 * float((np.stack(frames) == 255).mean())
    moved = 100.0 * float((np.stack(bloomed) != np.stack(plain)).any(-1).mean())
    print(f"{a.out}_bloom.npy, {a.out}_plain.npy: {a.frames} frames at {a.spp} samples each, {bloom.settings.levels} levels; "
          f"at code 255: {white(plain):.2f} % of the plain bytes, {white(bloomed):.2f} % with the bloom; {moved:.1f} % of the pixels differ")


if __name__ == "__main__":
    main()
