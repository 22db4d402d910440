#!/usr/bin/env python3
"""Orbit the c2 box (scenes.cornell16) as examples/film_temporal.py does, and show every frame through a display
(ray_tracer_s8_amd.FilmDisplay): the frame's variance-guided resolve, as a linear image, is metered, its exposure
follows the frames at rate 0.25, and the filmic curve compresses what the plain rgb clips: the lamp and the walls beside it.

    python examples/film_display.py [--frames 8] [--width 480 --height 270 --divisions 5] [--spp 8] [--curve filmic] [--dither]
                                    [--out film_display]

Writes OUT_display.npy and OUT_plain.npy, (frames, height, width, 3) uint8 RGB, top row first: every frame as the display shows it
and as the film's own rgb does; and OUT_scale.npy, (frames,) float32, the scale of every frame (numpy.load reads them)."""
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
    ap.add_argument("--curve", default="filmic", choices=("none", "reinhard", "filmic"))
    ap.add_argument("--dither", action="store_true")
    ap.add_argument("--out", default="film_display")
    a = ap.parse_args()
    sph, rq = scenes.config("c2")
    strips = [rt.default_request(width=a.width, height=a.height, divisions=a.divisions, division_no=k, spp=a.spp,
                                 max_bounces=rq.max_bounces, seed=rq.seed) for k in range(a.divisions)]
    shown, plain, scales = [], [], []
    with rt.Scene(0, rt.World(sph)) as scene:
        scene.set_light_sampling(rt.RT_LIGHTS_CONE)
        scene.set_glossy_sampling(rt.RT_GLOSSY_MIS)
        with rt.Film(scene, strips, integrator="nee", mode=rt.RT_NEE_MIS, moments=True) as film, \
                rt.FilmDisplay(film, curve=a.curve, rate=0.25, dither=a.dither) as display:
            for i in range(a.frames):
                scene.set_camera(orbit_camera(i, a.orbit))
                film.reset(seed=rq.seed + i)                 # a seed per frame
                film.render_pass(0, a.spp)
                planes = film.features(1, ("normal", "depth", "hits"))
                out = film.resolve_guided(planes, ("linear", "rgb"))
                rgb = display.display(out["linear"])["rgb"]
                scales.append(display.exposure()["scale"])   # (waits for the film's stream: the copies below are then safe)
                shown.append(rgb.cpu().numpy())
                plain.append(out["rgb"].cpu().numpy())
    np.save(f"{a.out}_display.npy", np.stack(shown))
    np.save(f"{a.out}_plain.npy", np.stack(plain))
    np.save(f"{a.out}_scale.npy", np.array(scales, np.float32))
    white = lambda frames: 100.0 * float((np.stack(frames) == 255).mean())
    print(f"{a.out}_display.npy, {a.out}_plain.npy, {a.out}_scale.npy: {a.frames} frames at {a.spp} samples each, scale "
          f"{min(scales):.3f} ... {max(scales):.3f}; at code 255: {white(plain):.2f} % of the plain rgb, {white(shown):.2f} % of the display's")


if __name__ == "__main__":
    main()
