#!/usr/bin/env python3
"""Orbit the c2 box (scenes.cornell16) as examples/film_display.py does, and deliver every displayed frame as the reference's
controller does, as a JPEG, encoded on the device (ray_tracer_s8_amd.FrameEncoder): the frame goes from the film
through the display into the encoder without leaving device memory, and only the file's bytes are copied to the host.

    python examples/film_jpeg.py [--frames 8] [--width 480 --height 270 --divisions 5] [--spp 8] [--quality 90] [--interval N]
                                 [--out film_jpeg]

Writes OUT_000.jpg ... (baseline JFIF, 4:4:4, restart intervals of 16 MCUs unless --interval says otherwise)."""
import argparse
import math
import sys
from pathlib import Path

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
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--interval", type=int, default=None, help="MCUs a restart interval (default: FrameEncoder's, 16)")
    ap.add_argument("--out", default="film_jpeg")
    a = ap.parse_args()
    sph, rq = scenes.config("c2")
    strips = [rt.default_request(width=a.width, height=a.height, divisions=a.divisions, division_no=k, spp=a.spp,
                                 max_bounces=rq.max_bounces, seed=rq.seed) for k in range(a.divisions)]
    sizes = []
    with rt.Scene(0, rt.World(sph)) as scene:
        scene.set_light_sampling(rt.RT_LIGHTS_CONE)
        scene.set_glossy_sampling(rt.RT_GLOSSY_MIS)
        with rt.Film(scene, strips, integrator="nee", mode=rt.RT_NEE_MIS, moments=True) as film, \
                rt.FilmDisplay(film, rate=0.25) as display, \
                rt.FrameEncoder(film, quality=a.quality, interval=a.interval) as encoder:
            for i in range(a.frames):
                scene.set_camera(orbit_camera(i, a.orbit))
                film.reset(seed=rq.seed + i)                 # a seed per frame
                film.render_pass(0, a.spp)
                planes = film.features(1, ("normal", "depth", "hits"))
                linear = film.resolve_guided(planes, ("linear",))["linear"]
                data = encoder.encode(display.display(linear)["rgb"])        # (waits for the film's stream: the only copy)
                Path(f"{a.out}_{i:03d}.jpg").write_bytes(data)
                sizes.append(len(data))
    raw = a.width * a.height * 3
    print(f"{a.out}_000.jpg ... {a.out}_{a.frames - 1:03d}.jpg: {a.frames} frames at {a.spp} samples each, quality {a.quality}, "
          f"{min(sizes)} ... {max(sizes)} bytes a file against {raw} of raw rgb")


if __name__ == "__main__":
    main()
