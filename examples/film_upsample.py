#!/usr/bin/env python3
"""Render the c2 box (scenes.cornell16) with next-event estimation on a film of a half (or a third, a quarter) of the frame's
resolution and reconstruct the full frame from it (ray_tracer_s8_amd.FilmUpsampler): the feature buffers are rendered at both
resolutions, one sample each, and steer a joint-bilateral upsampling of the film's resolve, with the albedo divided out of the
low-resolution colour and the full-resolution albedo multiplied back in.  Writes the upsampled resolve, the plain bilinear one (no
planes) for comparison, and the class plane: 1 where no tap of a pixel was admitted and it is the bilinear value.

    python examples/film_upsample.py OUT_DIR [--width 480 --height 270 --divisions 5] [--scale 2] [--spp 8]

--width and --height are the film's; the frame written is --scale times as large.  Writes OUT_DIR/upsampled.npy and
OUT_DIR/bilinear.npy, (scale height, scale width, 3) uint8 RGB, top row first, and OUT_DIR/class.npy, (scale height, scale width) uint8
(numpy.load reads them)."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch  # noqa: F401  (before the library: it then binds to torch's HIP runtime)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import film_upsampler, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out_dir", type=Path)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--divisions", type=int, default=5)
    ap.add_argument("--scale", type=int, default=2, choices=(2, 3, 4))
    ap.add_argument("--spp", type=int, default=8, help="the samples of every pixel of the low-resolution film")
    a = ap.parse_args()
    a.out_dir.mkdir(parents=True, exist_ok=True)
    sph, rq = scenes.config("c2")
    strips = lambda s: [rt.default_request(width=s * a.width, height=s * a.height, divisions=a.divisions, division_no=k, spp=a.spp,
                                           max_bounces=rq.max_bounces, seed=rq.seed) for k in range(a.divisions)]
    with rt.Scene(0, rt.World(sph)) as scene:
        scene.set_light_sampling(rt.RT_LIGHTS_CONE)
        scene.set_glossy_sampling(rt.RT_GLOSSY_MIS)
        with rt.Film(scene, strips(1), integrator="nee", mode=rt.RT_NEE_MIS) as film, \
                rt.FilmUpsampler(film, strips(a.scale)) as up:
            film.render_pass(0, a.spp)
            planes = film.features(1, film_upsampler.PLANES)           # the low-resolution planes, index among them
            up.features(1)                                             # the full-resolution ones
            guide = {n: planes[n] for n in ("albedo", "normal", "depth", "hits")}
            out = up.resolve("resolve", outputs=("rgb", "class"), planes=guide)
            film.sync()                                    # the film's stream: .cpu() below copies on torch's current one
            upsampled, cls = out["rgb"].cpu().numpy(), out["class"].cpu().numpy()
            linear = film.resolve(planes=guide, outputs=("linear",))["linear"]
            bilinear = up.upsample(linear, planes_lo={}, planes_hi={}, outputs=("rgb",))["rgb"]
            film.sync()
            np.save(a.out_dir / "upsampled.npy", upsampled)
            np.save(a.out_dir / "bilinear.npy", bilinear.cpu().numpy())
            np.save(a.out_dir / "class.npy", cls)
            print(f"{a.out_dir}: upsampled.npy, bilinear.npy, class.npy: {a.width} x {a.height} at {film.samples} samples to "
                  f"{up.width} x {up.rows}, {100.0 * cls.mean():.2f} % of the pixels by the bilinear fall-back")


if __name__ == "__main__":
    main()
