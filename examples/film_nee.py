#!/usr/bin/env python3
"""Orbit the c2 box (scenes.cornell16) and write one lit, denoised frame per viewpoint, without a host round trip until the frame is
done: the film (ray_tracer_s8_amd.Film) makes the tile's camera rays on the device, traces them with next-event estimation
(RT_NEE_MIS, sphere lights sampled over their cone, light samples at glossy hits too), folds the samples into its running sum in
progressive passes, renders the feature buffers and hands both to the a-trous denoiser.

    python examples/film_nee.py [--frames 4] [--width 480 --height 270 --divisions 5] [--spp 8] [--pass-spp 4] [--out film_nee]

Writes OUT_000.npy, OUT_001.npy, ...: (height, width, 3) uint8 RGB, top row first (numpy.load reads them)."""
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
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--divisions", type=int, default=5)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--pass-spp", type=int, default=4)
    ap.add_argument("--out", default="film_nee")
    a = ap.parse_args()
    sph, rq = scenes.config("c2")
    strips = [rt.default_request(width=a.width, height=a.height, divisions=a.divisions, division_no=k, spp=a.spp,
                                 max_bounces=rq.max_bounces, seed=rq.seed) for k in range(a.divisions)]
    with rt.Scene(0, rt.World(sph)) as scene:
        scene.set_light_sampling(rt.RT_LIGHTS_CONE)
        scene.set_glossy_sampling(rt.RT_GLOSSY_MIS)
        with rt.Film(scene, strips, integrator="nee", mode=rt.RT_NEE_MIS) as film:
            for i in range(a.frames):
                scene.set_camera(orbit_camera(i, a.frames))
                film.reset()
                for samples in film.render_progressive(a.pass_spp):
                    pass                                   # (film.preview() here shows the frame as it converges)
                out = film.resolve(planes=film.features(1), outputs=("rgb",))
                film.sync()                                # the film's stream: .cpu() below copies on torch's current one
                path = f"{a.out}_{i:03d}.npy"
                np.save(path, out["rgb"].cpu().numpy())
                st = film.collect()
                print(f"{path}: {samples} samples, {st.ray_segments} ray segments in {st.n_launches} launches, {st.kernel_ms:.2f} ms of kernels")


if __name__ == "__main__":
    main()
