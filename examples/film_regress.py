#!/usr/bin/env python3
"""Render the c2 box (scenes.cornell16) at 8 samples per pixel with next-event estimation on a film that keeps per-pixel sample
moments (ray_tracer_s8_amd.Film(moments=True)), and write the same frame reconstructed three ways: by the a-trous denoiser
(Film.resolve), by the variance-guided a-trous (Film.resolve_guided) and by the local feature regression (Film.resolve_regression),
which fits the colour, window by window, as a linear function of the albedo-demodulated frame's normal, depth and position.

    python examples/film_regress.py OUT_DIR [--width 480 --height 270 --divisions 5] [--spp 8]

Writes OUT_DIR/resolve.npy, OUT_DIR/resolve_guided.npy and OUT_DIR/resolve_regression.npy, (height, width, 3) uint8 RGB, top row
first (numpy.load reads them)."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch  # noqa: F401  (before the library: it then binds to torch's HIP runtime)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out_dir", type=Path)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--divisions", type=int, default=5)
    ap.add_argument("--spp", type=int, default=8)
    a = ap.parse_args()
    a.out_dir.mkdir(parents=True, exist_ok=True)
    sph, rq = scenes.config("c2")
    strips = [rt.default_request(width=a.width, height=a.height, divisions=a.divisions, division_no=k, spp=a.spp,
                                 max_bounces=rq.max_bounces, seed=rq.seed) for k in range(a.divisions)]
    with rt.Scene(0, rt.World(sph)) as scene:
        scene.set_light_sampling(rt.RT_LIGHTS_CONE)
        scene.set_glossy_sampling(rt.RT_GLOSSY_MIS)
        with rt.Film(scene, strips, integrator="nee", mode=rt.RT_NEE_MIS, moments=True) as film:
            film.render_pass(0, a.spp)
            planes = film.features(1)
            guide = {n: planes[n] for n in ("normal", "depth", "hits")}        # (the guided filter takes no albedo)
            plain = film.resolve(planes=guide, outputs=("rgb",))
            guided = film.resolve_guided(guide, outputs=("rgb",))
            fitted = film.resolve_regression({n: planes[n] for n in ("albedo", "normal", "depth", "hits")}, outputs=("rgb",))
            film.sync()                                    # the film's stream: .cpu() below copies on torch's current one
            np.save(a.out_dir / "resolve.npy", plain["rgb"].cpu().numpy())
            np.save(a.out_dir / "resolve_guided.npy", guided["rgb"].cpu().numpy())
            np.save(a.out_dir / "resolve_regression.npy", fitted["rgb"].cpu().numpy())
            solved = int(film.regression_model[..., 27].sum().item())
            print(f"{a.out_dir}: resolve.npy, resolve_guided.npy, resolve_regression.npy after {film.samples} samples "
                  f"({solved} of {film.regression_model.shape[0] * film.regression_model.shape[1]} nodes fitted)")


if __name__ == "__main__":
    main()
