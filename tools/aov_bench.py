#!/usr/bin/env python3
"""Throughput of the feature buffers of a strip (rt_scene_render_aovs_device): a 3840 x 2160 frame in 8 strips at
8 spp on c3 (rand1024), c5 (rand65536) and the 100 352-triangle mesh, every plane, one launch of the 8 strips.  Device buffers
(torch, on a stream of its own), the HIP-event time the library records around each launch (rt_scene_collect kernel_ms), after
warm-up launches; best and median of --runs.  Camera rays per second, exact root tests per ray, and the ratio to the beauty frame
of the same requests (rt_scene_render_tiles_device, one pass, timed the same way).

    python tools/aov_bench.py [--runs 5] [--warmup 2] [--spp 8] [--scenes c3,c5,mesh] [--aperture A]

--aperture replaces the reference's 0.1 (0: a pinhole, every sample's ray starts at the origin) to separate the lens's effect on
ray coherence from the rest.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch                                     # first: the library then binds to torch's HIP runtime

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import ray_tracer_s8_amd as rt                   # noqa: E402
from ray_tracer_s8_amd import _abi, scenes       # noqa: E402


def timed(launch, sc, runs, warmup):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    sc.collect()
    ms = []
    for _ in range(runs):
        launch()
        st = sc.collect()
        assert st.n_launches == 1, st.n_launches
        ms.append(st.kernel_ms)
    return min(ms), float(np.median(ms)), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--scenes", default="c3,c5,mesh")
    ap.add_argument("--aperture", type=float, default=None)
    a = ap.parse_args()
    rt.init()
    W, H, DIV = 3840, 2160, 8
    hs = H // DIV
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev).cuda_stream      # (not torch's default stream: that is the null stream, handle 0)
    lens = "the reference's aperture" if a.aperture is None else f"aperture {a.aperture}"
    print(f"# {W}x{H} in {DIV} strips, spp {a.spp}, {lens}, every plane; best / median of {a.runs} runs after {a.warmup} warm-up launches")
    print(f"{'scene':6} {'engine':>6} {'best ms':>9} {'median ms':>9} {'Mrays/s':>9} {'tests/ray':>9} {'beauty ms':>9} {'aov/beauty':>10}")
    for name in a.scenes.split(","):
        sph, tri, rq0 = scenes.config_world(name)
        reqs = []
        for k in range(DIV):
            rq = _abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=a.spp, max_bounces=rq0.max_bounces,
                                      seed=rq0.seed)
            if a.aperture is not None:
                rq.aperture = a.aperture
            reqs.append(rq)
        with rt.Scene(0, rt.World(sph, tri)) as sc:
            planes = [{"albedo": torch.empty((hs, W, 3), dtype=torch.float32, device=dev),
                       "normal": torch.empty((hs, W, 3), dtype=torch.float32, device=dev),
                       "depth": torch.empty((hs, W), dtype=torch.float32, device=dev),
                       "hits": torch.empty((hs, W), dtype=torch.int32, device=dev),
                       "index": torch.empty((hs, W), dtype=torch.int32, device=dev)} for _ in reqs]
            ptrs = [{k: v.data_ptr() for k, v in p.items()} for p in planes]
            rgb = [torch.empty(hs * W * 3, dtype=torch.uint8, device=dev) for _ in reqs]
            torch.cuda.synchronize()
            best, med, st = timed(lambda: sc.render_aovs_device(reqs, 0, a.spp, ptrs, stream=stream), sc, a.runs, a.warmup)
            rays = DIV * hs * W * a.spp
            assert st.primary_rays == st.ray_segments == rays
            tests = st.broad_candidates / rays
            engine = st.engine
            b_best, _, _ = timed(lambda: sc.render_tiles_device(reqs, [t.data_ptr() for t in rgb], hs * W * 3, stream=stream), sc,
                                 a.runs, a.warmup)
            print(f"{name:6} {engine:6d} {best:9.2f} {med:9.2f} {rays / best / 1e3:9.0f} {tests:9.2f} {b_best:9.2f} {best / b_best:10.3f}",
                  flush=True)
            del planes, rgb
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
