#!/usr/bin/env python3
"""Path-tracing throughput of caller rays (rt_scene_trace_device): ray segments/s on c3 (rand1024), c5 (rand65536) and
the 100 352-triangle mesh, for the pinhole camera rays of tools/query_bench.py (the reference camera at the origin looking down -z)
through the jittered pixels of a 1280 x 720 frame in pixel order (2^20 rays: the whole frame and the top of a second pass; the first
2^20 pixels of a 4K frame would be its top 273 rows, all sky for the mesh) and for a second pose (moved up and back, turned 20 degrees left and 15 degrees down), spp 8, 8 bounces, the seeded streams.
Device buffers (torch, on a stream of its own), the HIP-event time the library records around each launch (rt_scene_collect
kernel_ms), warmed up; best and median of --runs.

    python tools/trace_bench.py [--runs 5] [--warmup 2] [--rays-log2 20] [--spp 8] [--bounces 8] [--scenes c3,c5,mesh]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch                                     # first: the library then binds to torch's HIP runtime

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import ray_tracer_s8_amd as rt                   # noqa: E402
from ray_tracer_s8_amd import scenes             # noqa: E402
from query_bench import camera_rays, pack        # noqa: E402


def second_pose(o, d, yaw_deg=20.0, pitch_deg=-15.0, eye=(0.0, 1.5, 1.0)):
    """The same rays from another pinhole: origins moved to `eye`, directions turned by yaw (about y) then pitch (about x)."""
    cy, sy = np.cos(np.radians(yaw_deg)), np.sin(np.radians(yaw_deg))
    cp, sp = np.cos(np.radians(pitch_deg)), np.sin(np.radians(pitch_deg))
    yaw = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    pitch = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    r = (yaw @ pitch).astype(np.float32)
    return np.broadcast_to(np.asarray(eye, np.float32), o.shape).copy(), (d @ r.T).astype(np.float32)


def time_trace(sc, d_rays, n, d_rgb, args, runs, warmup, stream):
    kw = dict(spp=args.spp, max_bounces=args.bounces, seed=1, stream=stream)
    for _ in range(warmup):
        sc.trace_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), **kw)
    torch.cuda.synchronize()
    sc.collect()
    ms, segs, tests = [], 0, 0
    for _ in range(runs):
        sc.trace_device(d_rays.data_ptr(), n, d_rgb.data_ptr(), **kw)
        st = sc.collect()
        assert st.n_launches == 1 and st.primary_rays == n * args.spp
        ms.append(st.kernel_ms)
        segs = st.ray_segments                      # (the same every run: the seeded streams)
        tests += st.broad_candidates
    return min(ms), float(np.median(ms)), st.engine, segs, tests / (runs * segs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rays-log2", type=int, default=20)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--scenes", default="c3,c5,mesh")
    a = ap.parse_args()
    rt.init()
    n = 1 << a.rays_log2
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev).cuda_stream      # (not torch's default stream: that is the null stream, handle 0)
    print(f"# {n} rays per launch, spp {a.spp}, {a.bounces} bounces, best / median of {a.runs} runs after {a.warmup} warm-up launches")
    print(f"{'scene':6} {'camera':7} {'engine':>6} {'best ms':>9} {'median ms':>9} {'segs/ray':>8} {'Gsegs/s':>8} {'tests/seg':>9}")
    for name in a.scenes.split(","):
        sph, tri, _ = scenes.config_world(name)
        with rt.Scene(0, rt.World(sph, tri)) as sc:
            o, d = camera_rays(n, W=1280, H=720)
            poses = {"default": (o, d), "second": second_pose(o, d)}
            d_rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
            for pose, (po, pd) in poses.items():
                d_rays = torch.from_numpy(pack(po, pd).view(np.float32).reshape(n, 8)).to(dev)
                torch.cuda.synchronize()                       # (the upload ran on torch's stream)
                best, med, engine, segs, tests = time_trace(sc, d_rays, n, d_rgb, a, a.runs, a.warmup, stream)
                print(f"{name:6} {pose:7} {engine:6d} {best:9.2f} {med:9.2f} {segs / n:8.2f} {segs / best / 1e6:8.3f} {tests:9.2f}",
                      flush=True)
                del d_rays
            del d_rgb
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
