#!/usr/bin/env python3
"""A wavefront loop of path steps against the one-kernel trace (rt_scene_bounce_device against rt_scene_trace_device):
the rays of tools/trace_bench.py (2^20 pinhole camera rays through the jittered pixels of a 1280 x 720 frame, and a second pose) on
c3 (rand1024), c5 (rand65536) and the 100 352-triangle mesh, 8 bounces, one sample.  Timed with HIP events on one stream of its own:
  loop   bounces + 1 steps, the next list of one step the active list of the following one, all lengths read on the device (no host
         synchronisation between the steps); the rays and states are restored before every run (device-to-device copies, outside the
         timed region);
  trace  rt_scene_trace_device at spp = 1 with the same rays and states.
Best and median of --runs after --warmup; the rays stepped at every step are read back once, after the timed runs.

    python tools/bounce_bench.py [--runs 5] [--warmup 2] [--rays-log2 20] [--bounces 8] [--scenes c3,c5,mesh]
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
from trace_bench import second_pose              # noqa: E402


def timed(stream, fn, runs, warmup, before):
    """Best and median HIP-event time (ms) of fn() on `stream`, before() run ahead of each one outside the timed region."""
    ms = []
    for k in range(warmup + runs):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    return min(ms), float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rays-log2", type=int, default=20)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--scenes", default="c3,c5,mesh")
    a = ap.parse_args()
    rt.init()
    n, K = 1 << a.rays_log2, a.bounces + 1
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)      # (not torch's default stream: that is the null stream, handle 0)
    sp = stream.cuda_stream
    print(f"# {n} rays, {a.bounces} bounces ({K} steps), one sample, best / median of {a.runs} runs after {a.warmup} warm-ups")
    print(f"{'scene':6} {'camera':7} {'loop ms':>8} {'median':>8} {'trace ms':>8} {'median':>8} {'loop/trace':>10} {'segments':>9}  rays stepped per step")
    g = np.random.default_rng(1)
    states = torch.from_numpy(g.integers(1, 1 << 62, size=(n, 4), dtype=np.int64)).to(dev)
    for name in a.scenes.split(","):
        sph, tri, _ = scenes.config_world(name)
        with rt.Scene(0, rt.World(sph, tri)) as sc:
            o, d = camera_rays(n, W=1280, H=720)
            for pose, (po, pd) in {"default": (o, d), "second": second_pose(o, d)}.items():
                rays0 = torch.from_numpy(pack(po, pd).view(np.float32).reshape(n, 8)).to(dev)
                rays, st = torch.empty_like(rays0), torch.empty_like(states)
                bounce = torch.empty((n, 4), dtype=torch.float32, device=dev)
                rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
                lists = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
                counts = torch.zeros(K, dtype=torch.int32, device=dev)      # one length word per step: all readable afterwards
                torch.cuda.synchronize()

                def restore():
                    with torch.cuda.stream(stream):
                        rays.copy_(rays0)
                        st.copy_(states)

                def loop():
                    for k in range(K):
                        sc.bounce_device(rays.data_ptr(), n, st.data_ptr(), bounce.data_ptr(),
                                         d_active=lists[(k + 1) % 2].data_ptr() if k else 0,
                                         d_n_active=counts[k - 1:].data_ptr() if k else 0,
                                         d_next_active=lists[k % 2].data_ptr(), d_n_next=counts[k:].data_ptr(), as_given=k > 0, stream=sp)

                def trace():
                    sc.trace_device(rays.data_ptr(), n, rgb.data_ptr(), d_rng_state=st.data_ptr(), spp=1, max_bounces=a.bounces, stream=sp)

                lb, lm = timed(stream, loop, a.runs, a.warmup, restore)
                stepped = [n] + counts.cpu().numpy()[:-1].tolist()
                loop_segments = sc.collect().ray_segments // (a.runs + a.warmup)
                tb, tm = timed(stream, trace, a.runs, a.warmup, restore)
                segs = sc.collect().ray_segments // (a.runs + a.warmup)
                assert loop_segments == segs == sum(stepped), (loop_segments, segs, stepped)
                print(f"{name:6} {pose:7} {lb:8.2f} {lm:8.2f} {tb:8.2f} {tm:8.2f} {lb / tb:10.2f} {segs:9d}  {stepped}", flush=True)
                del rays0, rays, st, bounce, rgb, lists, counts
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
