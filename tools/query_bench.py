#!/usr/bin/env python3
"""Ray-query throughput (rt_scene_intersect_device): Mrays/s of the closest-hit and any-hit queries on c3 (rand1024),
c5 (rand65536) and the 100 352-triangle mesh, for 2^24 coherent camera rays of the 4K frame and 2^24 incoherent diffuse bounce rays
from the first hits of those rays.  Device buffers (torch, on a stream of its own), the HIP-event time the library records around each
launch (rt_scene_collect kernel_ms), warmed up; best and median of --runs.

    python tools/query_bench.py [--runs 5] [--warmup 2] [--rays-log2 24] [--scenes c3,c5,mesh]
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


def camera_rays(n, W=3840, H=2160, seed=1):
    """Pinhole rays of the reference camera (camera.rs:19-47, focal length 1, fov pi/2) through jittered pixels of the W x H frame,
    in row-major pixel order (neighbouring rays are neighbouring pixels: coherent)."""
    g = np.random.default_rng(seed)
    aspect = np.float32(W / H)
    vh = np.float32(2.0 * np.tan(np.float32(np.pi) / 4))
    vw = aspect * vh
    pix = np.arange(n, dtype=np.int64) % (W * H)
    x = (pix % W).astype(np.float32) + g.random(n, dtype=np.float32)
    y = (H - 1 - pix // W).astype(np.float32) + g.random(n, dtype=np.float32)
    d = np.empty((n, 3), np.float32)
    d[:, 0] = -vw / 2 + x / np.float32(W - 1) * vw
    d[:, 1] = -vh / 2 + y / np.float32(H - 1) * vh
    d[:, 2] = -1.0
    return np.zeros((n, 3), np.float32), d


def pack(o, d, t_min=0.001, t_max=1000.0):
    r = np.empty(len(o), _abi.RAY_DTYPE)
    r["ox"], r["oy"], r["oz"] = o.T
    r["dx"], r["dy"], r["dz"] = d.T
    r["t_min"], r["t_max"] = t_min, t_max
    return r


def bounce_rays(hits, n, seed=2):
    """Diffuse bounces from the hit points: normal + a random unit vector (main.rs:125-133's Lambertian form), origin P."""
    g = np.random.default_rng(seed)
    h = hits[hits["index"] != _abi.RT_HIT_NONE]
    if len(h) == 0:
        raise RuntimeError("no camera ray hit anything")
    pick = np.arange(n) % len(h)
    h = h[pick]
    u = g.normal(size=(n, 3)).astype(np.float32)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = np.stack([h["px"], h["py"], h["pz"]], 1).astype(np.float32)
    d = np.stack([h["nx"], h["ny"], h["nz"]], 1).astype(np.float32) + u
    return o, d


def time_queries(sc, d_rays, n, d_hits, any_hit, runs, warmup, stream):
    """HIP-event time of each launch as the library records it on the launch's stream (rt_scene_collect: kernel_ms)."""
    for _ in range(warmup):
        sc.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), any_hit=any_hit, stream=stream)
    torch.cuda.synchronize()
    sc.collect()
    ms, tests = [], 0
    for _ in range(runs):
        sc.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), any_hit=any_hit, stream=stream)
        st = sc.collect()
        assert st.n_launches == 1 and st.primary_rays == n
        ms.append(st.kernel_ms)
        tests += st.broad_candidates
    return min(ms), float(np.median(ms)), st.engine, tests / (runs * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rays-log2", type=int, default=24)
    ap.add_argument("--scenes", default="c3,c5,mesh")
    a = ap.parse_args()
    rt.init()
    n = 1 << a.rays_log2
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev).cuda_stream      # (not torch's default stream: that is the null stream, handle 0)
    print(f"# {n} rays per launch, best / median of {a.runs} runs after {a.warmup} warm-up launches")
    print(f"{'scene':6} {'rays':9} {'mode':8} {'engine':>6} {'best ms':>9} {'median ms':>9} {'Mrays/s':>9} {'root tests/ray':>14}")
    for name in a.scenes.split(","):
        sph, tri, _ = scenes.config_world(name)
        with rt.Scene(0, rt.World(sph, tri)) as sc:
            o, d = camera_rays(n)
            cam = pack(o, d)
            d_rays = torch.from_numpy(cam.view(np.float32).reshape(n, 8)).to(dev)
            d_hits = torch.empty((n, 8), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()                           # (the uploads ran on torch's stream)
            sc.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            sc.collect()
            first = d_hits.cpu().numpy().view(_abi.HIT_DTYPE).reshape(n)
            bo, bd = bounce_rays(first, n)
            sets = {"camera": d_rays, "bounce": torch.from_numpy(pack(bo, bd).view(np.float32).reshape(n, 8)).to(dev)}
            torch.cuda.synchronize()
            for kind, dr in sets.items():
                for any_hit in (False, True):
                    best, med, engine, tests = time_queries(sc, dr, n, d_hits, any_hit, a.runs, a.warmup, stream)
                    print(f"{name:6} {kind:9} {'any' if any_hit else 'closest':8} {engine:6d} {best:9.3f} {med:9.3f} "
                          f"{n / best / 1e3:9.0f} {tests:14.2f}", flush=True)
            del sets, d_rays, d_hits
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
