#!/usr/bin/env python3
"""Cost of the a-trous denoiser (rt_scene_denoise_device): a 3840 x 2160 frame of c3 in 8 strips at 8 spp — the
progressive accum and every feature plane over [0, 8), rendered on the device first — denoised with every guide (albedo, normal,
depth, hits) at I = 1 .. 5 iterations, all three outputs.  Device buffers (torch, on a stream of its own), the HIP-event time the
library records around each of the call's launches (rt_scene_collect kernel_ms, summed), after warm-up calls; best and median of
--runs.  ms per iteration ((I) minus (I - 1) would mix in the entry; this is best / I), Mpix/s, the effective GB/s of the traffic
the kernels must move at the least (inputs 44 B + outputs 27 B a pixel once, 48 B a pixel an iteration: a colour and a guide record
read, a colour record written), and the ratio to the beauty frame of the same requests (rt_scene_render_tiles_device, one pass).

    python tools/denoise_bench.py [--runs 5] [--warmup 2] [--iters 1,2,3,4,5] [--lds-step S]

--lds-step S (test library): stage the steps up to S in LDS, the larger ones gather through L2 (0: every step gathers); the
default is rtplan::DN_LDS_MAX_STEP.
"""
from __future__ import annotations

import argparse
import contextlib
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
        ms.append(st.kernel_ms)
    return min(ms), float(np.median(ms)), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", default="1,2,3,4,5")
    ap.add_argument("--lds-step", type=int, default=None)
    a = ap.parse_args()
    ctx = _abi.debug_library() if a.lds_step is not None else contextlib.nullcontext()
    with ctx:
        rt.init()
        if a.lds_step is not None:
            _abi.debug_set("RT_DENOISE_LDS_STEP", a.lds_step)
        run(a)


def run(a):
    W, H, DIV, SPP = 3840, 2160, 8, 8
    hs = H // DIV
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev).cuda_stream      # (not torch's default stream: that is the null stream, handle 0)
    sph, rq0 = scenes.config("c3")
    reqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=rq0.max_bounces, seed=rq0.seed)
            for k in range(DIV)]
    lds = "default" if a.lds_step is None else str(a.lds_step)
    print(f"# c3 {W}x{H} in {DIV} strips, accum and planes over [0, {SPP}), every guide, outputs rgb + f32 + linear, LDS steps: {lds}; "
          f"best / median of {a.runs} calls after {a.warmup} warm-up calls")
    with rt.Scene(0, rt.World(sph)) as sc:
        f = dict(dtype=torch.float32, device=dev)
        acc = [torch.empty((hs, W, 3), **f) for _ in reqs]
        planes = [{"albedo": torch.empty((hs, W, 3), **f), "normal": torch.empty((hs, W, 3), **f),
                   "depth": torch.empty((hs, W), **f), "hits": torch.empty((hs, W), dtype=torch.int32, device=dev)} for _ in reqs]
        rgb = [torch.empty(hs * W * 3, dtype=torch.uint8, device=dev) for _ in reqs]
        out_f = [torch.empty((hs, W, 3), **f) for _ in reqs]
        out_l = [torch.empty((hs, W, 3), **f) for _ in reqs]
        scratch = torch.empty(rt.denoise_scratch_bytes(W, H), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        sc.render_tiles_pass_device(reqs, 0, SPP, [t.data_ptr() for t in acc], [t.data_ptr() for t in rgb], hs * W * 3, stream=stream)
        sc.render_aovs_device(reqs, 0, SPP, [{k: v.data_ptr() for k, v in p.items()} for p in planes], stream=stream)
        torch.cuda.synchronize()
        sc.collect()
        b_best, _, _ = timed(lambda: sc.render_tiles_device(reqs, [t.data_ptr() for t in rgb], hs * W * 3, stream=stream), sc,
                             a.runs, a.warmup)
        npix = W * H
        print(f"{'I':>2} {'best ms':>9} {'median ms':>9} {'ms/iter':>8} {'Mpix/s':>8} {'GB/s':>7} {'launches':>8} {'beauty ms':>9} "
              f"{'dn/beauty':>9}")
        for it in [int(x) for x in a.iters.split(",")]:
            dq = _abi.DenoiseRequest.defaults(color_samples=SPP, aov_samples=SPP, iterations=it)
            call = lambda: sc.denoise_device(reqs, dq, [t.data_ptr() for t in acc],                      # noqa: E731
                                             [{k: v.data_ptr() for k, v in p.items()} for p in planes], scratch.data_ptr(),
                                             scratch.numel(), d_rgb=[t.data_ptr() for t in rgb], d_f32=[t.data_ptr() for t in out_f],
                                             d_linear=[t.data_ptr() for t in out_l], stream=stream)
            best, med, st = timed(call, sc, a.runs, a.warmup)
            bytes_ = npix * (44 + 27 + 48 * it)
            print(f"{it:2d} {best:9.3f} {med:9.3f} {best / max(it, 1):8.3f} {npix / best / 1e3:8.0f} {bytes_ / best / 1e6:7.0f} "
                  f"{st.n_launches:8d} {b_best:9.2f} {best / b_best:9.3f}", flush=True)


if __name__ == "__main__":
    main()
