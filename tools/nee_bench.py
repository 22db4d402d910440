#!/usr/bin/env python3
"""Direct lighting of caller rays (rt_scene_direct) and the integrator in one kernel (rt_scene_trace_nee): what one light sample per hit costs next to the path step it follows, and what
it buys, on the camera rays of a benchmark scene (default c2, cornell16).

  timing    the first path step of all camera rays alone (rt_scene_bounce), and the same step followed by rt_scene_direct on the
            rays that scattered: HIP-event time of the kernels (rt_tile_stats.kernel_ms), best and median of --runs after --warmup
            warm-ups;
  variance  K steps with a light sample after each but the last (the fold of examples/nee_rays.c) against rt_scene_trace with
            max_bounces = K - 1 on the same rays, one sample per ray each: the mean and the variance of the samples' luminance and
            the variance ratio at that equal sample count, over all samples and within the pixels' own samples.  (The means agree
            only where every hit has roughness 0: rt_tile.h.)
  fused     the integrator in one kernel (rt_scene_trace_nee) in both modes on the same rays, max_bounces = K - 1: HIP-event time of
            the kernel, best and median of --runs after --warmup warm-ups, beside the composed loop and rt_scene_trace timed the same
            way, and each mode's mean, variance and variance ratio against rt_scene_trace at that equal sample count.
  power     (--power) light selection by power, RT_FLAG_LIGHTS_BY_POWER, beside the uniform pick on the same rays and states in the same
            run: HIP-event time of rt_scene_direct on the first step's hits and of rt_scene_trace_nee in both modes (best and median
            of --runs after --warmup), the mean and the variance of the samples' luminance, and the variance ratio uniform / by power.
  cone      (--cone) cone sampling of sphere lights, RT_LIGHTS_CONE, beside RT_LIGHTS_AREA on the same rays and states in the same run
            (with --power: both under RT_FLAG_LIGHTS_BY_POWER): HIP-event time of rt_scene_direct on the first step's hits and of
            rt_scene_trace_nee in both modes (best and median of --runs after --warmup), the mean and the variance of the samples'
            luminance, the variance ratio area / cone and, per setting, the ratio rt_scene_trace / mode.
  glossy    (--glossy) light samples at glossy hits, RT_GLOSSY_MIS, beside RT_GLOSSY_BOUNCE in mode RT_NEE_MIS on the same rays and states
            in the same run (with --power / --cone: under RT_FLAG_LIGHTS_BY_POWER / RT_LIGHTS_CONE), on the config's camera rays and on
            the glossy room (a ground of roughness 0.5, spheres of roughness 0, 0.5 and 1, a sphere light and a triangle light, under
            fixed pinhole rays): HIP-event time of rt_scene_trace_nee (best, median and the spread of --runs after --warmup), the mean
            and the variance of the samples' luminance, the variance ratio bounce / MIS, the time ratio, and the figure of merit
            (variance x time) bounce / MIS.

--config lamps is the many-light scene scenes.lamp_room() (one lamp, 32 dim emitters) under its fixed pinhole rays.

    python tools/nee_bench.py [--config c2 | lamps] [--width 480 --height 270 --spp 4] [--steps 4] [--power] [--cone] [--glossy]
Prints one JSON line."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ray_tracer_s8_amd as rt  # noqa: E402
from ray_tracer_s8_amd import _abi, scenes  # noqa: E402

SCATTERED, EMITTED, MISSED = _abi.RT_BOUNCE_SCATTERED, _abi.RT_BOUNCE_EMITTED, _abi.RT_BOUNCE_MISSED
MODES = {"light_only": _abi.RT_NEE_LIGHT_ONLY, "mis": _abi.RT_NEE_MIS}


def _rgb(a):
    return np.stack([a["r"], a["g"], a["b"]], 1).astype(np.float64)


def _states(n, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)


def nee(sc, rays, states, K):
    """K steps, a light sample after each but the last; returns the colour per ray and the kernel time of steps and samples."""
    n = len(rays)
    T, col = np.ones((n, 3)), np.zeros((n, 3))
    act, ms_step, ms_direct = None, 0.0, 0.0
    for k in range(K):
        s = sc.bounce(rays, states, active=act, as_given=True, want_hits=True, want_next=True)
        rays, states, ms_step = s["rays"], s["states"], ms_step + s["stats"].kernel_ms
        idx = np.arange(n) if act is None else act.astype(np.int64)
        status, rgb = s["bounce"]["status"][idx], _rgb(s["bounce"])[idx]
        own = (status == MISSED) | ((status == EMITTED) & (k == 0))
        col[idx[own]] += T[idx[own]] * rgb[own]
        nxt = s["next"]
        T[nxt] *= _rgb(s["bounce"])[nxt]
        if k < K - 1 and len(nxt):
            d = sc.direct(s["hits"], states, active=nxt)
            states, ms_direct = d["states"], ms_direct + d["stats"].kernel_ms
            col[nxt] += T[nxt] * _rgb(d["direct"])[nxt]
        act = nxt
        if not len(act):
            break
    return col, ms_step, ms_direct


def lamp_rays(width, height, spp):
    """scenes.lamp_room_rays as rt_ray records with unit directions, spp records per pixel (record pixel * spp + s, as camera_rays)."""
    o, d = scenes.lamp_room_rays(width, height)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    r = np.zeros(len(d) * spp, _abi.RAY_DTYPE)
    o, d = np.repeat(o, spp, 0), np.repeat(d, spp, 0)
    r["ox"], r["oy"], r["oz"], r["dx"], r["dy"], r["dz"] = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
    r["t_min"], r["t_max"] = 0.001, 1000.0
    return r


def power_block(sc, a, step, rays, o, dd):
    """The uniform pick and the pick by power side by side: the light samples of the first step's scattered hits, and the integrator
    in both modes, on the same rays and the same states."""
    n = len(rays)
    best_median = lambda t: {"best": min(t), "median": statistics.median(t)}
    out = {}
    for name, flags in (("uniform", 0), ("by_power", _abi.RT_FLAG_LIGHTS_BY_POWER)):
        t_direct, t_fused, fused = [], {m: [] for m in MODES}, {}
        for i in range(a.warmup + a.runs):
            d = sc.direct(step["hits"], step["states"], active=step["next"], flags=flags)
            for m, mode in MODES.items():
                fused[m] = sc.trace_nee(o, dd, rays["t_min"], rays["t_max"], spp=1, max_bounces=a.steps - 1, rng_state=_states(n, 3 + mode),
                                        as_given=True, mode=mode, flags=flags)
            if i >= a.warmup:
                t_direct.append(d["stats"].kernel_ms)
                for m in MODES:
                    t_fused[m].append(fused[m][3].kernel_ms)
        ld = _rgb(d["direct"])[step["next"]].mean(1)
        out[name] = {"direct": {"kernel_ms": best_median(t_direct), "mean": float(ld.mean()), "variance": float(ld.var(ddof=1))}}
        for m in MODES:
            lf = fused[m][0].astype(np.float64).mean(1)
            out[name][m] = {"kernel_ms": best_median(t_fused[m]), "mean": float(lf.mean()), "variance": float(lf.var(ddof=1)),
                            "shadow_rays": int(fused[m][2].sum())}
    out["variance_ratio_uniform_over_by_power"] = {k: out["uniform"][k]["variance"] / out["by_power"][k]["variance"]
                                                   for k in ("direct", *MODES)}
    p = sc.light_table(_abi.RT_FLAG_LIGHTS_BY_POWER)[1]
    out["p"] = {"min": float(p.min()), "max": float(p.max())} if len(p) else {}
    return out


def cone_block(sc, a, step, rays, o, dd, trace_var):
    """RT_LIGHTS_AREA and RT_LIGHTS_CONE side by side: the light samples of the first step's scattered hits, and the integrator in both
    modes, on the same rays and the same states.  The scene is left at RT_LIGHTS_AREA."""
    n = len(rays)
    flags = _abi.RT_FLAG_LIGHTS_BY_POWER if a.power else 0
    best_median = lambda t: {"best": min(t), "median": statistics.median(t)}
    out = {"flags": "by_power" if a.power else "uniform"}
    for name, setting in (("area", _abi.RT_LIGHTS_AREA), ("cone", _abi.RT_LIGHTS_CONE)):
        sc.set_light_sampling(setting)
        t_direct, t_fused, fused = [], {m: [] for m in MODES}, {}
        for i in range(a.warmup + a.runs):
            d = sc.direct(step["hits"], step["states"], active=step["next"], flags=flags)
            for m, mode in MODES.items():
                fused[m] = sc.trace_nee(o, dd, rays["t_min"], rays["t_max"], spp=1, max_bounces=a.steps - 1, rng_state=_states(n, 3 + mode),
                                        as_given=True, mode=mode, flags=flags)
            if i >= a.warmup:
                t_direct.append(d["stats"].kernel_ms)
                for m in MODES:
                    t_fused[m].append(fused[m][3].kernel_ms)
        rec = d["direct"][step["next"]]
        ld = _rgb(rec).mean(1)
        out[name] = {"direct": {"kernel_ms": best_median(t_direct), "mean": float(ld.mean()), "variance": float(ld.var(ddof=1)),
                                "largest": float(ld.max()), "shadow_rays": int(d["stats"].ray_segments),
                                "facing_away": int((rec["status"] == _abi.RT_DIRECT_FACING_AWAY).sum())}}
        for m in MODES:
            lf = fused[m][0].astype(np.float64).mean(1)
            out[name][m] = {"kernel_ms": best_median(t_fused[m]), "mean": float(lf.mean()), "variance": float(lf.var(ddof=1)),
                            "variance_ratio_trace_over_mode": trace_var / float(lf.var(ddof=1)), "shadow_rays": int(fused[m][2].sum())}
    sc.set_light_sampling(_abi.RT_LIGHTS_AREA)
    out["variance_ratio_area_over_cone"] = {k: out["area"][k]["variance"] / out["cone"][k]["variance"] for k in ("direct", *MODES)}
    return out


def glossy_room():
    """(spheres, triangles): a ground of roughness 0.5, spheres of roughness 0, 0.5 and 1, a sphere light and a triangle light."""
    sph = np.zeros(5, _abi.SPHERE_DTYPE)
    sph["cx"], sph["cy"], sph["cz"] = [0.0, -1.2, 0.0, 1.2, 0.2], [-100.5, 0.0, 0.0, 0.0, 2.3], [-3.0, -3.2, -3.0, -2.8, -3.0]
    sph["radius"] = [100.0, 0.5, 0.5, 0.5, 0.5]
    sph["albedo_r"], sph["albedo_g"], sph["albedo_b"] = [0.5, 0.8, 0.3, 0.7, 1.0], [0.6, 0.3, 0.7, 0.7, 0.9], [0.4, 0.3, 0.4, 0.2, 0.7]
    sph["roughness"], sph["emission"] = [0.5, 0.0, 0.5, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0, 6.0]
    tri = np.zeros(1, _abi.TRIANGLE_DTYPE)
    tri["a"][0], tri["b"][0], tri["c"][0] = (-2.5, 0.2, -4.5), (-1.5, 1.8, -4.8), (-2.8, 1.5, -3.6)
    tri["albedo_r"], tri["albedo_g"], tri["albedo_b"], tri["emission"] = 0.6, 0.8, 1.0, 3.0
    return sph, tri


def room_rays(width, height, spp):
    """Fixed pinhole rays from the origin down -z, pitched down onto the room's spheres, spp records per pixel, unit directions."""
    ys, xs = np.mgrid[0:height, 0:width]
    u = ((xs + 0.5) / width * 2 - 1) * 0.3 * width / height
    v = (1 - (ys + 0.5) / height * 2) * 0.3 - 0.1
    d = np.stack([u, v, -np.ones_like(u)], -1).reshape(-1, 3)
    d = np.repeat((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32), spp, 0)
    r = np.zeros(len(d), _abi.RAY_DTYPE)
    r["dx"], r["dy"], r["dz"], r["t_min"], r["t_max"] = d[:, 0], d[:, 1], d[:, 2], 0.001, 1000.0
    return r


def glossy_block(sc, a, rays):
    """RT_GLOSSY_BOUNCE and RT_GLOSSY_MIS side by side in mode RT_NEE_MIS on the same rays and states, next to rt_scene_trace.  The
    scene is left at RT_GLOSSY_BOUNCE."""
    n = len(rays)
    o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)
    dd = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)
    flags = _abi.RT_FLAG_LIGHTS_BY_POWER if a.power else 0
    sc.set_light_sampling(_abi.RT_LIGHTS_CONE if a.cone else _abi.RT_LIGHTS_AREA)
    spread = lambda t: {"best": min(t), "median": statistics.median(t), "worst": max(t), "runs": len(t)}
    t_trace = []
    for i in range(a.warmup + a.runs):
        tr = sc.trace(o, dd, rays["t_min"], rays["t_max"], spp=1, max_bounces=a.steps - 1, rng_state=_states(n, 2), as_given=True)
        if i >= a.warmup:
            t_trace.append(tr[2].kernel_ms)
    lt = tr[0].astype(np.float64).mean(1)
    out = {"rays": n, "lights": sc.n_lights, "flags": "by_power" if a.power else "uniform", "light_sampling": "cone" if a.cone else "area",
           "trace": {"kernel_ms": spread(t_trace), "mean": float(lt.mean()), "variance": float(lt.var(ddof=1))}}
    for name, setting in (("bounce", _abi.RT_GLOSSY_BOUNCE), ("mis", _abi.RT_GLOSSY_MIS)):
        sc.set_glossy_sampling(setting)
        t = []
        for i in range(a.warmup + a.runs):
            got = sc.trace_nee(o, dd, rays["t_min"], rays["t_max"], spp=1, max_bounces=a.steps - 1, rng_state=_states(n, 4), as_given=True,
                               mode=_abi.RT_NEE_MIS, flags=flags)
            if i >= a.warmup:
                t.append(got[3].kernel_ms)
        lf = got[0].astype(np.float64).mean(1)
        out[name] = {"kernel_ms": spread(t), "mean": float(lf.mean()), "variance": float(lf.var(ddof=1)),
                     "standard_error": float(np.sqrt(lf.var(ddof=1) / n)), "largest": float(lf.max()), "segments": int(got[1].sum()),
                     "shadow_rays": int(got[2].sum()), "variance_ratio_trace_over_this": float(lt.var(ddof=1) / lf.var(ddof=1))}
    sc.set_glossy_sampling(_abi.RT_GLOSSY_BOUNCE)
    sc.set_light_sampling(_abi.RT_LIGHTS_AREA)
    vr = out["bounce"]["variance"] / out["mis"]["variance"]
    tr_ = out["mis"]["kernel_ms"]["median"] / out["bounce"]["kernel_ms"]["median"]
    out["variance_ratio_bounce_over_mis"] = vr
    out["time_ratio_mis_over_bounce"] = tr_
    out["variance_x_time_bounce_over_mis"] = vr / tr_
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c2")
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--power", action="store_true", help="also time and compare RT_FLAG_LIGHTS_BY_POWER against the uniform pick")
    ap.add_argument("--cone", action="store_true", help="also time and compare RT_LIGHTS_CONE against RT_LIGHTS_AREA (with --power: by power)")
    ap.add_argument("--glossy", action="store_true",
                    help="also time and compare RT_GLOSSY_MIS against RT_GLOSSY_BOUNCE in mode RT_NEE_MIS, on these rays and on the glossy room")
    a = ap.parse_args()
    rt.init()
    lamps = a.config == "lamps"
    sph, rq = (scenes.lamp_room(), _abi.default_request()) if lamps else scenes.config(a.config)
    rq.width, rq.height, rq.divisions, rq.division_no, rq.spp = a.width, a.height, 1, 0, a.spp
    with rt.Scene(0, rt.World(sph)) as sc:
        if lamps:
            rays = lamp_rays(a.width, a.height, a.spp)
            states = _states(len(rays), 0)
        else:
            rays, states, _ = sc.camera_rays(rq)
        n = len(rays)
        t_step, t_direct = [], []
        for i in range(a.warmup + a.runs):
            s = sc.bounce(rays, states, as_given=True, want_hits=True, want_next=True)
            d = sc.direct(s["hits"], s["states"], active=s["next"])
            if i >= a.warmup:
                t_step.append(s["stats"].kernel_ms)
                t_direct.append(d["stats"].kernel_ms)
        both = [x + y for x, y in zip(t_step, t_direct)]
        col, ms_step, ms_direct = nee(sc, rays, _states(n, 1), a.steps)
        o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)
        dd = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)
        ref = sc.trace(o, dd, rays["t_min"], rays["t_max"], spp=1, max_bounces=a.steps - 1, rng_state=_states(n, 2), as_given=True)
        la, lb = ref[0].astype(np.float64).mean(1), col.mean(1)
        # the variance within a pixel's spp samples (records (row W + x) spp + s), averaged: the noise without the image's own variance
        wa, wb = (float(x.reshape(-1, a.spp).var(1, ddof=1).mean()) if a.spp > 1 else float("nan") for x in (la, lb))
        # the composed loop, the one-kernel trace and the fused integrator in both modes, timed alike on the same rays
        t_loop, t_trace, t_fused = [], [], {m: [] for m in MODES}
        fused = {}
        for i in range(a.warmup + a.runs):
            _, ms_s, ms_d = nee(sc, rays, _states(n, 1), a.steps)
            tr = sc.trace(o, dd, rays["t_min"], rays["t_max"], spp=1, max_bounces=a.steps - 1, rng_state=_states(n, 2), as_given=True)
            for name, mode in MODES.items():
                fused[name] = sc.trace_nee(o, dd, rays["t_min"], rays["t_max"], spp=1, max_bounces=a.steps - 1,
                                           rng_state=_states(n, 3 + mode), as_given=True, mode=mode)
            if i >= a.warmup:
                t_loop.append(ms_s + ms_d)
                t_trace.append(tr[2].kernel_ms)
                for name in MODES:
                    t_fused[name].append(fused[name][3].kernel_ms)
        best_median = lambda t: {"best": min(t), "median": statistics.median(t)}
        fused_out = {}
        for name in MODES:
            lf = fused[name][0].astype(np.float64).mean(1)
            wf = float(lf.reshape(-1, a.spp).var(1, ddof=1).mean()) if a.spp > 1 else float("nan")
            fused_out[name] = {"kernel_ms": best_median(t_fused[name]), "mean": float(lf.mean()), "variance": float(lf.var(ddof=1)),
                               "variance_ratio": float(la.var(ddof=1) / lf.var(ddof=1)), "within_pixel_variance_ratio": wa / wf,
                               "segments": int(fused[name][1].sum()), "shadow_rays": int(fused[name][2].sum())}
        out = {
            "config": a.config, "rays": n, "lights": sc.n_lights, "scattered": int(len(s["next"])), "shadow_rays": int(d["stats"].ray_segments),
            "step_ms": {"best": min(t_step), "median": statistics.median(t_step)},
            "direct_ms": {"best": min(t_direct), "median": statistics.median(t_direct)},
            "step_plus_direct_ms": {"best": min(both), "median": statistics.median(both)},
            "steps": a.steps, "nee_kernel_ms": {"steps": ms_step, "direct": ms_direct}, "trace_kernel_ms": ref[2].kernel_ms,
            "trace": {"mean": float(la.mean()), "variance": float(la.var(ddof=1))},
            "nee": {"mean": float(lb.mean()), "variance": float(lb.var(ddof=1))},
            "variance_ratio": float(la.var(ddof=1) / lb.var(ddof=1)),
            "within_pixel_variance": {"trace": wa, "nee": wb, "ratio": wa / wb},
            "composed_loop_ms": best_median(t_loop), "trace_ms": best_median(t_trace), "fused": fused_out,
        }
        if a.power:
            out["power"] = power_block(sc, a, s, rays, o, dd)
        if a.cone:
            out["cone"] = cone_block(sc, a, s, rays, o, dd, float(la.var(ddof=1)))
        if a.glossy:
            out["glossy"] = {"config": glossy_block(sc, a, rays)}
    if a.glossy:
        with rt.Scene(0, rt.World(*glossy_room())) as room:
            out["glossy"]["room"] = glossy_block(room, a, room_rays(a.width, a.height, a.spp))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
