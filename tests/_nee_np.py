"""The CPU reference for the next-event-estimation integrator (rt_scene_trace_nee, rt_tile.h "next-event estimation"), from the oracle's
entry points and float32 numpy alone, one IEEE operation per numpy operation in the order the header writes them.  The path step is
tests/_bounce_np.py's `step` (oracle.intersect_batch, oracle.draw, oracle.sky), the light sample is made of tests/_direct_np.py's pick,
points, geometry, weights and radiance with the shadow rays through oracle.intersect_batch in each ray's own window; what is written
here is the contract's own: the forward fold, the sampled rule, the two MIS weights and the samplable test.  The draws and the path of
a sample do not depend on the mode, so one pass returns the colours of both modes.  tests/test_nee_host.py pins the weights and the
samplable test against csrc/rt_nee_math.h under g++; tests/test_gpu_nee.py compares the GPU with `nee` bit for bit."""
import numpy as np

from ray_tracer_s8_amd import _abi

import _bounce_np as B
import _direct_np as D

F32 = np.float32
ONE = F32(1)
LIGHT_ONLY, MIS = _abi.RT_NEE_LIGHT_ONLY, _abi.RT_NEE_MIS
MODES = (LIGHT_ONLY, MIS)


# ---------------------------------------------------------------- the arithmetic of csrc/rt_nee_math.h
def light_weight(W):
    """wl = 1 / (1 + W)"""
    with np.errstate(all="ignore"):
        return ONE / (ONE + F32(W))


def bounce_weight(W):
    """wb = 1 - 1 / (1 + W')"""
    with np.errstate(all="ignore"):
        return ONE - ONE / (ONE + F32(W))


def emitter_view(n, d, nh, distance, sphere):
    """(cs', cl', d2', samplable) of an emitter the bounce reached: n the previous hit's normal, d the segment's unit direction, nh and
    distance this hit's rt_hit normal and distance."""
    with np.errstate(all="ignore"):
        cs = D.dot(n, d)
        c = D.dot(nh, d)
        cl = -c if sphere else np.abs(c)
        d2 = F32(distance) * F32(distance)
        samplable = bool(cs > 0 and cl > 0 and d2 > 0 and np.isfinite(d2))
    return cs, cl, d2, samplable


def view_weight(cs, cl, d2, sphere, size, M):
    """W' of that view: the weight of a light sample with this geometry (size: the radius, or the triangle's area)."""
    return D.sphere_weight(cs, cl, size, M, d2) if sphere else D.triangle_weight(cs, cl, size, M, d2)


# ---------------------------------------------------------------- the scene as the integrator reads it
class Lights:
    """The emitter list and, by world position (the value rt_hit.index reports), each primitive's roughness, kind and size."""

    def __init__(self, sph, tri, wi=None):
        ns, nt = len(sph), len(tri)
        pos = np.arange(ns + nt) if wi is None else np.asarray(wi, np.int64)
        self.list = D.emitters(sph, tri, wi)
        self.M = len(self.list)
        self.rough = np.zeros(ns + nt, F32)
        self.rough[pos[:ns]] = sph["roughness"]
        self.rough[pos[ns:]] = tri["roughness"]
        self.sphere = np.zeros(ns + nt, bool)
        self.sphere[pos[:ns]] = True
        self.rec = {int(pos[i]): sph[i] for i in range(ns)}
        self.rec.update({int(pos[ns + j]): tri[j] for j in range(nt)})

    def size(self, position):
        rec = self.rec[int(position)]
        if self.sphere[position]:
            return F32(rec["radius"])
        return D.triangle_area(np.array(rec["a"], F32), np.array(rec["b"], F32), np.array(rec["c"], F32))


def light_sample(oracle, state, lights, P, n):
    """One light sample for the hit (P, n) as rt_scene_direct specifies it, the draws taken from `state` (advanced in place).  Returns
    (world position of the emitter, v = L - P, facing, D, W)."""
    M = lights.M
    pos, kind, rec = lights.list[D.pick(oracle.draw(state, 0)[0], M)]
    geo, alb, em = D.light_fields(kind, rec)
    sphere = kind == "sphere"
    if sphere:
        us = oracle.draw(state, 3).astype(F32)
        L, nl = D.sphere_point(geo[0], geo[1], us), us
    else:
        u1 = oracle.draw(state, 0)[0]
        u2 = oracle.draw(state, 0)[0]
        u1, u2 = D.fold_pair(u1, u2)
        L, nl = D.triangle_point(geo[0], geo[1], geo[2], u1, u2), D.normalize_or_zero(D.cross(geo[0] - geo[1], geo[0] - geo[2]))
    v, d2, w, cs, cl, facing = D.geometry(P, n, L, nl, sphere)
    W = D.sphere_weight(cs, cl, geo[1], M, d2) if sphere else D.triangle_weight(cs, cl, D.triangle_area(*geo), M, d2)
    return pos, v, facing, D.radiance(alb, em, W), W


# ---------------------------------------------------------------- one sample of every ray, then the sum over the samples
def _add(c, i, T, x):
    """c[m][i] = c[m][i] + T * x[m] for both modes: one multiplication, then one addition, per channel."""
    with np.errstate(all="ignore"):
        for m in MODES:
            if x[m] is not None:
                c[m][i] = c[m][i] + T * x[m]


def one_sample(oracle, sph, tri, lights, rays, states, max_bounces, backend, wi=None, as_given=False):
    """One sample of every ray.  Returns (c: {mode: (n, 3) float32}, segments (n,), shadow (n,), the advanced states)."""
    n = len(rays)
    T = np.ones((n, 3), F32)
    c = {m: np.zeros((n, 3), F32) for m in MODES}
    segs, shadow = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    sampled = np.zeros(n, bool)
    n_prev = np.zeros((n, 3), F32)
    cur_rays, cur_states = rays, np.array(states, np.uint64)
    act = np.arange(n)
    for k in range(max_bounces + 1):
        if not len(act):
            break
        given = as_given or k > 0
        s = B.step(oracle, sph, tri, cur_rays, cur_states, backend, wi, as_given=given, active=act)
        d_in = B.directions(np.ascontiguousarray(cur_rays[act]), given)      # the direction each segment was traced with
        cur_rays, cur_states = s["rays"], s["states"]
        segs[act] += 1
        status, rgb, hits = s["bounce"]["status"], B.rgb_of(s["bounce"]), s["hits"]
        pending, shadow_rays = [], []
        for a, i in enumerate(act):
            if status[i] == B.MISSED:
                _add(c, i, T[i], {m: rgb[i] for m in MODES})
            elif status[i] == B.EMITTED:
                e = rgb[i]
                term = {m: e for m in MODES}
                if k != 0 and sampled[i]:
                    j = int(hits["index"][i])
                    sphere = bool(lights.sphere[j])
                    nh = D.v3(hits["nx"][i], hits["ny"][i], hits["nz"][i])
                    cs, cl, d2, samplable = emitter_view(n_prev[i], d_in[a], nh, hits["distance"][i], sphere)
                    if samplable:
                        with np.errstate(all="ignore"):
                            wb = bounce_weight(view_weight(cs, cl, d2, sphere, lights.size(j), lights.M))
                            term = {LIGHT_ONLY: None, MIS: (e * wb).astype(F32)}
                _add(c, i, T[i], term)
            else:
                with np.errstate(all="ignore"):
                    T[i] = T[i] * rgb[i]
                if k == max_bounces:
                    continue
                j = int(hits["index"][i])
                sampled[i] = bool(lights.rough[j] == 0 and lights.M > 0)
                P, nrm = D.v3(hits["px"][i], hits["py"][i], hits["pz"][i]), D.v3(hits["nx"][i], hits["ny"][i], hits["nz"][i])
                n_prev[i] = nrm
                if not sampled[i]:
                    continue
                st = cur_states[i].copy()
                pos, v, facing, Dv, W = light_sample(oracle, st, lights, P, nrm)
                cur_states[i] = st
                if facing:
                    shadow[i] += 1
                    with np.errstate(all="ignore"):
                        pending.append((i, pos, {LIGHT_ONLY: Dv, MIS: (Dv * light_weight(W)).astype(F32)}))
                    shadow_rays.append((P[0], P[1], P[2], cur_rays["t_min"][i], v[0], v[1], v[2], cur_rays["t_max"][i]))
        if pending:
            e = oracle.intersect_batch(sph, tri, np.array(shadow_rays, _abi.RAY_DTYPE), backend=backend, world_index=wi)
            for q, (i, pos, term) in enumerate(pending):
                if e["hit"][q] and int(e["index"][q]) == pos:
                    _add(c, i, T[i], term)
        act = act[status[act] == B.SCATTERED] if k < max_bounces else act[:0]
    return c, segs, shadow, cur_states


def sample_states(seed, n, spp, s):
    """The seeded state of sample s of every ray: seed_from_u64(seed + 4 PHI (i spp + s))."""
    from oracle import oracle as orc
    return np.array([orc.seed_from_u64((seed + B.PHI4 * (i * spp + s)) & B.M64) for i in range(n)], np.uint64).reshape(n, 4)


def nee(oracle, sph, tri, rays, spp, max_bounces, backend, wi=None, as_given=False, states=None, seed=0):
    """rt_scene_trace_nee in both modes.  states: (n, 4) uint64 (the ray's samples draw one after the other), or None: the seeded
    streams of `seed`.  Returns a dict: rgb ({mode: (n, 3) float32 sums}), segments, shadow, states (None when seeded)."""
    n = len(rays)
    lights = Lights(sph, tri, wi)
    total = {m: np.zeros((n, 3), F32) for m in MODES}
    segs, shadow = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    cur = None if states is None else np.array(states, np.uint64)
    for s in range(spp):
        st = sample_states(seed, n, spp, s) if states is None else cur
        c, sg, sh, out_states = one_sample(oracle, sph, tri, lights, rays, st, max_bounces, backend, wi, as_given)
        if states is not None:
            cur = out_states
        with np.errstate(all="ignore"):
            for m in MODES:
                total[m] = total[m] + c[m]
        segs += sg
        shadow += sh
    return dict(rgb=total, segments=segs, shadow=shadow, states=cur)
