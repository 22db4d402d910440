"""The CPU reference for cone sampling of sphere lights (RT_LIGHTS_CONE, rt_tile.h "cone sampling of sphere lights"), from the oracle's
entry points and float32 numpy alone, one IEEE operation per numpy operation in the order the header writes them.  The light table,
the pick and the area weights are tests/_lightpick_np.py's, points, geometry, radiance and the emitter list tests/_direct_np.py's, the
MIS weights and the area view tests/_nee_np.py's, the path step tests/_bounce_np.py's; what is restated here is the setting's own: the
regime, the cone direction about the Duff frame, its weight and point, the cone view of an emitter the bounce reached, and the two
driver loops (rt_scene_direct, rt_scene_trace_nee) with the setting as a parameter — cone=False is _lightpick_np's `direct` and
`nee` byte for byte.  The UnitSphere pair is drawn here, two oracle.draw(state, 1) per rejection round, and checked on a copy of the
state against oracle.draw(copy, 3).  tests/test_cone_host.py pins the arithmetic against csrc/rt_direct_math.h and csrc/rt_nee_math.h
under g++; tests/test_gpu_cone.py compares the GPU with `direct` and `nee` bit for bit."""
import numpy as np

from ray_tracer_s8_amd import _abi

import _bounce_np as B
import _direct_np as D
import _lightpick_np as LP
import _nee_np as N

F32 = np.float32
ZERO, ONE, TWO = F32(0), F32(1), F32(2)
Q_MIN = F32(2.0 ** -10)
AREA, CONE = _abi.RT_LIGHTS_AREA, _abi.RT_LIGHTS_CONE
LIGHT_ONLY, MIS, MODES = N.LIGHT_ONLY, N.MIS, N.MODES


# ---------------------------------------------------------------- the draws
def unit_sphere_vec(x1, x2, s):
    """us = (x1 f, x2 f, 1 - 2 s), f = 2 sqrt(1 - s)"""
    f = TWO * np.sqrt(ONE - s)
    return D.v3(x1 * f, x2 * f, ONE - TWO * s)


def draw_pair(oracle, state):
    """The accepted pair of the UnitSphere draw from `state` (advanced in place): Uniform(-1, 1) twice per round, rejected while
    s >= 1.  Returns (x1, x2, s, us); us and the state left are checked against the oracle's own UnitSphere draw."""
    chk = state.copy()
    while True:
        x1 = F32(oracle.draw(state, 1)[0])
        x2 = F32(oracle.draw(state, 1)[0])
        s = F32(x1 * x1 + x2 * x2)
        if not (s >= ONE):
            break
    us = unit_sphere_vec(x1, x2, s)
    want = oracle.draw(chk, 3).astype(F32)
    assert np.array_equal(us.view(np.uint32), want.view(np.uint32)) and np.array_equal(chk, state), (x1, x2, us, want)
    return x1, x2, s, us


# ---------------------------------------------------------------- the arithmetic of csrc/rt_direct_math.h
# (on float32 scalars and 3-vectors, or on arrays of them with the components first: vectors of shape (3, n), scalars of shape (n,))
def cone_axis(P, c, r):
    """(a, dc2, r2, q) of the sphere (c, r) seen from P"""
    with np.errstate(all="ignore"):
        a = (c - P).astype(F32)
        dc2 = D.dot(a, a)
        r = F32(r)
        r2 = r * r
        q = r2 / dc2
    return a, dc2, r2, q


def cone_regime(q):
    with np.errstate(all="ignore"):
        return (q >= Q_MIN) & (q < ONE)


def cone_omc(q):
    with np.errstate(all="ignore"):
        ctm = np.sqrt(ONE - q)
        return q / (ONE + ctm)


def cone_sample(P, c, r, x1, x2, s):
    """The cone sample of an in-regime point: a dict v, omc, dc2, dc, ct, st (and r2)."""
    a, dc2, r2, q = cone_axis(P, c, r)
    omc = cone_omc(q)
    with np.errstate(all="ignore"):
        e = s * omc
        ct = ONE - e
        st = np.sqrt(e * (TWO - e))
        rs = np.sqrt(s)
        cp = np.where(s > 0, x1 / rs, ZERO)
        sp = np.where(s > 0, x2 / rs, ZERO)
        dc = np.sqrt(dc2)
        w = (a / dc).astype(F32)
        sg = np.copysign(ONE, w[2])
        A = -ONE / (sg + w[2])
        Bq = (w[0] * w[1]) * A
        t1 = D.v3(ONE + (sg * (w[0] * w[0])) * A, sg * Bq, -(sg * w[0]))
        t2 = D.v3(Bq, sg + (w[1] * w[1]) * A, -w[1])
        ka, kb = st * cp, st * sp
        v = ((ka * t1 + kb * t2) + ct * w).astype(F32)
    return dict(v=v, omc=omc, dc2=dc2, dc=dc, ct=ct, st=st, r2=r2, q=q)


def cone_geometry(n, v):
    """(wn, cs, facing): the shadow ray's direction v / sqrt(v.v), n.wn, cs > 0"""
    with np.errstate(all="ignore"):
        wn = (v / np.sqrt(D.dot(v, v))).astype(F32)
        cs = D.dot(n, wn)
        return wn, cs, cs > 0


def cone_weight(cs, omc, ip):
    with np.errstate(all="ignore"):
        return (cs * (omc + omc)) * F32(ip)


def cone_point(P, wn, k):
    with np.errstate(all="ignore"):
        h = k["r2"] - k["dc2"] * (k["st"] * k["st"])
        h = np.where(h > 0, h, ZERO)
        ts = k["dc"] * k["ct"] - np.sqrt(h)
        return (P + ts * wn).astype(F32)


# ---------------------------------------------------------------- the arithmetic of csrc/rt_nee_math.h
def emitter_view_cone(o, n, d, c, r):
    """(cs', omc', in_regime, samplable) of the emissive sphere (c, r) the bounce reached from o (normal n there, unit direction d)"""
    _, _, _, q = cone_axis(o, c, r)
    in_regime = cone_regime(q)
    with np.errstate(all="ignore"):
        cs = D.dot(n, d)
        omc = np.where(in_regime, cone_omc(q), ZERO)
        return cs, omc, in_regime, in_regime & (cs > 0)


# ---------------------------------------------------------------- one light sample
def light_sample(oracle, state, table, P, n, cone):
    """One light sample for the hit (P, n) under the setting `cone`, the draws taken from `state` (advanced in place).  Returns (world
    position, L, v, facing, D, W, in_cone): L is rt_direct.l*, v the direction handed to Ray::new."""
    k = table.pick(oracle.draw(state, 0)[0])
    pos, kind, rec = table.list[k]
    geo, alb, em = D.light_fields(kind, rec)
    ip = table.ip[k]
    if kind == "sphere":
        x1, x2, s, us = draw_pair(oracle, state)
        if cone and cone_regime(cone_axis(P, geo[0], geo[1])[3]):
            ks = cone_sample(P, geo[0], geo[1], x1, x2, s)
            wn, cs, facing = cone_geometry(n, ks["v"])
            W = cone_weight(cs, ks["omc"], ip)
            return pos, cone_point(P, wn, ks), ks["v"], facing, D.radiance(alb, em, W), W, True
        L, nl = D.sphere_point(geo[0], geo[1], us), us
        v, d2, w, cs, cl, facing = D.geometry(P, n, L, nl, True)
        W = LP.sphere_weight(cs, cl, geo[1], ip, d2)
    else:
        u1 = oracle.draw(state, 0)[0]
        u2 = oracle.draw(state, 0)[0]
        u1, u2 = D.fold_pair(u1, u2)
        L, nl = D.triangle_point(geo[0], geo[1], geo[2], u1, u2), D.normalize_or_zero(D.cross(geo[0] - geo[1], geo[0] - geo[2]))
        v, d2, w, cs, cl, facing = D.geometry(P, n, L, nl, False)
        W = LP.triangle_weight(cs, cl, D.triangle_area(*geo), ip, d2)
    return pos, L, v, facing, D.radiance(alb, em, W), W, False


# ---------------------------------------------------------------- rt_scene_direct
def direct(oracle, sph, tri, hits, states, backend, wi=None, active=None, t_min=0.001, t_max=1000.0, by_power=False, cone=True):
    """As _lightpick_np.direct, a sphere light sampled under the setting `cone`.  Also returns in_cone (bool per record)."""
    n = len(hits)
    act = np.arange(n) if active is None else np.asarray(active, np.int64)
    out, out_states = np.zeros(n, _abi.DIRECT_DTYPE), np.array(states, np.uint64)
    shadow, in_cone = np.zeros(n, bool), np.zeros(n, bool)
    table = LP.Table(sph, tri, wi, by_power)
    pending, rays = [], []
    for i in act:
        h = hits[i]
        if h["index"] == D.NONE or table.M == 0:
            out[i] = (0, 0, 0, D.NONE, 0, 0, 0, D.SKIPPED if h["index"] == D.NONE else D.NO_LIGHTS)
            continue
        st = out_states[i].copy()
        P, nrm = D.v3(h["px"], h["py"], h["pz"]), D.v3(h["nx"], h["ny"], h["nz"])
        pos, L, v, facing, rgb, _, in_cone[i] = light_sample(oracle, st, table, P, nrm, cone)
        out_states[i] = st
        out[i] = (0, 0, 0, pos, L[0], L[1], L[2], D.FACING_AWAY)
        if facing:
            shadow[i] = True
            pending.append((i, pos, rgb))
            rays.append((P[0], P[1], P[2], t_min, v[0], v[1], v[2], t_max))
    if pending:
        e = oracle.intersect_batch(sph, tri, np.array(rays, _abi.RAY_DTYPE), backend=backend, world_index=wi)
        for j, (i, pos, rgb) in enumerate(pending):
            if e["hit"][j] and int(e["index"][j]) == pos:
                out["r"][i], out["g"][i], out["b"][i] = rgb
                out["status"][i] = D.LIT
            else:
                out["status"][i] = D.OCCLUDED
    return dict(direct=out, states=out_states, shadow=shadow, in_cone=in_cone)


# ---------------------------------------------------------------- rt_scene_trace_nee
def one_sample(oracle, sph, tri, lights, table, rays, states, max_bounces, backend, wi=None, as_given=False, cone=True):
    """As _lightpick_np.one_sample: one sample of every ray in both modes, the light sample and the emitter's view under `cone`."""
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
        seg = np.ascontiguousarray(cur_rays[act])
        d_in = B.directions(seg, given)
        o_in = np.stack([seg["ox"], seg["oy"], seg["oz"]], 1).astype(F32)      # the segment's origin: the previous hit point
        cur_rays, cur_states = s["rays"], s["states"]
        segs[act] += 1
        status, rgb, hits = s["bounce"]["status"], B.rgb_of(s["bounce"]), s["hits"]
        pending, shadow_rays = [], []
        for a, i in enumerate(act):
            if status[i] == B.MISSED:
                N._add(c, i, T[i], {m: rgb[i] for m in MODES})
            elif status[i] == B.EMITTED:
                e = rgb[i]
                term = {m: e for m in MODES}
                if k != 0 and sampled[i]:
                    j = int(hits["index"][i])
                    sphere = bool(lights.sphere[j])
                    in_regime = False
                    if cone and sphere:
                        rec = lights.rec[j]
                        cs, omc, in_regime, samplable = emitter_view_cone(o_in[a], n_prev[i], d_in[a], D.v3(rec["cx"], rec["cy"], rec["cz"]),
                                                                          rec["radius"])
                        if samplable:
                            Wv = cone_weight(cs, omc, table.ip_at[j])
                            term = {LIGHT_ONLY: None, MIS: (e * N.bounce_weight(Wv)).astype(F32)}
                    if not in_regime:
                        nh = D.v3(hits["nx"][i], hits["ny"][i], hits["nz"][i])
                        cs, cl, d2, samplable = N.emitter_view(n_prev[i], d_in[a], nh, hits["distance"][i], sphere)
                        if samplable:
                            with np.errstate(all="ignore"):
                                Wv = (LP.sphere_weight if sphere else LP.triangle_weight)(cs, cl, lights.size(j), table.ip_at[j], d2)
                                term = {LIGHT_ONLY: None, MIS: (e * N.bounce_weight(Wv)).astype(F32)}
                N._add(c, i, T[i], term)
            else:
                with np.errstate(all="ignore"):
                    T[i] = T[i] * rgb[i]
                if k == max_bounces:
                    continue
                j = int(hits["index"][i])
                sampled[i] = bool(lights.rough[j] == 0 and table.M > 0)
                P, nrm = D.v3(hits["px"][i], hits["py"][i], hits["pz"][i]), D.v3(hits["nx"][i], hits["ny"][i], hits["nz"][i])
                n_prev[i] = nrm
                if not sampled[i]:
                    continue
                st = cur_states[i].copy()
                pos, _, v, facing, Dv, W, _ = light_sample(oracle, st, table, P, nrm, cone)
                cur_states[i] = st
                if facing:
                    shadow[i] += 1
                    with np.errstate(all="ignore"):
                        pending.append((i, pos, {LIGHT_ONLY: Dv, MIS: (Dv * N.light_weight(W)).astype(F32)}))
                    shadow_rays.append((P[0], P[1], P[2], cur_rays["t_min"][i], v[0], v[1], v[2], cur_rays["t_max"][i]))
        if pending:
            e = oracle.intersect_batch(sph, tri, np.array(shadow_rays, _abi.RAY_DTYPE), backend=backend, world_index=wi)
            for q, (i, pos, term) in enumerate(pending):
                if e["hit"][q] and int(e["index"][q]) == pos:
                    N._add(c, i, T[i], term)
        act = act[status[act] == B.SCATTERED] if k < max_bounces else act[:0]
    return c, segs, shadow, cur_states


def nee(oracle, sph, tri, rays, spp, max_bounces, backend, wi=None, as_given=False, states=None, seed=0, by_power=False, cone=True):
    """As _lightpick_np.nee: rt_scene_trace_nee in both modes under the setting `cone`."""
    n = len(rays)
    lights, table = N.Lights(sph, tri, wi), LP.Table(sph, tri, wi, by_power)
    total = {m: np.zeros((n, 3), F32) for m in MODES}
    segs, shadow = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    cur = None if states is None else np.array(states, np.uint64)
    for s in range(spp):
        st = N.sample_states(seed, n, spp, s) if states is None else cur
        c, sg, sh, out_states = one_sample(oracle, sph, tri, lights, table, rays, st, max_bounces, backend, wi, as_given, cone)
        if states is not None:
            cur = out_states
        with np.errstate(all="ignore"):
            for m in MODES:
                total[m] = total[m] + c[m]
        segs += sg
        shadow += sh
    return dict(rgb=total, segments=segs, shadow=shadow, states=cur)


# ---------------------------------------------------------------- the scene the CPU and the GPU tests share
def regimes_scene():
    """Every arm of the regime test in one small world.  A diffuse ground sphere (radius 1000, its top at y = 0) under:
      - a BIG emissive sphere of radius 5 about (20, 3, 0): hit points inside it (q > 1) and just outside;
      - a NEAR light of radius 0.5 whose lowest point is 1/64 above the ground: q just below 1 for the points under it;
      - a FAR light of radius 0.25 about (0, 3, -6): near the ground circle about (0, 0, -6) of radius sqrt(64 - 9) its distance is 8 and
        q = (1/32)^2 = 2^-10, so that points inside and outside that circle fall on either side of the threshold;
      - one emissive triangle, so that M = 4.
    (spheres, triangles)."""
    sph = np.zeros(4, _abi.SPHERE_DTYPE)
    sph["cx"] = [0.0, 20.0, 0.0, 0.0]
    sph["cy"] = [-1000.0, 3.0, 0.5 + 1.0 / 64, 3.0]
    sph["cz"] = [0.0, 0.0, 0.0, -6.0]
    sph["radius"] = [1000.0, 5.0, 0.5, 0.25]
    sph["albedo_r"] = [0.6, 1.0, 0.9, 0.7]
    sph["albedo_g"] = [0.5, 0.8, 0.9, 0.8]
    sph["albedo_b"] = [0.4, 0.6, 0.8, 1.0]
    sph["emission"] = [0.0, 2.0, 5.0, 40.0]
    tri = np.zeros(1, _abi.TRIANGLE_DTYPE)
    tri["a"][0], tri["b"][0], tri["c"][0] = (-3.0, 2.0, 2.0), (-2.0, 2.5, 3.0), (-3.5, 3.0, 3.0)
    tri["albedo_r"], tri["albedo_g"], tri["albedo_b"], tri["emission"] = 0.8, 0.9, 1.0, 6.0
    return sph, tri


def regimes_rays(n, seed=5):
    """Rays straight down onto regimes_scene's ground, a quarter each: inside the big sphere (they start inside it), under the near
    light, and on either side of the far light's q = 2^-10 circle; the rest spread over the ground."""
    g = np.random.default_rng(seed)
    x, z = g.uniform(-9, 9, n), g.uniform(-14, 4, n)
    q = n // 4
    x[:q], z[:q] = g.uniform(16.5, 23.5, q), g.uniform(-3, 3, q)                       # inside the big sphere, and around it
    x[q:2 * q], z[q:2 * q] = g.uniform(-0.6, 0.6, (2, q))                              # under the near light
    phi, rad = g.uniform(0, 2 * np.pi, q), np.sqrt(55.0) + g.uniform(-0.3, 0.3, q)   # the threshold circle of the far light
    x[2 * q:3 * q], z[2 * q:3 * q] = rad * np.cos(phi), -6.0 + rad * np.sin(phi)
    o = np.stack([x, np.full(n, 1.0), z], 1).astype(F32)
    o[q:2 * q, 1] = 0.01                                                               # (below the near light, not above it)
    d = np.tile(np.array([0.0, -1.0, 0.0], F32), (n, 1))
    return B.R.make_rays(o, d)
