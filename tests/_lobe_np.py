"""The CPU reference for light samples at glossy hits (RT_GLOSSY_MIS, rt_tile.h "light samples at glossy hits"), from the oracle's entry
points and float32 numpy alone, one IEEE operation per numpy operation in the order the header writes them.  The light table, the
pick and the area weights are tests/_lightpick_np.py's, the cone sample and the cone view tests/_cone_np.py's, points, geometry and
radiance tests/_direct_np.py's, the MIS weights and the area view tests/_nee_np.py's, the path step tests/_bounce_np.py's; what is
restated here is the setting's own: the sampled-class rule, the lobe, its factor, the added rejection, and the driver loop
(rt_scene_trace_nee in mode RT_NEE_MIS) with the setting as a parameter — glossy=False is _cone_np's `nee` byte for byte.  Under
glossy=True the draws of a path depend on the mode's light samples, so only RT_NEE_MIS is returned.  tests/test_lobe_host.py pins the
arithmetic against csrc/rt_lobe_math.h under g++; tests/test_gpu_lobe.py compares the GPU with `nee` bit for bit."""
import numpy as np

from ray_tracer_s8_amd import _abi

import _bounce_np as B
import _cone_np as CN
import _direct_np as D
import _lightpick_np as LP
import _nee_np as N

F32 = np.float32
ZERO, ONE = F32(0), F32(1)
BOUNCE, GLOSSY = _abi.RT_GLOSSY_BOUNCE, _abi.RT_GLOSSY_MIS
LIGHT_ONLY, MIS = N.LIGHT_ONLY, N.MIS
NONE, DIFFUSE, LOBE = 0, 1, 2


# ---------------------------------------------------------------- the arithmetic of csrc/rt_lobe_math.h
# (on float32 scalars and 3-vectors, or on arrays of them with the components first: vectors of shape (3, n), scalars of shape (n,))
def glossy_dir(d, n):
    """g = d - (2 (d.n)) n, the glossy_dir of the path step"""
    with np.errstate(all="ignore"):
        return (d - (F32(2) * D.dot(d, n)) * n).astype(F32)


def sampled_class(rho, gn):
    """NONE, DIFFUSE or LOBE of a scattering hit (arrays: an int array)"""
    with np.errstate(all="ignore"):
        rho, gn = np.asarray(rho, F32), np.asarray(gn, F32)
        lobe = (ZERO < rho) & (rho < ONE) & (gn >= ZERO)
        return np.where(rho == ZERO, DIFFUSE, np.where(lobe, LOBE, NONE))


def lobe_of(n, g, rho):
    """(c, r, kappa) of a lobe-sampled hit"""
    with np.errstate(all="ignore"):
        rho = F32(rho) if np.ndim(rho) == 0 else np.asarray(rho, F32)
        r = ONE - rho
        c = (r * n + rho * g).astype(F32)
        gn, gg = D.dot(n, g), D.dot(g, g)
        kappa = rho * (rho * gg + (r + r) * gn)
    return c, r, kappa


def lobe_factor(lobe, w):
    """(b, D, in_lobe, cg) of the unit direction w; cg = 0 outside the lobe"""
    c, r, kappa = lobe
    with np.errstate(all="ignore"):
        b = D.dot(c, w)
        Dd = b * b - kappa
        inl = (b > 0) & (Dd > 0)
        cg = np.where(inl, (b * b + Dd) / ((r + r) * np.sqrt(np.where(inl, Dd, ONE))), ZERO).astype(F32)
    return b, Dd, inl, cg


def lobe_factor_scatter(lobe, us):
    """(m, t, cg, in_lobe) of the direction the scatter itself takes with the UnitSphere vector us (X = c + r us): m = r (c.us + r),
    t = sqrt(kappa + (m + m)), cg = ((kappa + m)^2 + m^2) / (((r + r) |m|) t), in the lobe iff cg > 0"""
    c, r, kappa = lobe
    with np.errstate(all="ignore"):
        m = r * (D.dot(c, us) + r)
        t = np.sqrt(kappa + (m + m))
        km = kappa + m
        cg = ((km * km + m * m) / (((r + r) * np.abs(m)) * t)).astype(F32)
        return m, t, cg, cg > 0


def sample_taken(in_lobe, W):
    with np.errstate(all="ignore"):
        return in_lobe & (W < F32(np.inf))


# ---------------------------------------------------------------- one light sample at a lobe-sampled hit
def light_sample(oracle, state, table, P, n, cone, lobe):
    """One light sample for the lobe-sampled hit (P, n) with the lobe `lobe`, the draws taken from `state` (advanced in place), a sphere
    light sampled under the setting `cone`.  Returns (world position, v, traced, D, W): traced is False when one of rt_scene_direct's
    rejections or the lobe's applies."""
    k = table.pick(oracle.draw(state, 0)[0])
    pos, kind, rec = table.list[k]
    geo, alb, em = D.light_fields(kind, rec)
    ip = table.ip[k]
    if kind == "sphere":
        x1, x2, s, us = CN.draw_pair(oracle, state)
        if cone and CN.cone_regime(CN.cone_axis(P, geo[0], geo[1])[3]):
            ks = CN.cone_sample(P, geo[0], geo[1], x1, x2, s)
            wn, cs, facing = CN.cone_geometry(n, ks["v"])
            _, _, inl, cg = lobe_factor(lobe, wn)
            W = CN.cone_weight(cg, ks["omc"], ip)
            return pos, ks["v"], bool(facing and sample_taken(inl, W)), D.radiance(alb, em, W), W
        L, nl = D.sphere_point(geo[0], geo[1], us), us
        v, d2, w, cs, cl, facing = D.geometry(P, n, L, nl, True)
        _, _, inl, cg = lobe_factor(lobe, w)
        W = LP.sphere_weight(cg, cl, geo[1], ip, d2)
    else:
        u1 = oracle.draw(state, 0)[0]
        u2 = oracle.draw(state, 0)[0]
        u1, u2 = D.fold_pair(u1, u2)
        L, nl = D.triangle_point(geo[0], geo[1], geo[2], u1, u2), D.normalize_or_zero(D.cross(geo[0] - geo[1], geo[0] - geo[2]))
        v, d2, w, cs, cl, facing = D.geometry(P, n, L, nl, False)
        _, _, inl, cg = lobe_factor(lobe, w)
        W = LP.triangle_weight(cg, cl, D.triangle_area(*geo), ip, d2)
    return pos, v, bool(facing and sample_taken(inl, W)), D.radiance(alb, em, W), W


# ---------------------------------------------------------------- rt_scene_trace_nee, mode RT_NEE_MIS, under RT_GLOSSY_MIS
def one_sample(oracle, sph, tri, lights, table, rays, states, max_bounces, backend, wi=None, as_given=False, cone=False):
    """One RT_NEE_MIS sample of every ray under RT_GLOSSY_MIS.  Returns (c (n, 3) float32, segments, shadow, the advanced states,
    counts: a dict of how many hits fell in each class and how many lobe samples were dropped by the added rejection)."""
    n = len(rays)
    T, c = np.ones((n, 3), F32), np.zeros((n, 3), F32)
    segs, shadow = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    cls = np.zeros(n, np.int64)
    cg_prev = np.zeros(n, F32)                     # the lobe factor of the direction the last lobe-sampled hit's scatter took
    n_prev = np.zeros((n, 3), F32)
    cur_rays, cur_states = rays, np.array(states, np.uint64)
    act = np.arange(n)
    counts = dict(none=0, diffuse=0, lobe=0, dropped=0, emitted_after_lobe=0, emitted_outside_lobe=0)

    def add(i, x):
        with np.errstate(all="ignore"):
            c[i] = c[i] + T[i] * x

    for k in range(max_bounces + 1):
        if not len(act):
            break
        given = as_given or k > 0
        s = B.step(oracle, sph, tri, cur_rays, cur_states, backend, wi, as_given=given, active=act)
        seg = np.ascontiguousarray(cur_rays[act])
        d_in = B.directions(seg, given)
        o_in = np.stack([seg["ox"], seg["oy"], seg["oz"]], 1).astype(F32)      # the segment's origin: the previous hit point
        before = cur_states                                                    # (the step's UnitSphere draw is its first draw)
        cur_rays, cur_states = s["rays"], s["states"]
        segs[act] += 1
        status, rgb, hits = s["bounce"]["status"], B.rgb_of(s["bounce"]), s["hits"]
        pending, shadow_rays = [], []
        for a, i in enumerate(act):
            if status[i] == B.MISSED:
                add(i, rgb[i])
            elif status[i] == B.EMITTED:
                e = rgb[i]
                term = e
                if k != 0 and cls[i] != NONE:
                    j = int(hits["index"][i])
                    sphere = bool(lights.sphere[j])
                    lobed = cls[i] == LOBE
                    inl, cg = True, None
                    if lobed:
                        cg = cg_prev[i]
                        inl = bool(cg > 0)
                        counts["emitted_after_lobe"] += 1
                        counts["emitted_outside_lobe"] += int(not inl)
                    in_regime = False
                    if cone and sphere:
                        rec = lights.rec[j]
                        cs, omc, in_regime, samplable = CN.emitter_view_cone(o_in[a], n_prev[i], d_in[a], D.v3(rec["cx"], rec["cy"], rec["cz"]),
                                                                             rec["radius"])
                        if samplable and inl:
                            Wv = CN.cone_weight(cg if lobed else cs, omc, table.ip_at[j])
                            term = (e * N.bounce_weight(Wv)).astype(F32)
                    if not in_regime:
                        nh = D.v3(hits["nx"][i], hits["ny"][i], hits["nz"][i])
                        cs, cl, d2, samplable = N.emitter_view(n_prev[i], d_in[a], nh, hits["distance"][i], sphere)
                        if samplable and inl:
                            with np.errstate(all="ignore"):
                                Wv = (LP.sphere_weight if sphere else LP.triangle_weight)(cg if lobed else cs, cl, lights.size(j), table.ip_at[j], d2)
                                term = (e * N.bounce_weight(Wv)).astype(F32)
                add(i, term)
            else:
                with np.errstate(all="ignore"):
                    T[i] = T[i] * rgb[i]
                if k == max_bounces:
                    continue
                j = int(hits["index"][i])
                P, nrm = D.v3(hits["px"][i], hits["py"][i], hits["pz"][i]), D.v3(hits["nx"][i], hits["ny"][i], hits["nz"][i])
                rho = lights.rough[j]
                g = glossy_dir(d_in[a], nrm)
                cls[i] = int(sampled_class(rho, D.dot(nrm, g))) if table.M > 0 else NONE
                counts[("none", "diffuse", "lobe")[cls[i]]] += 1
                n_prev[i] = nrm
                if cls[i] == NONE:
                    continue
                st = cur_states[i].copy()
                if cls[i] == LOBE:
                    lobe = lobe_of(nrm, g, rho)
                    us = oracle.draw(before[i].copy(), 3).astype(F32)          # the UnitSphere vector the step scattered with
                    cg_prev[i] = lobe_factor_scatter(lobe, us)[2]
                    pos, v, traced, Dv, W = light_sample(oracle, st, table, P, nrm, cone, lobe)
                    counts["dropped"] += int(not traced)
                else:
                    pos, _, v, traced, Dv, W, _ = CN.light_sample(oracle, st, table, P, nrm, cone)
                cur_states[i] = st
                if traced:
                    shadow[i] += 1
                    with np.errstate(all="ignore"):
                        pending.append((i, pos, (Dv * N.light_weight(W)).astype(F32)))
                    shadow_rays.append((P[0], P[1], P[2], cur_rays["t_min"][i], v[0], v[1], v[2], cur_rays["t_max"][i]))
        if pending:
            e = oracle.intersect_batch(sph, tri, np.array(shadow_rays, _abi.RAY_DTYPE), backend=backend, world_index=wi)
            for q, (i, pos, term) in enumerate(pending):
                if e["hit"][q] and int(e["index"][q]) == pos:
                    add(i, term)
        act = act[status[act] == B.SCATTERED] if k < max_bounces else act[:0]
    return c, segs, shadow, cur_states, counts


def nee(oracle, sph, tri, rays, spp, max_bounces, backend, wi=None, as_given=False, states=None, seed=0, by_power=False, cone=False,
        glossy=True):
    """As _cone_np.nee with the scene's glossy sampling as a parameter.  glossy=False: _cone_np.nee itself (both modes).  glossy=True:
    rgb holds RT_NEE_MIS only (RT_NEE_LIGHT_ONLY ignores the setting), and `counts` the classes met."""
    if not glossy:
        return CN.nee(oracle, sph, tri, rays, spp, max_bounces, backend, wi, as_given, states, seed, by_power, cone)
    n = len(rays)
    lights, table = N.Lights(sph, tri, wi), LP.Table(sph, tri, wi, by_power)
    total = np.zeros((n, 3), F32)
    segs, shadow = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    cur = None if states is None else np.array(states, np.uint64)
    counts = {}
    for s in range(spp):
        st = N.sample_states(seed, n, spp, s) if states is None else cur
        c, sg, sh, out_states, cnt = one_sample(oracle, sph, tri, lights, table, rays, st, max_bounces, backend, wi, as_given, cone)
        if states is not None:
            cur = out_states
        with np.errstate(all="ignore"):
            total = total + c
        segs += sg
        shadow += sh
        for key, v in cnt.items():
            counts[key] = counts.get(key, 0) + v
    return dict(rgb={MIS: total}, segments=segs, shadow=shadow, states=cur, counts=counts)


# ---------------------------------------------------------------- the scene of the class boundaries
BOUNDARY_RHOS = (2.0 ** -24, 0.5, 1 - 2.0 ** -24, 1.0, -0.5, float("nan"), 0.0)


def boundary_scene():
    """A row of ground-level spheres (radius 1, centres at y = 1, x = 4 i) with the roughnesses BOUNDARY_RHOS, a rough triangle
    (rho 0.5) standing beside them whose normal faces +z, so that rays from z < its plane hit its back (gn < 0) and rays from z > it its
    front, a sphere light and a large triangle light above.  (spheres, triangles)."""
    m = len(BOUNDARY_RHOS)
    sph = np.zeros(m + 1, _abi.SPHERE_DTYPE)
    sph["cx"][:m] = 4.0 * np.arange(m)
    sph["cy"][:m], sph["radius"][:m] = 1.0, 1.0
    sph["roughness"][:m] = np.array(BOUNDARY_RHOS, F32)
    sph["albedo_r"], sph["albedo_g"], sph["albedo_b"] = 0.9, 0.8, 0.7
    sph["cx"][m], sph["cy"][m], sph["cz"][m], sph["radius"][m], sph["emission"][m] = 12.0, 7.0, 1.0, 1.5, 6.0
    tri = np.zeros(2, _abi.TRIANGLE_DTYPE)
    tri["a"][0], tri["b"][0], tri["c"][0] = (-8.0, 0.0, -1.0), (-2.0, 0.0, -1.0), (-5.0, 5.0, -1.0)      # (a - b) x (a - c) = (0, 0, +30)
    tri["albedo_r"][0], tri["albedo_g"][0], tri["albedo_b"][0], tri["roughness"][0] = 0.8, 0.8, 0.9, 0.5
    tri["a"][1], tri["b"][1], tri["c"][1] = (-20.0, 8.0, -15.0), (35.0, 8.0, -15.0), (7.0, 8.0, 25.0)        # a ceiling light: many bounces end on it
    tri["albedo_r"][1], tri["albedo_g"][1], tri["albedo_b"][1], tri["emission"][1] = 1.0, 0.9, 0.8, 4.0
    return sph, tri


def boundary_rays(per=40, seed=9):
    """Rays from above and from the sides onto every sphere of boundary_scene, and onto both faces of its rough triangle."""
    g = np.random.default_rng(seed)
    m = len(BOUNDARY_RHOS)
    o, d = [], []
    for i in range(m):
        src = np.array([4.0 * i, 1.0, 0.0]) + g.normal(size=(per, 3)) * [1.5, 0.5, 1.5] + [0.0, 4.0, 3.0]
        dst = np.array([4.0 * i, 1.0, 0.0]) + g.uniform(-0.7, 0.7, (per, 3))
        o.append(src)
        d.append(dst - src)
    for side in (+1.0, -1.0):
        src = np.array([-5.0, 2.0, -1.0]) + g.uniform(-2, 2, (per, 3)) + [0.0, 0.0, 6.0 * side]
        dst = np.array([-5.0, 1.5, -1.0]) + g.uniform(-1, 1, (per, 3)) * [1.0, 1.0, 0.0]
        o.append(src)
        d.append(dst - src)
    return B.R.make_rays(np.concatenate(o).astype(F32), np.concatenate(d).astype(F32))
