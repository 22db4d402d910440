"""The arithmetic of direct lighting (rt_scene_direct, rt_tile.h "direct lighting") in float32 numpy: the pick, the point on the light,
the cosines, the weight and the radiance are float32 numpy scalars, one IEEE operation per numpy operation in the order the header
writes them (a dot product is (x x' + y y') + z z').  tests/test_direct_host.py pins it against csrc/rt_direct_math.h under g++.  The
kernel's restatement — the draws, the shadow ray, the record — is tests/_lights_np.py's `direct`.  Also here: the emitter list, the
K-step integrator's fold and the scenes the tests share."""
import numpy as np

from ray_tracer_s8_amd import _abi

import _bounce_np as B

F32 = np.float32
NONE = _abi.RT_HIT_NONE
LIT, OCCLUDED, FACING_AWAY, NO_LIGHTS, SKIPPED = (_abi.RT_DIRECT_LIT, _abi.RT_DIRECT_OCCLUDED, _abi.RT_DIRECT_FACING_AWAY,
                                                  _abi.RT_DIRECT_NO_LIGHTS, _abi.RT_DIRECT_SKIPPED)
PI = F32(np.pi)
DIRECT_F = ("r", "g", "b", "lx", "ly", "lz")
DIRECT_I = ("light", "status")
MAX_LIGHTS = 1 << 23


def v3(x, y, z):
    return np.array([x, y, z], F32)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return v3(a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def normalize_or_zero(a):
    with np.errstate(all="ignore"):
        rcp = F32(1) / np.sqrt(dot(a, a))
        return a * rcp if np.isfinite(rcp) and rcp > 0 else np.zeros(3, F32)


def emitters(sph, tri, wi=None):
    """[(world position, 'sphere' | 'triangle', record)] of the primitives with emission > 0, in ascending world position."""
    ns, nt = len(sph), len(tri)
    pos = np.arange(ns + nt) if wi is None else np.asarray(wi, np.int64)
    out = [(int(pos[i]), "sphere", sph[i]) for i in range(ns) if sph["emission"][i] > 0]
    out += [(int(pos[ns + j]), "triangle", tri[j]) for j in range(nt) if tri["emission"][j] > 0]
    return sorted(out, key=lambda e: e[0])


def pick(u, M):
    """k = min((uint32_t)(u * (float)M), M - 1)"""
    return min(int(F32(u) * F32(M)), M - 1)


def fold_pair(u1, u2):
    u1, u2 = F32(u1), F32(u2)
    if u1 + u2 > F32(1):
        return F32(1) - u1, F32(1) - u2
    return u1, u2


def sphere_point(c, r, us):
    return (c + F32(r) * us).astype(F32)


def triangle_point(a, b, c, u1, u2):
    return (a + (u1 * (b - a) + u2 * (c - a))).astype(F32)


def triangle_area(a, b, c):
    n = cross(a - b, a - c)
    return F32(0.5) * np.sqrt(dot(n, n))


def geometry(P, n, L, nl, sphere):
    """(v, d2, w, cs, cl, facing) of one sample."""
    with np.errstate(all="ignore"):
        v = (L - P).astype(F32)
        d2 = dot(v, v)
        w = (v / np.sqrt(d2)).astype(F32)
        cs = dot(n, w)
        c = dot(nl, w)
        cl = -c if sphere else np.abs(c)
        facing = bool(cs > 0 and cl > 0 and d2 > 0 and np.isfinite(d2))
    return v, d2, w, cs, cl, facing


def sphere_weight(cs, cl, r, M, d2):
    with np.errstate(all="ignore"):
        r = F32(r)
        return ((cs * cl) * ((F32(4) * (r * r)) * F32(M))) / d2


def triangle_weight(cs, cl, A, M, d2):
    with np.errstate(all="ignore"):
        return ((cs * cl) * (A * F32(M))) / (PI * d2)


def radiance(albedo, emission, W):
    with np.errstate(all="ignore"):
        return ((albedo * F32(emission)) * W).astype(F32)


def light_fields(kind, rec):
    """(geometry vectors, albedo, emission) of an emitter record."""
    alb = v3(rec["albedo_r"], rec["albedo_g"], rec["albedo_b"])
    if kind == "sphere":
        return (v3(rec["cx"], rec["cy"], rec["cz"]), F32(rec["radius"])), alb, F32(rec["emission"])
    return (np.array(rec["a"], F32), np.array(rec["b"], F32), np.array(rec["c"], F32)), alb, F32(rec["emission"])


def rgb_of(d):
    return np.stack([d["r"], d["g"], d["b"]], 1).astype(F32)


def records_equal(a, b):
    return B.records_equal(a, b, DIRECT_F, DIRECT_I)


def integrate(step_fn, direct_fn, rays, states, K):
    """The K-step integrator with next-event estimation, as a caller folds it: per step the bounce of the active rays, then one
    light sample at every hit that scattered.  Right to left per ray, term_K = 0 and
        term_k = rgb_k                                   for a step that MISSED, or EMITTED at k = 1 (a light seen directly),
        term_k = 0                                       for a step k > 1 that EMITTED (the sample of step k - 1 counted that light),
        term_k = a_k * (direct_k + term_{k+1})           for a step that SCATTERED (a_k its albedo, direct_k the sample's rgb).
    step_fn(rays, states, active, as_given) and direct_fn(hits, states, active) return the dicts of B.step / direct (or of
    Scene.bounce / Scene.direct).  Returns (rgb (n, 3) float32, final states)."""
    n = len(rays)
    act = np.arange(n)
    cur_rays, cur_states = rays, states
    log = []
    for k in range(K):
        s = step_fn(cur_rays, cur_states, act, k > 0)
        cur_rays, cur_states = s["rays"], s["states"]
        nxt = act[s["bounce"]["status"][act] == B.SCATTERED]
        d = direct_fn(s["hits"], cur_states, nxt)
        cur_states = d["states"]
        log.append((s["bounce"], d["direct"], act))
        act = nxt
    term = np.zeros((n, 3), F32)
    for k in range(K - 1, -1, -1):
        bnc, dr, act = log[k]
        a, status = B.rgb_of(bnc)[act], bnc["status"][act]
        with np.errstate(all="ignore"):
            scat = (a * (rgb_of(dr)[act] + term[act])).astype(F32)
        own = a if k == 0 else np.where((status == B.EMITTED)[:, None], F32(0), a).astype(F32)
        term[act] = np.where((status == B.SCATTERED)[:, None], scat, own)
    return term, cur_states


# ---------------------------------------------------------------- scenes shared by the CPU and the GPU tests
def two_spheres():
    """One diffuse sphere under one emissive sphere."""
    sph = np.zeros(2, _abi.SPHERE_DTYPE)
    sph["cx"], sph["cy"], sph["cz"], sph["radius"] = [0.0, 0.3], [0.0, 2.5], [-3.0, -3.0], [1.0, 0.5]
    sph["albedo_r"], sph["albedo_g"], sph["albedo_b"] = [0.8, 1.0], [0.6, 0.9], [0.4, 0.8]
    sph["emission"] = [0.0, 4.0]
    return sph, B.NO_TRI, None


def lit_room(light_radius=0.5):
    """Roughness 0 throughout: a ground sphere, three diffuse spheres, one emissive sphere about 2 units above them and one emissive
    triangle.  (spheres, triangles)."""
    sph = np.zeros(5, _abi.SPHERE_DTYPE)
    sph["cx"] = [0.0, -1.2, 0.0, 1.2, 0.2]
    sph["cy"] = [-100.5, 0.0, 0.0, 0.0, 2.3]
    sph["cz"] = [-3.0, -3.2, -3.0, -2.8, -3.0]
    sph["radius"] = [100.0, 0.5, 0.5, 0.5, light_radius]
    sph["albedo_r"] = [0.5, 0.8, 0.3, 0.7, 1.0]
    sph["albedo_g"] = [0.6, 0.3, 0.7, 0.7, 0.9]
    sph["albedo_b"] = [0.4, 0.3, 0.4, 0.2, 0.7]
    sph["emission"] = [0.0, 0.0, 0.0, 0.0, 6.0]
    tri = np.zeros(1, _abi.TRIANGLE_DTYPE)
    tri["a"][0], tri["b"][0], tri["c"][0] = (-2.5, 0.2, -4.5), (-1.5, 1.8, -4.8), (-2.8, 1.5, -3.6)
    tri["albedo_r"], tri["albedo_g"], tri["albedo_b"], tri["emission"] = 0.6, 0.8, 1.0, 3.0
    return sph, tri


def camera_rays(width, height, fov_scale=1.0, pitch=0.0):
    """Fixed pinhole rays from the origin down -z, one per pixel centre (rt_ray records, the default window); pitch shifts the
    view up (+) or down (-) in units of the image plane at distance 1."""
    ys, xs = np.mgrid[0:height, 0:width]
    u = ((xs + 0.5) / width * 2 - 1) * fov_scale * width / height
    v = (1 - (ys + 0.5) / height * 2) * fov_scale + pitch
    d = np.stack([u, v, -np.ones_like(u)], -1).reshape(-1, 3).astype(F32)
    return B.R.make_rays(np.zeros_like(d), d)
