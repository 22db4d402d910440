"""The arithmetic of light selection by power (RT_FLAG_LIGHTS_BY_POWER, rt_tile.h "light selection by power") in float32 numpy, one
IEEE operation per numpy operation in the order the header writes them: an emitter's power, and the weights with ip in the place of
(float)M.  The light table built from the powers and its pick are tests/_lights_np.py's `Table`; tests/test_lightpick_host.py pins
all three against csrc/rt_scene_host.h and csrc/rt_direct_math.h under g++.  Also here: the scenes with many lights."""
import numpy as np

from ray_tracer_s8_amd import _abi, scenes

import _bounce_np as B
import _direct_np as D

F32 = np.float32


# ---------------------------------------------------------------- the power of an emitter, the weights with ip
def power(kind, rec):
    """q = lum * area of one emitter record, 0 unless q > 0."""
    geo, alb, em = D.light_fields(kind, rec)
    with np.errstate(all="ignore"):
        lum = ((alb[0] + alb[1]) + alb[2]) * em
        if kind == "sphere":
            r = geo[1]
            area = (F32(4) * (r * r)) * D.PI
        else:
            A = D.triangle_area(*geo)
            area = A + A
        q = F32(lum * area)
    return q if q > 0 else F32(0)


def sphere_weight(cs, cl, r, ip, d2):
    with np.errstate(all="ignore"):
        r = F32(r)
        return ((cs * cl) * ((F32(4) * (r * r)) * F32(ip))) / d2


def triangle_weight(cs, cl, A, ip, d2):
    with np.errstate(all="ignore"):
        return ((cs * cl) * (A * F32(ip))) / (D.PI * d2)


# ---------------------------------------------------------------- scenes shared by the CPU and the GPU tests
def two_lights():
    """M = 2: D.lit_room, one sphere light and one triangle light.  (spheres, triangles, world_index)."""
    sph, tri = D.lit_room()
    return sph, tri, None


def many_lights(seed=33):
    """M = 33 on D.lit_room's diffuse spheres: 24 sphere lights and 9 triangle lights above them with emissions over six decades, one
    emitter of albedo 0, one of radius 0, and a permuted world_index.  (spheres, triangles, world_index)."""
    g = np.random.default_rng(seed)
    room, _ = D.lit_room()
    ns_l, nt_l = 24, 9
    sph = np.zeros(4 + ns_l, _abi.SPHERE_DTYPE)
    sph[:4] = room[:4]
    l = sph[4:]
    l["cx"], l["cy"], l["cz"] = g.uniform(-2.5, 2.5, ns_l), g.uniform(1.2, 3.0, ns_l), g.uniform(-5.0, -1.5, ns_l)
    l["radius"] = g.uniform(0.05, 0.3, ns_l)
    l["albedo_r"], l["albedo_g"], l["albedo_b"] = g.uniform(0.2, 1.0, (3, ns_l))
    l["emission"] = (10.0 ** g.uniform(-3, 3, ns_l)).astype(F32)
    l["albedo_r"][3], l["albedo_g"][3], l["albedo_b"][3] = 0.0, 0.0, 0.0     # emits by the list's rule, has no power
    l["radius"][7] = 0.0                                                   # likewise
    tri = np.zeros(nt_l, _abi.TRIANGLE_DTYPE)
    p = np.stack([g.uniform(-2.5, 2.5, nt_l), g.uniform(1.0, 2.5, nt_l), g.uniform(-5.0, -1.5, nt_l)], 1)
    tri["a"], tri["b"], tri["c"] = p, p + g.normal(0, 0.3, (nt_l, 3)), p + g.normal(0, 0.3, (nt_l, 3))
    tri["albedo_r"], tri["albedo_g"], tri["albedo_b"] = g.uniform(0.2, 1.0, (3, nt_l))
    tri["emission"] = (10.0 ** g.uniform(-3, 3, nt_l)).astype(F32)
    return sph, tri, g.permutation(len(sph) + nt_l).astype(np.uint32)


def lamp_room(n_dim=32):
    """The roughness-0 room of D.lit_room's spheres with one lamp (emission 6, radius 0.5) and n_dim dim spheres (emission 0.05, radius
    0.05) on a ring around it: M = n_dim + 1 (ray_tracer_s8_amd.scenes.lamp_room).  (spheres, triangles)."""
    sph = scenes.lamp_room(n_dim)
    assert np.array_equal(sph[:5], D.lit_room()[0])
    return sph, B.NO_TRI
