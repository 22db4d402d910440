"""The arithmetic of light samples at glossy hits (RT_GLOSSY_MIS, rt_tile.h "light samples at glossy hits") in float32 numpy, one IEEE
operation per numpy operation in the order the header writes them: the sampled-class rule, the glossy direction, the lobe, its factor
of a direction and of the scatter's own draw, and the added rejection.  tests/test_lobe_host.py pins it against csrc/rt_lobe_math.h
under g++.  Where the integrator applies them is tests/_lights_np.py's `light_sample` (lobe=) and `one_sample` (glossy=).  Also here:
the scene of the class boundaries."""
import numpy as np

from ray_tracer_s8_amd import _abi

import _bounce_np as B
import _direct_np as D

F32 = np.float32
ZERO, ONE = F32(0), F32(1)
BOUNCE, GLOSSY = _abi.RT_GLOSSY_BOUNCE, _abi.RT_GLOSSY_MIS
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
