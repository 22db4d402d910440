"""Array restatement of the sphere and triangle hit paths, beside restate_np.py (which states them one ray at a time).

*** TEST INFRASTRUCTURE ONLY. ***

Every function takes (n, k) float32 records in the layout of rt_oracle_operands_batch (rt_oracle.cpp) and evaluates the reference's
NESTED form: each branch of the cited lines is a boolean mask over the records, and a value computed on a branch is used only under
that branch's mask.  numpy performs one IEEE binary32 operation per array operation (no contraction), which is what the cited Rust
does.  Besides (hit, t) the functions return every intermediate a decision is taken on, for the classifier of
tests/_operand_cases.py.

  S = ray-tracer-slave/src, B = ray-tracer-slave/local-dependencies/bvh/src, roots = roots 0.0.8, glam = glam 0.23.0
"""
from __future__ import annotations

import numpy as np

F = np.float32
EPSILON = F(0.00001)                                # S/shapes/mesh.rs:110


def _f(a):
    a = np.ascontiguousarray(a)
    return a.view(np.float32) if a.dtype != np.float32 else a


def dot(a, b):                                      # glam sse2 dot3: (x*x' + y*y') + z*z'
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def normalize(v):                                   # glam normalize: v / sqrt(dot(v, v))
    ln = np.sqrt(dot(v, v))
    return (v[0] / ln, v[1] / ln, v[2] / ln)


def try_normalize(v):                               # glam try_normalize: v * (1 / length) if that is finite and > 0
    rcp = F(1.0) / np.sqrt(dot(v, v))
    ok = np.isfinite(rcp) & (rcp > F(0.0))
    return ok, (v[0] * rcp, v[1] * rcp, v[2] * rcp)


def _in_window(x, t_min, t_max):                    # (T_MIN..T_MAX).contains(&x), S/shapes/mod.rs:108
    return (x >= t_min) & (x < t_max)


def sphere(rec, ray_new: bool):
    """Sphere::get_roots (S/shapes/sphere.rs:42-47) -> find_roots_quadratic(1, b, c) -> S/shapes/mod.rs:106-129.
    ray_new: the direction goes through Ray::new (B/ray.rs:133-143) first; otherwise it is taken bit for bit."""
    r = _f(rec)
    with np.errstate(all="ignore"):
        o, d, cen = (r[:, 0], r[:, 1], r[:, 2]), (r[:, 3], r[:, 4], r[:, 5]), (r[:, 6], r[:, 7], r[:, 8])
        rad, t_min, t_max = r[:, 9], r[:, 10], r[:, 11]
        if ray_new:
            d = normalize(d)
        oc = sub(o, cen)
        b = dot((F(2.0) * d[0], F(2.0) * d[1], F(2.0) * d[2]), oc)
        ln = np.sqrt(dot(oc, oc))
        c = ln * ln - rad * rad
        a2 = F(1.0)
        disc = b * b - F(4.0) * a2 * c              # roots: a1 * a1 - _4 * a2 * a0
        none = disc < F(0.0)                        # -> Roots::No
        one = ~none & (disc == F(0.0))              # -> Roots::One([-a1 / a2x2])
        two = ~none & ~one                          # (a NaN discriminant arrives here, as in roots)
        a2x2 = F(2.0) * a2
        r_one = -b / a2x2
        sq = np.sqrt(disc)
        bneg = b < F(0.0)
        same = np.where(bneg, -b + sq, -b - sq)
        diff = np.where(bneg, -b - sq, -b + sq)
        big_s = np.abs(same) > np.abs(a2x2)
        big_d = np.abs(diff) > np.abs(a2x2)
        a0x2 = F(2.0) * c
        # if |same| > |a2x2| { if |diff| > |a2x2| {(a0x2/same, a0x2/diff)} else {(a0x2/same, same/a2x2)} } else {(diff/a2x2, same/a2x2)}
        x1 = np.where(big_s, a0x2 / same, diff / a2x2)
        x2 = np.where(big_s & big_d, a0x2 / diff, same / a2x2)
        lt = x1 < x2                                # if x1 < x2 { Two([x1, x2]) } else { Two([x2, x1]) }
        lo, hi = np.where(lt, x1, x2), np.where(lt, x2, x1)
        # S/shapes/mod.rs:106-129
        in_one = one & _in_window(r_one, t_min, t_max)
        xin, yin = two & _in_window(lo, t_min, t_max), two & _in_window(hi, t_min, t_max)
        both = xin & yin
        hit = in_one | xin | yin
        t = np.where(in_one, r_one, np.where(both, np.where(lo < hi, lo, hi), np.where(xin, lo, hi)))
        t = np.where(hit, t, F(0.0)).astype(np.float32)
    return {"hit": hit, "t": t, "d": d, "b": b, "c": c, "disc": disc, "none": none, "one": one, "two": two, "r_one": r_one,
            "same": same, "diff": diff, "x1": x1, "x2": x2, "lo": lo, "hi": hi, "xin": xin, "yin": yin, "in_one": in_one,
            "rad": rad, "t_min": t_min, "t_max": t_max}


def triangle(rec, ray_new: bool = False):
    """Triangle::get_roots (S/shapes/mesh.rs:109-161), then S/shapes/mod.rs:109-115.  ray_new: the direction goes through Ray::new
    (B/ray.rs:133-143) first; otherwise it is taken bit for bit."""
    r = _f(rec)
    with np.errstate(all="ignore"):
        o, d = (r[:, 0], r[:, 1], r[:, 2]), (r[:, 3], r[:, 4], r[:, 5])
        if ray_new:
            d = normalize(d)
        A, B, C = (r[:, 6], r[:, 7], r[:, 8]), (r[:, 9], r[:, 10], r[:, 11]), (r[:, 12], r[:, 13], r[:, 14])
        t_min, t_max = r[:, 15], r[:, 16]
        a_to_b, a_to_c = sub(B, A), sub(C, A)
        u_vec = cross(d, a_to_c)
        det = dot(a_to_b, u_vec)
        live0 = ~((det < EPSILON) & (det > -EPSILON))             # :122
        inv_det = F(1.0) / det
        a_to_origin = sub(o, A)
        u = dot(a_to_origin, u_vec) * inv_det
        live1 = live0 & ((u >= F(0.0)) & (u <= F(1.0)))            # !(0.0..=1.0).contains(&u) -> None
        v_vec = cross(a_to_origin, a_to_b)
        v = dot(d, v_vec) * inv_det
        live2 = live1 & ~((v < F(0.0)) | (u + v > F(1.0)))
        dist = dot(a_to_c, v_vec) * inv_det
        root = live2 & (dist > EPSILON)
        hit = root & _in_window(dist, t_min, t_max)
        t = np.where(hit, dist, F(0.0)).astype(np.float32)
        upv = u + v
    return {"hit": hit, "t": t, "det": det, "u": u, "v": v, "upv": upv, "dist": dist, "live0": live0, "live1": live1,
            "live2": live2, "root": root, "t_min": t_min, "t_max": t_max}


def _minss(x, y):                                   # B/ray.rs:81-112: if x < y { x } else { y }
    return np.where(x < y, x, y)


def _maxss(x, y):
    return np.where(x > y, x, y)


def aabb(o, d, lo, hi):
    """Ray::intersects_aabb (B/ray.rs:174-194) for the ray whose direction is d bit for bit; o, d, lo, hi: 3-tuples of arrays.
    Returns (passes, ray_min, ray_max, finite) with finite = every component of inv_direction finite."""
    with np.errstate(all="ignore"):
        inv = tuple(F(1.0) / d[k] for k in range(3))
        sign = tuple(d[k] < F(0.0) for k in range(3))
        near = tuple(np.where(sign[k], hi[k], lo[k]) for k in range(3))
        far = tuple(np.where(sign[k], lo[k], hi[k]) for k in range(3))
        ray_min = (near[0] - o[0]) * inv[0]
        ray_max = (far[0] - o[0]) * inv[0]
        for k in (1, 2):
            ray_min = _maxss(ray_min, (near[k] - o[k]) * inv[k])
            ray_max = _minss(ray_max, (far[k] - o[k]) * inv[k])
        passes = _maxss(ray_min, F(0.0)) <= ray_max
        finite = np.isfinite(inv[0]) & np.isfinite(inv[1]) & np.isfinite(inv[2])
    return passes, ray_min, ray_max, finite


def as_u8(v):                                       # Rust `f32 as u8`: NaN -> 0, saturating, truncating
    v = _f(v)
    with np.errstate(all="ignore"):
        w = np.where(np.isnan(v), F(0.0), np.clip(v, F(0.0), F(255.0)))
        return np.trunc(w).astype(np.uint8)
