"""Operands for the device functions of the closest-hit arithmetic: a classifier per family, a directed corpus, seeded random records.

The record layouts are those of ray_tracer_s8_amd/csrc/rt_unit.hip.h and rt_oracle_operands_batch (32-bit words per record).
A classifier is a numpy function of the records alone (through oracle/restate_ops_np.py, the reference's nested form): it says
which decisions of the reference a record exercises.  The class lists below are ENUMERATED, not derived from what occurred; the
CPU test tests/test_operand_corpus.py holds every listed class to FLOOR records of the directed corpus.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

from oracle import restate_ops_np as R
from oracle.oracle import AABB, AS_U8, CHAIN, NORMALIZE, RNG, SPHERE, SPHERE_NORM, TRIANGLE  # noqa: F401  (the family numbers)
from oracle.oracle import OPERAND_WORDS as WORDS  # noqa: F401  (words per record in / out)

F = np.float32
FLOOR = 64
EPS = R.EPSILON
T_MIN, T_MAX = F(0.001), F(1000.0)
PHI = 0x9E3779B97F4A7C15
TINY = F(np.finfo(np.float32).tiny)                      # the smallest normal


# ------------------------------------------------------------------------------------------------ sphere
SPHERE_CLASSES = (
    "disc<0", "disc==0", "disc>0", "disc NaN",
    "b<0", "b>=0",                                        # (of the records with two roots)
    "|same|<2", "|same|==2", "|same|>2",
    "|diff|<2", "|diff|==2", "|diff|>2",                  # (where roots takes that decision: |same| > 2)
    "x1<x2", "!(x1<x2)",
    "window both", "window first only", "window second only", "window none",
    "root==t_min", "root==t_max",
    "origin on surface", "origin inside", "r==0", "r<0", "r subnormal", "non-finite operand",
)
# (disc class) x (window class) as the reference can reach them: Roots::No and a NaN discriminant (two NaN roots) have no root in any
# window; Roots::One holds one root, so "both" and "second only" do not exist for it — its root in the window is "first only".
SPHERE_PAIRS = (("disc<0", "window none"), ("disc NaN", "window none"), ("disc==0", "window first only"), ("disc==0", "window none"),
                ("disc>0", "window both"), ("disc>0", "window first only"), ("disc>0", "window second only"),
                ("disc>0", "window none"))


def classify_sphere(rec, ray_new: bool = False):
    s = R.sphere(rec, ray_new)
    r = np.ascontiguousarray(rec).view(np.float32)
    with np.errstate(all="ignore"):
        two = s["two"] & ~np.isnan(s["disc"])
        nan = np.isnan(s["disc"])
        a_s, a_d = np.abs(s["same"]), np.abs(s["diff"])
        big_s = two & (a_s > F(2.0))
        first = s["in_one"] | (s["xin"] & ~s["yin"])
        root_a = np.where(s["one"], s["r_one"], s["lo"])
        root_b = np.where(s["one"], s["r_one"], s["hi"])
        has = s["one"] | two
        rad = s["rad"]
        c = {
            "disc<0": s["none"], "disc==0": s["one"], "disc>0": two, "disc NaN": nan,
            "b<0": two & (s["b"] < F(0.0)), "b>=0": two & ~(s["b"] < F(0.0)),
            "|same|<2": two & (a_s < F(2.0)), "|same|==2": two & (a_s == F(2.0)), "|same|>2": big_s,
            "|diff|<2": big_s & (a_d < F(2.0)), "|diff|==2": big_s & (a_d == F(2.0)), "|diff|>2": big_s & (a_d > F(2.0)),
            "x1<x2": two & (s["x1"] < s["x2"]), "!(x1<x2)": two & ~(s["x1"] < s["x2"]),
            "window both": s["xin"] & s["yin"], "window first only": first, "window second only": s["yin"] & ~s["xin"],
            "window none": ~s["hit"],
            "root==t_min": has & ((root_a == s["t_min"]) | (root_b == s["t_min"])),
            "root==t_max": has & ((root_a == s["t_max"]) | (root_b == s["t_max"])),
            "origin on surface": s["c"] == F(0.0), "origin inside": s["c"] < F(0.0),
            "r==0": rad == F(0.0), "r<0": rad < F(0.0), "r subnormal": (rad != F(0.0)) & (np.abs(rad) < TINY),
            "non-finite operand": ~np.isfinite(r).all(axis=1),
        }
    assert tuple(c) == SPHERE_CLASSES
    return c


def _perm(cols, k):
    """the three coordinates of every vector of `cols` (arrays (n, 3)) rotated k places: an axis permutation of the whole record"""
    return [np.roll(v, k, axis=1) for v in cols]


def _windows(lo, hi):
    """window variants round the roots lo <= hi of each record: (t_min, t_max) pairs as arrays (n, 9, 2)"""
    with np.errstate(all="ignore"):
        lo = np.where(np.isfinite(lo), lo, F(1.0)).astype(np.float32)
        hi = np.where(np.isfinite(hi), hi, lo).astype(np.float32)
        mid = ((lo + hi) / F(2.0)).astype(np.float32)
        one = np.ones_like(lo)
        w = [(T_MIN * one, T_MAX * one), (lo, hi + F(1000.0)), (lo - F(1000.0), lo), (hi, hi + F(1000.0)), (lo - F(1.0), hi),
             (hi + F(1.0), hi + F(2.0)), (lo - F(1.0), hi + F(1.0)), (mid, hi + F(1.0)), (lo - F(1.0), mid)]
    return np.stack([np.stack(p, axis=1) for p in w], axis=1).astype(np.float32)


def _with_windows(geo, roots_of):
    """every record of geo (n, k + 2; the last two words are the window) under each window variant round its own roots"""
    lo, hi = roots_of(geo)
    w = _windows(lo, hi)
    out = np.repeat(geo[:, None, :], w.shape[1], axis=1)
    out[:, :, -2:] = w
    return out.reshape(-1, geo.shape[1])


def _sphere_roots(geo):
    s = R.sphere(geo, False)
    return np.where(s["one"], s["r_one"], s["lo"]), np.where(s["one"], s["r_one"], s["hi"])


PYTHAGOREAN = ((3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29), (12, 35, 37), (9, 40, 41), (28, 45, 53))
CENTRES = ((0.0, 0.0, 0.0), (0.5, -0.25, 2.0), (-4.0, 1.0, 0.125))


@functools.lru_cache(maxsize=None)
def sphere_directed():
    rows = []
    # a ray along one axis: origin k before (or, pointing away, behind) the centre and e to the side, radius r, direction scaled by s.
    # All dyadic, so b = -+2ks, c = k^2 + e^2 - r^2 and the discriminant are exact and the |.| == 2 and root == window-end cases exist.
    ks = (0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 5.0, 8.0)
    rs = (0.125, 0.25, 0.5, 0.75, 1.0, 2.0, 4.0)
    for k, r, sgn, ef, s in itertools.product(ks, rs, (1.0, -1.0), (0.0, 0.5, 1.0, 2.0), (1.0, 0.5, 2.0)):
        rows.append(((e := ef * r), 0.0, -k, 0.0, 0.0, sgn * s, r))
    # tangent rays whose |oc| is exact: (e, k, len) a Pythagorean triple scaled by a power of two, r = e: disc == 0
    for (a, b_, _), j, sgn, swap in itertools.product(PYTHAGOREAN, range(-6, 3), (1.0, -1.0), (False, True)):
        e, k = (b_, a) if swap else (a, b_)
        rows.append((e * 2.0 ** j, 0.0, -k * 2.0 ** j, 0.0, 0.0, sgn, e * 2.0 ** j))
    # r == 0 (a ray through the centre has disc == 0), r < 0 (r * r is that of |r|), subnormal r (r * r == 0)
    for k, sgn, e in itertools.product(ks, (1.0, -1.0), (0.0, 0.5)):
        for r in (0.0, -0.0, -0.5, -1.0, -2.0, 1e-40, -1e-40, 1e-45, 3e-39):
            rows.append((e, 0.0, -k, 0.0, 0.0, sgn, r))
    # |same| == 2 / |diff| == 2 with an INEXACT square root (the dyadic rows above give quotient and halved roots the same bits, so
    # a `>= 2` for `> 2` would not show in them): k -+ sqrt(r^2 - e^2) = 1 in f32 and its neighbours, kept where the classifier
    # finds the equality
    cand = []
    for r, ef, side, ulp in itertools.product((0.3, 0.5, 0.7, 0.9, 1.1, 1.3, 1.7, 2.5), (0.1, 0.3, 0.45, 0.6, 0.75, 0.9), (1.0, -1.0),
                                              range(-3, 4)):
        e = float(F(ef * r))
        k = F(1.0 - side * np.sqrt(max(float(F(r)) ** 2 - e * e, 0.0)))
        for _ in range(abs(ulp)):
            k = np.nextafter(k, F(np.inf if ulp > 0 else -np.inf))
        cand.append((e, 0.0, -float(k), 0.0, 0.0, 1.0, float(F(r))))
    cand = np.array(cand, np.float64)
    probe = np.zeros((len(cand), 12), np.float32)
    probe[:, 0:3], probe[:, 3:6], probe[:, 9], probe[:, 10], probe[:, 11] = cand[:, 0:3], cand[:, 3:6], cand[:, 6], T_MIN, T_MAX
    cp = classify_sphere(probe)
    rows += [tuple(x) for x in cand[cp["|same|==2"] | cp["|diff|==2"]]]
    loc = np.array(rows, np.float64)
    recs = []
    for rot, cen in zip(range(3), CENTRES):
        cen = np.array(cen)
        o, d = _perm([loc[:, 0:3], loc[:, 3:6]], rot)
        g = np.zeros((len(loc), 12), np.float32)
        g[:, 0:3], g[:, 3:6], g[:, 6:9], g[:, 9] = o + cen, d, cen, loc[:, 6]
        recs.append(g)
    geo = np.concatenate(recs)
    out = [_with_windows(geo, _sphere_roots)]
    # non-finite operands: one field of a plain hitting record replaced by +-inf / NaN, every field in turn
    base = np.array([0.25, -0.5, -3.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, T_MIN, T_MAX], np.float32)
    nf = []
    for field, val, k in itertools.product(range(12), (np.inf, -np.inf, np.nan), (1.0, 2.0, 4.0)):
        b = base.copy()
        b[2] = -3.0 * k
        b[field] = val
        nf.append(b)
    out.append(np.array(nf, np.float32))
    # the discriminant overflows to inf - inf: every operand finite, disc NaN
    big = []
    for k, r in itertools.product((1e19, 3e19, 1e20, 1e25, 1e30, 3e30, 1e35, 3e37), (1e19, 1e20, 1e25, 1e30, 1e35, 1e37, 2e19, 5e22, 3e38)):
        for sgn in (1.0, -1.0):
            big.append((0.0, 0.0, -k, 0.0, 0.0, sgn, 0.0, 0.0, 0.0, r, T_MIN, T_MAX))
    out.append(np.array(big, np.float32))
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------ triangle
TRIANGLE_CLASSES = (
    "det<-eps", "det==-eps", "det in band", "det==+eps", "det>eps", "det NaN",
    "u<0", "u==0", "0<u<1", "u==1", "u>1", "u NaN",          # (of the records whose det passes)
    "v<0", "v==0",                                           # (of the records whose u passes)
    "u+v<1", "u+v==1", "u+v>1",
    "dist<=eps", "dist>eps",                                 # (of the records whose u, v pass)
    "dist==t_min", "dist==t_max",
    "two equal vertices", "collinear vertices",
)


def classify_triangle(rec, ray_new: bool = False):
    t = R.triangle(rec, ray_new)
    r = np.ascontiguousarray(rec).view(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        det, u, v, upv, dist = t["det"], t["u"], t["v"], t["upv"], t["dist"]
        l0, l1, l2 = t["live0"], t["live1"], t["live2"]
        A, B, C = r[:, 6:9], r[:, 9:12], r[:, 12:15]
        equal = (A == B).all(axis=1) | (A == C).all(axis=1) | (B == C).all(axis=1)
        coll = ~equal & (np.cross(B - A, C - A) == 0.0).all(axis=1)       # (exact for the dyadic vertices that build this class)
        c = {
            "det<-eps": det < -EPS, "det==-eps": det == -EPS, "det in band": (det < EPS) & (det > -EPS), "det==+eps": det == EPS,
            "det>eps": det > EPS, "det NaN": np.isnan(det),
            "u<0": l0 & (u < F(0.0)), "u==0": l0 & (u == F(0.0)), "0<u<1": l0 & (u > F(0.0)) & (u < F(1.0)), "u==1": l0 & (u == F(1.0)),
            "u>1": l0 & (u > F(1.0)), "u NaN": l0 & np.isnan(u),
            "v<0": l1 & (v < F(0.0)), "v==0": l1 & (v == F(0.0)),
            "u+v<1": l1 & (upv < F(1.0)), "u+v==1": l1 & (upv == F(1.0)), "u+v>1": l1 & (upv > F(1.0)),
            "dist<=eps": l2 & (dist <= EPS), "dist>eps": l2 & (dist > EPS),
            "dist==t_min": t["root"] & (dist == t["t_min"]), "dist==t_max": t["root"] & (dist == t["t_max"]),
            "two equal vertices": equal, "collinear vertices": coll,
        }
    assert tuple(c) == TRIANGLE_CLASSES
    return c


def _triangle_roots(geo):
    t = R.triangle(geo)
    d = np.where(t["root"], t["dist"], F(1.0)).astype(np.float32)
    return d, d


@functools.lru_cache(maxsize=None)
def triangle_directed():
    # A = 0, B = (sx, 0, 0), C = (0, sy, 0), d = (0, 0, -m), o = (x sx, y sy, z m): with powers of two for sx, sy, m every product is
    # exact and u = x, v = y, dist = z, det = sx sy m.  Swapping B and C turns the face round (det < 0).
    rows = []
    uv = (-0.25, 0.0, 0.25, 0.5, 0.75, 1.0, 1.25)
    zs = (float(EPS), float(np.nextafter(EPS, F(1.0))), float(np.nextafter(EPS, F(0.0))), 2.0 ** -20, 0.0, -1.0, 1.0, 4.0)
    for (sx, sy), m, x, y, z, swap in itertools.product(((1.0, 1.0), (0.5, 2.0), (4.0, 0.25), (2.0, 2.0)), (0.5, 1.0, 2.0), uv, uv, zs,
                                                        (False, True)):
        B, C = (sx, 0.0, 0.0), (0.0, sy, 0.0)
        o = (x * sx, y * sy, z * m)
        if swap:
            B, C, o = C, B, (y * sx, x * sy, z * m)
        rows.append(o + (0.0, 0.0, -m) + (0.0, 0.0, 0.0) + B + C)
    # det at and round +-eps: B.x = +-eps / (m sy) (a power-of-two quotient: exact) and its neighbours
    e = float(EPS)
    for sy, m, sgn, x, y in itertools.product((0.5, 1.0, 2.0, 4.0), (0.5, 1.0, 2.0), (1.0, -1.0), (0.0, 0.25, 0.5, 1.0), (0.0, 0.25, 0.5)):
        bx = F(sgn * e / (m * sy))
        for b in (bx, np.nextafter(bx, F(0.0)), np.nextafter(bx, F(sgn))):
            rows.append((x * float(b), y * sy, m) + (0.0, 0.0, -m) + (0.0, 0.0, 0.0) + (float(b), 0.0, 0.0) + (0.0, sy, 0.0))
    # degenerate faces: two equal vertices, collinear vertices (det == 0)
    for k, m, x in itertools.product((0.5, 1.0, 2.0, 4.0), (0.5, 1.0, 2.0), (0.0, 0.25, 0.5, 0.75, 1.0, 1.5)):
        P, Q = (k, 0.25, 0.0), (0.0, k, 0.5)
        for A, B, C in ((P, P, Q), (P, Q, P), (Q, P, P), (P, P, P)):
            rows.append((x, x, m) + (0.0, 0.0, -m) + A + B + C)
        for A, B, C in (((0.0, 0.0, 0.0), (k, k, 0.0), (2 * k, 2 * k, 0.0)), ((k, 0.0, 0.0), (0.0, 0.0, 0.0), (-k, 0.0, 0.0)),
                        ((0.0, k, 1.0), (0.0, 2 * k, 1.0), (0.0, 4 * k, 1.0)), ((1.0, 1.0, 1.0), (1.0 + k, 1.0, 1.0), (1.0 + 3 * k, 1.0, 1.0))):
            rows.append((x, x, m) + (0.0, 0.0, -m) + A + B + C)
    loc = np.array(rows, np.float64)
    geo = []
    for rot in range(3):
        g = np.zeros((len(loc), 17), np.float32)
        for j, v in enumerate(_perm([loc[:, 3 * i:3 * i + 3] for i in range(5)], rot)):
            g[:, 3 * j:3 * j + 3] = v
        geo.append(g)
    geo = np.concatenate(geo)
    out = [_with_windows(geo, _triangle_roots)[np.tile(np.arange(9) < 3, len(geo))]]          # windows: default, (dist, ..), (.., dist)
    # non-finite operands: det NaN (a vertex or the direction), u NaN with a finite det (the origin)
    base = np.array([0.25, 0.25, 1.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, T_MIN, T_MAX], np.float32)
    nf = []
    for field, val, k in itertools.product(range(15), (np.inf, -np.inf, np.nan), (0.5, 1.0, 2.0, 4.0)):
        b = base.copy()
        b[9], b[13] = k, k
        b[field] = val
        nf.append(b)
    out.append(np.array(nf, np.float32))
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------ boxes
AABB_CLASSES = tuple(f"d.{a} {s}" for a in "xyz" for s in ("+", "-", "+0", "-0")) + (
    "0*inf slab", "ray_min==ray_max", "ray_max==0", "origin inside", "zero extent", "empty box", "overflowing products",
    "NaN slab product")
# "NaN slab product": a (plane - origin) * (1 / d) that is NaN.  With a zero direction component that is the 0 * inf slab; with a
# FINITE inverse direction it takes a NaN origin component (or inf - inf, or inf * 0 from an infinite direction component).  The
# reference's `if x < y` min / max keep such a NaN when it is their second operand (the box then fails), fminf / fmaxf always drop it: intersects_aabb_finite
# is NOT intersects_aabb there (found by tests/test_gpu_operands.py; 123 of 2^20 seeded records).  No hit depends on it: a NaN origin
# component makes every sphere's discriminant and every triangle's u NaN, so whatever candidates the box test admits are misses.
# The records stay in the corpus as the counter-example; the equality of the two forms is claimed where no slab product is NaN.
# the classes every record of which has a zero direction component (RayAux::finite is false there by definition)
AABB_ZERO_DIR = tuple(f"d.{a} {s}" for a in "xyz" for s in ("+0", "-0")) + ("0*inf slab",)


def classify_aabb(rec):
    r = np.ascontiguousarray(rec).view(np.float32)
    o, d, lo, hi = ([r[:, 3 * i + k] for k in range(3)] for i in range(4))
    passes, rmin, rmax, finite = R.aabb(o, d, lo, hi)
    c = {}
    with np.errstate(all="ignore"):
        for k, a in enumerate("xyz"):
            zero = d[k] == F(0.0)
            c[f"d.{a} +"] = d[k] > F(0.0)
            c[f"d.{a} -"] = d[k] < F(0.0)
            c[f"d.{a} +0"] = zero & ~np.signbit(d[k])
            c[f"d.{a} -0"] = zero & np.signbit(d[k])
        c["0*inf slab"] = np.any([(d[k] == F(0.0)) & ((lo[k] - o[k] == F(0.0)) | (hi[k] - o[k] == F(0.0))) for k in range(3)], axis=0)
        c["ray_min==ray_max"] = rmin == rmax
        c["ray_max==0"] = rmax == F(0.0)
        c["origin inside"] = np.all([(lo[k] < o[k]) & (o[k] < hi[k]) for k in range(3)], axis=0)
        c["zero extent"] = np.any([lo[k] == hi[k] for k in range(3)], axis=0)
        c["empty box"] = np.any([lo[k] > hi[k] for k in range(3)], axis=0)
        prods = [(b[k] - o[k]) * (F(1.0) / d[k]) for k in range(3) for b in (lo, hi)]
        c["overflowing products"] = np.isfinite(r).all(axis=1) & np.all([d[k] != F(0.0) for k in range(3)], axis=0) & \
            np.any([~np.isfinite(p) for p in prods], axis=0)
        c["NaN slab product"] = np.any([np.isnan(p) for p in prods], axis=0)
    assert tuple(c) == AABB_CLASSES
    c["finite"] = finite
    c["ordered"] = ~c["empty box"] & ~np.isnan(r[:, 6:12]).any(axis=1)
    return c


@functools.lru_cache(maxsize=None)
def aabb_directed():
    comps = (1.0, -1.0, 0.0, -0.0, 0.5, -2.0)
    boxes = (((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), ((0.0, 0.5, -2.0), (4.0, 0.75, -1.0)), ((-1.0, -1.0, -1.0), (-1.0, 1.0, 1.0)),
             ((2.0, 2.0, 2.0), (2.0, 2.0, 2.0)), ((1.0, -1.0, -1.0), (-1.0, 1.0, 1.0)), ((-1.0, 1.0, -1.0), (1.0, -1.0, 1.0)))
    # origins relative to the box as (lo + f * (hi - lo)) per axis: inside, on a plane, on the exit face, outside before / after, on
    # the line through an edge
    fr = ((0.5, 0.5, 0.5), (0.0, 0.5, 0.5), (1.0, 0.5, 0.5), (0.5, 0.0, 1.0), (-1.0, 0.5, 0.5), (2.0, 0.5, 0.5), (-0.5, -0.5, 0.5),
          (-1.0, -1.0, -1.0), (1.5, 1.5, 1.5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (-0.5, 0.5, -0.5))
    rows = []
    for d, (lo, hi), f in itertools.product(itertools.product(comps, repeat=3), boxes, fr):
        o = tuple(l + t * (h - l) for l, h, t in zip(lo, hi, f))
        rows.append(o + d + lo + hi)
    # coordinates at which (plane - origin) * (1 / d) overflows: around 1e19 against small direction components, and above
    for (m, s), d, sg in itertools.product(((1e19, 1e-20), (1e20, 1e-19), (3e25, 1e-15), (1e30, 1e-10), (1e38, 0.05), (2e38, 0.5)),
                                           itertools.product((1.0, -1.0), repeat=3), ((1.0, 1.0), (-1.0, 1.0), (0.5, 2.0))):
        lo, hi = (sg[0] * m,) * 3, ((sg[0] + sg[1]) * m,) * 3
        for o in ((0.0, 0.0, 0.0), (-m, -m, -m), (m, 0.0, -m)):
            rows.append(o + tuple(s * c for c in d) + tuple(min(a, b) for a, b in zip(lo, hi)) + tuple(max(a, b) for a, b in zip(lo, hi)))
    # a NaN origin component under a finite inverse direction, the ray otherwise through the box: the counter-example of
    # "NaN slab product" above (the reference: no; min / max that drop NaN: yes)
    for d, k, (lo, hi), t in itertools.product(itertools.product((1.0, -1.0), repeat=3), range(3), boxes[:2], (2.0, 3.0, 5.0)):
        mid = tuple(0.5 * (a + b) for a, b in zip(lo, hi))
        o = [m - t * c for m, c in zip(mid, d)]
        o[k] = float("nan")
        rows.append(tuple(o) + d + lo + hi)
    with np.errstate(over="ignore"):                                      # (the largest boxes reach +inf: non-finite operands)
        return np.array(rows, np.float32)


def join_boxes(lo_a, hi_a, lo_b, hi_b):
    """AABB::join as f32 min / max (B/aabb.rs:357-372): exact, no rounding"""
    return np.fmin(lo_a, lo_b), np.fmax(hi_a, hi_b)


def chain_records(aabb_rec, seed=11):
    """CHAIN records of AABB records: the leaf box is the record's, the outer box its join with a second box (another record's,
    moved by a dyadic offset); empty leaves are left out (a BVH holds none)."""
    r = aabb_rec[classify_aabb(aabb_rec)["ordered"]]
    rng = np.random.default_rng(seed)
    other = r[rng.permutation(len(r))]
    off = rng.choice(np.array([-2.0, -0.5, 0.0, 0.25, 1.0, 8.0], np.float32), size=(len(r), 1))
    with np.errstate(all="ignore"):
        lo, hi = join_boxes(r[:, 6:9], r[:, 9:12], other[:, 6:9] + off, other[:, 9:12] + off)
    return np.concatenate([r, lo, hi], axis=1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ as u8, normalize, RNG
AS_U8_CLASSES = ("NaN", "+inf", "-inf", "negative", "-0", "integer k", "just below k", "just above k", "subnormal")


def classify_as_u8(rec):
    v = np.ascontiguousarray(rec).view(np.float32)[:, 0]
    with np.errstate(all="ignore"):
        integer = np.isfinite(v) & (v == np.trunc(v)) & (v >= F(0.0)) & (v <= F(256.0)) & ~((v == 0) & np.signbit(v))
        below = np.nextafter(v, F(np.inf))
        above = np.nextafter(v, F(-np.inf))
        k_of = lambda w: np.isfinite(w) & (w == np.trunc(w)) & (w >= F(0.0)) & (w <= F(256.0))      # noqa: E731
        c = {"NaN": np.isnan(v), "+inf": v == F(np.inf), "-inf": v == F(-np.inf), "negative": v < F(0.0),
             "-0": (v == F(0.0)) & np.signbit(v), "integer k": integer, "just below k": ~integer & k_of(below),
             "just above k": ~integer & k_of(above), "subnormal": (v != F(0.0)) & (np.abs(v) < TINY)}
    assert tuple(c) == AS_U8_CLASSES
    return c


@functools.lru_cache(maxsize=None)
def as_u8_directed():
    k = np.arange(257, dtype=np.float32)
    nan = (np.arange(FLOOR, dtype=np.uint32) * np.uint32(0x10001) + np.uint32(0x7F800001)).view(np.float32)
    nan2 = (nan.view(np.uint32) | np.uint32(0x80000000)).view(np.float32)
    sub = (np.arange(1, 2 * FLOOR + 1, dtype=np.uint32) * np.uint32(0xFFFF)).view(np.float32)
    # +inf, -inf and -0 have one encoding each: the floor is met by repetition
    one = np.repeat(np.array([np.inf, -np.inf, -0.0], np.float32), FLOOR)
    neg = -np.geomspace(1e-30, 1e30, 2 * FLOOR).astype(np.float32)
    v = np.concatenate([k, np.nextafter(k, F(np.inf)), np.nextafter(k, F(-np.inf)), nan, nan2, sub, -sub, one, neg, k + F(0.5),
                        k * F(255.999) / F(256.0)])
    return v.reshape(-1, 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def normalize_directed():
    mags = np.array([0.0, -0.0, 1e-45, 1e-40, 1e-30, 1e-23, 1e-19, 1e-10, 1e-3, 0.5, 1.0, 3.0, 1e3, 1e10, 1e18, 1.8e19, 1.9e19, 1e20,
                     1e30, 3e38, np.inf, -np.inf, np.nan], np.float32)
    v = np.array(list(itertools.product(mags, repeat=3)), np.float32)
    sg = np.array(list(itertools.product((1.0, -1.0), repeat=3)), np.float32)
    return np.concatenate([v, (v[:4096] * sg[np.arange(4096) % 8])]).astype(np.float32)


def rng_seeds(n=1 << 16, seed=5):
    """u64 seeds as (n, 2) uint32 (low, high): 0, 2^64 - 1, values round multiples of PHI (the stride of sample_seed), random"""
    m = (1 << 64) - 1
    s = [0, 1, m, m - 1, 1 << 32, (1 << 32) - 1, 1 << 63]
    for k in range(1, 2049):
        for dlt in (-1, 0, 1):
            s.append((k * PHI + dlt) & m)
            s.append((4 * k * PHI + dlt) & m)
    s = np.array(s, np.uint64)
    rest = np.random.default_rng(seed).integers(0, m, size=n - len(s), dtype=np.uint64, endpoint=True)
    a = np.concatenate([s, rest])
    return np.stack([(a & np.uint64(0xFFFFFFFF)).astype(np.uint32), (a >> np.uint64(32)).astype(np.uint32)], axis=1)


# ------------------------------------------------------------------------------------------------ seeded random records
def _coords(rng, shape, wide):
    """log-uniform magnitudes with random signs: 1e-3 ... 1e3, or (wide) 1e-30 ... 1e30"""
    e = rng.uniform(-30.0, 30.0, shape) if wide else rng.uniform(-3.0, 3.0, shape)
    return (np.sign(rng.uniform(-1.0, 1.0, shape)) * 10.0 ** e).astype(np.float32)


def _sprinkle(rng, rec, cols, rate=1.0 / 256):
    """a record in `rate` gets one field of `cols` replaced by +-0, +-inf or NaN"""
    n = len(rec)
    pick = np.nonzero(rng.uniform(size=n) < rate)[0]
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    rec[pick, rng.integers(0, cols, len(pick))] = vals[rng.integers(0, len(vals), len(pick))]
    return rec


def _mix(rng, n, make):
    """nine tenths at the scenes' magnitudes, a tenth wide"""
    nw = n // 10
    return np.concatenate([make(rng, n - nw, False), make(rng, nw, True)])


def _aimed_dir(rng, o, target, spread):
    with np.errstate(all="ignore"):
        d = (target - o) + spread * rng.normal(size=o.shape).astype(np.float32)
        unit = rng.uniform(size=(len(o), 1)) < 0.5                       # half of them normalised, as the engines' rays are
        ln = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1, keepdims=True))
        return np.where(unit & (ln > 0) & np.isfinite(ln), d / ln, d).astype(np.float32)


def sphere_random(n, seed=1):
    def make(rng, m, wide):
        with np.errstate(all="ignore"):
            o, cen = _coords(rng, (m, 3), wide), _coords(rng, (m, 3), wide)
            r = np.abs(_coords(rng, (m, 1), wide))
            d = _aimed_dir(rng, o, cen, r * rng.uniform(0.0, 1.5, (m, 1)).astype(np.float32))
            w = np.tile(np.array([T_MIN, T_MAX], np.float32), (m, 1))
        return np.concatenate([o, d, cen, r, w], axis=1).astype(np.float32)
    rng = np.random.default_rng(seed)
    return _sprinkle(rng, _mix(rng, n, make), 12)


def triangle_random(n, seed=2):
    def make(rng, m, wide):
        with np.errstate(all="ignore"):
            o = _coords(rng, (m, 3), wide)
            A, B, C = (_coords(rng, (m, 3), wide) for _ in range(3))
            bu, bv = rng.uniform(-0.2, 1.2, (m, 1)).astype(np.float32), rng.uniform(-0.2, 1.2, (m, 1)).astype(np.float32)
            d = _aimed_dir(rng, o, A + bu * (B - A) + bv * (C - A), np.float32(0.0))
            w = np.tile(np.array([T_MIN, T_MAX], np.float32), (m, 1))
        return np.concatenate([o, d, A, B, C, w], axis=1).astype(np.float32)
    rng = np.random.default_rng(seed)
    return _sprinkle(rng, _mix(rng, n, make), 17)


def aabb_random(n, seed=3):
    def make(rng, m, wide):
        with np.errstate(all="ignore"):
            o, p, q = (_coords(rng, (m, 3), wide) for _ in range(3))
            lo, hi = np.minimum(p, q), np.maximum(p, q)
            f = rng.uniform(-0.3, 1.3, (m, 3)).astype(np.float32)
            d = _aimed_dir(rng, o, lo + f * (hi - lo), np.float32(0.0))
            d[rng.uniform(size=(m, 3)) < 1.0 / 64] = 0.0                 # axis-parallel rays: the chain is walked for these
        return np.concatenate([o, d, lo, hi], axis=1).astype(np.float32)
    rng = np.random.default_rng(seed)
    return _sprinkle(rng, _mix(rng, n, make), 6)                         # (non-finite values in the ray only: the boxes stay ordered)


def normalize_random(n, seed=4):
    rng = np.random.default_rng(seed)
    return _sprinkle(rng, _mix(rng, n, lambda g, m, wide: _coords(g, (m, 3), wide)), 3)


def as_u8_random(n, seed=6):
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.uniform(-8.0, 264.0, n // 2).astype(np.float32), rng.integers(0, 1 << 32, n - n // 2, dtype=np.uint64)
                        .astype(np.uint32).view(np.float32)])
    return v.reshape(-1, 1)


def describe(classes, i):
    """the class tuple of record i: the names of the classes it belongs to"""
    return tuple(k for k, m in classes.items() if m[i])


# ------------------------------------------------------------------------------------------------ the corpus as rays on scenes
SPHERE_EXACT = ("disc==0", "|same|==2", "|diff|==2", "root==t_min", "root==t_max", "origin on surface")
TRIANGLE_EXACT = ("det==-eps", "det==+eps", "u==0", "u==1", "v==0", "u+v==1", "dist==t_min", "dist==t_max")


def primitive_groups(rec, prim_cols, classes, exact, cap):
    """The finite directed records grouped by their primitive (the words prim_cols): at most `cap` groups, chosen greedily so that
    each class of `exact` is met by as many groups as possible — a group is scored by the classes it holds that the chosen groups
    have not yet covered FLOOR times, then by its number of exact-equality records.  Returns [(primitive words, record indices)]."""
    ok = np.isfinite(rec).all(axis=1)
    keys = np.ascontiguousarray(rec[:, prim_cols]).view(np.uint32)
    _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    per = []
    for g in range(len(first)):
        idx = np.nonzero((inv == g) & ok)[0]
        if len(idx):
            per.append((first[g], idx, {k: int(classes[k][idx].sum()) for k in exact}))
    have = {k: 0 for k in exact}
    out = []
    while per and len(out) < cap:
        score = [(sum(1 for k in exact if have[k] < FLOOR and cnt[k]), sum(cnt.values())) for _, _, cnt in per]
        j = max(range(len(per)), key=lambda i: score[i])
        f, idx, cnt = per.pop(j)
        for k in exact:
            have[k] += cnt[k]
        out.append((rec[f, prim_cols], idx))
    return out
