"""Operands for the device functions that sample a light or scatter a ray: per family a numpy restatement, a classifier, a directed
corpus and seeded random records.

The record layouts are those of ray_tracer_s8_amd/csrc/rt_unit_sampling.hip.h (32-bit words per record); families DIRECT, WEIGHT_IP,
CONE, CONE_VIEW and NEE_VIEW take the layouts of the g++ harnesses tests/host/{direct,lightpick,cone,nee}_host.cpp, so one corpus
feeds g++, numpy and the device.  The restatements are the lines of csrc/rt_direct_math.h, csrc/rt_nee_math.h and the shade lines
of csrc/rt_path_steps.hip.h on float32 arrays, one IEEE operation per numpy operation in the written order, every operation through
an `Ops` object: the plain one is numpy, `TraceOps` also records which records met a subnormal division result, a subnormal square
root operand, any subnormal, an inexact last product of a dot, an inexact reciprocal — the classifier's evidence — and the mutated
ones are the negative controls of tests/test_sampling_corpus.py.  (tests/_direct_np.py, _lightpick_np.py, _cone_np.py and _nee_np.py
restate the same two headers function by function for the scene tests; both sets are held to the g++ harnesses bit for bit, so a
change to a header's arithmetic is made in both.)  A classifier is a function of the records alone, through the
restatement's intermediate values.  The class lists are ENUMERATED, not derived from what occurred; tests/test_sampling_corpus.py
holds every listed class to FLOOR records of the directed corpus.

Classes one might list that no f32 operand reaches, and what stands in their place (DESIGN.md 9.3 has the arguments):
  * "len subnormal": len = sqrt(d2) >= 2^-74.5 for every positive f32 d2.  In its place: d2 underflows to 0 under a non-zero v, so
    that v / len is +-inf ("d2==0, v!=0").
  * "u = 1 - 2^-24 with an M whose product rounds up to M": M - M 2^-24 lies at least half a spacing below M for every M <= 2^23, so
    the product never rounds up and pick_light's clamp is dead code for u < 1.  Kept: "u==1-2^-24" over every M, and "u==1", the one
    operand (outside the contract u in [0, 1), but defined: the product is M exactly) that takes the clamp.
  * "d2 = inf failing alone": w = v / inf is 0 or NaN, so cs and cl are never positive; the class is "d2==inf".
  * a subnormal division result or square root operand in a family that has no such operation or cannot reach it: WEIGHT_IP and
    NEE_VIEW take no square root, PICK_POWER neither divides nor takes a root, CONE_VIEW's only root is sqrt(1 - q) with 1 - q >= 2^-24 in the
    regime, SKY's only division 1 / len has len <= 2^64.
"""
from __future__ import annotations

import contextlib
import functools
import itertools

import numpy as np

F = np.float32
U32 = np.uint32
FLOOR = 64
ZERO, HALF, ONE, TWO, FOUR = F(0), F(0.5), F(1), F(2), F(4)
PI = F(np.pi)
INF = F(np.inf)
TINY = F(np.finfo(np.float32).tiny)                      # the smallest normal
Q_MIN = F(2.0 ** -10)
MAX_LIGHTS = 1 << 23
PICK_TABLE = 16
DC2_UNIT = F(2.0 ** -130)                                # from here up dc2's rounding is at most 2^-150 / 2^-130 = 2^-20 of it
U_LAST = F(1) - F(2.0 ** -24)                            # the largest u01

DIRECT, WEIGHT_IP, PICK_POWER, CONE, CONE_VIEW, NEE_VIEW, SCATTER, SKY = range(8, 16)
NAMES = {DIRECT: "direct", WEIGHT_IP: "weight_ip", PICK_POWER: "pick_power", CONE: "cone", CONE_VIEW: "cone_view",
         NEE_VIEW: "nee_view", SCATTER: "scatter", SKY: "sky"}
WORDS = {DIRECT: (28, 16), WEIGHT_IP: (6, 2), PICK_POWER: (4 + PICK_TABLE, 2), CONE: (16, 20), CONE_VIEW: (14, 5), NEE_VIEW: (14, 8),
         SCATTER: (10, 7), SKY: (3, 3)}
# the output words that are flags (compared as booleans) or counts (compared as integers); every other word is a float32 (equal
# bits, or NaN on both sides)
FLAG_WORDS = {DIRECT: (7,), WEIGHT_IP: (), PICK_POWER: (), CONE: (1, 14), CONE_VIEW: (2, 3), NEE_VIEW: (3,), SCATTER: (6,), SKY: ()}
COUNT_WORDS = {DIRECT: (0,), WEIGHT_IP: (), PICK_POWER: (0, 1), CONE: (), CONE_VIEW: (), NEE_VIEW: (), SCATTER: (), SKY: ()}
# rt_debug_unit's units and the families each carries
UNITS = {"direct": 3, "nee": 4, "bounce": 5, "trace": 6}
CARRIES = {"direct": (DIRECT, WEIGHT_IP, PICK_POWER, CONE), "nee": (DIRECT, WEIGHT_IP, PICK_POWER, CONE, CONE_VIEW, NEE_VIEW),
           "bounce": (SCATTER, SKY), "trace": (SCATTER, SKY)}


def nb(x, up):
    return np.nextafter(F(x), F(np.inf if up else -np.inf))


def is_sub(x):
    """a subnormal float32 (not zero)"""
    with np.errstate(all="ignore"):
        return (x != ZERO) & (np.abs(x) < TINY)


# ------------------------------------------------------------------------------------------------ the operations
class Ops:
    """One IEEE binary32 operation per call, on float32 arrays (numpy's are correctly rounded)."""

    def add(self, a, b):
        return a + b

    def sub(self, a, b):
        return a - b

    def mul(self, a, b):
        return a * b

    def div(self, a, b):
        return a / b

    def sqrt(self, a):
        return np.sqrt(a)

    def vdiv(self, v, ln):
        """x / len per component: the normalisations"""
        return tuple(self.div(x, ln) for x in v)

    def dot(self, a, b):
        """glam's dot3 order: (x x' + y y') + z z'"""
        return self.add(self.add(self.mul(a[0], b[0]), self.mul(a[1], b[1])), self.mul(a[2], b[2]))

    @contextlib.contextmanager
    def only(self, mask):
        yield


PLAIN = Ops()


class TraceOps(Ops):
    """PLAIN, and which records met what (masks over the records; `only` limits the marking to the records of an arm)."""
    KEYS = ("div subnormal", "sqrt subnormal", "subnormal", "dot inexact", "rcp inexact")

    def __init__(self, n):
        self.m = {k: np.zeros(n, bool) for k in self.KEYS}
        self.act = np.ones(n, bool)

    def _mark(self, key, cond):
        self.m[key] |= np.broadcast_to(cond, self.act.shape) & self.act

    def _seen(self, *xs):
        for x in xs:
            self._mark("subnormal", is_sub(np.asarray(x, F)))

    def add(self, a, b):
        r = a + b
        self._seen(a, b, r)
        return r

    def sub(self, a, b):
        r = a - b
        self._seen(a, b, r)
        return r

    def mul(self, a, b):
        r = a * b
        self._seen(a, b, r)
        return r

    def div(self, a, b):
        r = a / b
        self._seen(a, b, r)
        self._mark("div subnormal", is_sub(r))
        return r

    def sqrt(self, a):
        r = np.sqrt(a)
        self._seen(a, r)
        self._mark("sqrt subnormal", is_sub(np.asarray(a, F)))
        return r

    def vdiv(self, v, ln):
        rcp = ONE / ln
        exact = np.isfinite(rcp) & (rcp.astype(np.float64) * np.asarray(ln, np.float64) == 1.0)
        self._mark("rcp inexact", ~exact)
        return super().vdiv(v, ln)

    def dot(self, a, b):
        p = np.asarray(a[2], np.float64) * np.asarray(b[2], np.float64)
        self._mark("dot inexact", ~(p == self.mul(a[2], b[2]).astype(np.float64)))
        return super().dot(a, b)

    @contextlib.contextmanager
    def only(self, mask):
        old = self.act
        self.act = old & mask
        try:
            yield
        finally:
            self.act = old


class FusedDot(Ops):
    """mutation: dot3 with the last product fused — (x x' + y y') + z z' in float64, rounded once"""

    def dot(self, a, b):
        t = self.add(self.mul(a[0], b[0]), self.mul(a[1], b[1]))
        return (np.asarray(t, np.float64) + np.asarray(a[2], np.float64) * np.asarray(b[2], np.float64)).astype(F)


class RcpDiv(Ops):
    """mutation: x / len as x * (1 / len)"""

    def vdiv(self, v, ln):
        rcp = ONE / ln
        return tuple(x * rcp for x in v)


def _ftz(x):
    x = np.asarray(x, F)
    return np.where(is_sub(x), np.copysign(ZERO, x), x)


class FlushOps(Ops):
    """mutation: subnormal inputs and results flushed to zero (sign kept)"""

    def add(self, a, b):
        return _ftz(_ftz(a) + _ftz(b))

    def sub(self, a, b):
        return _ftz(_ftz(a) - _ftz(b))

    def mul(self, a, b):
        return _ftz(_ftz(a) * _ftz(b))

    def div(self, a, b):
        return _ftz(_ftz(a) / _ftz(b))

    def sqrt(self, a):
        return _ftz(np.sqrt(_ftz(a)))


# ------------------------------------------------------------------------------------------------ helpers of the restatements
def _f(rec):
    rec = np.ascontiguousarray(rec)
    assert rec.dtype.itemsize == 4
    return rec.view(F)


def _v(f, k):
    return (f[:, k], f[:, k + 1], f[:, k + 2])


def _vsub(o, a, b):
    return tuple(o.sub(x, y) for x, y in zip(a, b))


def _cross(o, a, b):
    return (o.sub(o.mul(a[1], b[2]), o.mul(a[2], b[1])), o.sub(o.mul(a[2], b[0]), o.mul(a[0], b[2])),
            o.sub(o.mul(a[0], b[1]), o.mul(a[1], b[0])))


def _where3(c, a, b):
    return tuple(np.where(c, x, y) for x, y in zip(a, b))


def _words(n, family):
    return np.zeros((n, WORDS[family][1]), U32)


def _put(out, k, x, mask=None):
    x = np.broadcast_to(np.asarray(x, F), (len(out),))
    w = np.ascontiguousarray(x).view(U32)
    out[:, k] = w if mask is None else np.where(mask, w, U32(0))


def _put3(out, k, v, mask=None):
    for j in range(3):
        _put(out, k + j, v[j], mask)


def _flag(out, k, b, mask=None):
    b = np.broadcast_to(b, (len(out),))
    out[:, k] = (b if mask is None else b & mask).astype(U32)


def pick_light(o, u, M, clamp=True):
    """k = min((uint32_t)(u * (float)M), M - 1)"""
    k = o.mul(u, M.astype(F)).astype(np.int64)
    return np.minimum(k, M.astype(np.int64) - 1) if clamp else k


def _light_geometry(o, P, n, L, nl, sphere):
    v = _vsub(o, L, P)
    d2 = o.dot(v, v)
    ln = o.sqrt(d2)
    w = o.vdiv(v, ln)
    cs = o.dot(n, w)
    c = o.dot(nl, w)
    cl = np.where(sphere, -c, np.abs(c))
    facing = (cs > ZERO) & (cl > ZERO) & (d2 > ZERO) & (d2 < INF)
    return dict(v=v, d2=d2, len=ln, w=w, cs=cs, c=c, cl=cl, facing=facing)


def _sphere_weight(o, cs, cl, r, ip, d2):
    return o.div(o.mul(o.mul(cs, cl), o.mul(o.mul(FOUR, o.mul(r, r)), ip)), d2)


def _triangle_weight(o, cs, cl, A, ip, d2):
    return o.div(o.mul(o.mul(cs, cl), o.mul(A, ip)), o.mul(PI, d2))


# ------------------------------------------------------------------------------------------------ the restatements
# Each returns (out words (n, words out) uint32, a dict of intermediate values); mut names the mutations of the negative controls.
def restate_direct(rec, o=PLAIN, mut=()):
    f, n = _f(rec), len(rec)
    out = _words(n, DIRECT)
    with np.errstate(all="ignore"):
        sphere, M = rec[:, 0] == 0, rec[:, 1]
        k = pick_light(o, f[:, 2], M, "no clamp" not in mut)
        P, nrm = _v(f, 3), _v(f, 6)
        with o.only(sphere):
            r = f[:, 12]
            Ls = tuple(o.add(c, o.mul(r, us)) for c, us in zip(_v(f, 9), _v(f, 13)))
        with o.only(~sphere):
            a, b, c = _v(f, 9), _v(f, 12), _v(f, 15)
            u1, u2 = f[:, 18], f[:, 19]
            usum = o.add(u1, u2)
            fold = (usum >= ONE) if "fold >=" in mut else (usum > ONE)
            v1, v2 = np.where(fold, o.sub(ONE, u1), u1), np.where(fold, o.sub(ONE, u2), u2)
            e1, e2 = _vsub(o, b, a), _vsub(o, c, a)
            Lt = tuple(o.add(a[j], o.add(o.mul(v1, e1[j]), o.mul(v2, e2[j]))) for j in range(3))
            nx = _cross(o, _vsub(o, a, b), _vsub(o, a, c))
            nn = o.dot(nx, nx)
            area = o.mul(HALF, o.sqrt(nn))
        L, nl = _where3(sphere, Ls, Lt), _where3(sphere, _v(f, 13), _v(f, 20))
        g = _light_geometry(o, P, nrm, L, nl, sphere)
        Mf = M.astype(F)
        with o.only(sphere):
            Ws = _sphere_weight(o, g["cs"], g["cl"], r, Mf, g["d2"])
        with o.only(~sphere):
            Wt = _triangle_weight(o, g["cs"], g["cl"], area, Mf, g["d2"])
        W = np.where(sphere, Ws, Wt)
        em = f[:, 26]
        rgb = tuple(o.mul(o.mul(al, em), W) for al in _v(f, 23))
        out[:, 0] = k.astype(U32)
        _put3(out, 1, L)
        _put(out, 4, g["d2"]), _put(out, 5, g["cs"]), _put(out, 6, g["cl"])
        _flag(out, 7, g["facing"])
        _put(out, 8, W)
        _put3(out, 9, rgb), _put3(out, 12, g["w"])
        _put(out, 15, area, ~sphere)
    return out, dict(g, sphere=sphere, M=M, u=f[:, 2], k=k, usum=usum, fold=fold, area=area, cross=nx, nn=nn, W=W, L=L, r=r)


def restate_weight_ip(rec, o=PLAIN, mut=()):
    f, n = _f(rec), len(rec)
    out = _words(n, WEIGHT_IP)
    with np.errstate(all="ignore"):
        sphere = rec[:, 0] == 0
        cs, cl, size, ip, d2 = (f[:, k] for k in range(1, 6))
        with o.only(sphere):
            Ws = _sphere_weight(o, cs, cl, size, ip, d2)
        with o.only(~sphere):
            Wt = _triangle_weight(o, cs, cl, size, ip, d2)
        W = np.where(sphere, Ws, Wt)
        _put(out, 0, W), _put(out, 1, W)
    return out, dict(sphere=sphere, W=W, d2=d2)


def restate_pick_power(rec, o=PLAIN, mut=()):
    f, n = _f(rec), len(rec)
    out = _words(n, PICK_POWER)
    with np.errstate(all="ignore"):
        u, M, total, M_big, c = f[:, 0], rec[:, 1], f[:, 2], rec[:, 3], f[:, 4:4 + PICK_TABLE]
        clamp = "no clamp" not in mut
        valid = (M >= 1) & (M <= PICK_TABLE) & (M_big >= 1) & (M_big <= MAX_LIGHTS)
        Mi = M.astype(np.int64)
        degenerate = ~((total > ZERO) & (total < INF))
        lower = u < HALF
        h = o.sub(u, HALF)
        x = o.mul(o.add(h, h), total)
        idx = np.arange(PICK_TABLE)[None, :]
        below = ((x[:, None] <= c) if "x <= c" in mut else (x[:, None] < c)) & (idx < Mi[:, None])
        first = np.where(below.any(axis=1), below.argmax(axis=1), Mi)          # the smallest k with x < c[k], or M
        k_pow = np.minimum(first, Mi - 1)
        k = np.where(degenerate, pick_light(o, u, M, clamp), np.where(lower, pick_light(o, o.add(u, u), M, clamp), k_pow))
        out[:, 0] = np.where(valid, k, 0).astype(U32)
        out[:, 1] = np.where(valid, pick_light(o, u, M_big, clamp), 0).astype(U32)
    return out, dict(u=u, M=M, total=total, M_big=M_big, c=c, valid=valid, degenerate=degenerate, lower=lower, x=x, first=first, k=k)


def _cone_axis(o, P, c, r):
    a = _vsub(o, c, P)
    dc2 = o.dot(a, a)
    r2 = o.mul(r, r)
    return a, dc2, r2, o.div(r2, dc2)


def _cone_regime(q, mut=()):
    return ((q > Q_MIN) if "q >" in mut else (q >= Q_MIN)) & (q < ONE)


def _cone_omc(o, q):
    return o.div(q, o.add(ONE, o.sqrt(o.sub(ONE, q))))


def restate_cone(rec, o=PLAIN, mut=()):
    f, n = _f(rec), len(rec)
    out = _words(n, CONE)
    with np.errstate(all="ignore"):
        P, c, r, x1, x2, s, nrm, ip = _v(f, 0), _v(f, 3), f[:, 6], f[:, 7], f[:, 8], f[:, 9], _v(f, 10), f[:, 13]
        a, dc2, r2, q = _cone_axis(o, P, c, r)
        reg = _cone_regime(q, mut)
        with o.only(reg):
            omc = _cone_omc(o, q)
            e = o.mul(s, omc)
            ct = o.sub(ONE, e)
            st = o.sqrt(o.mul(e, o.sub(TWO, e)))
            rs = o.sqrt(s)
            pos = s > ZERO
            with o.only(pos):
                cpd, spd = o.div(x1, rs), o.div(x2, rs)
            cp, sp = np.where(pos, cpd, ZERO), np.where(pos, spd, ZERO)
            dc = o.sqrt(dc2)
            w = o.vdiv(a, dc)
            sg = np.copysign(ONE, w[2])
            A = o.div(-ONE, o.add(sg, w[2]))
            Bq = o.mul(o.mul(w[0], w[1]), A)
            t1 = (o.add(ONE, o.mul(o.mul(sg, o.mul(w[0], w[0])), A)), o.mul(sg, Bq), -o.mul(sg, w[0]))
            t2 = (Bq, o.add(sg, o.mul(o.mul(w[1], w[1]), A)), -w[1])
            ka, kb = o.mul(st, cp), o.mul(st, sp)
            v = tuple(o.add(o.add(o.mul(ka, t1[j]), o.mul(kb, t2[j])), o.mul(ct, w[j])) for j in range(3))
            vv = o.dot(v, v)
            wn = o.vdiv(v, o.sqrt(vv))
            cs = o.dot(nrm, wn)
            facing = cs > ZERO
            W = o.mul(o.mul(cs, o.add(omc, omc)), ip)
            h_raw = o.sub(o.mul(r, r), o.mul(dc2, o.mul(st, st)))
            hh = np.where(h_raw > ZERO, h_raw, ZERO)
            ts = o.sub(o.mul(dc, ct), o.sqrt(hh))
            L = tuple(o.add(P[j], o.mul(ts, wn[j])) for j in range(3))
        _put(out, 0, q)
        _flag(out, 1, reg)
        _put3(out, 2, v, reg)
        for k, x in ((5, omc), (6, dc2), (7, dc), (8, ct), (9, st), (13, cs), (15, W), (19, vv)):
            _put(out, k, x, reg)
        _put3(out, 10, wn, reg), _put3(out, 16, L, reg)
        _flag(out, 14, facing, reg)
    return out, dict(a=a, dc2=dc2, r2=r2, q=q, reg=reg, s=s, w=w, h_raw=h_raw, cs=cs, facing=facing, W=W, vv=vv, n=nrm, ip=ip, x1=x1,
                     x2=x2, v=v, L=L, omc=omc)


def restate_cone_view(rec, o=PLAIN, mut=()):
    f, n = _f(rec), len(rec)
    out = _words(n, CONE_VIEW)
    with np.errstate(all="ignore"):
        org, nrm, d, c, r, ip = _v(f, 0), _v(f, 3), _v(f, 6), _v(f, 9), f[:, 12], f[:, 13]
        _, dc2, r2, q = _cone_axis(o, org, c, r)
        reg = _cone_regime(q, mut)
        cs = o.dot(nrm, d)
        with o.only(reg):
            omc_r = _cone_omc(o, q)
        omc = np.where(reg, omc_r, ZERO)
        samplable = reg & (cs > ZERO)
        W = o.mul(o.mul(cs, o.add(omc, omc)), ip)
        _put(out, 0, cs), _put(out, 1, omc)
        _flag(out, 2, reg), _flag(out, 3, samplable)
        _put(out, 4, W)
    return out, dict(dc2=dc2, r2=r2, q=q, reg=reg, cs=cs, samplable=samplable, n=nrm, W=W)


def restate_nee_view(rec, o=PLAIN, mut=()):
    f, n = _f(rec), len(rec)
    out = _words(n, NEE_VIEW)
    with np.errstate(all="ignore"):
        sphere, M = rec[:, 0] == 0, rec[:, 1]
        nrm, d, nh, dist, size, Win = _v(f, 2), _v(f, 5), _v(f, 8), f[:, 11], f[:, 12], f[:, 13]
        cs = o.dot(nrm, d)
        c = o.dot(nh, d)
        cl = np.where(sphere, -c, np.abs(c))
        d2 = o.mul(dist, dist)
        samplable = (cs > ZERO) & (cl > ZERO) & (d2 > ZERO) & (d2 < INF)
        Mf = M.astype(F)
        with o.only(sphere):
            Ws = _sphere_weight(o, cs, cl, size, Mf, d2)
        with o.only(~sphere):
            Wt = _triangle_weight(o, cs, cl, size, Mf, d2)
        W = np.where(sphere, Ws, Wt)
        wb = o.sub(ONE, o.div(ONE, o.add(ONE, W)))
        wl_in = o.div(ONE, o.add(ONE, Win))
        wb_in = o.sub(ONE, o.div(ONE, o.add(ONE, Win)))
        _put(out, 0, cs), _put(out, 1, cl), _put(out, 2, d2)
        _flag(out, 3, samplable)
        _put(out, 4, W), _put(out, 5, wb), _put(out, 6, wl_in), _put(out, 7, wb_in)
    return out, dict(sphere=sphere, cs=cs, c=c, cl=cl, d2=d2, samplable=samplable, W=W, wb=wb, Win=Win, wl_in=wl_in, wb_in=wb_in)


def _try_normalize(o, a):
    """glam try_normalize: a * (1 / length) when that reciprocal is finite and > 0"""
    rcp = o.div(ONE, o.sqrt(o.dot(a, a)))
    return (rcp > ZERO) & (rcp < INF), tuple(o.mul(x, rcp) for x in a), rcp


def unit_sphere_vec(o, x1, x2, sm):
    fct = o.mul(TWO, o.sqrt(o.sub(ONE, sm)))
    return (o.mul(x1, fct), o.mul(x2, fct), o.sub(ONE, o.mul(TWO, sm)))


def restate_scatter(rec, o=PLAIN, mut=()):
    f, n = _f(rec), len(rec)
    out = _words(n, SCATTER)
    with np.errstate(all="ignore"):
        d, nrm, rough, x1, x2, sm = _v(f, 0), _v(f, 3), f[:, 6], f[:, 7], f[:, 8], f[:, 9]
        us = unit_sphere_vec(o, x1, x2, sm)
        diffuse = tuple(o.add(a, b) for a, b in zip(us, nrm))
        dn2 = o.mul(TWO, o.dot(d, nrm))
        glossy = tuple(o.sub(a, o.mul(dn2, b)) for a, b in zip(d, nrm))
        pre = tuple(o.add(a, o.mul(rough, o.sub(b, a))) for a, b in zip(diffuse, glossy))
        ok, tn, rcp = _try_normalize(o, pre)
        xdir = _where3(ok, tn, nrm)
        ln = o.sqrt(o.dot(xdir, xdir))
        out_d = o.vdiv(xdir, ln)
        _put3(out, 0, us), _put3(out, 3, out_d)
        _flag(out, 6, ~ok)
    return out, dict(d=d, n=nrm, rough=rough, sm=sm, us=us, pre=pre, ok=ok, rcp=rcp, out=out_d)


def restate_sky(rec, o=PLAIN, mut=()):
    f, n = _f(rec), len(rec)
    out = _words(n, SKY)
    with np.errstate(all="ignore"):
        d = _v(f, 0)
        ok, tn, rcp = _try_normalize(o, d)
        ny = np.where(ok, tn[1], ZERO)
        t = o.add(o.mul(ny, HALF), ONE)
        omt = o.sub(ONE, t)
        rg = o.add(o.mul(ONE, t), o.mul(F(0.3), omt))
        _put(out, 0, rg), _put(out, 1, rg), _put(out, 2, o.add(o.mul(ONE, t), o.mul(F(0.8), omt)))
    return out, dict(d=d, ok=ok, ny=ny, rcp=rcp)


RESTATE = {DIRECT: restate_direct, WEIGHT_IP: restate_weight_ip, PICK_POWER: restate_pick_power, CONE: restate_cone,
           CONE_VIEW: restate_cone_view, NEE_VIEW: restate_nee_view, SCATTER: restate_scatter, SKY: restate_sky}


def expected(family, rec):
    """the words the device must store for the records"""
    return RESTATE[family](rec)[0]


def words_equal(family, got, want):
    """(n, words out) bool: count words equal, flag words equal as booleans, float words equal bits or NaN on both sides.  Any NaN
    matches any NaN: no output word of these families has a payload the restatement defines (every NaN here comes out of an
    arithmetic operation, whose payload and sign IEEE 754 leaves open, and none is passed through by a copy or a select alone)."""
    eq = (got == want) | (np.isnan(got.view(F)) & np.isnan(want.view(F)))
    for k in COUNT_WORDS[family]:
        eq[:, k] = got[:, k] == want[:, k]
    for k in FLAG_WORDS[family]:
        eq[:, k] = (got[:, k] != 0) == (want[:, k] != 0)
    return eq


# ------------------------------------------------------------------------------------------------ the classes
_TRACE = ("div subnormal", "sqrt subnormal")
_REGIME = ("q==pred(2^-10)", "q==2^-10", "q==succ(2^-10)", "q==pred(1)", "q==1", "q>1", "q==0", "q NaN", "dc2==0, q==inf", "dc2==inf",
           "r*r subnormal", "dc2 subnormal", "q subnormal")
CLASSES = {
    DIRECT: ("d2==0", "d2 subnormal", "d2==inf", "d2==0, v!=0", "cs==0", "cl==0", "fails on cs alone", "fails on cl alone",
             "fails on d2>0 alone", "facing", "sphere cl>0", "sphere cl<0", "triangle c>0", "triangle c<0",
             "u1+u2<1", "u1+u2==1", "u1+u2==succ(1)", "area 0: equal vertices", "area 0: collinear", "subnormal cross product",
             "u==0", "u==1-2^-24", "u==1", "M==1", "M==2^23", "W==0", "W subnormal", "W==inf") + _TRACE,
    WEIGHT_IP: ("sphere", "triangle", "W==0", "W subnormal", "W==inf", "d2 subnormal", "div subnormal"),
    PICK_POWER: ("u==pred(0.5)", "u==0.5", "x on a running sum", "equal consecutive sums", "x>=total", "total==0", "total<0",
                 "total==inf", "total NaN", "u==0", "u==1-2^-24", "u==1", "M_big==1", "M_big==2^23")
    + tuple(f"M=={m}" for m in range(1, PICK_TABLE + 1)),
    CONE: _REGIME + ("s==0", "s==2^-149", "s==pred(1)", "w.z==+0", "w.z==-0", "w.z==+1", "w.z==-1", "axis +x", "axis -x", "axis +y",
                     "axis -y", "h clamped", "h>0", "cs>0", "cs==0", "cs<0", "NaN normal", "in the regime, dc2<2^-130") + _TRACE,
    CONE_VIEW: _REGIME + ("cs>0", "cs==0", "cs<0", "NaN normal", "samplable", "in the regime, not samplable", "div subnormal"),
    NEE_VIEW: ("fails on cs alone", "fails on cl alone", "fails on d2>0 alone", "fails on d2<inf alone", "samplable", "sphere cl>0",
               "sphere cl<0", "triangle c>0", "triangle c<0", "W'==0", "W' subnormal", "W'==inf", "d2 subnormal",
               "W' of a view not samplable", "light_weight(inf)==0", "bounce_weight(inf)==1", "W==0", "W subnormal", "div subnormal"),
    SCATTER: ("try_normalize fails", "zero n gives NaN", "roughness==0", "roughness==1", "sm==0", "sm==pred(1)", "d zero", "NaN d")
    + _TRACE,
    SKY: ("d zero", "d.y==+1", "d.y==-1", "NaN d", "try_normalize fails", "sqrt subnormal"),
}
# the classes a twin with one mutation may differ in (tests/test_sampling_corpus.py)
MUTATION_CLASSES = ("dot inexact", "rcp inexact", "subnormal")


def _regime_classes(i):
    q, dc2, r2 = i["q"], i["dc2"], i["r2"]
    return {
        "q==pred(2^-10)": q == nb(Q_MIN, False), "q==2^-10": q == Q_MIN, "q==succ(2^-10)": q == nb(Q_MIN, True),
        "q==pred(1)": q == nb(1, False), "q==1": q == ONE, "q>1": (q > ONE) & (q < INF), "q==0": q == ZERO, "q NaN": np.isnan(q),
        "dc2==0, q==inf": (dc2 == ZERO) & (q == INF), "dc2==inf": dc2 == INF, "r*r subnormal": is_sub(r2), "dc2 subnormal": is_sub(dc2),
        "q subnormal": is_sub(q),
    }


def classify(family, rec, trace=True):
    """class name -> mask over the records (the family's CLASSES and MUTATION_CLASSES), from the restatement's intermediates;
    trace=False leaves out the classes TraceOps finds (the subnormal and inexact operations): for large record sets"""
    n = len(rec)
    t = TraceOps(n) if trace else PLAIN
    f = _f(rec)
    with np.errstate(all="ignore"):
        _, i = RESTATE[family](rec, t)
        if family == DIRECT:
            sph, v, d2 = i["sphere"], i["v"], i["d2"]
            cs_ok, cl_ok, pos, fin = i["cs"] > ZERO, i["cl"] > ZERO, d2 > ZERO, d2 < INF
            a, b, cc = (np.stack(_v(f, k), 1) for k in (9, 12, 15))
            same = (a == b).all(1) | (a == cc).all(1) | (b == cc).all(1)
            zero_cross = (np.stack(i["cross"], 1) == 0).all(1)
            c = {
                "d2==0": d2 == ZERO, "d2 subnormal": is_sub(d2), "d2==inf": d2 == INF,
                "d2==0, v!=0": (d2 == ZERO) & ((v[0] != 0) | (v[1] != 0) | (v[2] != 0)),
                "cs==0": i["cs"] == ZERO, "cl==0": i["cl"] == ZERO,
                "fails on cs alone": ~cs_ok & cl_ok & pos & fin, "fails on cl alone": cs_ok & ~cl_ok & pos & fin,
                "fails on d2>0 alone": cs_ok & cl_ok & ~pos & fin, "facing": i["facing"],
                "sphere cl>0": sph & (i["cl"] > ZERO), "sphere cl<0": sph & (i["cl"] < ZERO),
                "triangle c>0": ~sph & (i["c"] > ZERO), "triangle c<0": ~sph & (i["c"] < ZERO),
                "u1+u2<1": ~sph & (i["usum"] < ONE), "u1+u2==1": ~sph & (i["usum"] == ONE), "u1+u2==succ(1)": ~sph & (i["usum"] == nb(1, True)),
                "area 0: equal vertices": ~sph & same & (i["area"] == ZERO),
                "area 0: collinear": ~sph & ~same & zero_cross & (i["area"] == ZERO),
                "subnormal cross product": ~sph & (is_sub(i["cross"][0]) | is_sub(i["cross"][1]) | is_sub(i["cross"][2])),
                "u==0": i["u"] == ZERO, "u==1-2^-24": i["u"] == U_LAST, "u==1": i["u"] == ONE,
                "M==1": i["M"] == 1, "M==2^23": i["M"] == MAX_LIGHTS,
                "W==0": i["W"] == ZERO, "W subnormal": is_sub(i["W"]), "W==inf": i["W"] == INF,
            }
        elif family == WEIGHT_IP:
            c = {"sphere": i["sphere"], "triangle": ~i["sphere"], "W==0": i["W"] == ZERO, "W subnormal": is_sub(i["W"]),
                 "W==inf": i["W"] == INF, "d2 subnormal": is_sub(i["d2"])}
        elif family == PICK_POWER:
            u, M, total, x, cc = i["u"], i["M"].astype(np.int64), i["total"], i["x"], i["c"]
            search = i["valid"] & ~i["degenerate"] & ~i["lower"]
            idx = np.arange(PICK_TABLE)[None, :]
            inside = idx < M[:, None]
            prev = np.concatenate([np.zeros((n, 1), F), cc[:, :-1]], axis=1)
            last = cc[np.arange(n), np.clip(M - 1, 0, PICK_TABLE - 1)]
            c = {
                "u==pred(0.5)": u == nb(0.5, False), "u==0.5": u == HALF,
                "x on a running sum": search & ((x[:, None] == cc) & inside).any(1),
                "equal consecutive sums": search & ((cc == prev) & inside).any(1),
                "x>=total": search & (x >= last),
                "total==0": total == ZERO, "total<0": total < ZERO, "total==inf": total == INF, "total NaN": np.isnan(total),
                "u==0": u == ZERO, "u==1-2^-24": u == U_LAST, "u==1": u == ONE,
                "M_big==1": i["M_big"] == 1, "M_big==2^23": i["M_big"] == MAX_LIGHTS,
            }
            c.update({f"M=={m}": i["valid"] & (M == m) for m in range(1, PICK_TABLE + 1)})
        elif family == CONE:
            reg, w, s, nrm = i["reg"], i["w"], i["s"], i["n"]
            neg = np.signbit(w[2])
            c = _regime_classes(i)
            c.update({
                "s==0": reg & (s == ZERO), "s==2^-149": reg & (s == F(2.0 ** -149)), "s==pred(1)": reg & (s == nb(1, False)),
                "w.z==+0": reg & (w[2] == ZERO) & ~neg, "w.z==-0": reg & (w[2] == ZERO) & neg,
                "w.z==+1": reg & (w[2] == ONE), "w.z==-1": reg & (w[2] == -ONE),
                "axis +x": reg & (w[0] == ONE), "axis -x": reg & (w[0] == -ONE), "axis +y": reg & (w[1] == ONE), "axis -y": reg & (w[1] == -ONE),
                "h clamped": reg & ~(i["h_raw"] > ZERO), "h>0": reg & (i["h_raw"] > ZERO),
                "cs>0": reg & (i["cs"] > ZERO), "cs==0": reg & (i["cs"] == ZERO), "cs<0": reg & (i["cs"] < ZERO),
                "NaN normal": reg & (np.isnan(nrm[0]) | np.isnan(nrm[1]) | np.isnan(nrm[2])),
                # found by this corpus: below DC2_UNIT a subnormal dc2 has lost so many bits that w = a / sqrt(dc2), and v with it,
                # is not unit to 2^-18 (the premise now stands in rt_direct_math.h's comment on Cone::v)
                "in the regime, dc2<2^-130": reg & (i["dc2"] < DC2_UNIT),
            })
        elif family == CONE_VIEW:
            nrm = i["n"]
            c = _regime_classes(i)
            c.update({"cs>0": i["cs"] > ZERO, "cs==0": i["cs"] == ZERO, "cs<0": i["cs"] < ZERO,
                      "NaN normal": np.isnan(nrm[0]) | np.isnan(nrm[1]) | np.isnan(nrm[2]), "samplable": i["samplable"],
                      "in the regime, not samplable": i["reg"] & ~i["samplable"]})
        elif family == NEE_VIEW:
            sph, d2 = i["sphere"], i["d2"]
            cs_ok, cl_ok, pos, fin = i["cs"] > ZERO, i["cl"] > ZERO, d2 > ZERO, d2 < INF
            c = {
                "fails on cs alone": ~cs_ok & cl_ok & pos & fin, "fails on cl alone": cs_ok & ~cl_ok & pos & fin,
                "fails on d2>0 alone": cs_ok & cl_ok & ~pos & fin, "fails on d2<inf alone": cs_ok & cl_ok & pos & ~fin,
                "samplable": i["samplable"],
                "sphere cl>0": sph & (i["cl"] > ZERO), "sphere cl<0": sph & (i["cl"] < ZERO),
                "triangle c>0": ~sph & (i["c"] > ZERO), "triangle c<0": ~sph & (i["c"] < ZERO),
                "W'==0": i["W"] == ZERO, "W' subnormal": is_sub(i["W"]), "W'==inf": i["W"] == INF, "d2 subnormal": is_sub(d2),
                "W' of a view not samplable": ~i["samplable"],
                "light_weight(inf)==0": (i["Win"] == INF) & (i["wl_in"] == ZERO),
                "bounce_weight(inf)==1": ((i["Win"] == INF) & (i["wb_in"] == ONE)) | ((i["W"] == INF) & (i["wb"] == ONE)),
                "W==0": i["Win"] == ZERO, "W subnormal": is_sub(i["Win"]),
            }
        elif family == SCATTER:
            d, nrm = i["d"], i["n"]
            zero_n = (nrm[0] == 0) & (nrm[1] == 0) & (nrm[2] == 0)
            c = {
                "try_normalize fails": ~i["ok"], "zero n gives NaN": ~i["ok"] & zero_n & np.isnan(i["out"][0]),
                "roughness==0": i["rough"] == ZERO, "roughness==1": i["rough"] == ONE,
                "sm==0": i["sm"] == ZERO, "sm==pred(1)": i["sm"] == nb(1, False),
                "d zero": (d[0] == 0) & (d[1] == 0) & (d[2] == 0), "NaN d": np.isnan(d[0]) | np.isnan(d[1]) | np.isnan(d[2]),
            }
        else:
            d = i["d"]
            c = {"d zero": (d[0] == 0) & (d[1] == 0) & (d[2] == 0), "d.y==+1": i["ny"] == ONE, "d.y==-1": i["ny"] == -ONE,
                 "NaN d": np.isnan(d[0]) | np.isnan(d[1]) | np.isnan(d[2]), "try_normalize fails": ~i["ok"]}
    if not trace:
        return c
    for k in CLASSES[family]:
        if k in t.m:
            c[k] = t.m[k]
    assert tuple(c) == CLASSES[family], (family, [k for k in CLASSES[family] if k not in c], [k for k in c if k not in CLASSES[family]])
    for k in MUTATION_CLASSES:
        c[k] = t.m[k]
    return c


def cone_invariants(rec, words, classes):
    """The bounds of tests/test_cone_host.py on CONE output words (the restatement's here, the device's in the GPU test), on every
    record in the regime: no NaN in any word but cs and W under a NaN normal; 0 <= W <= 2 ip where facing; and |v.v - 1| <= 2^-18 —
    that one on every record in the regime but the named class "in the regime, dc2<2^-130", the operands this corpus found to break
    it (a subnormal dc2 carries an absolute rounding error of up to 2^-150, w = a / sqrt(dc2) takes it on, v is as long as w; from
    2^-130 up that error is at most 2^-20 of dc2, a quarter of the bound).  Returns the counts of records in the regime and of
    facing ones."""
    f = words.view(F)
    reg = words[:, 1] != 0
    geo = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 17, 18, 19]
    assert not np.isnan(f[reg][:, geo]).any(), "a NaN among the geometric words of an in-regime record"
    ordinary = reg & ~classes["NaN normal"] & np.isfinite(rec.view(F)[:, 13])
    assert not np.isnan(f[ordinary][:, [13, 15]]).any(), "a NaN cs or W without a NaN normal"
    dev = np.abs(f[:, 19].astype(np.float64) - 1.0)
    bad = reg & ~classes["in the regime, dc2<2^-130"] & ~(dev <= 2.0 ** -18)
    assert not bad.any(), ("|v.v - 1| > 2^-18", int(bad.sum()), _bound_report(rec, words, classes, bad))
    fac = reg & (words[:, 14] != 0)
    W, ip = f[:, 15].astype(np.float64), rec.view(F)[:, 13].astype(np.float64)
    bad = fac & ~((W >= 0) & (W <= 2 * ip))
    assert not bad.any(), ("W outside [0, 2 ip] where facing", int(bad.sum()), _bound_report(rec, words, classes, bad))
    return int(reg.sum()), int(fac.sum())


def _bound_report(rec, words, classes, bad):
    i = int(np.nonzero(bad)[0][0])
    return f"first: record {i} = {rec[i].view(F).tolist()}, classes {describe(classes, i)}, words {[hex(w) for w in words[i]]}"


def describe(classes, i):
    return tuple(k for k, m in classes.items() if m[i])


# ------------------------------------------------------------------------------------------------ helpers of the generators
def _rows(family, n):
    return np.zeros((n, WORDS[family][0]), U32)


def _unit(g, n):
    v = g.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(F)


def _u01(g, n):
    """24-bit u01 draws"""
    return (g.integers(0, 1 << 24, n).astype(np.float64) * 2.0 ** -24).astype(F)


def _accepted_pairs(g, m):
    """m accepted pairs of the UnitSphere draw: (x1, x2, s = x1 x1 + x2 x2 < 1 as the kernel forms it)"""
    x = np.zeros((0, 2), F)
    while len(x) < m:
        c = (g.integers(0, 1 << 24, (2 * m, 2)).astype(np.float64) * 2.0 ** -23 - 1.0).astype(F)
        x = np.concatenate([x, c[(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) < ONE]])
    x = x[:m]
    return x[:, 0].copy(), x[:, 1].copy(), (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]).astype(F)


def _step_ulps(x, k):
    x = np.asarray(x, F).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
    return x


def pairs_with_sum(target, count, seed):
    """pairs (x1, x2) of float32 with x1 x1 + x2 x2 == target in float32, by search round the float64 solution"""
    g = np.random.default_rng(seed)
    got = []
    while sum(len(p) for p in got) < count:
        x1 = g.uniform(-0.95, 0.95, 4 * count).astype(F) * F(np.sqrt(float(target)))
        x2 = np.sqrt(np.maximum(float(target) - x1.astype(np.float64) ** 2, 0.0)).astype(F) * np.where(g.random(len(x1)) < 0.5, F(1), F(-1))
        for k in range(-2, 3):
            y = _step_ulps(x2, k)
            hit = (x1 * x1 + y * y).astype(F) == F(target)
            got.append(np.stack([x1[hit], y[hit]], 1))
            x1, x2 = x1[~hit], x2[~hit]
    return np.concatenate(got)[:count]


def radius_for_q(P, c, target):
    """per row of (P, c): a radius whose q = (r r) / dc2 is exactly `target` in float32, NaN where the search finds none"""
    with np.errstate(all="ignore"):
        a = (c - P).astype(F)
        dc2 = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]).astype(F)
        r0 = np.sqrt(float(target) * dc2.astype(np.float64)).astype(F)
        r = np.full(len(P), np.nan, F)
        for k in range(-3, 4):
            y = _step_ulps(r0, k)
            hit = np.isnan(r) & (((y * y).astype(F) / dc2).astype(F) == F(target))
            r = np.where(hit, y, r)
    return r


AXES = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


# ------------------------------------------------------------------------------------------------ CONE and CONE_VIEW
def _cone_rows(P, c, r, x1, x2, n, ip):
    m = len(r)
    rec = _rows(CONE, m)
    f = rec.view(F)
    f[:, 0:3], f[:, 3:6], f[:, 6], f[:, 7], f[:, 8], f[:, 10:13], f[:, 13] = P, c, r, x1, x2, n, ip
    with np.errstate(all="ignore"):
        f[:, 9] = f[:, 7] * f[:, 7] + f[:, 8] * f[:, 8]
    return rec


@functools.lru_cache(maxsize=None)
def cone_directed():
    parts = []
    tiny = F(2.0 ** -75)
    top = pairs_with_sum(nb(1, False), 6, 11)
    pairs = [(0.0, 0.0), (tiny, 0.0), (0.0, -tiny), (F(2.0 ** -74.5), 0.0), (nb(1, False), 0.0), (F(0.70710677), F(0.70710671)),
             (-0.6, 0.79999995), (0.3, -0.4), (-0.0, 0.0), (1e-40, 0.5)] + [tuple(p) for p in top]
    lo = F(2.0 ** -5)
    ratios = [0.0, 1e-41, nb(lo, False), lo, nb(lo, True), 0.3, 0.9, nb(1, False), 1.0, nb(1, True), 1.5, np.inf, np.nan]
    axes = list(AXES) + [(1, 0, -0.0), (0, 1, -0.0), (-1, 0, -0.0), (0, -1, -0.0), (0.6, 0.8, 0.0), (0.6, 0.0, -0.8), (0.0, 0.28, 0.96)]
    # (a) every axis at three distances (dc2 = scale^2 and q = ratio^2 exactly on the exact axes), every pair, every ratio r / dc
    rows = [(a, sc, p, rt) for a in axes for sc in (1.0, 2.0, 0.5) for p in pairs for rt in ratios]
    c = np.array([[x * sc for x in a] for a, sc, _, _ in rows], F)
    x1, x2 = np.array([p[0] for _, _, p, _ in rows], F), np.array([p[1] for _, _, p, _ in rows], F)
    with np.errstate(all="ignore"):
        r = np.array([rt * sc for _, sc, _, rt in rows], F)
    nrm = np.array([a for a, _, _, _ in rows], F)
    parts.append(_cone_rows(np.zeros_like(c), c, r, x1, x2, nrm, F(33)))
    # (b) the normal against the exact axes: perpendicular (cs == 0 exactly under s == 0: v is w), opposite, zero, NaN
    rows = []
    for a, sc, rt, p in itertools.product(AXES, (1.0, 2.0, 0.5), (lo, nb(lo, True), 0.3, 0.9, nb(1, False)), ((0.0, 0.0), (0.3, -0.4))):
        perp = [b for b in AXES if sum(x * y for x, y in zip(a, b)) == 0]
        for nv in perp + [tuple(-x for x in a), (0, 0, 0), (np.nan, np.nan, np.nan), (np.nan, 0, 0)]:
            rows.append((a, sc, rt, p, nv))
    c = np.array([[x * sc for x in a] for a, sc, _, _, _ in rows], F)
    parts.append(_cone_rows(np.zeros_like(c), c, np.array([rt * sc for _, sc, rt, _, _ in rows], F), np.array([p[0] for *_, p, _ in rows], F),
                            np.array([p[1] for *_, p, _ in rows], F), np.array([nv for *_, nv in rows], F), F(2)))
    # (c) q on the regime's ends and their neighbours from general positions: the radius is searched per point
    g = np.random.default_rng(31)
    m = 400
    for target in (nb(Q_MIN, False), Q_MIN, nb(Q_MIN, True), nb(1, False), ONE, nb(1, True)):
        P = g.uniform(-5, 5, (m, 3)).astype(F)
        c = (P + _unit(g, m) * (10.0 ** g.uniform(-1, 1.5, m))[:, None]).astype(F)
        r = radius_for_q(P, c, target)
        keep = ~np.isnan(r)
        x1, x2, _ = _accepted_pairs(g, m)
        parts.append(_cone_rows(P, c, r, x1, x2, _unit(g, m), F(7))[keep][:160])
    # (d) degenerate spheres and distances; subnormal r r, dc2 and q, in the regime and outside
    rows = []
    sub = (1e-20, 1.5e-20, 2e-20, 3e-20, 5e-20, 7e-20, 9e-20, 1.2e-19)
    for a, p in itertools.product(axes[:9], pairs[:10]):
        for rr, dd in ((0.0, 1.0), (1e-30, 1.0), (0.0, 0.0), (np.nan, 1.0), (np.inf, 1e20), (0.5, 0.0), (1e-3, 0.0), (0.5, 1e20),
                       (0.5, np.inf), (0.5, 3e19), (1e-15, 1e5), (3e-15, 2e5), (1e-16, 1e4)):
            rows.append((a, dd, rr, p))
        for t in sub:
            rows.append((a, 3.0 * t, t, p))                      # r r and dc2 subnormal, q about 1/9: in the regime
            rows.append((a, 1.0, t, p))                          # r r subnormal, dc2 = 1: q subnormal
            rows.append((a, t, 1e-22, p))                        # dc2 subnormal, q tiny
        for t in (1.5e-21, 2.5e-21, 4e-22, 6e-23):
            rows.append((a, 3.0 * t, t, p))                      # ... in the regime with a dc2 of 15 down to 5 bits: v is not unit
    with np.errstate(all="ignore"):
        c = np.array([[x * dd if x != 0 else x for x in a] for a, dd, _, _ in rows], F)
    parts.append(_cone_rows(np.zeros_like(c), c, np.array([rr for _, _, rr, _ in rows], F), np.array([p[0] for *_, p in rows], F),
                            np.array([p[1] for *_, p in rows], F), np.array([a for a, *_ in rows], F), F(4)))
    # (e) the rim: the largest s below 1 and its neighbours over many q, where h = r r - dc2 st st rounds to either side of 0
    m = 600
    P = g.uniform(-2, 2, (m, 3)).astype(F)
    w = _unit(g, m)
    r = (10.0 ** g.uniform(-1, 0.5, m)).astype(F)
    c = (P + w * (r / g.uniform(0.04, 0.99, m))[:, None]).astype(F)
    rim = pairs_with_sum(nb(1, False), m, 12)
    parts.append(_cone_rows(P, c, r, rim[:, 0], rim[:, 1], w, F(3)))
    return np.concatenate(parts)


def cone_random(n, seed=2020):
    g = np.random.default_rng(seed)
    P = g.uniform(-5, 5, (n, 3)).astype(F)
    w = _unit(g, n)
    r = (10.0 ** g.uniform(-2, 1, n)).astype(F)
    ratio = np.where(g.random(n) < 0.15, g.uniform(0.02, 0.04, n), g.uniform(0.02, 1.1, n))     # r / dc: the regime's ends well covered
    c = (P + w * (r / ratio)[:, None]).astype(F)
    x1, x2, _ = _accepted_pairs(g, n)
    ip = np.where(g.random(n) < 0.5, g.integers(1, 40, n), 1 / g.uniform(0.01, 1, n)).astype(F)
    return _cone_rows(P, c, r, x1, x2, _unit(g, n), ip)


def _views_of(cone, d):
    """CONE_VIEW records of CONE records: the same point, normal, sphere and ip, the segment's direction d"""
    rec = _rows(CONE_VIEW, len(cone))
    rec[:, 0:3], rec[:, 3:6], rec[:, 9:13], rec[:, 13] = cone[:, 0:3], cone[:, 10:13], cone[:, 3:7], cone[:, 13]
    rec.view(F)[:, 6:9] = d
    return rec


def _towards(cone):
    f = cone.view(F)
    with np.errstate(all="ignore"):
        a = f[:, 3:6].astype(np.float64) - f[:, 0:3].astype(np.float64)
        d = a / np.linalg.norm(a, axis=1)[:, None]
    return np.where(np.isfinite(d).all(1)[:, None], d, np.array([0.0, 0.0, 1.0])).astype(F)


@functools.lru_cache(maxsize=None)
def cone_view_directed():
    cone = cone_directed()
    return _views_of(cone, _towards(cone))


def cone_view_random(n, seed=2021):
    g = np.random.default_rng(seed)
    cone = cone_random(n, seed)
    d = _towards(cone) + g.normal(0, 0.1, (n, 3))
    return _views_of(cone, (d / np.linalg.norm(d, axis=1)[:, None]).astype(F))


# ------------------------------------------------------------------------------------------------ DIRECT
def _direct_sphere(M, u, P, n, c, r, us, alb=(0.8, 0.6, 0.4), em=4.0):
    m = len(r)
    rec = _rows(DIRECT, m)
    f = rec.view(F)
    rec[:, 0], rec[:, 1] = 0, M
    f[:, 2], f[:, 3:6], f[:, 6:9], f[:, 9:12], f[:, 12], f[:, 13:16], f[:, 23:26], f[:, 26] = u, P, n, c, r, us, alb, em
    return rec


def _tri_normal(a, b, c):
    with np.errstate(all="ignore"):
        nx = np.cross(a.astype(np.float64) - b, a.astype(np.float64) - c)
        ln = np.linalg.norm(nx, axis=1)[:, None]
        return np.where((ln > 0) & np.isfinite(ln), nx / ln, 0.0).astype(F)


def _direct_triangle(M, u, P, n, a, b, c, u1, u2, alb=(0.6, 0.8, 1.0), em=3.0):
    m = len(u1)
    rec = _rows(DIRECT, m)
    f = rec.view(F)
    rec[:, 0], rec[:, 1] = 1, M
    f[:, 2], f[:, 3:6], f[:, 6:9], f[:, 9:12], f[:, 12:15], f[:, 15:18], f[:, 18], f[:, 19] = u, P, n, a, b, c, u1, u2
    f[:, 20:23], f[:, 23:26], f[:, 26] = _tri_normal(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F)), alb, em
    return rec


PICK_US = (0.0, 2.0 ** -24, 0.25, float(nb(0.5, False)), 0.5, 0.75, float(U_LAST), 1.0)
PICK_MS = (1, 2, 3, 5, 7, 16, 33, 1000, 65535, (1 << 23) - 1, 1 << 23)


@functools.lru_cache(maxsize=None)
def direct_directed():
    parts = []
    arr = lambda rows, k: np.array([r[k] for r in rows], F)      # noqa: E731
    # (a) a sphere light on an axis at distance D, the point drawn along +-axis or a perpendicular axis, centred so that L lies on the
    # axis (w is the axis exactly: cs and cl are exact dot products, 0 among them), every normal of the hit
    rows = []
    for ax, D, r, sgn in itertools.product(AXES, (0.5, 1.0, 3.0), (0.0, 0.25, 1e-22, 1e19), (1.0, -1.0)):
        for us in [tuple(sgn * x for x in ax)] + [b for b in AXES if sum(x * y for x, y in zip(ax, b)) == 0][:2]:
            L = tuple(D * x for x in ax)
            with np.errstate(all="ignore"):
                c = tuple(F(l) - F(r) * F(s) for l, s in zip(L, us))
            for nv in (ax, tuple(-x for x in ax), [b for b in AXES if sum(x * y for x, y in zip(ax, b)) == 0][0], (0, 0, 0)):
                rows.append((c, r, us, nv))
    m = len(rows)
    parts.append(_direct_sphere(3, 0.25, np.zeros((m, 3), F), arr(rows, 3), arr(rows, 0), arr(rows, 1), arr(rows, 2)))
    # (b) d2 == 0 under a non-zero v, d2 subnormal and d2 == inf: v = t * (a sign pattern), n along it, the light's normal against it
    rows = []
    for t, sg in itertools.product((1e-38, 1e-35, 1e-30, 1e-25, 1e-41, 1e-44, 1e-20, 2e-20, 4e-20, 1e-19, 1e19, 1e20, 1e25, 3e38, 0.0),
                                   itertools.product((1.0, -1.0), repeat=3)):
        for flip_n, flip_l in ((1, -1), (-1, -1), (1, 1)):
            rows.append((tuple(t * s for s in sg), tuple(flip_n * s for s in sg), tuple(flip_l * s for s in sg)))
    m = len(rows)
    z = np.zeros((m, 3), F)
    parts.append(_direct_sphere(2, 0.5, z, arr(rows, 1), arr(rows, 0), np.zeros(m, F), arr(rows, 2)))
    parts.append(_direct_triangle(2, 0.5, z, arr(rows, 1), arr(rows, 0), arr(rows, 0), arr(rows, 0), np.zeros(m, F), np.zeros(m, F)))
    parts[-1].view(F)[:, 20:23] = arr(rows, 2)                   # (a point triangle has no normal of its own: the operand is given)
    # (c) triangles: the fold at u1 + u2 == 1 and its neighbours, both sides of the plane, degenerate and tiny ones
    e = F(2.0 ** -24)
    folds = [(0.25, 0.5), (0.0, 0.0), (0.75, 0.5), (0.5, 0.5), (0.25, 0.75), (float(U_LAST), float(e)), (0.5, 0.5 + 2 * float(e)),
             (0.5, 0.5 + float(e)), (0.75, 0.25 + 2 * float(e)), (0.125, 0.875), (0.125 + float(e) / 4, 0.875), (float(U_LAST), float(U_LAST)),
             (0.625, 0.375), (0.625, 0.375 + 2 * float(e))]
    A0 = (-1.0, 0.5, -3.0)
    tris = {
        "plain": (A0, (0.5, 0.25, -3.5), (-0.25, 1.75, -2.5)),
        "equal": (A0, A0, A0), "two equal": (A0, A0, (0.0, 1.0, -2.0)),
        "collinear": (A0, (0.0, 1.0, -2.0), (1.0, 1.5, -1.0)), "collinear axis": ((0, 0, -2.0), (1.0, 0, -2.0), (4.0, 0, -2.0)),
        "tiny": ((0, 0, 0), (1e-20, 0, 0), (0, 2e-20, 0)), "tiny 2": ((0, 0, 0), (3e-20, 1e-20, 0), (0, 2e-20, 1e-20)),
        "small": ((0, 0, 0), (1e-10, 0, 0), (0, 2e-10, 0)), "small 2": ((0, 0, 0), (3e-10, 1e-10, 0), (0, 2e-10, 1e-10)),
        "huge": ((-1e10, -1e10, -5), (1e10, -1e10, -5), (0, 1e10, -5)),
    }
    rows = []
    for (name, (a, b, c)), (u1, u2), side in itertools.product(tris.items(), folds, (1.0, -1.0)):
        for P in ((0.1, 0.2, side * 1.0), (0.3, -0.1, side * 1e-3)):
            rows.append((a, b, c, u1, u2, P, (0.0, 0.0, -side)))
    parts.append(_direct_triangle(5, 0.5, arr(rows, 5), arr(rows, 6), arr(rows, 0), arr(rows, 1), arr(rows, 2), arr(rows, 3), arr(rows, 4)))
    # (d) the pick: u at its ends and M at its ends, on ten geometries
    g = np.random.default_rng(41)
    rows = list(itertools.product(PICK_US, PICK_MS, range(10)))
    m = len(rows)
    geo = (g.uniform(-2, 2, (10, 3)).astype(F), _unit(g, 10), g.uniform(-2, 2, (10, 3)).astype(F), _unit(g, 10))
    j = np.array([r[2] for r in rows])
    parts.append(_direct_sphere(np.array([r[1] for r in rows], U32), arr(rows, 0), geo[0][j], geo[1][j], geo[2][j] + F(4), np.full(m, 0.5, F),
                                geo[3][j]))
    # (e) the weights at their ends: tiny and huge radii and areas against near and far points
    rows = []
    for r, D, M in itertools.product((0.0, 1e-23, 1e-22, 3e-22, 1e-21, 1e-6, 1.0, 1e6, 1e18, 1e19, 3e19), (1e-3, 1.0, 1e3, 1e15),
                                     (1, 7, 1 << 23)):
        for ax in AXES[:3]:
            rows.append((tuple(D * x for x in ax), r, tuple(-x for x in ax), ax, M))
    m = len(rows)
    parts.append(_direct_sphere(np.array([r[4] for r in rows], U32), 0.5, np.zeros((m, 3), F), arr(rows, 3), arr(rows, 0), arr(rows, 1),
                                arr(rows, 2)))
    return np.concatenate(parts)


def direct_random(n, seed=2022):
    g = np.random.default_rng(seed)
    h = n // 2
    P, nrm = g.uniform(-3, 3, (n, 3)).astype(F), _unit(g, n)
    M = np.where(g.random(n) < 0.9, g.integers(1, 65, n), g.integers(1, MAX_LIGHTS + 1, n)).astype(U32)
    alb, em = g.uniform(0, 1, (n, 3)).astype(F), g.uniform(0.5, 8, n).astype(F)
    u = _u01(g, n)
    s = _direct_sphere(M[:h], u[:h], P[:h], nrm[:h], g.uniform(-3, 3, (h, 3)).astype(F), g.uniform(0.05, 2, h).astype(F), _unit(g, h),
                       alb[:h], em[:h])
    k = n - h
    a = g.uniform(-3, 3, (k, 3)).astype(F)
    t = _direct_triangle(M[h:], u[h:], P[h:], nrm[h:], a, (a + g.normal(0, 1, (k, 3))).astype(F), (a + g.normal(0, 1, (k, 3))).astype(F),
                         _u01(g, k), _u01(g, k), alb[h:], em[h:])
    return np.concatenate([s, t])


# ------------------------------------------------------------------------------------------------ WEIGHT_IP
@functools.lru_cache(maxsize=None)
def weight_ip_directed():
    rows = list(itertools.product((0, 1), (0.0, 1e-30, 0.5, 1.0), (0.0, 1e-30, 0.5, 1.0), (0.0, 1e-22, 1e-10, 1.0, 1e10, 1e19),
                                  (1.0, 33.0, 1e-3, 1e6, float(1 << 23)), (1e-42, 1e-40, 1e-38, 1e-10, 1.0, 1e10, 1e38)))
    rec = _rows(WEIGHT_IP, len(rows))
    rec[:, 0] = [r[0] for r in rows]
    rec.view(F)[:, 1:6] = np.array([r[1:] for r in rows], F)
    return rec


def weight_ip_random(n, seed=2023):
    g = np.random.default_rng(seed)
    rec = _rows(WEIGHT_IP, n)
    rec[:, 0] = g.integers(0, 2, n)
    f = rec.view(F)
    f[:, 1], f[:, 2] = g.uniform(0, 1, n), g.uniform(0, 1, n)
    f[:, 3], f[:, 4], f[:, 5] = 10.0 ** g.uniform(-3, 2, n), 1 / g.uniform(1e-3, 1, n), 10.0 ** g.uniform(-4, 4, n)
    wide = g.random(n) < 0.1                                       # a tenth over the whole exponent range
    f[wide, 3], f[wide, 5] = (10.0 ** g.uniform(-30, 18, n))[wide], (10.0 ** g.uniform(-44, 38, n))[wide]
    return rec


# ------------------------------------------------------------------------------------------------ PICK_POWER
def _pick_rows(u, M, total, M_big, c):
    m = len(u)
    rec = _rows(PICK_POWER, m)
    f = rec.view(F)
    f[:, 0], rec[:, 1], f[:, 2], rec[:, 3], f[:, 4:] = u, M, total, M_big, c
    # the words behind the table are never read: alternately 0 and +inf, so that a read beyond M - 1 would move a pick
    idx = np.arange(PICK_TABLE)[None, :]
    fill = np.where((np.arange(m) % 2 == 0)[:, None], ZERO, INF)
    f[:, 4:] = np.where(idx < np.asarray(M)[:, None], f[:, 4:], fill)
    return rec


M_BIGS = (1, 2, 3, 1000, (1 << 23) - 1, 1 << 23)


@functools.lru_cache(maxsize=None)
def pick_power_directed():
    rows = []
    g = np.random.default_rng(51)
    for M in range(1, PICK_TABLE + 1):
        tables = []
        for total in (1.0, 16.0, 0.03125):                        # dyadic sums: c[k] = total (k + 1) / M' exactly, x exact
            step = total / 16.0
            q = np.full(M, step)
            tables.append((np.cumsum(q), None))
            if M >= 2:
                z = q.copy()
                z[::2] = 0.0                                       # every other emitter has no power: equal consecutive sums
                tables.append((np.cumsum(z), None))
                z = q.copy()
                z[M // 2:] = 0.0                                   # ... and a tail without power
                tables.append((np.cumsum(z), None))
        pw = (10.0 ** g.uniform(-3, 3, M)).astype(F)               # general powers: the running sum rounds
        c = np.zeros(M, F)
        run = F(0)
        for k in range(M):
            run = F(run + pw[k])
            c[k] = run
        tables.append((c.astype(np.float64), None))
        tables.append((np.cumsum(np.full(M, 0.0625)), 2.0))        # a total beyond the last sum: x >= c[M - 1] takes the last index
        for t in (0.0, -1.0, np.inf, np.nan, -0.0):                # degenerate tables
            tables.append((np.cumsum(np.full(M, 0.0625)), t))
        for c, total in tables:
            c = np.asarray(c, F)
            tot = F(c[-1]) if total is None else F(total)
            us = list(PICK_US) + [float(nb(0.5, True)), 0.5 + 2.0 ** -24]
            if np.isfinite(tot) and tot > 0:
                for k in range(M):                                 # x exactly on c[k] (and one u01 step to either side)
                    uu = 0.5 + float(c[k]) / (2.0 * float(tot))
                    us += [uu, uu - 2.0 ** -24, uu + 2.0 ** -24]
            for j, uu in enumerate(us):
                if 0.0 <= uu <= 1.0:
                    rows.append((F(uu), M, tot, M_BIGS[(j + M) % len(M_BIGS)], np.concatenate([c, np.zeros(PICK_TABLE - M, F)])))
    return _pick_rows(np.array([r[0] for r in rows], F), np.array([r[1] for r in rows], U32), np.array([r[2] for r in rows], F),
                      np.array([r[3] for r in rows], U32), np.array([r[4] for r in rows], F))


def pick_power_random(n, seed=2024):
    g = np.random.default_rng(seed)
    M = g.integers(1, PICK_TABLE + 1, n).astype(U32)
    pw = np.where(g.random((n, PICK_TABLE)) < 0.2, 0.0, 10.0 ** g.uniform(-3, 3, (n, PICK_TABLE))).astype(F)
    pw[np.arange(PICK_TABLE)[None, :] >= M[:, None]] = 0
    c = np.zeros((n, PICK_TABLE), F)
    run = np.zeros(n, F)
    for k in range(PICK_TABLE):
        run = (run + pw[:, k]).astype(F)
        c[:, k] = run
    M_big = np.where(g.random(n) < 0.5, g.integers(1, 65, n), g.integers(1, MAX_LIGHTS + 1, n)).astype(U32)
    return _pick_rows(_u01(g, n), M, run, M_big, c)


# ------------------------------------------------------------------------------------------------ NEE_VIEW
NEE_WS = (0.0, 1e-45, 1e-40, 1e-8, 0.5, 1.0, 2.0, 1e8, 3e38, np.inf)


@functools.lru_cache(maxsize=None)
def nee_view_directed():
    dirs = ((0, 0, 1), (0, 0, -1), (0.6, 0, 0.8), (1, 0, 0), (0, 0, 0))
    rows = list(itertools.product((0, 1), dirs, dirs, dirs, (0.0, 1e-30, 1e-20, 2e-20, 1e-19, 1.0, 7.5, 1e19, 3e19, np.inf),
                                  (0.5, 1e-22, 1e19, 0.0), (1, 3, 1 << 23)))
    m = len(rows)
    rec = _rows(NEE_VIEW, m)
    f = rec.view(F)
    rec[:, 0], rec[:, 1] = [r[0] for r in rows], [r[6] for r in rows]
    f[:, 2:5], f[:, 5:8], f[:, 8:11] = (np.array([r[k] for r in rows], F) for k in (1, 2, 3))
    f[:, 11], f[:, 12] = [r[4] for r in rows], [r[5] for r in rows]
    f[:, 13] = np.array(NEE_WS, F)[np.arange(m) % len(NEE_WS)]
    # general unit vectors (the dot products round), every kind, distance and W
    g = np.random.default_rng(71)
    m = 1024
    gen = _rows(NEE_VIEW, m)
    f = gen.view(F)
    gen[:, 0], gen[:, 1] = np.arange(m) % 2, np.array([1, 3, 33, 1 << 23], U32)[(np.arange(m) // 2) % 4]
    f[:, 2:5], f[:, 5:8], f[:, 8:11] = _unit(g, m), _unit(g, m), _unit(g, m)
    f[:, 11] = np.array([1e-20, 1e-3, 1.0, 7.5, 1e3, 1e19], F)[(np.arange(m) // 8) % 6]
    f[:, 12], f[:, 13] = 0.5, np.array(NEE_WS, F)[np.arange(m) % len(NEE_WS)]
    return np.concatenate([rec, gen])


def nee_view_random(n, seed=2025):
    g = np.random.default_rng(seed)
    rec = _rows(NEE_VIEW, n)
    f = rec.view(F)
    rec[:, 0], rec[:, 1] = g.integers(0, 2, n), g.integers(1, 65, n)
    f[:, 2:5], f[:, 5:8], f[:, 8:11] = _unit(g, n), _unit(g, n), _unit(g, n)
    f[:, 11], f[:, 12], f[:, 13] = 10.0 ** g.uniform(-3, 3, n), 10.0 ** g.uniform(-2, 1, n), 10.0 ** g.uniform(-6, 6, n)
    wide = g.random(n) < 0.1
    f[wide, 11], f[wide, 13] = (10.0 ** g.uniform(-22, 19.5, n))[wide], (10.0 ** g.uniform(-44, 38, n))[wide]
    return rec


# ------------------------------------------------------------------------------------------------ SCATTER and SKY
def _scatter_rows(d, n, rough, x1, x2):
    m = len(rough)
    rec = _rows(SCATTER, m)
    f = rec.view(F)
    f[:, 0:3], f[:, 3:6], f[:, 6], f[:, 7], f[:, 8] = d, n, rough, x1, x2
    with np.errstate(all="ignore"):
        f[:, 9] = f[:, 7] * f[:, 7] + f[:, 8] * f[:, 8]
    return rec


@functools.lru_cache(maxsize=None)
def scatter_directed():
    top = pairs_with_sum(nb(1, False), 3, 13)
    pairs = [(0.0, 0.0), (0.3, -0.4), (F(2.0 ** -75), 0.0), (-0.6, 0.79999995), (1e-40, 0.5), (-0.0, 0.0)] + [tuple(p) for p in top]
    ds = list(AXES) + [(0, 0, 0), (0.6, 0, -0.8), (np.nan, 0, 0), (np.nan, np.nan, np.nan)]
    # normals: the axes, zero, the negated draw of the pair (0, 0) and of general pairs (us + n = 0 or tiny: try_normalize fails or
    # takes the square root of a subnormal), a normal with a subnormal component
    ns = list(AXES) + [(0, 0, 0), (1e-20, 0, -1.0), (0, 3e-20, -1.0), (1e-30, 0, -1.0), (1e-42, 1.0, 0), (0.6, 0, 0.8)]
    rows = list(itertools.product(ds, ns, (0.0, 1.0, 0.5, 3e38, 0.25), pairs))
    arr = lambda k: np.array([r[k] for r in rows], F)              # noqa: E731
    rec = [_scatter_rows(arr(0), arr(1), arr(2), np.array([r[3][0] for r in rows], F), np.array([r[3][1] for r in rows], F))]
    # n = -us exactly, for every pair: the diffuse direction is 0
    g = np.random.default_rng(61)
    m = 256
    x1, x2, s = _accepted_pairs(g, m)
    us = np.stack(unit_sphere_vec(PLAIN, x1, x2, s), 1)
    rough = np.array([0.0, 1.0, 0.5, 0.0], F)[np.arange(m) % 4]
    rec.append(_scatter_rows(_unit(g, m), -us, rough, x1, x2))
    rec.append(_scatter_rows(np.zeros((m, 3), F), (-us + np.array([1e-20, 0, 0], F)).astype(F), np.zeros(m, F), x1, x2))
    return np.concatenate(rec)


def scatter_random(n, seed=2026):
    g = np.random.default_rng(seed)
    x1, x2, _ = _accepted_pairs(g, n)
    rough = np.where(g.random(n) < 0.2, np.where(g.random(n) < 0.5, 0.0, 1.0), g.uniform(0, 1, n)).astype(F)
    return _scatter_rows(_unit(g, n), _unit(g, n), rough, x1, x2)


@functools.lru_cache(maxsize=None)
def sky_directed():
    # every power of two from where d.d underflows to where it overflows (a scaled axis normalises to +-1 exactly), and a few others
    scales = [2.0 ** e for e in range(-78, 66)] + [3.0, 1e-10, 1e-20, 5e-20, 1e-30, 1e-45, 1e10, 1e19, 3e38, np.inf]
    base = list(AXES) + [(0.6, 0.8, 0), (0.6, -0.8, 0), (0, 0.28, 0.96), (1, 1, 1), (-1, 1, -1), (0, -1, 1e-3), (np.nan, 1, 0), (0, np.nan, 0),
                         (1, 0, np.nan), (-0.0, 1, 0.0), (0.0, -1, -0.0), (3, 4, 0), (1, -1, 1)]
    with np.errstate(all="ignore"):
        d = np.array([[x * s if x != 0 else x for x in b] for b in base for s in scales], F)
    # the zero vector has eight bit patterns: each eight times
    d = np.concatenate([d, np.array(list(itertools.product((0.0, -0.0), repeat=3)) * 8, F)])
    # general directions at general lengths: the dot product rounds, and some of those roundings reach the colour
    g = np.random.default_rng(81)
    d = np.concatenate([d, (_unit(g, 16384) * (10.0 ** g.uniform(-2, 2, 16384))[:, None]).astype(F)])
    rec = _rows(SKY, len(d))
    rec.view(F)[:] = d
    return rec


def sky_random(n, seed=2027):
    g = np.random.default_rng(seed)
    rec = _rows(SKY, n)
    rec.view(F)[:] = _unit(g, n) * (10.0 ** np.where(g.random(n) < 0.8, g.uniform(-1, 1, n), g.uniform(-24, 20, n)))[:, None].astype(F)
    return rec


DIRECTED = {DIRECT: direct_directed, WEIGHT_IP: weight_ip_directed, PICK_POWER: pick_power_directed, CONE: cone_directed,
            CONE_VIEW: cone_view_directed, NEE_VIEW: nee_view_directed, SCATTER: scatter_directed, SKY: sky_directed}
RANDOM = {DIRECT: direct_random, WEIGHT_IP: weight_ip_random, PICK_POWER: pick_power_random, CONE: cone_random,
          CONE_VIEW: cone_view_random, NEE_VIEW: nee_view_random, SCATTER: scatter_random, SKY: sky_random}


def records(family, n_random):
    """the directed corpus followed by n_random seeded records"""
    return np.ascontiguousarray(np.concatenate([DIRECTED[family](), RANDOM[family](n_random)]))
