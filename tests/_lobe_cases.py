"""Operands for the lobe arithmetic of the light samples at glossy hits (csrc/rt_lobe_math.h): a directed corpus, seeded random records
and the numpy restatement's words (tests/_lobe_np.py), in the pattern of tests/_sampling_cases.py.  The record layout is family 16
(LOBE) of ray_tracer_s8_amd/csrc/rt_unit_sampling.hip.h and of the g++ harness tests/host/lobe_host.cpp, so one corpus feeds g++,
numpy and the device:
    in, 16 words (f32 as bits):  [0..2] n, [3..5] d (the incoming direction), [6] rho, [7..9] w, [10] W, [11..13] us, [14..15] unused;
    out, 20 words:  [0] sampled class, [1..3] g, [4] gn, [5..7] c, [8] r, [9] kappa, [10] b, [11] D, [12] in the lobe, [13] cg,
                    [14] the sample is taken (in the lobe and W < inf); of the scatter's own direction, from us: [15] m, [16] t,
                    [17] cg, [18] in the lobe; [19] 0.
The lobe and its factors are formed whatever the class is.  Classes are ENUMERATED below; tests/test_lobe_host.py holds every one of
them to at least FLOOR records of the directed corpus."""
import numpy as np

import _lobe_np as L

F = np.float32
U32 = np.uint32
FLOOR = 16
LOBE = 16                                                # the family number
UNIT_NEE = 4                                             # rt_debug_unit's unit that carries it
WORDS = (16, 20)
FLAG_WORDS = (12, 14, 18)
COUNT_WORDS = (0, 19)
RHO_EDGES = (F(2.0 ** -24), F(0.5), F(1) - F(2.0 ** -24))


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rec(n, d, rho, w, W=1.0, us=None):
    """us: the UnitSphere vector of the scatter; None: the one whose scattered point c + r us lies along w on the near side of the lobe
    (for a w on the rim: the tangent point), or w itself where there is none"""
    r = np.zeros(WORDS[0], F)
    r[0:3], r[3:6], r[6], r[7:10], r[10] = n, d, rho, w, W
    if us is None:
        with np.errstate(all="ignore"):
            c, rr, kappa = _lobe64(r[0:3], r[3:6], r[6])
            w64 = r[7:10].astype(np.float64)
            b = c @ w64
            x = (b - np.sqrt(max(b * b - kappa, 0.0))) * w64 - c
            us = x / np.linalg.norm(x)
        if not np.isfinite(us).all():
            us = r[7:10]
    r[11:14] = us
    return r


def _lobe64(n, d, rho):
    """(c, r, kappa) of the f32 operands in float64: where the rim lies"""
    n, d = np.asarray(n, F).astype(np.float64), np.asarray(d, F).astype(np.float64)
    rho = float(F(rho))
    g = d - 2 * (d @ n) * n
    r = 1 - rho
    c = r * n + rho * g
    return c, r, c @ c - r * r


def _rim_directions(n, d, rho, g, count):
    """Unit directions on the rim of the lobe of (n, d, rho) — b^2 = kappa — rounded to f32, each with its neighbours a few ulps to
    either side in the component that moves D most."""
    c, r, kappa = _lobe64(n, d, rho)
    ch = c / np.linalg.norm(c)
    ct = np.sqrt(max(kappa, 0.0)) / np.linalg.norm(c)                 # (kappa of a rounded, not exactly unit, n may be -1e-8)
    out = []
    for _ in range(count):
        t = np.cross(ch, g.normal(size=3))
        t /= np.linalg.norm(t)
        w = (ct * ch + np.sqrt(max(0.0, 1 - ct * ct)) * t).astype(F)
        k = int(np.argmax(np.abs(c)))
        for step in range(-6, 7):
            v = w.copy()
            for _ in range(abs(step)):
                v[k] = np.nextafter(v[k], F(np.inf if step > 0 else -np.inf))
            out.append(v)
    return out


def directed():
    """The directed corpus (m, 12) float32."""
    g = np.random.default_rng(1600)
    recs = []
    up = np.array([0.0, 1.0, 0.0])
    # rho on the class boundaries, at a front-face hit, a back-face hit and a grazing one (gn = 0 exactly), normal incidence (gn = 1)
    rhos = [0.0, -0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -23, 3e38, -0.5, np.nan, np.inf, -np.inf, 1e-45, 2.0 ** -126]
    for rho in rhos:
        for d in ([0.6, -0.8, 0.0], [0.6, 0.8, 0.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]):
            for _ in range(FLOOR // 4 + 1):
                recs.append(_rec(up, d, rho, _unit(g.normal(size=3) + [0, 1.5, 0]), g.choice([0.5, 40.0, np.inf, np.nan])))
    # the rim to the ulp, at every rho edge and a few inner ones, random unit normals and front-face directions
    for rho in list(RHO_EDGES) + [0.05, 0.3, 0.7, 0.95]:
        for _ in range(4):
            n = _unit(g.normal(size=3)).astype(F)
            d = _unit(g.normal(size=3))
            if d @ n > 0:
                d = -d
            d = d.astype(F)
            for w in _rim_directions(n, d, rho, g, 3):
                recs.append(_rec(n, d, rho, w))
    # b <= 0: directions behind the lobe, and b == 0 exactly
    for rho in (0.1, 0.5, 0.9):
        for _ in range(FLOOR):
            n = _unit(g.normal(size=3)).astype(F)
            d = (-n).astype(F)                             # normal incidence: g = n, c = n
            w = _unit(g.normal(size=3))
            if w @ n > 0:
                w = -w
            recs.append(_rec(n, d, rho, w))
        for _ in range(FLOOR):
            recs.append(_rec(up, [0.0, -1.0, 0.0], rho, [g.choice([-1.0, 1.0]), 0.0, 0.0]))
    # a non-unit incoming direction (RT_TRACE_RAY_AS_GIVEN): |d| from 2^-20 to 2^20
    for e in range(-20, 21, 2):
        for _ in range(2):
            n = _unit(g.normal(size=3)).astype(F)
            d = _unit(g.normal(size=3))
            if d @ n > 0:
                d = -d
            recs.append(_rec(n, (d * 2.0 ** e).astype(F), g.choice([0.1, 0.5, 0.9]), _unit(n + 0.3 * g.normal(size=3))))
    # NaN and inf in every operand
    for bad in (np.nan, np.inf, -np.inf):
        for slot in range(11):
            for _ in range(2):
                r = _rec(up, [0.6, -0.8, 0.0], 0.5, _unit(g.normal(size=3) + [0, 2, 0]))
                r[slot] = bad
                recs.append(r)
    # a zero normal (a degenerate triangle's) and a zero direction
    for _ in range(FLOOR):
        recs.append(_rec([0, 0, 0], _unit(g.normal(size=3)), 0.5, _unit(g.normal(size=3))))
        recs.append(_rec(up, [0, 0, 0], 0.5, _unit(g.normal(size=3))))
    return np.array(recs, F)


def seeded(m, seed=1601):
    """m seeded records: unit normals, directions of either face (three quarters front), rho over [0, 1.1) with the edges mixed in,
    w anywhere on the sphere or, half of the time, near the mirrored direction."""
    g = np.random.default_rng(seed)
    n = _unit(g.normal(size=(m, 3)))
    d = _unit(g.normal(size=(m, 3)))
    flip = (np.einsum("ij,ij->i", d, n) > 0) & (g.uniform(size=m) < 0.75)
    d[flip] = -d[flip]
    rho = g.uniform(0, 1.1, m)
    edge = g.uniform(size=m) < 0.05
    rho[edge] = g.choice([0.0, 2.0 ** -24, 1 - 2.0 ** -24, 1.0], edge.sum())
    gl = d - 2 * np.einsum("ij,ij->i", d, n)[:, None] * n
    w = _unit(g.normal(size=(m, 3)))
    near = g.uniform(size=m) < 0.5
    c = (1 - rho)[:, None] * n + rho[:, None] * gl
    w[near] = _unit(c[near] + (1 - rho[near])[:, None] * g.uniform(0.2, 1.2, near.sum())[:, None] * _unit(g.normal(size=(near.sum(), 3))))
    rec = np.zeros((m, WORDS[0]), F)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 7:10] = n, d, rho, w
    rec[:, 11:14] = _unit(g.normal(size=(m, 3)))                        # us: uniform on the sphere, as the scatter draws it
    rec[:, 10] = np.where(g.uniform(size=m) < 0.02, np.inf, g.uniform(0, 50, m))
    return rec


def records(n_random):
    return np.ascontiguousarray(np.concatenate([directed(), seeded(n_random)]))


def expected(rec):
    """The restatement's words (m, 16) uint32 for the records (m, 12) float32."""
    rec = np.ascontiguousarray(rec, F)
    n, d, rho, w, W = rec[:, 0:3].T.copy(), rec[:, 3:6].T.copy(), rec[:, 6].copy(), rec[:, 7:10].T.copy(), rec[:, 10].copy()
    us = rec[:, 11:14].T.copy()
    with np.errstate(all="ignore"):
        g = L.glossy_dir(d, n)
        gn = L.D.dot(n, g)
        cls = L.sampled_class(rho, gn)
        c, r, kappa = L.lobe_of(n, g, rho)
        # cg is defined by the header's formula in the lobe only, and is 0 outside it
        b, Dd, inl, cg = L.lobe_factor((c, r, kappa), w)
        taken = L.sample_taken(inl, W)
        sm, st, scg, sin = L.lobe_factor_scatter((c, r, kappa), us)
    out = np.zeros((len(rec), WORDS[1]), U32)
    out[:, 0] = cls
    for k, x in zip((1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 16, 17), (*g, gn, *c, r, kappa, b, Dd, cg, sm, st, scg)):
        out[:, k] = np.ascontiguousarray(np.broadcast_to(x, (len(rec),)), F).view(U32)
    out[:, 12], out[:, 14], out[:, 18] = inl, taken, sin
    return out


def words_equal(got, want):
    """(m, 16) bool: counts as integers, flags as booleans, floats bit for bit with NaN matching NaN"""
    ok = got == want
    gf, wf = got.view(F), want.view(F)
    ok |= np.isnan(gf) & np.isnan(wf)
    for k in FLAG_WORDS:
        ok[:, k] = (got[:, k] != 0) == (want[:, k] != 0)
    for k in COUNT_WORDS:
        ok[:, k] = got[:, k] == want[:, k]
    return ok


CLASSES = ("class none", "class diffuse", "class lobe", "rho==2^-24", "rho==0.5", "rho==1-2^-24", "rho==1", "rho<0", "rho NaN",
           "gn==0", "gn==1", "gn<0", "rim D>0 within 2^-20", "rim D<=0 within 2^-20", "b<=0", "b==0", "non-unit d", "NaN operand",
           "inf operand", "in lobe", "W==inf in lobe", "zero normal", "scatter in lobe", "scatter near the rim", "scatter cg NaN or 0")


def classify(rec, want):
    """{class: mask} over the records, from the records and the restatement's words alone."""
    f = want.view(F)
    rho, gn, kappa, b, Dd = rec[:, 6], f[:, 4], f[:, 9], f[:, 10], f[:, 11]
    with np.errstate(all="ignore"):
        dd = np.sqrt(np.einsum("ij,ij->i", rec[:, 3:6].astype(np.float64), rec[:, 3:6].astype(np.float64)))
        near = np.abs(Dd) <= F(2.0 ** -20) * kappa
        lobe_hit = want[:, 0] == L.LOBE
        m = {"class none": want[:, 0] == L.NONE, "class diffuse": want[:, 0] == L.DIFFUSE, "class lobe": lobe_hit,
             "rho==2^-24": rho == RHO_EDGES[0], "rho==0.5": rho == RHO_EDGES[1], "rho==1-2^-24": rho == RHO_EDGES[2], "rho==1": rho == 1,
             "rho<0": rho < 0, "rho NaN": np.isnan(rho), "gn==0": gn == 0, "gn==1": gn == 1, "gn<0": gn < 0,
             "rim D>0 within 2^-20": lobe_hit & near & (Dd > 0) & (b > 0), "rim D<=0 within 2^-20": lobe_hit & near & (Dd <= 0) & (b > 0),
             "b<=0": lobe_hit & (b <= 0), "b==0": lobe_hit & (b == 0), "non-unit d": np.isfinite(dd) & (np.abs(dd - 1) > 0.25) & (dd > 0),
             "NaN operand": np.isnan(rec[:, :11]).any(1), "inf operand": np.isinf(rec[:, :11]).any(1), "in lobe": want[:, 12] != 0,
             "W==inf in lobe": (want[:, 12] != 0) & np.isinf(rec[:, 10]), "zero normal": ~rec[:, 0:3].any(1),
             "scatter in lobe": lobe_hit & (want[:, 18] != 0), "scatter near the rim": lobe_hit & (np.abs(f[:, 15]) <= F(2.0 ** -10) * kappa),
             "scatter cg NaN or 0": ~(f[:, 17] > 0)}
    assert set(m) == set(CLASSES)
    return m
