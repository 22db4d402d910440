"""numpy restatement of the film library's regression resolve (ray_tracer_s8_amd/film_csrc/rt_film.h "Regression resolve", DESIGN.md
4.31), written from the header's text and vectorised over nodes and pixels.  With dtype=np.float32 every step is an f32 ufunc on f32
operands (correctly rounded, never fused) in the order the text writes, so the library's result must equal it bit for bit; with
dtype=np.float64 the same text is evaluated in double precision on the same inputs, which is what the f32 evaluation's rounding error
is measured against.

resolve(C, e, ...) takes the image P: C (R, W, 3) float32 colour sums; planes as (R, W, 3) / (R, W) arrays or None.  Returns
dict(model=(NY, NX, 32), linear=, f32=, rgb=) and, for the tests of properties, valid= and r= (the entry colour)."""
from __future__ import annotations

import numpy as np

import _denoise_np as dn

f32 = np.float32
T = 16
M = 8
RECORD = 32


def nodes(W, R):
    return (R - 1) // T + 2, (W - 1) // T + 2


def entry(C, e, A, k, eps, N, D, hits, ft):
    """r_p, d_p (None without albedo), the unit normal (zeros without a plane), z_p and validity, all in ft."""
    R, W = C.shape[:2]
    with np.errstate(all="ignore"):
        c = C.astype(ft) / ft(e)
        d = None
        if A is not None:
            d = A.astype(ft) / ft(k) + ft(eps)
            r = c / d
        else:
            r = c
        n = np.zeros((R, W, 3), ft)
        if N is not None:
            Nf = N.astype(ft)
            L = np.sqrt((Nf[..., 0] * Nf[..., 0] + Nf[..., 1] * Nf[..., 1]) + Nf[..., 2] * Nf[..., 2])
            n = np.where((L > 0)[..., None], Nf / L[..., None], ft(0)).astype(ft)
        z = np.zeros((R, W), ft)
        if D is not None:
            assert hits is not None, "depth needs hits"
            z = np.where(hits > 0, D.astype(ft) / hits.astype(ft), ft(0)).astype(ft)
        g = hits > 0 if hits is not None else np.ones((R, W), bool)
        zg = np.where(g, z, ft(-1)).astype(ft)
    valid = zg >= 0
    zp = np.where(zg > 0, zg, ft(0)).astype(ft)
    return r.astype(ft), d, n, zp, valid


def windows(a, NY, NX, fill):
    """(NY * NX, 1024): the 32 x 32 window of every node out of an (R, W) plane, lane 32 wy + wx, `fill` outside P."""
    R, W = a.shape
    pad = np.full((T * (NY + 1), T * (NX + 1)), fill, a.dtype)
    pad[T:T + R, T:T + W] = a
    v = np.lib.stride_tricks.sliding_window_view(pad, (2 * T, 2 * T))[::T, ::T]
    assert v.shape == (NY, NX, 2 * T, 2 * T), v.shape
    return np.ascontiguousarray(v).reshape(NY * NX, 4 * T * T)


def window_sum(v, valid, ft):
    """S(v) of every node: v (NN, 1024), +0 where not valid; sixteen adjacent-pair trees of 64 lanes, their totals added in order."""
    with np.errstate(all="ignore"):
        t = np.where(valid, v, ft(0)).astype(ft).reshape(v.shape[0], 16, 64)
        for _ in range(6):
            t = (t[..., 0::2] + t[..., 1::2]).astype(ft)
        t = t[..., 0]
        s = np.zeros(v.shape[0], ft)
        for k in range(16):
            s = (s + t[:, k]).astype(ft)
    return s


def features(nrm, z, zlo, s, dx, dy, ft):
    """phi [8] of pixels: nrm (..., 3), z, the node's zlo and s, dx = x - 16 i and dy = y - 16 j as integers (all broadcastable)."""
    with np.errstate(all="ignore"):
        shape = np.broadcast(z, zlo, dx, dy).shape
        zeta = np.broadcast_to(np.where(s > 0, (z - zlo) / s, ft(0)).astype(ft), shape)
        phi6 = np.broadcast_to(((dx.astype(ft) + ft(0.5)) / ft(16)).astype(ft), shape)
        phi7 = np.broadcast_to(((dy.astype(ft) + ft(0.5)) / ft(16)).astype(ft), shape)
        return [np.ones(shape, ft), nrm[..., 0], nrm[..., 1], nrm[..., 2], zeta, (zeta * zeta).astype(ft), phi6, phi7]


def fit(r, nrm, z, valid, depth_given, ridge, ft):
    """The records (NY, NX, 32) of every node."""
    R, W = z.shape
    NY, NX = nodes(W, R)
    NN = NY * NX
    wv = windows(valid, NY, NX, False)
    wz = windows(z, NY, NX, ft(0))
    wr = [windows(np.ascontiguousarray(r[..., c]), NY, NX, ft(0)) for c in range(3)]
    wn = np.stack([windows(np.ascontiguousarray(nrm[..., c]), NY, NX, ft(0)) for c in range(3)], -1)
    n = wv.sum(1)
    n_f = n.astype(ft)
    with np.errstate(all="ignore"):
        zlo = np.fmin.reduce(np.where(wv, wz, ft(np.inf)), axis=1).astype(ft)
        zhi = np.fmax.reduce(np.where(wv, wz, ft(0)), axis=1).astype(ft)
        if not depth_given:
            zlo[:], zhi[:] = 0, 0
        zlo[n == 0] = 0
        zhi[n == 0] = 0
        s = (zhi - zlo).astype(ft)
        lane = np.arange(4 * T * T)
        dx, dy = (lane % (2 * T) - T)[None, :], (lane // (2 * T) - T)[None, :]
        phi = features(wn, wz, zlo[:, None], s[:, None], dx, dy, ft)
        A = [[None] * M for _ in range(M)]
        for a in range(M):
            for b in range(a, M):
                A[a][b] = window_sum((phi[a] * phi[b]).astype(ft), wv, ft)
        B = [[window_sum((phi[a] * wr[c]).astype(ft), wv, ft) for c in range(3)] for a in range(M)]
        rn = (ft(ridge) * n_f).astype(ft)
        for a in range(1, M):
            A[a][a] = (A[a][a] + rn).astype(ft)
        # Cholesky
        ok = n > 0
        L = [[None] * M for _ in range(M)]
        for a in range(M):
            p = A[a][a]
            for t in range(a):
                p = (p - L[a][t] * L[a][t]).astype(ft)
            ok = ok & (p > 0)
            L[a][a] = np.sqrt(p).astype(ft)
            for b in range(a + 1, M):
                q = A[a][b]
                for t in range(a):
                    q = (q - L[b][t] * L[a][t]).astype(ft)
                L[b][a] = (q / L[a][a]).astype(ft)
        model = np.zeros((NN, RECORD), ft)
        for c in range(3):
            y = [None] * M
            for a in range(M):
                v = B[a][c]
                for t in range(a):
                    v = (v - L[a][t] * y[t]).astype(ft)
                y[a] = (v / L[a][a]).astype(ft)
            w = [None] * M
            for a in range(M - 1, -1, -1):
                v = y[a]
                for t in range(a + 1, M):
                    v = (v - L[t][a] * w[t]).astype(ft)
                w[a] = (v / L[a][a]).astype(ft)
            const = np.where(n > 0, B[0][c] / np.where(n > 0, n_f, ft(1)), ft(0)).astype(ft)
            model[:, c] = np.where(ok, w[0], const)
            for a in range(1, M):
                model[:, 3 * a + c] = np.where(ok, w[a], ft(0))
        model[:, 24], model[:, 25], model[:, 26] = zlo, s, n_f
        model[:, 27] = np.where(ok, ft(1), ft(0))
    return model.reshape(NY, NX, RECORD)


def apply(r, nrm, z, valid, model, ft):
    """r' (R, W, 3): the blend of the four nodes' models at every valid pixel, r elsewhere."""
    R, W = z.shape
    yy, xx = np.mgrid[0:R, 0:W]
    ci, cj = xx >> 4, yy >> 4
    with np.errstate(all="ignore"):
        fx = (((xx & 15).astype(ft) + ft(0.5)) / ft(16)).astype(ft)
        fy = (((yy & 15).astype(ft) + ft(0.5)) / ft(16)).astype(ft)
        wts = [(ft(1) - fx) * (ft(1) - fy), fx * (ft(1) - fy), (ft(1) - fx) * fy, fx * fy]
        acc = np.zeros((R, W, 3), ft)
        for k in range(4):
            i, j = ci + (k & 1), cj + (k >> 1)
            rec = model[j, i]
            phi = features(nrm, z, rec[..., 24], rec[..., 25], xx - T * i, yy - T * j, ft)
            for c in range(3):
                m = np.zeros((R, W), ft)
                for a in range(M):
                    m = (m + rec[..., 3 * a + c] * phi[a]).astype(ft)
                acc[..., c] = (acc[..., c] + wts[k].astype(ft) * m).astype(ft)
        acc = np.where(acc > 0, acc, ft(0)).astype(ft)
    return np.where(valid[..., None], acc, r).astype(ft)


def resolve(C, e, *, A=None, k=1, albedo_eps=f32(2.0 ** -8), N=None, D=None, hits=None, ridge=f32(1e-3), dtype=np.float32):
    """The regression resolve on the image P in `dtype` arithmetic (ridge and albedo_eps are the call's float32 values)."""
    assert e >= 1
    ft = dtype
    C = np.ascontiguousarray(C, f32)
    ridge, albedo_eps = f32(ridge), f32(albedo_eps)
    r, d, nrm, z, valid = entry(C, e, A, k, albedo_eps, N, D, hits, ft)
    model = fit(r, nrm, z, valid, D is not None, ridge, ft)
    rp = apply(r, nrm, z, valid, model, ft)
    with np.errstate(all="ignore"):
        m = (rp * d).astype(ft) if d is not None else rp
        f = np.sqrt(m).astype(ft)
        rgb = dn.as_u8((f * ft(255.999)).astype(f32)) if ft is np.float32 else None
    return dict(model=model, linear=m, f32=f, rgb=rgb, valid=valid, r=r, fitted=rp)


# ---- synthetic images ---------------------------------------------------------------------------------------------------------------
def synthetic(rng, R, W, e=8, k=4):
    """Sums as the film writes them after e colour samples and k feature samples: a sky band (hits 0), partial hits, zero normal sums,
    two depth layers with a gradient, an albedo texture, and a colour that is albedo times a smooth shading plus noise.  Returns
    dict(C, A, N, D, hits) in the film's layout."""
    yy, xx = np.mgrid[0:R, 0:W]
    hits = rng.integers(1, k + 1, (R, W)).astype(np.uint32)
    hits[: max(1, R // 4)] = 0
    hits[rng.random((R, W)) < 0.05] = 0
    if R * W == 1:
        hits[:] = k
    geo = hits > 0
    nrm = rng.normal(size=(R, W, 3)).astype(f32) * f32(0.2) + np.array([0.3, 0.5, 0.8], f32)
    nrm = (nrm * hits[..., None].astype(f32)).astype(f32)
    nrm[rng.random((R, W)) < 0.05] = 0
    nrm[~geo] = 0
    layer = np.where(xx > W // 2, f32(2), f32(9)).astype(f32)
    dep = ((layer + f32(0.01) * yy.astype(f32)) * hits.astype(f32)).astype(f32)
    dep[~geo] = 0
    alb = (rng.random((R, W, 3)).astype(f32) * f32(0.8) + f32(0.1)) * f32(k)
    alb[~geo] = 0
    shade = (f32(0.5) + f32(0.3) * np.sin(xx / f32(7.0)) * np.cos(yy / f32(5.0))).astype(f32)
    noise = rng.random((R, W, 3)).astype(f32)
    col = ((alb / f32(k)) * shade[..., None] * (f32(0.5) + noise)).astype(f32)
    col[~geo] = np.array([0.6, 0.7, 0.9], f32)
    return dict(C=(col * f32(e)).astype(f32), A=alb.astype(f32), N=nrm, D=dep, hits=hits)


# the plane subsets of the tests: none, hits, normal, depth with hits, all four
SUBSETS = ((), ("hits",), ("normal",), ("depth", "hits"), ("albedo", "normal", "depth", "hits"))
KEYS = dict(albedo="A", normal="N", depth="D", hits="hits")


def np_planes(s, names):
    """resolve()'s plane arguments for a subset of names out of a synthetic image."""
    return {KEYS[n]: (s[KEYS[n]] if n in names else None) for n in KEYS}


# ---- extreme planes (tests/_extreme_planes.py) ------------------------------------------------------------------------
EXTREME_ROLES = dict(C="colour", A="albedo", N="normal", D="depth", hits="hits")
EXTREME_SETS = (("albedo",), ("normal", "depth", "hits"), ("albedo", "normal", "depth", "hits"))


def extreme_cases(tier, eps):
    """(name, plane names, planes) of a tier, what both the CPU and the GPU test run: the synthetic image of the tier's size with the
    tier's values salted into (small) or placed sparsely on (huge, nonfinite) the planes of one role at a time and of all at once."""
    import _extreme_planes as xp
    R, W = xp.FILTER_SIZES[tier]
    base = synthetic(np.random.default_rng(4310 + R), R, W, xp.E, xp.K)
    zero = f32(-(f32(eps) * f32(xp.K)))
    for i, names in enumerate(EXTREME_SETS):
        roles = ("colour",) + tuple(n for n in names if n != "hits")
        for j, (name, which) in enumerate(xp._distinct(xp.cases(tier, roles))):
            yield name, names, xp.apply(base, EXTREME_ROLES, tier, which, 100 * i + j, dict(A=zero), block=xp.FLOAT_ROLES)
