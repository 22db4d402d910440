"""numpy restatement of the a-trous denoiser's contract (include/rt_tile.h "denoiser"), vectorised per tap.  Every step is an f32 ufunc
on f32 operands (correctly rounded, never fused), in the order the header writes, so the library's result must equal it bit for bit.

denoise(C, e, ...) takes the image P stacked from the strips: C (R, W, 3) float32 sums; planes as (R, W, 3) / (R, W) arrays or None."""
from __future__ import annotations

import numpy as np

f32 = np.float32
H = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], f32)


def defaults():
    """rt_denoise_request_defaults, as a dict of the fields this module reads."""
    return dict(iterations=5, k_color=f32(0.01), color_step_scale=f32(4.0), k_normal=f32(1.0), k_depth=f32(4.0),
                albedo_eps=f32(2.0 ** -8))


def entry(C, e, A=None, k=1, eps=f32(2.0 ** -8), N=None, D=None, hits=None):
    """r0, d (None without albedo), the unit normal n (or None), zg (g ? z : -1)."""
    c = C / f32(e)
    d = None
    if A is not None:
        d = A / f32(k) + f32(eps)
        r = c / d
    else:
        r = c
    n = None
    if N is not None:
        L = np.sqrt((N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.where((L > 0)[..., None], N / L[..., None], f32(0)).astype(f32)
    R, W = C.shape[:2]
    z = np.zeros((R, W), f32)
    if D is not None:
        assert hits is not None, "depth needs hits"
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(hits > 0, D / hits.astype(f32), f32(0)).astype(f32)
    g = hits > 0 if hits is not None else np.ones((R, W), bool)
    zg = np.where(g, z, f32(-1)).astype(f32)
    return r.astype(f32), d, n, zg


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx] where that lies in the image, else fill."""
    R, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys, ye = max(0, -dy), min(R, R - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        b[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
    return b


def step(r, n, zg, s, kc, kn, kd, guided, depth):
    """One iteration at step s: r (R, W, 3) -> (R, W, 3)."""
    R, W = r.shape[:2]
    kc, kn, kd = f32(kc), f32(kn), f32(kd)
    with np.errstate(divide="ignore"):
        qp = np.where(zg > 0, f32(1) / zg, f32(0)).astype(f32) if depth else None
    zp = np.where(zg > 0, zg, f32(0)).astype(f32)
    nzero_p = np.all(n == 0, axis=-1) if n is not None else None
    yy, xx = np.mgrid[0:R, 0:W]
    sw = np.zeros((R, W), f32)
    sc = np.zeros((R, W, 3), f32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = s * dy, s * dx
            inside = (yy + oy >= 0) & (yy + oy < R) & (xx + ox >= 0) & (xx + ox < W)
            h = H[dy + 2] * H[dx + 2]
            if dy == 0 and dx == 0:
                w = np.full((R, W), h, f32)
                rq = r
                take = inside
            else:
                rq = _shift(r, oy, ox, f32(0))
                zq_g = _shift(zg, oy, ox, f32(0))
                take = inside
                if guided:
                    take = take & ((zq_g >= 0) == (zg >= 0))
                dd = rq - r
                x = ((dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]) * kc
                if n is not None:
                    nq = _shift(n, oy, ox, f32(0))
                    both = nzero_p & np.all(nq == 0, axis=-1)
                    dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    x = np.where(both, x, x + (f32(1) - dot) * kn).astype(f32)
                if depth:
                    zq = np.where(zq_g > 0, zq_g, f32(0)).astype(f32)
                    x = x + (np.abs(zq - zp) * qp) * kd
                u = f32(1) - x
                t = np.where(u > 0, u, f32(0)).astype(f32)
                w = h * (t * t)
            sw = np.where(take, sw + w, sw).astype(f32)
            sc = np.where(take[..., None], sc + w[..., None] * rq, sc).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (sc / sw[..., None]).astype(f32)


def as_u8(v):
    """Rust `as u8` from f32: truncate, saturate, NaN -> 0."""
    v = np.asarray(v, f32)
    out = np.zeros(v.shape, np.uint8)
    ok = v == v
    hi = ok & (v >= 255)
    mid = ok & (v > 0) & (v < 255)
    out[hi] = 255
    out[mid] = v[mid].astype(np.int32).astype(np.uint8)
    return out


def denoise(C, e, *, A=None, k=1, N=None, D=None, hits=None, iterations=5, k_color=f32(0.01), color_step_scale=f32(4.0),
            k_normal=f32(1.0), k_depth=f32(4.0), albedo_eps=f32(2.0 ** -8)):
    """The filter on the image P; returns dict(linear=, f32=, rgb=)."""
    C = np.ascontiguousarray(C, f32)
    r, d, n, zg = entry(C, e, A, k, albedo_eps, N, D, hits)
    guided = N is not None or D is not None or hits is not None
    kc = f32(k_color)
    for i in range(iterations):
        r = step(r, n, zg, 1 << i, kc, k_normal, k_depth, guided, D is not None)
        kc = f32(kc * f32(color_step_scale))
    m = (r * d).astype(f32) if d is not None else r
    with np.errstate(invalid="ignore"):
        f = np.sqrt(m).astype(f32)
    return dict(linear=m, f32=f, rgb=as_u8(f * f32(255.999)))
