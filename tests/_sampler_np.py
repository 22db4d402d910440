"""The film sampler restated in numpy from the text of ray_tracer_s8_amd/sampler_csrc/rt_sampler.h: np.float32
operations one at a time, in the order the header writes them, so that the library's result must equal it bit for bit.  Also the
seeded adversarial inputs the CPU and the GPU tests share, and the rounds of an rt.FilmSampler over given per-(pixel, sample) records."""
from __future__ import annotations

import numpy as np

f32 = np.float32
QNAN = np.array([0x7FC00000], np.uint32).view(f32)[0]
U = 2.0 ** -24


def canonical(x):
    return np.where(np.isnan(x), QNAN, x).astype(f32)


def spread(S1, S2, n_f):
    with np.errstate(all="ignore"):
        m = (S1 / n_f).astype(f32)
        a = (S2 / n_f).astype(f32)
        d = (a - (m * m).astype(f32)).astype(f32)
        return np.where(d > 0, d, f32(0)).astype(f32)


def pixel_error(M, counts, eps):
    """err of every pixel: M (..., 2) float32, counts (...) int32."""
    eps = f32(eps)
    n = np.asarray(counts, np.int32)
    n_f = n.astype(f32)
    S1, S2 = M[..., 0].astype(f32), M[..., 1].astype(f32)
    with np.errstate(all="ignore"):
        m = (S1 / n_f).astype(f32)
        d = spread(S1, S2, n_f)
        v = (d / (n_f - f32(1)).astype(f32)).astype(f32)
        err = (np.sqrt(v).astype(f32) / (np.abs(m) + eps).astype(f32)).astype(f32)
    return np.where(n < 2, QNAN, canonical(err)).astype(f32)


def noisy(err, threshold):
    with np.errstate(invalid="ignore"):
        return err > f32(threshold)


def dilated(flags, dilate):
    """active: any noisy pixel in the (2 dilate + 1)^2 window, clipped to the image."""
    R, W = flags.shape
    out = np.zeros((R, W), bool)
    for dy in range(-dilate, dilate + 1):
        for dx in range(-dilate, dilate + 1):
            src = flags[max(0, dy):R + min(0, dy), max(0, dx):W + min(0, dx)]
            out[max(0, -dy):R + min(0, -dy), max(0, -dx):W + min(0, -dx)] |= src
    return out


def select(M, counts, hs, threshold, dilate, eps):
    """rts_select: (err (R, W), [strip i's ascending uint32 strip indices], strip counts (R / hs) uint32)."""
    R, W = counts.shape
    assert R % hs == 0
    err = pixel_error(M, counts, eps)
    act = dilated(noisy(err, threshold), dilate)
    lists = [np.flatnonzero(act[i * hs:(i + 1) * hs].reshape(-1)).astype(np.uint32) for i in range(R // hs)]
    return err, lists, np.array([len(l) for l in lists], np.uint32)


def gather(active, k, records):
    """rts_gather on one buffer: records (pixels * k, ...) -> (len(active) * k, ...)."""
    idx = (active.astype(np.int64)[:, None] * k + np.arange(k)[None, :]).reshape(-1)
    return records[idx]


def fold(accum, moments, counts, active, rgb, k):
    """rts_fold on a strip: accum (P, 3), moments (P, 2), counts (P) and rgb (len(active) * k, 3); returns the new three."""
    acc, mom, cnt = accum.astype(f32).copy(), moments.astype(f32).copy(), counts.astype(np.int32).copy()
    p = active.astype(np.int64)
    rec = rgb.reshape(len(p), k, 3).astype(f32)
    with np.errstate(all="ignore"):
        for j in range(k):
            c = rec[:, j]
            acc[p] = (acc[p] + c).astype(f32)
            y = ((c[:, 0] + c[:, 1]).astype(f32) + c[:, 2]).astype(f32)
            mom[p, 0] = (mom[p, 0] + y).astype(f32)
            mom[p, 1] = (mom[p, 1] + (y * y).astype(f32)).astype(f32)
    cnt[p] += k
    return acc, mom, cnt


def normalise(A, M, counts, e0):
    """rts_normalise: the sums at the film's count e0.  A (..., 3), M (..., 2), counts (...)."""
    n = np.asarray(counts, np.int32)
    n_f, e0_f = n.astype(f32), f32(e0)
    S1, S2 = M[..., 0].astype(f32), M[..., 1].astype(f32)
    with np.errstate(all="ignore"):
        r = (e0_f / n_f).astype(f32)
        Ap = canonical((A * r[..., None]).astype(f32))
        S1p = (S1 * r).astype(f32)
        d = spread(S1, S2, n_f)
        g = ((e0_f - f32(1)) / (n_f - f32(1)).astype(f32)).astype(f32)
        mm = (S1p / e0_f).astype(f32)
        S2p = (((mm * mm).astype(f32) + (d * g).astype(f32)).astype(f32) * e0_f).astype(f32)
    same = n == e0
    oA = np.where(same[..., None], A, Ap).astype(f32)
    oM = np.stack([np.where(same, S1, canonical(S1p)), np.where(same, S2, canonical(S2p))], -1).astype(f32)
    # (np.where keeps the bytes of the operand it picks: a pixel at the film's count is a copy)
    return oA, oM


def true_variance(M, counts):
    """v = d / (n_f - 1) at every pixel's own count."""
    n_f = np.asarray(counts, np.int32).astype(f32)
    with np.errstate(all="ignore"):
        return (spread(M[..., 0].astype(f32), M[..., 1].astype(f32), n_f) / (n_f - f32(1)).astype(f32)).astype(f32)


def variance_bound(v_true, Mp, e0):
    """The bound of rt_sampler.h on |v0' - v|, in float64: 6u v + 4u a' / (e0 - 1) with a' = S2' / e0."""
    a = Mp[..., 1].astype(np.float64) / e0
    return 6 * U * v_true.astype(np.float64) + 4 * U * a / (e0 - 1)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------

def moments_of(rng, R, W, counts):
    """Sums as a film writes them at the given counts: per-pixel constant-plus-noise samples, with a quarter of the pixels constant
    (d is rounding noise, sometimes below 0) and a few dark."""
    n = np.asarray(counts, np.int64)
    base = rng.random((R, W)).astype(f32) * f32(3)
    base[rng.random((R, W)) < 0.1] = 0
    sig = rng.random((R, W)).astype(f32) * f32(0.5)
    sig[rng.random((R, W)) < 0.25] = 0
    n_f = n.astype(f32)
    S1 = (base * n_f).astype(f32)
    S2 = ((base * base + sig * sig).astype(f32) * n_f).astype(f32)
    return np.stack([S1, S2], -1).astype(f32)


def pattern(name, rng, R, W):
    """The noisy plane a test wants: 'none', 'all', 'first', 'last', 'random'."""
    flags = np.zeros((R, W), bool)
    if name == "all":
        flags[:] = True
    elif name == "first":
        flags[0, 0] = True
    elif name == "last":
        flags[-1, -1] = True
    elif name == "random":
        flags = rng.random((R, W)) < 0.5
    else:
        assert name == "none", name
    return flags


def moments_for(flags, n=8):
    """(M, counts, threshold, eps) whose noisy plane is exactly `flags`: a noisy pixel has err = 1 / sqrt(7) / (1 + eps), a quiet
    one err = 0, around the threshold 0.1."""
    R, W = flags.shape
    counts = np.full((R, W), n, np.int32)
    M = np.zeros((R, W, 2), f32)
    M[..., 0] = n                                                         # m = 1
    M[..., 1] = np.where(flags, f32(2 * n), f32(n))                       # a = 2 or 1: d = 1 or 0
    return M, counts, f32(0.1), f32(2.0 ** -6)


def adversarial(seed=0x5A11):
    """One 6 x 8 image of the cases a select must get right, as (M, counts, eps): cancellation (d < 0), infinite sums, NaNs, m = 0,
    n = 2 and n = 2^24, n < 2, negative means, subnormals."""
    rng = np.random.default_rng(seed)
    R, W = 6, 8
    counts = rng.integers(2, 40, (R, W)).astype(np.int32)
    M = moments_of(rng, R, W, counts)
    inf, nan = f32(np.inf), f32(np.nan)
    flat_M, flat_n = M.reshape(-1, 2), counts.reshape(-1)
    cases = [((3.0000002, 3.0), 3), ((inf, inf), 5), ((1.0, inf), 5), ((-inf, 7.0), 4), ((nan, 1.0), 4), ((1.0, nan), 4),
             ((0.0, 0.0), 6), ((0.0, 4.0), 6), ((-0.0, 1e-30), 9), ((2.0, 2.5), 2), ((2.0 ** 24, 2.0 ** 25), 1 << 24),
             ((5.0, 9.0), 1), ((5.0, 9.0), 0), ((5.0, 9.0), -3), ((-8.0, 40.0), 4), ((1e-40, 1e-44), 3), ((3e38, 3e38), 2),
             ((1e-20, 1e-38), 7)]
    at = rng.permutation(R * W)[:len(cases)]
    for i, (m, n) in zip(at, cases):
        flat_M[i] = m
        flat_n[i] = n
    return M, counts, f32(2.0 ** -6)


# ---- an rt.FilmSampler over given records -----------------------------------------------------------------------------------------------

class Rounds:
    """The state of an rt.FilmSampler restated: records (R, W, SPP, 3) holds the integrator's colour of every (pixel, sample); the
    floor is samples [0, e0) of every pixel."""

    def __init__(self, records, hs, e0, threshold, dilate, eps):
        R, W, spp, _ = records.shape
        self.records, self.hs, self.e0, self.spp = records.astype(f32), hs, e0, spp
        self.threshold, self.dilate, self.eps = f32(threshold), dilate, f32(eps)
        P = R * W
        acc, mom = np.zeros((P, 3), f32), np.zeros((P, 2), f32)
        acc, mom, cnt = fold(acc, mom, np.zeros(P, np.int32), np.arange(P, dtype=np.uint32), self.records[:, :, :e0].reshape(-1, 3), e0)
        self.accum, self.moments, self.counts = acc.reshape(R, W, 3), mom.reshape(R, W, 2), cnt.reshape(R, W)
        self.samples = e0
        self.err = self.lists = None

    def render_pass(self, n):
        b, e = self.samples, min(self.samples + n, self.spp)
        if b >= e:
            return 0
        R, W = self.counts.shape
        self.err, self.lists, cnt = select(self.moments, self.counts, self.hs, self.threshold, self.dilate, self.eps)
        if cnt.sum() == 0:
            return 0
        P = self.hs * W
        for i, active in enumerate(self.lists):
            if not len(active):
                continue
            rows = slice(i * self.hs, (i + 1) * self.hs)
            rec = self.records[rows, :, b:e].reshape(P, e - b, 3)[active.astype(np.int64)].reshape(-1, 3)
            a, m, c = fold(self.accum[rows].reshape(P, 3), self.moments[rows].reshape(P, 2), self.counts[rows].reshape(P), active, rec,
                           e - b)
            self.accum[rows], self.moments[rows], self.counts[rows] = a.reshape(self.hs, W, 3), m.reshape(self.hs, W, 2), c.reshape(self.hs, W)
        self.samples = e
        return int(cnt.sum())
