"""The numpy restatement of ray_tracer_s8_amd/bloom_csrc/rt_bloom.h, operation by operation in f32: the level shapes
and the scratch layout, the sanitised input, the threshold, down, up, the accumulation, both mixes and norm; the rule that places the
tail; and the seeded images the CPU and the GPU tests share.  Plain numpy, no GPU, and nothing of the product is imported."""
import struct

import numpy as np

import _extreme_planes as xp

f32, u32 = np.float32, np.uint32
MAX_LEVELS = 8
MIX, ADD = 0, 1
LEVELS, TAIL = 0, 1
LDS_BUDGET = 160 * 1024
THREE, EPS = f32(3), f32(1e-5)
DEFAULTS = dict(spread=0.7, strength=0.05, mode=MIX, threshold=0.0, knee=0.5, cap=65536.0)


def level_shapes(shape, levels):
    """[(R_0, W_0), ..., (R_L, W_L)]."""
    R, W = shape
    out = [(R, W)]
    for _ in range(levels):
        R, W = (R + 1) >> 1, (W + 1) >> 1
        out.append((R, W))
    return out


def default_levels(shape):
    k = 0
    while (2 << k) <= min(shape):
        k += 1
    return max(1, min(MAX_LEVELS, k))


def scratch_layout(shape, levels):
    """(the byte offsets of levels 1 ... L, the size): every level rounded up to 16 bytes."""
    at, offsets = 0, []
    for R, W in level_shapes(shape, levels)[1:]:
        offsets.append(at)
        at += -(-(R * W * 12) // 16) * 16
    return offsets, at


def tail_from(shape, levels, budget=LDS_BUDGET):
    """The least k >= 1 with the pixels of levels k ... L, 12 bytes each, within the budget; L + 1 if there is none."""
    sizes = [R * W * 12 for R, W in level_shapes(shape, levels)]
    fits = [k for k in range(1, levels + 1) if sum(sizes[k:]) <= budget]
    return min(fits) if fits else levels + 1


def launches(shape, levels, form):
    """How many kernels a call launches."""
    tf = tail_from(shape, levels) if form == TAIL else levels + 1
    return 2 * levels if tf > levels else (tf - 1) + 1 + (tf - 1) + 1


def as_f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def norm_of(spread, levels):
    """The f32 nearest to 1 / (spread^0 + ... + spread^(L-1)) in double, spread being the f32 the library sees."""
    s, total, term = as_f32(spread), 0.0, 1.0
    for _ in range(levels):
        total += term
        term *= s
    return f32(1.0 / total)


def knee_of(threshold, knee):
    return f32(f32(threshold) * f32(knee))


# ---- the input -------------------------------------------------------------------------------------------------------------------------
def positive(c):
    """q: a NaN, both zeros and every negative give +0."""
    c = np.asarray(c, f32)
    with np.errstate(invalid="ignore"):
        return np.where(c > 0, c, f32(0)).astype(f32)


def sanitise(c, cap):
    q = positive(c)
    return np.where(q < f32(cap), q, f32(cap)).astype(f32)


def threshold_factor(p, T, K):
    """f of the pixels p[..., 3] (sanitised)."""
    T, K = f32(T), f32(K)
    m = np.where(p[..., 0] > p[..., 1], p[..., 0], p[..., 1])
    m = np.where(m > p[..., 2], m, p[..., 2]).astype(f32)
    with np.errstate(all="ignore"):
        s = (m - f32(T - K)).astype(f32)
        s = np.where(s > 0, s, f32(0)).astype(f32)
        k2 = f32(K + K)
        s = np.where(s < k2, s, k2).astype(f32)
        g = ((s * s).astype(f32) / f32(f32(k2 + k2) + EPS)).astype(f32)
        e = (m - T).astype(f32)
        g = np.where(g > e, g, e).astype(f32)
        g = np.where(g > 0, g, f32(0)).astype(f32)
        return (g / np.where(m > EPS, m, EPS).astype(f32)).astype(f32)


def source(img, cap, T=0.0, K=0.0):
    """The pixels the pyramid starts from: sanitised, and under the threshold where T > 0."""
    p = sanitise(img, cap)
    if f32(T) > 0:
        with np.errstate(all="ignore"):
            p = (p * threshold_factor(p, T, K)[..., None]).astype(f32)
    return p


# ---- down ------------------------------------------------------------------------------------------------------------------------------
def down_taps(n_out, n_in):
    """[4][n_out]: clamp(2 i - 1 + a, 0, n_in - 1)."""
    i = np.arange(n_out)
    return [np.clip(2 * i - 1 + a, 0, n_in - 1) for a in range(4)]


def sum_1331(s0, s1, s2, s3):
    with np.errstate(all="ignore"):
        return ((s0 + (THREE * s1).astype(f32)).astype(f32) + ((THREE * s2).astype(f32) + s3).astype(f32)).astype(f32)


def down(S):
    """D_{k+1} of a level S [R][W][3]."""
    S = np.asarray(S, f32)
    R, W = S.shape[:2]
    cols, rows = down_taps((W + 1) >> 1, W), down_taps((R + 1) >> 1, R)
    h = sum_1331(*(S[:, c] for c in cols))                             # [R][W'][3]: h of every source row
    with np.errstate(all="ignore"):
        return (sum_1331(*(h[r] for r in rows)) * f32(0.015625)).astype(f32)


# ---- up --------------------------------------------------------------------------------------------------------------------------------
def up_taps(n_fine, n_coarse):
    """(a, b, wa, wb) of every fine index: the weights are chosen before the clamp."""
    y = np.arange(n_fine)
    ya = (y + 1) // 2 - 1
    wa = np.where(y & 1, 3, 1).astype(f32)
    return np.clip(ya, 0, n_coarse - 1), np.clip(ya + 1, 0, n_coarse - 1), wa, (f32(4) - wa).astype(f32)


def up(X, shape):
    """up(X) at the level of `shape` = (R, W), X being the level below it."""
    X = np.asarray(X, f32)
    ya, yb, wya, wyb = up_taps(shape[0], X.shape[0])
    xa, xb, wxa, wxb = up_taps(shape[1], X.shape[1])
    wxa, wxb = wxa[None, :, None], wxb[None, :, None]
    wya, wyb = wya[:, None, None], wyb[:, None, None]
    with np.errstate(all="ignore"):
        g = lambda r: ((wxa * X[r][:, xa]).astype(f32) + (wxb * X[r][:, xb]).astype(f32)).astype(f32)
        return (((wya * g(ya)).astype(f32) + (wyb * g(yb)).astype(f32)).astype(f32) * f32(0.0625)).astype(f32)


# ---- the whole -------------------------------------------------------------------------------------------------------------------------
def pyramid(img, levels, spread=0.7, cap=65536.0, T=0.0, K=0.0):
    """(D, U): dicts of the levels 1 ... L before and after the accumulation."""
    img = np.asarray(img, f32)
    shapes = level_shapes(img.shape[:2], levels)
    D, S = {}, source(img, cap, T, K)
    for k in range(1, levels + 1):
        S = D[k] = down(S)
        assert S.shape[:2] == shapes[k]
    U = {levels: D[levels]}
    with np.errstate(all="ignore"):
        for k in range(levels - 1, 0, -1):
            U[k] = (D[k] + (f32(spread) * up(U[k + 1], shapes[k])).astype(f32)).astype(f32)
    return D, U


def bloom(img, levels=None, spread=0.7, strength=0.05, mode=MIX, threshold=0.0, knee=0.5, cap=65536.0):
    """(out, b, U): the mixed image, the normalised bloom and the accumulated levels, as rtb_apply gives them."""
    img = np.asarray(img, f32)
    levels = default_levels(img.shape[:2]) if levels is None else levels
    _, U = pyramid(img, levels, spread, cap, threshold, knee_of(threshold, knee))
    q, g = positive(img), f32(strength)
    with np.errstate(all="ignore"):
        b = (up(U[1], img.shape[:2]) * norm_of(spread, levels)).astype(f32)
        if mode == MIX:
            out = ((f32(f32(1) - g) * q).astype(f32) + (g * b).astype(f32)).astype(f32)
        else:
            out = (q + (g * b).astype(f32)).astype(f32)
    return out, b, U


# ---- images ----------------------------------------------------------------------------------------------------------------------------
# rows x columns and levels: what the GPU test runs (tests/test_gpu_bloom.py says why each is there)
SHAPES = [((1, 1), 1), ((1, 1), 8), ((2, 3), 2), ((5, 37), 3), ((67, 9), 6), ((131, 71), 8), ((200, 260), 1), ((240, 260), 1),
          ((200, 260), 6), ((75, 283), 4)]


def log_uniform(shape, seed, lo=-12.0, hi=8.0):
    """Colours 2^lo ... 2^hi, a tenth of them negative."""
    rng = np.random.default_rng(seed)
    v = np.exp2(rng.uniform(lo, hi, (*shape, 3)))
    return (v * np.where(rng.random(v.shape) < 0.1, -1.0, 1.0)).astype(f32)


def impulse(shape, at, value=1000.0):
    img = np.zeros((*shape, 3), f32)
    img[at] = (value, value / 2, value / 4)
    return img


def extreme(shape, tier, seed):
    """A log-uniform image with the tier's values of tests/_extreme_planes.py in it: salted for the small tier (with its block of
    subnormal pixels), on a lattice of pitch 3 for the other two, whole pixels of them too, so that the values meet in the taps."""
    base = np.abs(log_uniform(shape, seed))
    rng = np.random.default_rng([seed, 7])
    if tier == "small":
        return xp.salted(base, xp.SMALL, 0.25, rng, block=True)
    vals = xp.values(tier, "colour")
    out = xp.sparse(base, vals, (0, 0), pitch=3, first=seed)
    flat = out.reshape(-1, 3)
    for j, v in enumerate(vals):                                         # and whole pixels
        flat[(5 * j + 1) % len(flat)] = v
    return out


def threshold_pixels(T, K):
    """Pixels whose m lies on, just below and just above T - K, T and T + K, and tiny ones; the other channels below m."""
    T, K = f32(T), f32(K)
    ms = []
    for c in (f32(T - K), T, f32(T + K)):
        ms += [np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))]
    ms += [f32(0), f32(1e-45), f32(1e-30), f32(9.99e-6), f32(1e-5), f32(1.01e-5), f32(2e-5), f32(65536)]
    ms = np.maximum(np.array(ms, f32), f32(0))
    px = np.stack([ms, (ms * f32(0.5)).astype(f32), (ms * f32(0.125)).astype(f32)], -1)
    return np.concatenate([px, px[:, ::-1], px[:, [1, 0, 2]]])


THRESHOLDS = [(1.0, 0.5), (1.0, 0.0), (1.0, 1.0), (0.25, 0.125), (1e-4, 5e-5), (40000.0, 20000.0), (3.0, 0.75)]     # (T, K)
