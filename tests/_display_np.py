"""The numpy restatement of ray_tracer_s8_amd/display_csrc/rt_display.h, every operation cast to f32 in the order the
header writes it: `bins` (with a second writing of the definition from np.frexp, `bins_frexp`), `histogram`, `expose` (a record in, a
record out) and `apply`; and the corpora the CPU test (tests/test_display_host.py) and the GPU test (tests/test_gpu_display.py) share.
Plain numpy, no GPU."""
import numpy as np

import _extreme_planes as xp

f32 = np.float32
u32 = np.uint32
INF = f32(np.inf)
BINS, WORDS, EXCLUDED, BASE = 256, 257, 256, 888
AUTO, MANUAL = 0, 1
NONE, REINHARD, FILMIC = 0, 1, 2
CURVES = (NONE, REINHARD, FILMIC)
FIELDS = ("scale", "white", "target", "bin_key", "bin_white", "counted", "excluded", "frames")
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.uint32)
DEFAULTS = dict(key=0.54, key_q16=32768, white_q16=64880, rate=1.0, scale_min=2.0 ** -8, scale_max=2.0 ** 8)


def _quiet():
    return np.errstate(all="ignore")


# ---- metering --------------------------------------------------------------------------------------------------------------------------
def luminance(img):
    img = np.asarray(img, f32)
    with _quiet():
        return ((img[..., 0] + img[..., 1]).astype(f32) + img[..., 2]).astype(f32)


def bins(y):
    """The histogram word of every luminance: 0 ... 255, or 256 for the excluded (NaN, both zeros, negatives)."""
    y = np.ascontiguousarray(y, f32)
    with _quiet():
        excluded = (y != y) | ~(y > 0)
    q = (y.view(u32) >> u32(20)).astype(np.int64)
    return np.where(excluded, EXCLUDED, np.clip(q - BASE, 0, BINS - 1)).astype(np.int64)


def bins_frexp(y):
    """The definition a second time, from the value and not the bits: eight bins an octave over 2^-16 ... 2^16.  With y = m 2^E,
    m in [1, 2): 8 E + floor(8 (m - 1)), offset by 128 and clamped; +inf in the last bin."""
    with _quiet():
        y = np.ascontiguousarray(y, f32).astype(np.float64)
        excluded = (y != y) | ~(y > 0)
        m, e = np.frexp(np.where(excluded | np.isinf(y), 1.0, y))          # y = m 2^e, m in [0.5, 1)
    b = 8 * (e.astype(np.int64) - 1) + np.floor(8 * (2 * m - 1)).astype(np.int64) + 128
    b = np.where(np.isinf(y), BINS - 1, np.clip(b, 0, BINS - 1))
    return np.where(excluded, EXCLUDED, b).astype(np.int64)


def histogram(img):
    """The 257 counts of an image (..., 3)."""
    return np.bincount(bins(luminance(img)).reshape(-1), minlength=WORDS).astype(u32)


# ---- exposure --------------------------------------------------------------------------------------------------------------------------
def record0():
    """The record a display starts with."""
    return dict(scale=f32(1), white=INF, target=f32(1), bin_key=0, bin_white=0, counted=0, excluded=0, frames=0)


def rep(b):
    return np.array([((int(b) + BASE) << 20) | 0x80000], u32).view(f32)[0]


def bin_at(H, q16):
    """(N, the least b with H[0] + ... + H[b] > t) for t = (N q16) >> 16, in Python integers; b is None where N == 0."""
    N = int(np.asarray(H[:BINS], np.uint64).sum())
    t = ((N * int(q16)) >> 16) & 0xFFFFFFFF
    cum = 0
    for b in range(BINS):
        cum += int(H[b])
        if cum > t:
            return N, b
    return N, None


def _next(frames):
    return frames if frames == 0xFFFFFFFF else frames + 1


def expose(H, rec, mode=AUTO, key=0.54, key_q16=32768, white_q16=64880, rate=1.0, scale_min=2.0 ** -8, scale_max=2.0 ** 8, scale=1.0,
           white=np.inf):
    """The record after rtd_expose: `rec` is not written."""
    r = dict(rec)
    if mode == MANUAL:
        r.update(scale=f32(scale), white=f32(white), target=f32(scale), bin_key=0, bin_white=0, frames=_next(rec["frames"]))
        return r
    key, rate, smin, smax = f32(key), f32(rate), f32(scale_min), f32(scale_max)
    N, bk = bin_at(H, key_q16)
    _, bw = bin_at(H, white_q16)
    if N == 0:
        r.update(bin_key=0, bin_white=0)
        if rec["frames"] == 0:
            r.update(scale=f32(1), white=INF, target=f32(1))
    else:
        with _quiet():
            target = f32(key / rep(bk))
            target = smin if target < smin else target
            target = target if target < smax else smax
            if rec["frames"] == 0 or rate >= 1:
                s = target
            else:
                d = f32(target - rec["scale"])
                s = f32(rec["scale"] + f32(rate * d))
            w = f32(f32(rep(bw) * s) / f32(3))
            w = w if w > 1 else f32(1)
        r.update(scale=f32(s), white=f32(w), target=f32(target), bin_key=bk, bin_white=bw)
    r.update(counted=N, excluded=int(H[EXCLUDED]), frames=_next(rec["frames"]))
    return r


def record_words(rec):
    """A record as its eight 32-bit words."""
    w = np.zeros(8, u32)
    w[:3] = np.array([rec["scale"], rec["white"], rec["target"]], f32).view(u32)
    w[3:] = [rec[k] for k in FIELDS[3:]]
    return w


def record_of(words):
    words = np.ascontiguousarray(words).view(u32)
    r = dict(zip(FIELDS[:3], words[:3].view(f32)))
    r.update(zip(FIELDS[3:], (int(v) for v in words[3:])))
    return r


def same_record(got, want, what):
    """Bit for bit: the record's floats are never NaN under arguments the library accepts."""
    a, b = record_words(got), record_words(want)
    assert (a == b).all(), (what, {k: (got[k], want[k]) for k in FIELDS if got[k] != want[k]})


# ---- display ---------------------------------------------------------------------------------------------------------------------------
def tone(c, curve, scale, white):
    """Steps 1 and 2: t of every channel value."""
    c = np.asarray(c, f32)
    scale, white = f32(scale), f32(white)
    one = f32(1)
    with _quiet():
        x = (c * scale).astype(f32)
        x = np.where(x > 0, x, f32(0)).astype(f32)
        if curve == NONE:
            return x
        if curve == REINHARD:
            w2 = f32(white * white)
            t = ((x * (one + (x / w2).astype(f32)).astype(f32)).astype(f32) / (one + x).astype(f32)).astype(f32)
        else:
            n = (x * ((f32(2.51) * x).astype(f32) + f32(0.03)).astype(f32)).astype(f32)
            d = ((x * ((f32(2.43) * x).astype(f32) + f32(0.59)).astype(f32)).astype(f32) + f32(0.14)).astype(f32)
            t = (n / d).astype(f32)
        return np.where(t < 1, t, one).astype(f32)


def as_u8(v):
    v = np.asarray(v, f32)
    with _quiet():
        body = np.where((v > 0) & (v < 255), v, f32(0)).astype(np.int64)                   # (NaN and v <= 0 are 0)
        return np.where(v >= 255, 255, body).astype(np.uint8)


def quantise(f, dither=False, row=None, col=None):
    """Step 4 of values f at pixels (row, col), arrays that broadcast against f."""
    f = np.asarray(f, f32)
    with _quiet():
        if not dither:
            return as_u8((f * f32(255.999)).astype(f32))
        off = ((BAYER[np.asarray(row) & 3, np.asarray(col) & 3].astype(f32) + f32(0.5)).astype(f32) / f32(16)).astype(f32)
        return as_u8(((f * f32(255)).astype(f32) + off).astype(f32))


def apply(img, rec, curve, dither=False):
    """(f32, rgb) of an image (R, W, 3) under a record."""
    img = np.asarray(img, f32)
    R, W = img.shape[:2]
    with _quiet():
        f = np.sqrt(tone(img, curve, rec["scale"], rec["white"])).astype(f32)
    row, col = np.arange(R)[:, None, None], np.arange(W)[None, :, None]
    return f, quantise(f, dither, row, col)


# ---- corpora ---------------------------------------------------------------------------------------------------------------------------
def from_bits(b):
    return np.asarray(b, u32).view(f32)


def edge_luminances():
    """For every q in 880 ... 1150 the floats with bits q << 20, (q << 20) - 1 and (q << 20) | 0xFFFFF; both zeros, negatives, NaNs of
    both signs, both infinities, subnormals; the SMALL, HUGE and NONFINITE values of tests/_extreme_planes.py."""
    q = np.arange(880, 1151, dtype=np.uint64)
    edges = np.concatenate([q << 20, (q << 20) - 1, (q << 20) | 0xFFFFF]).astype(u32)
    fixed = from_bits([0, 0x80000000, 0xBF800000, 0x80000001, xp.QNAN, xp.NEG_QNAN, xp.SNAN, 0x7F800000, 0xFF800000, 1, 0x00400000,
                       0x007FFFFF, 0x00800000])
    return np.concatenate([from_bits(edges), fixed, xp.SMALL, xp.HUGE, xp.NONFINITE]).astype(f32)


def edge_colours():
    """The edge luminances as colours: (y, +0, +0), whose channel sum is y itself (but for -0, which the sum turns into +0, excluded like
    it), (+0, y, -0) likewise, and the grey (y, y, y), whose sum lands elsewhere."""
    y = edge_luminances()
    z = np.zeros_like(y)
    return np.concatenate([np.stack([y, z, z], 1), np.stack([z, y, -z], 1), np.stack([y, y, y], 1)]).astype(f32)


def tiled(colours, R, W, shift=0):
    """An image (R, W, 3) with the colours repeated over it in order, from colour `shift`."""
    idx = (np.arange(R * W) + shift) % len(colours)
    return np.ascontiguousarray(colours[idx].reshape(R, W, 3), f32)


def log_uniform(rng, R, W, lo=-20.0, hi=20.0, negative=0.1):
    """Log-uniform channel values in 2^lo ... 2^hi, a share of them with a random sign."""
    v = np.exp2(rng.uniform(lo, hi, (R, W, 3))).astype(f32)
    return np.where(rng.random((R, W, 3)) < negative, -v, v).astype(f32)


def extreme_image(R, W, tier):
    """Log-uniform noise with a quarter of the entries replaced by the tier's values (tests/_extreme_planes.py)."""
    rng = np.random.default_rng([4300, R, W, xp.TIERS.index(tier)])
    vals = dict(small=xp.SMALL, huge=xp.HUGE, nonfinite=xp.NONFINITE)[tier]
    return xp.salted(log_uniform(rng, R, W, -6, 6, 0.0), vals, 0.25, rng)


def meter_images(R, W):
    """{name: image} of the metering corpus at a size: a constant image, the bin edges tiled, log-uniform noise, the extreme tiers."""
    rng = np.random.default_rng([4301, R, W])
    out = {"constant": np.full((R, W, 3), 0.18, f32), "edges": tiled(edge_colours(), R, W), "noise": log_uniform(rng, R, W)}
    for tier in xp.TIERS:
        out[tier] = extreme_image(R, W, tier)
    return out


def in_one_bin(b, n):
    H = np.zeros(WORDS, u32)
    H[b] = n
    return H


def expose_histograms():
    """[(name, H, arguments of expose)]: the histograms of the exposure tests."""
    cases = []
    for b in (0, 120, 255):
        cases.append((f"all in bin {b}", in_one_bin(b, 1000), {}))
    two = np.zeros(WORDS, u32)
    two[100] = two[140] = 1 << 15                    # N = 2^16: t = q16, and the boundary rank is 32768
    for q in (32767, 32768, 32769):
        cases.append((f"two bins, q16 {q}", two, dict(key_q16=q, white_q16=65535)))
        cases.append((f"two bins, white q16 {q}", two, dict(key_q16=0, white_q16=q)))
    cases.append(("2^31 - 1 in one bin", in_one_bin(77, 0x7FFFFFFF), dict(key_q16=65535, white_q16=65535)))
    big = in_one_bin(60, 0x7FFFFFFF - 5)
    big[200] = 5
    big[EXCLUDED] = 11
    cases.append(("2^31 - 1 in two bins", big, dict(key_q16=65535, white_q16=65535)))
    cases.append(("the least clamp", in_one_bin(255, 10), {}))                 # key / 2^16 is below 2^-8
    cases.append(("the greatest clamp", in_one_bin(0, 10), {}))                # key / 2^-16 is above 2^8
    cases.append(("a narrow range", in_one_bin(120, 10), dict(scale_min=3.0, scale_max=3.0)))
    rng = np.random.default_rng(4302)
    for k in range(200):
        H = np.zeros(WORDS, u32)
        n = int(rng.integers(1, 257))
        at = rng.choice(WORDS, n, replace=False)
        H[at] = rng.integers(0, 1 << int(rng.integers(1, 22)), n)
        kq = int(rng.integers(0, 65536))
        cases.append((f"random {k}", H, dict(key_q16=kq, white_q16=int(rng.integers(kq, 65536)), key=float(np.exp2(rng.uniform(-4, 4))),
                                             rate=float(rng.choice([1.0, 0.5, 0.25, 0.01])))))
    return cases


def adaptation_histograms():
    """Five frames' histograms for a sequence at rate 0.25: the key bin moves, one frame is empty."""
    rng = np.random.default_rng(4303)
    out = []
    for k, centre in enumerate((120, 90, 90, None, 150)):
        H = np.zeros(WORDS, u32)
        if centre is not None:
            H[centre - 8:centre + 9] = rng.integers(1, 500, 17)
        H[EXCLUDED] = k
        out.append(H)
    return out


def apply_colours(n=4096):
    """n log-uniform colours in 2^-20 ... 2^20 with a random sign on a tenth of the values, then the edge values as greys."""
    rng = np.random.default_rng(4304)
    return np.concatenate([log_uniform(rng, n, 1, negative=0.1).reshape(n, 3), edge_colours()]).astype(f32)


APPLY_SCALES = (2.0 ** -8, 0.37, 1.0, 2.0 ** 8)
APPLY_WHITES = (1.0, 4.0, np.inf)


def sweep():
    """Every finite float from +0 up whose low 10 mantissa bits are zero, ascending: 2 088 960 values."""
    return from_bits(np.arange(0, 0x7F800000, 1 << 10, dtype=np.uint64).astype(u32))
