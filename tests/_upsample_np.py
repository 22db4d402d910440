"""The film upsampler restated with numpy from the text of ray_tracer_s8_amd/upsample_csrc/rt_upsample.h: np.float32
operations one by one, in the order the header writes them, over whole planes at once.  Written from the header, not from
rt_upsample_math.h.  Also the seeded synthetic frame pairs the CPU and GPU tests share (pair(), SIZES, SCALES)."""
import itertools

import numpy as np

f32 = np.float32
NONE = 0xFFFFFFFF                                 # RT_HIT_NONE
PLANES = ("albedo", "normal", "depth", "hits", "index")
TESTS = ("index", "hits", "depth", "normal")      # the admission tests, in the header's order


def plane_subsets():
    """Every plane set a call may have: each plane optional, depth only with hits.  24 of them, () first."""
    out = []
    for n in range(len(PLANES) + 1):
        for sub in itertools.combinations(PLANES, n):
            if "depth" in sub and "hits" not in sub:
                continue
            out.append(sub)
    return out


def frame_dens(W, H):
    """u_den and v_den of a W x H frame as fill_camera forms them."""
    aspect = f32(W) / f32(H)
    return f32(aspect * f32(H)) - f32(1), f32(H) - f32(1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def as_u8(v):
    """The tile's `as u8` from f32: truncate, saturate, NaN -> 0."""
    v = np.asarray(v, f32)
    out = np.zeros(v.shape, np.uint8)
    ok = v == v
    out[ok & (v >= 255)] = 255
    mid = ok & (v > 0) & (v < 255)
    out[mid] = v[mid].astype(np.int32).astype(np.uint8)
    return out


def upsample(L, lo, hi, geom, k_depth=f32(0.1), k_normal=f32(0.9), eps=f32(0.01), kl=1, kh=1):
    """rt_upsample.h steps 1 to 7.  L: (Rl, Wl, 3) float32.  lo, hi: {plane: array} of the feature sums of the two sides, the same
    names on both (albedo, normal (R, W, 3) float32; depth (R, W) float32; hits, index (R, W) uint32).  geom: dict(Hl, y0l, Hh, y0h, Rh,
    Wh).  Returns dict(linear, f32, rgb, cls) and, under "counts", how often each test rejected a tap, how many taps were admitted and
    how many pixels fell in each class."""
    L = np.ascontiguousarray(L, f32)
    Rl, Wl = L.shape[:2]
    Hl, y0l, Hh, y0h, Rh, Wh = (int(geom[k]) for k in ("Hl", "y0l", "Hh", "y0h", "Rh", "Wh"))
    assert set(lo) == set(hi) and ("depth" not in lo or "hits" in lo)
    k_depth, k_normal, eps = f32(k_depth), f32(k_normal), f32(eps)
    kn2 = f32(k_normal * k_normal)
    u_den_l, v_den_l = frame_dens(Wl, Hl)
    u_den_h, v_den_h = frame_dens(Wh, Hh)
    counts = {t: 0 for t in TESTS}
    with np.errstate(all="ignore"):
        # 1
        hit_h = hi["hits"] > 0 if "hits" in hi else np.ones((Rh, Wh), bool)
        if "depth" in hi:
            zh = np.where(hit_h, hi["depth"].astype(f32) / np.maximum(hi["hits"], 1).astype(f32), f32(0)).astype(f32)
        # 2
        x = np.arange(Wh, dtype=np.uint32)[None, :]
        r = np.arange(Rh, dtype=np.uint32)[:, None]
        u = (x.astype(f32) + f32(0.5)) / u_den_h
        fx = u * u_den_l - f32(0.5)
        v = ((np.uint32(Hh) - (np.uint32(y0h) + r) - np.uint32(1)).astype(f32) + f32(0.5)) / v_den_h
        cv = v * v_den_l - f32(0.5)
        fy = (f32(Hl - 1) - cv) - f32(y0l)
        flx, fly = np.floor(fx), np.floor(fy)
        x0, y0t = flx.astype(np.int64), fly.astype(np.int64)
        ax, ay = (fx - flx).astype(f32), (fy - fly).astype(f32)
        ax, ay = np.broadcast_to(ax, (Rh, Wh)), np.broadcast_to(ay, (Rh, Wh))
        x0, y0t = np.broadcast_to(x0, (Rh, Wh)), np.broadcast_to(y0t, (Rh, Wh))
        # 3, 4
        taps = []
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = np.clip(x0 + dx, 0, Wl - 1), np.clip(y0t + dy, 0, Rl - 1)
                b = ((ax if dx else f32(1) - ax) * (ay if dy else f32(1) - ay)).astype(f32)
                ok = np.ones((Rh, Wh), bool)
                if "index" in lo:
                    t = lo["index"][qy, qx] == hi["index"]
                    counts["index"] += int((ok & ~t).sum())
                    ok &= t
                if "hits" in lo:
                    hl = lo["hits"][qy, qx]
                    t = (hl == 0) == (hi["hits"] == 0)
                    counts["hits"] += int((ok & ~t).sum())
                    ok &= t
                if "depth" in lo:
                    both = hit_h & (hl > 0)
                    zl = np.where(hl > 0, lo["depth"][qy, qx].astype(f32) / np.maximum(hl, 1).astype(f32), f32(0)).astype(f32)
                    t = ~both | (np.abs(zh - zl) <= k_depth * zh)
                    counts["depth"] += int((ok & ~t).sum())
                    ok &= t
                if "normal" in lo:
                    both = hit_h & (lo["hits"][qy, qx] > 0) if "hits" in lo else np.ones((Rh, Wh), bool)
                    nh, nl = hi["normal"].astype(f32), lo["normal"][qy, qx].astype(f32)
                    c = dot(nh, nl)
                    t = ~both | ((c > 0) & (c * c >= kn2 * (dot(nh, nh) * dot(nl, nl))))
                    counts["normal"] += int((ok & ~t).sum())
                    ok &= t
                Vq = L[qy, qx]
                if "albedo" in lo:
                    Vq = Vq / (lo["albedo"][qy, qx].astype(f32) / f32(kl) + eps)
                taps.append((b, ok, Vq.astype(f32)))
        # 5
        def sums(all_taps):
            sw, sv = np.zeros((Rh, Wh), f32), np.zeros((Rh, Wh, 3), f32)
            for b, ok, Vq in taps:
                take = np.ones_like(ok) if all_taps else ok
                sw = np.where(take, sw + b, sw)
                sv = np.where(take[..., None], sv + b[..., None] * Vq, sv)
            return sw, sv
        sw, sv = sums(False)
        cls = ~(sw > 0)
        sw1, sv1 = sums(True)
        sw, sv = np.where(cls, sw1, sw), np.where(cls[..., None], sv1, sv)
        V = (sv / sw[..., None]).astype(f32)
        # 6, 7
        out = V
        if "albedo" in hi:
            out = V * (hi["albedo"].astype(f32) / f32(kh) + eps)
        out = out.astype(f32)
        f = np.sqrt(out)
        rgb = as_u8(f * f32(255.999))
    counts["admitted"] = int(sum(int(ok.sum()) for _, ok, _ in taps))
    counts["class0"], counts["class1"] = int((~cls).sum()), int(cls.sum())
    return dict(linear=out, f32=f.astype(f32), rgb=rgb, cls=cls.astype(np.uint8), counts=counts)


# ---- the synthetic frame pairs -------------------------------------------------------------------------------------------------------

REGIONS = 6                                       # region 0 is the sky


def _side(rng, sites, consts, W, H, y0, R, k, thin, holes, outliers):
    """The feature sums of rows [y0, y0 + R) of a W x H frame of the pair's world: piecewise regions (the nearest of `sites` to the
    pixel's centre in the unit square), each with its own depth, normal and albedo."""
    xs = (np.arange(W) + 0.5) / W
    ys = (np.arange(y0, y0 + R) + 0.5) / H
    d2 = (xs[None, :, None] - sites[None, None, :, 0]) ** 2 + (ys[:, None, None] - sites[None, None, :, 1]) ** 2
    reg = np.argmin(d2, axis=2)
    depth_r, normal_r, albedo_r = consts
    kf = f32(k)
    index = np.where(reg == 0, NONE, reg + 10).astype(np.uint32)
    hits = np.where(reg == 0, 0, k).astype(np.uint32)
    depth = (depth_r[reg] * kf * (f32(1) + f32(0.01) * rng.standard_normal((R, W)).astype(f32))).astype(f32)
    normal = (normal_r[reg] * kf + f32(0.02) * rng.standard_normal((R, W, 3)).astype(f32)).astype(f32)
    albedo = (albedo_r[reg] * kf).astype(f32)                     # exactly constant over a region
    pick = rng.random((R, W))
    if thin:                                                      # geometry below the other side's pixel: its own index, distance and facing
        t = (pick < thin) & (reg != 0)
        index[t] = (reg[t] + 1000).astype(np.uint32)
        depth[t] = depth[t] * f32(3)
        normal[t] = -normal[t]
    if holes:                                                     # pixels whose samples all missed, inside a region
        h = (pick > 1 - holes) & (reg != 0)
        hits[h] = 0
        depth[h] = 0
        normal[h] = 0
    if outliers:                                                  # the same primitive at another distance, or turned away
        o = rng.random((R, W))
        far = (o < outliers) & (hits > 0)
        depth[far] = depth[far] * f32(1.6)
        turned = (o > 1 - outliers) & (hits > 0)
        normal[turned] = -normal[turned]
    depth[hits == 0] = 0
    normal[hits == 0] = 0
    return dict(albedo=albedo, normal=normal, depth=depth, hits=hits, index=index), reg


def pair(seed, Wl, Rl, s, strips_above=0, strips_below=0, kl=2, kh=1):
    """A seeded pair of frames of one synthetic world: a low film of Wl x Rl, rows [y0l, y0l + Rl) of a frame of
    Hl = (strips_above + 1 + strips_below) Rl rows, and the output of s Wl x s Rl.  Returns (L, lo, hi, geom, kl, kh, reg_lo): L a
    noisy colour, the planes of both sides, the geometry upsample() takes, the sample counts and the low side's region map."""
    rng = np.random.default_rng(seed)
    n = strips_above + 1 + strips_below
    Hl, y0l = n * Rl, strips_above * Rl
    Wh, Rh, Hh, y0h = s * Wl, s * Rl, s * n * Rl, s * strips_above * Rl
    sites = rng.random((REGIONS, 2))
    sites[:, 1] = (y0l + sites[:, 1] * Rl) / Hl                     # inside the film's band of the frame
    consts = (rng.uniform(1, 9, REGIONS).astype(f32), _unit(rng.standard_normal((REGIONS, 3))).astype(f32),
              rng.uniform(0.1, 0.9, (REGIONS, 3)).astype(f32))
    lo, reg_lo = _side(rng, sites, consts, Wl, Hl, y0l, Rl, kl, 0.0, 0.08, 0.06)
    hi, _ = _side(rng, sites, consts, Wh, Hh, y0h, Rh, kh, 0.10, 0.14, 0.0)
    L = rng.uniform(0.0, 2.0, (Rl, Wl, 3)).astype(f32)
    L[rng.random((Rl, Wl)) < 0.05] = 0                              # black pixels
    geom = dict(Hl=Hl, y0l=y0l, Hh=Hh, y0h=y0h, Rh=Rh, Wh=Wh)
    return L, lo, hi, geom, kl, kh, reg_lo


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def take(planes, names):
    return {n: planes[n] for n in names}


# (Wl, Rl, strips above, strips below) of the low film: one pixel; partial workgroups in both directions at every scale; a second
# workgroup column at every scale
SIZES = [(1, 1, 0, 0), (5, 3, 1, 1), (33, 7, 2, 0), (64, 9, 1, 1)]
SCALES = (2, 3, 4)
K_DEPTH, K_NORMAL, EPS = f32(0.1), f32(0.9), f32(0.01)


def seed_of(Wl, Rl, s):
    return 7000 + 100 * Wl + 10 * Rl + s
