"""Extreme plane values for the film stage: the value classes, the two placements and the comparison rule that the
CPU tests (tests/test_extreme_planes_host.py) and the GPU tests (tests/test_gpu_film_extremes.py) of the denoiser, the guided resolve,
the history with its clip and the upsampler share, as tests/_operand_cases.py is shared on the traversal side.  Plain numpy, no GPU.

Three tiers of float values:
  small      +0, -0, subnormals from the least to the largest, the least normal, and values whose squares or pairwise products
             underflow (1e-19 ... 1e-30); salted: a seeded share of a plane's entries is replaced, half of them by the listed values and
             half by seeded subnormals and tiny normals of their own, so that two salted entries are rarely equal; and the right half of
             the columns is a block of subnormals on every float plane, whose interior stays subnormal through three blurring
             iterations (salted()).  A colour plane takes -0 but no other negative value here: the outputs take its square root, and the
             tier is held to make no NaN;
  huge       finite values either side of sqrt(FLT_MAX), 1e25, 3e38, +-FLT_MAX; sparse;
  nonfinite  +-inf, quiet NaNs of both signs, one signalling NaN, negative values (on planes whose sums are expected non-negative) and,
             on an albedo plane, exactly -eps k on one channel, which makes d = A / k + eps = 0; sparse.
Sparse placement puts one special value at each pixel of a lattice whose pixels are at least PITCH = 14 apart, one plane at a time
(`which` names it) or on every plane at once with a lattice origin of its own for every plane, so that no two planes are special at
one pixel.  Where NaNs spread (the two a-trous filters) only the first lattice pixel of a plane takes a value that makes one
(`spreading`), its case is repeated for each such value in turn (_filter_cases()), and a plane that only stops edges has its case
carry a colour special too (cases()).  The integer planes carry their specials in every tier, on a lattice of pitch INT_PITCH = 5: hits of 0 under a depth and a normal that are not zero, hits of 1, 2^24, 2^24 + 1 and 0xFFFFFFFF, and an
index of RT_HIT_NONE under hits > 0.

Only plane values change: sizes, strides, cameras, poses, sample counts and the k constants are the existing synthetic cases'."""
import numpy as np

f32 = np.float32
NONE = 0xFFFFFFFF                                 # RT_HIT_NONE
PITCH = 14
TIERS = ("small", "huge", "nonfinite")
FLOAT_ROLES = ("colour", "moments", "albedo", "normal", "depth")
TINY = float(np.finfo(f32).tiny)                  # 2^-126, the least normal

QNAN, NEG_QNAN, SNAN = 0x7FC00000, 0xFFC00000, 0x7F800001


def _from_bits(*b):
    return np.array(b, np.uint32).view(f32)


SMALL = np.concatenate([
    _from_bits(0x00000000, 0x80000000,                         # +0, -0
               0x00000001, 0x80000001,                         # the least subnormal, both signs
               0x00000400, 0x00012345, 0x80400000,             # mid subnormals
               0x007FFFFF, 0x807FFFFF,                         # the largest subnormal, both signs
               0x00800000),                                    # the least normal
    np.array([1e-19, -1e-19, 3e-20, 1e-22, 1e-25, -1e-25, 3e-30, 1e-30], f32)])           # squares and products underflow
# on a colour plane the negative ones are left out but -0: the outputs take a square root of the colour, and the small tier is held to
# produce no NaN.  The other planes carry them.
SMALL_COLOUR = SMALL[(SMALL >= 0)]
HUGE = np.array([1.8e19, 1.9e19, 1e25, 3e38, np.finfo(f32).max, -np.finfo(f32).max], f32)       # sqrt(FLT_MAX) = 1.8447e19
NEGATIVE = np.array([-1.5, -0.25], f32)
# in lattice order: the values that make NaNs stand between values that do not, so that a lattice of a few pixels holds both kinds
NONFINITE = np.concatenate([_from_bits(0x7F800000), NEGATIVE[:1], _from_bits(QNAN, 0xFF800000), NEGATIVE[1:],
                            _from_bits(NEG_QNAN, SNAN)])

# the lattice origin (row, column) of every role: rows below 9 (the smallest film has 9 rows), no two at one pixel modulo PITCH
ORIGINS = dict(colour=(2, 3), moments=(4, 6), albedo=(6, 9), normal=(8, 12), depth=(1, 1), hits=(3, 10), index=(7, 5))
HITS_SPECIALS = (0, 1, 1 << 24, (1 << 24) + 1, 0xFFFFFFFF)
INT_PITCH = 5                                     # the integer planes' lattice: seven pixels and all of HITS_SPECIALS in a 33 x 7 film too


def values(tier, role, albedo_zero=None):
    """The special values of a tier on a plane of `role`.  albedo_zero: -eps k of the call, for an albedo plane."""
    if tier == "small":
        return SMALL_COLOUR if role == "colour" else SMALL
    if tier == "huge":
        return HUGE
    assert tier == "nonfinite", tier
    if role == "albedo" and albedo_zero is not None:
        return np.concatenate([NONFINITE[:1], np.array([albedo_zero], f32), NONFINITE[1:]])
    return NONFINITE


def makers(vals):
    """Of a non-finite plane's values, those that make a NaN: the infinities, the NaNs, the albedo that makes d = 0."""
    return vals[~np.isin(vals, NEGATIVE)]


def lattice(R, W, origin, pitch=PITCH):
    """The pixels (row, column) of the lattice with the given origin inside an R x W plane, row by row."""
    return [(y, x) for y in range(origin[0] % pitch, R, pitch) for x in range(origin[1] % pitch, W, pitch)]


def salted(plane, vals, share, rng, block=False):
    """A copy of a float plane with a seeded `share` of its entries replaced by `vals`; of the small tier's, half by seeded
    subnormals and tiny normals of their own instead.  block: the right half of the plane's columns (block_columns) is then filled
    with seeded subnormals of magnitude 2^-128 and up (signed where the tier's values are), every entry of every pixel: the salt's
    1e-19 ... 1e-30 are normal numbers and dominate any average they enter, so a salted pixel among ordinary or merely small ones does
    not come out of a blurring iteration subnormal; a pixel whose whole footprint lies in the block does, through three iterations
    too (their reach is 14 columns, the block is half the plane wide), and its sums, products and quotients are all subnormal."""
    out = np.array(plane, f32, copy=True)
    flat = out.reshape(-1)
    if out.ndim == 3:
        # half of the share as single entries, half as whole pixels: a pixel that is small in every channel stays small through a
        # filter whose weights stop at a colour edge, one that is small in one channel does not
        C = out.shape[2]
        whole = np.repeat(rng.random(flat.size // C) < share / 2, C)
        pick = np.flatnonzero(whole | (rng.random(flat.size) < share / 2))
    else:
        pick = np.flatnonzero(rng.random(flat.size) < share)
    new =vals[rng.integers(0, len(vals), pick.size)].copy()
    if vals is SMALL or vals is SMALL_COLOUR:
        own = rng.random(pick.size) < 0.5
        sign = rng.integers(0, 2, pick.size).astype(np.uint32) * np.uint32(vals is SMALL)
        bits = rng.integers(1, 0x00800000, pick.size).astype(np.uint32) | (sign << np.uint32(31))
        tiny = (10.0 ** rng.uniform(-30, -19, pick.size) * (1.0 - 2.0 * sign)).astype(f32)
        seeded = np.where(rng.random(pick.size) < 0.5, bits.view(f32), tiny)
        new = np.where(own, seeded, new)
    flat.view(np.uint32)[pick] = new.astype(f32).view(np.uint32)              # (bits: a NaN's payload is kept)
    if block:
        cols = block_columns(out.shape[1])
        shape = out[:, cols].shape
        sign = rng.integers(0, 2, shape).astype(np.uint32) * np.uint32(vals is SMALL)
        out.view(np.uint32)[:, cols] = rng.integers(0x00200000, 0x00800000, shape).astype(np.uint32) | (sign << np.uint32(31))
    return out


def block_columns(W):
    """The columns of the small tier's block of subnormal pixels in a plane W columns wide: the right half."""
    return slice(W - W // 2, W)


def sparse(plane, vals, origin, shift=0, pitch=PITCH, first=0, spreading=None):
    """A copy of a float plane (R, W) or (R, W, C) with vals[first + j] at the j-th lattice pixel, on channel (first + j) % C.  shift moves
    the lattice's origin by that many columns (a frame of a sequence gets its own).  spreading: how many lattice pixels, the first
    ones, take `vals`; the others take NEGATIVE values, which make no NaN that spreads.  (Through three a-trous iterations one
    infinity or NaN reaches the 29 x 29 pixels around it, 41 % of a 70 x 22 image: a second one further along the lattice would put
    more than half of the image's pixels at NaN, and the test that compares them would see little else.)"""
    out = np.array(plane, f32, copy=True)
    R, W = out.shape[:2]
    bits = out.view(np.uint32)
    for j, (y, x) in enumerate(lattice(R, W, (origin[0], origin[1] + shift), pitch)):
        if spreading is None:
            v = vals[(first + j) % len(vals)]
        elif j < spreading:
            v = makers(vals)[(first + j) % len(makers(vals))]
        else:
            v = NEGATIVE[j % len(NEGATIVE)]
        v = v.view(np.uint32)
        if out.ndim == 3:
            bits[y, x, (first + j) % out.shape[2]] = v
        else:
            bits[y, x] = v
    return out


def integer_specials(hits, index, shift=0):
    """Copies of the integer planes (either may be None) with their specials on their lattices: HITS_SPECIALS in turn on hits (the
    planes beside it keep their values, so a 0 stands under a depth and a normal that are not zero) and RT_HIT_NONE on index, which
    lies under hits > 0 wherever the hits plane has them.  Their lattice has pitch INT_PITCH: nothing spreads from an integer."""
    if hits is not None:
        hits = np.array(hits, np.uint32, copy=True)
        for j, (y, x) in enumerate(lattice(*hits.shape, (ORIGINS["hits"][0], ORIGINS["hits"][1] + shift), INT_PITCH)):
            hits[y, x] = HITS_SPECIALS[j % len(HITS_SPECIALS)]
    if index is not None:
        index = np.array(index, np.uint32, copy=True)
        for y, x in lattice(*index.shape, (ORIGINS["index"][0], ORIGINS["index"][1] + shift), INT_PITCH):
            index[y, x] = NONE
    return hits, index


def cases(tier, roles):
    """The cases of a tier for a library whose planes have the float `roles`: (name, the roles that carry specials).  The salted
    tiers have one case, every plane salted; the sparse ones a case a role and one with every role special, at different pixels."""
    roles = tuple(r for r in FLOAT_ROLES if r in roles)
    if tier == "small":
        return [("every plane", roles)]
    # (a normal or a depth only stops edges, and the entry variance clamps what a non-finite first moment makes to 0: no value of
    # theirs need reach an output, so their cases carry a colour special too, whose NaNs then meet the plane's specials in the taps)
    carries = lambda r: (r,) if r in ("colour", "albedo") else (r, "colour")
    return [(r, carries(r)) for r in roles] + [("every plane", roles)]


def apply(planes, roles, tier, which, seed, albedo_zero=None, share=None, shift=0, placement=None, spreading=None, maker=None,
          block=()):
    """The planes of a case.  planes: {name: array or None}; roles: {name: role}, a float role or "hits" or "index"; which: the float
    roles that carry specials.  Returns a new dict of new arrays (the caller's are not written).  The float planes of the roles in
    `which` are salted (tier "small", or placement "salted") or take the tier's values on their lattice; the integer planes take
    their specials in every case.  spreading: sparse()'s, for the colour, moments and albedo planes of the non-finite tier.
    maker: which of the plane's NaN-making values its first lattice pixel takes (None: seed's turn); block: the roles whose planes
    get salted()'s block of subnormal pixels.  albedo_zero: {name: -eps k} of the albedo planes.  Every salted plane draws from a
    generator of its own, seeded by `seed` and the
    plane's position in `planes`."""
    placement = placement or ("salted" if tier == "small" else "sparse")
    out = {}
    for k, (name, a) in enumerate(planes.items()):
        role = roles[name]
        if a is None or role in ("hits", "index") or role not in which:
            out[name] = None if a is None else np.array(a, copy=True)
            continue
        vals = values(tier, role, (albedo_zero or {}).get(name))
        if placement == "salted":
            out[name] = salted(a, vals, 0.25 if share is None else share, np.random.default_rng([seed, k]), role in block)
        else:
            limited = tier == "nonfinite" and role in ("colour", "moments", "albedo")
            out[name] = sparse(a, vals, ORIGINS[role], shift, first=seed + k if maker is None or not limited else maker,
                               spreading=spreading if limited else None)
    names = {r: [n for n in planes if roles[n] == r and planes[n] is not None] for r in ("hits", "index")}
    for n in names["hits"]:
        out[n] = integer_specials(planes[n], None, shift)[0]
    for n in names["index"]:
        out[n] = integer_specials(None, planes[n], shift)[1]
    return out


# ---- the comparison rule ---------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def differing(got, want):
    """Where two arrays differ under the rule: a float is NaN in one exactly where it is NaN in the other (payload and sign of a NaN
    are not compared), every other float is bit-equal (signed zeros and infinities included), integers are equal."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype != np.float32:
        return got != want
    gn, wn = np.isnan(got), np.isnan(want)
    return (gn != wn) | (~gn & ~wn & (bits(got) != bits(want)))


def same(got, want, what, footprint=None):
    """Assert the rule; on failure name the first position, both values with their bits and, from footprint(position), the inputs
    the pixel read."""
    bad = np.argwhere(differing(got, want))
    if len(bad):
        p = tuple(bad[0])
        show = lambda v: (v, hex(int(np.asarray(v).view(np.uint32)))) if np.asarray(v).dtype == np.float32 else int(v)
        raise AssertionError((what, len(bad), bad[:4].tolist(), "got", show(got[p]), "want", show(want[p]),
                              footprint(p) if footprint else None))


def identical(got, want, what):
    """Raw bits, NaN payloads included: what the inputs of a call are held to after it."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (what, "an input changed")


# ---- what the CPU test measures of a case's outputs ------------------------------------------------------------------------------------
def pixel_nan(outputs):
    """(R, W) bool: the pixels with a NaN in any of the float outputs [(R, W) or (R, W, C) arrays]."""
    m = None
    for a in outputs:
        if a.dtype != np.float32:
            continue
        n = np.isnan(a) if a.ndim == 2 else np.isnan(a).any(-1)
        m = n if m is None else m | n
    return m


def finite_beside_nan(nan):
    """Whether some pixel without a NaN has a 4-neighbour with one."""
    near = np.zeros_like(nan)
    near[1:] |= nan[:-1]
    near[:-1] |= nan[1:]
    near[:, 1:] |= nan[:, :-1]
    near[:, :-1] |= nan[:, 1:]
    return bool((near & ~nan).any())


class Shares:
    """Counts over the float outputs of the cases of one library and tier."""

    def __init__(self):
        self.values = self.subnormal = self.inf = self.nan = self.neg_zero = 0
        self.pixels = self.nan_pixels = 0

    def add(self, outputs):
        for a in outputs:
            if a.dtype != np.float32:
                continue
            mag = np.abs(a)
            self.values += a.size
            self.subnormal += int(((mag > 0) & (mag < TINY)).sum())
            self.inf += int(np.isinf(a).sum())
            self.nan += int(np.isnan(a).sum())
            self.neg_zero += int(((a == 0) & np.signbit(a)).sum())
        n = pixel_nan(outputs)
        self.pixels += n.size
        self.nan_pixels += int(n.sum())

    def line(self, library, tier):
        pc = lambda a, b: f"{100.0 * a / max(b, 1):.1f} %"
        return (f"{library:9s} {tier:9s}: NaN pixels {pc(self.nan_pixels, self.pixels)}, of the values: NaN {pc(self.nan, self.values)}, "
                f"subnormal {pc(self.subnormal, self.values)}, inf {pc(self.inf, self.values)} ({self.inf} values), -0 {self.neg_zero} values")


# ---- the cases of the four libraries ---------------------------------------------------------------------------------------------------
# Each generator starts from the library's existing seeded synthetic planes (their generators are imported where they are used, so
# that this module stays importable without them) and yields what both the CPU and the GPU test run: the same bytes on both.
SPARSE_ITERATIONS = (0, 1, 3)                       # at most 3 for the sparse tiers: a NaN reaches 2 (1 + 2 + 4) pixels in 3 iterations
FILTER_SIZES = dict(small=(9, 70), huge=(22, 70), nonfinite=(22, 70))      # (R, W): 64 x 4 tiles, partial in both directions
E, K = 8, 4                                         # the colour and feature sample counts of the synthetic images


def _distinct(cs):
    seen, out = set(), []
    for name, which in cs:
        if which and which not in seen:
            seen.add(which)
            out.append((name, which))
    return out


def _filter_cases(tier, roles, albedo_zero=None):
    """cases() for the two filters, as (name, which, maker): in the non-finite tier the case of a plane whose values reach the
    outputs is repeated for each of its NaN-making values in turn, since only one lattice pixel of it takes one (sparse())."""
    for name, which in _distinct(cases(tier, roles)):
        if tier == "nonfinite" and name in ("colour", "moments", "albedo"):
            for m in range(len(makers(values(tier, name, albedo_zero)))):
                yield f"{name}, maker {m}", which, m
        else:
            yield name, which, None


DENOISE_ROLES = dict(C="colour", A="albedo", N="normal", D="depth", hits="hits")
DENOISE_SETS = ((), ("A",), ("A", "N", "D", "hits"))                      # none, albedo only, all planes
DENOISE_EPS = f32(2.0 ** -8)                                              # rt_denoise_request_defaults' albedo_eps


def denoise_consts(tier):
    """(k_color, k_normal, k_depth) of a tier's runs: test_denoise_host's first constants, under which the filter blurs, and for
    the small tier its edge-stopping ones too, under which a small pixel averages with small pixels only and stays small."""
    return [(1.0, 4.0, 16.0)] + ([(1e6, 1e6, 1e6)] if tier == "small" else [])


def denoise_cases(tier):
    """(name, plane set, planes): planes is dict(C, A, N, D, hits) with the planes outside the set left as the generator made them
    (the call does not pass them)."""
    from test_denoise_host import synthetic
    R, W = FILTER_SIZES[tier]
    base = synthetic(np.random.default_rng(4280 + R), R, W, E, K)
    for names in DENOISE_SETS:
        roles = ("colour",) + tuple(DENOISE_ROLES[n] for n in names if n != "hits")
        zero = f32(-(DENOISE_EPS * f32(K)))
        for j, (name, which, maker) in enumerate(_filter_cases(tier, roles, zero)):
            yield name, names, apply(base, DENOISE_ROLES, tier, which, 100 * len(names) + j, dict(A=zero), spreading=1, maker=maker,
                                     block=FLOAT_ROLES)


FILM_ROLES = dict(C="colour", M="moments", N="normal", D="depth", hits="hits")
FILM_SUBSETS = [(n, d) for n in (False, True) for d in ("", "hits", "depth")]          # test_film_guided_host.SUBSETS


def film_consts(tier):
    """(sigma_l, var_eps, k_normal, k_depth) of a tier's runs: resolve_guided's defaults, and for the small tier
    test_film_guided_host's sigma_l = 0 set too (a_p = 1 / var_eps = 1000 everywhere: a hard luminance edge)."""
    return [(16.0, 2.0 ** -8, 1.0, 4.0)] + ([(0.0, 1e-3, 0.0, 0.0)] if tier == "small" else [])


def film_cases(tier):
    """(name, (normal, depth), planes): planes is dict(C, M, N, D, hits)."""
    import _film_np as fnp
    R, W = FILTER_SIZES[tier]
    base = fnp.synthetic(np.random.default_rng(4281 + R), R, W, E, K)
    for s, (normal, depth) in enumerate(FILM_SUBSETS):
        roles = ("colour", "moments") + (("normal",) if normal else ()) + (("depth",) if depth == "depth" else ())
        for j, (name, which, maker) in enumerate(_filter_cases(tier, roles)):
            yield name, (normal, depth), apply(base, FILM_ROLES, tier, which, 100 * s + j, spreading=1, maker=maker, block=FLOAT_ROLES)


HISTORY_ROLES = dict(C="colour", M="moments", depth="depth", hits="hits", index="index", normal="normal")
HISTORY_FILM = (70, 9, 3)                                                 # W, H, divisions: the whole frame is the film
HISTORY_CONSTS = ((0.4, 3.0, 0.05, 0.9), (0.05, 8.0, 0.1, None))          # alpha, n_max, k_depth, k_normal: test_history_host's
HISTORY_PATHS = {"still": [None, None, None],
                 "half a pixel": [None, ((0.02, 0.013, 0.0), (0.02, 0.013, -1.0), (0.0, 1.0, 0.0)),
                                  ((0.04, 0.03, 0.0), (0.04, 0.03, -1.0), (0.0, 1.0, 0.0))]}      # test_history_host.PATHS', three frames
HISTORY_SAMPLES = 4                                                       # synthetic_frame's e


def history_cases(tier, rq):
    """(name, path name, consts, frames): frames is [(pose, frame)] of three frames of 70 x 9, every frame with the case's specials,
    the lattices of frame i moved by 5 i columns so that a special of one frame is read back beside, not under, the next one's.
    The small tier's block of subnormal pixels leaves the depth plane out: a pixel of subnormal depth reprojects nowhere and takes no
    history, and the block is there for the blend of subnormal sums.
    rq: the request of the film's first strip (the caller's: ray_tracer_s8_amd._abi makes it)."""
    import _history_np as hnp
    W, H, _ = HISTORY_FILM
    for p, (path, poses) in enumerate(HISTORY_PATHS.items()):
        for c, consts in enumerate(HISTORY_CONSTS):
            rng = np.random.default_rng(4282 + 10 * p + c)
            base = [hnp.synthetic_frame(rng, rq, pose, H, consts[2], consts[3]) for pose in poses]
            roles = ("colour", "moments", "depth") + (("normal",) if consts[3] is not None else ())
            for j, (name, which) in enumerate(_distinct(cases(tier, roles))):
                frames = [(pose, apply(fr, HISTORY_ROLES, tier, which, 100 * p + 10 * c + j + i, shift=5 * i,
                                       block=("colour", "moments", "normal")))
                          for i, (pose, fr) in enumerate(zip(poses, base))]
                yield name, path, consts, frames


UPSAMPLE_LOW = (33, 7, 2, 0)                                              # Wl, Rl, strips above, strips below: _upsample_np.SIZES[2]
UPSAMPLE_SCALES = (2, 3)
UPSAMPLE_SETS = (("albedo", "normal", "depth", "hits", "index"), (), ("depth", "hits"))
# salted in every tier: nothing spreads.  (An output pixel is the mean of four taps, subnormal only where all four are: the small
# tier's block sees to that.  Its normals stay ordinary, so that taps are admitted inside it.)
UPSAMPLE_SHARE = dict(small=0.25, huge=0.02, nonfinite=0.02)


def upsample_cases(tier, s):
    """(name, L, lo, hi, geom, kl, kh): the pair of scale s with L and every plane of both sides salted, then a case a role (the
    normal's and the depth's with L salted too: they only admit taps, and what they admit has to show)."""
    import _upsample_np as unp
    Wl, Rl, above, below = UPSAMPLE_LOW
    L, lo, hi, geom, kl, kh, _ = unp.pair(unp.seed_of(Wl, Rl, s), Wl, Rl, s, above, below)
    flat = dict(L=L, **{f"lo.{n}": a for n, a in lo.items()}, **{f"hi.{n}": a for n, a in hi.items()})
    roles = {n: ("colour" if n == "L" else n.split(".")[1]) for n in flat}
    zero = {"lo.albedo": f32(-(unp.EPS * f32(kl))), "hi.albedo": f32(-(unp.EPS * f32(kh)))}
    every = ("colour", "albedo", "normal", "depth")
    per_role = [("colour", ("colour",)), ("albedo", ("albedo",)), ("normal", ("normal", "colour")), ("depth", ("depth", "colour"))]
    for j, (name, which) in enumerate([("every plane", every)] + (per_role if tier != "small" else [])):
        share = UPSAMPLE_SHARE[tier] * (1 if tier == "small" or name == "every plane" else 4)
        got = apply(flat, roles, tier, which, 1000 * s + j, zero, share=share, placement="salted",
                    block=("colour", "albedo", "depth") if tier == "small" else ())
        yield (name, got["L"], {n: got[f"lo.{n}"] for n in lo}, {n: got[f"hi.{n}"] for n in hi}, geom, kl, kh)
