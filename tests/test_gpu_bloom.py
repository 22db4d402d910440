"""The bloom on the GPU (ray_tracer_s8_amd/film_bloom.py, bloom_csrc/): rtb_apply equals the restatement
tests/_bloom_np.py bit for bit in whole tensors (the mixed image, the bloom alone and every level the scratch holds), under both forms,
which are compared with each other too; the input is read back unchanged, the outputs are written into sentinel-filled tensors with
sentinels behind them, and the scratch is followed by guard words that must survive.

The shapes (_bloom_np.SHAPES, rows x columns and levels; the tail's place is asserted for each):
  1 x 1 with L = 1 and L = 8     every tap clamped, sides stuck at 1;
  2 x 3 (L = 2), 5 x 37 (L = 3)  odd both ways, a ragged wave;
  67 x 9 (L = 6)                 the whole pyramid inside the tail, tail_from = 1;
  131 x 71 (L = 8)               eight levels, all in the tail;
  200 x 260 (L = 1)              level 1 is 156 000 bytes and lies within the 160 KiB of the tail, which then reads the image itself;
  240 x 260 (L = 1)              level 1 is 187 200 bytes: L < tail_from = 2, the TAIL form launches no tail (the LDS budget is the
                                 whole 160 KiB, which 200 x 260 with one level still fits);
  200 x 260 (L = 6)              level 1 and the deeper levels pass 160 KiB: the tail starts mid-pyramid, at level 2;
  75 x 283 (L = 4)               level 1 is 38 x 142 and level 2 19 x 71: five and three tiles of 8 x 32 in each direction for the two
                                 instances of the down kernel, three tiles of 2 x 2 blocks each way for the up-add, no side a
                                 multiple of a tile, so every halo crosses tile borders.
Contents: a constant 0.75 image that must stay exactly 0.75; single impulses at a corner, at the centre and on a tile border;
log-uniform noise; the three extreme tiers (no NaN out, +inf stays +inf); every instance (threshold on and off x mix and add x the
second output on and off); and end to end on c2 at 64 x 36 in 3 strips, 8 samples: apply of the film's preview and FilmDisplay.display
of the result, an upsampled frame through shape=, the refusals, the film's sums untouched.
Every body runs in a child process that imports torch first.  Without the feature every test here fails: there is no film_bloom, no
_bloom_lib and no librt_bloom.so.  No timing is asserted."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

_PRELUDE = r"""
import ctypes as C
import math
import sys
import numpy as np
import torch                                                      # first: the libraries then bind to torch's HIP runtime
sys.path.insert(0, "tests")
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _bloom_lib as bl, film_bloom as fb, scenes
import _extreme_planes as xp
import _bloom_np as bnp

f32, u32 = np.float32, np.uint32
dev = torch.device("cuda", 0)
SENTINEL, GUARD = f32(-7777.0), 64
FORMS = (bnp.LEVELS, bnp.TAIL)
TAIL_FROM = {((1, 1), 1): 1, ((1, 1), 8): 1, ((2, 3), 2): 1, ((5, 37), 3): 1, ((67, 9), 6): 1, ((131, 71), 8): 1, ((200, 260), 1): 1,
             ((240, 260), 1): 2, ((200, 260), 6): 2, ((75, 283), 4): 1}
assert all(bnp.tail_from(s, l) == TAIL_FROM[(s, l)] for s, l in bnp.SHAPES) and len(TAIL_FROM) == len(bnp.SHAPES)

def refused(call, *a, **kw):
    try:
        call(*a, **kw)
    except ValueError:
        return True
    return False

def upload(stream, a):
    with torch.cuda.stream(stream):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

def device_apply(lib, stream, img, levels, form, mode=bnp.MIX, spread=0.7, strength=0.05, threshold=0.0, knee=0.5, cap=65536.0, second=True):
    # rtb_apply into sentinel-filled outputs with GUARD floats behind each and a scratch of exactly its size with GUARD bytes behind
    # it: (out, bloom or None, {k: level k of the scratch}, the bytes of the scratch)
    img = np.ascontiguousarray(img, f32)
    R, W = img.shape[:2]
    n = C.c_uint64(0)
    bl.check("rtb_scratch_bytes", lib.rtb_scratch_bytes(W, R, levels, C.byref(n)))
    offsets, size = bnp.scratch_layout((R, W), levels)
    assert n.value == size
    d_in = upload(stream, img)
    fill = np.full(img.size + GUARD, SENTINEL, f32)
    d_out, d_b = upload(stream, fill), upload(stream, fill) if second else None
    d_scratch = upload(stream, np.full(size + GUARD, 0xA5, np.uint8))
    a = bl.ApplyArgs(W=W, R=R, levels=levels, mode=mode, form=form, spread=spread, strength=strength, norm=bnp.norm_of(spread, levels),
                     cap=cap, T=threshold, K=bnp.knee_of(threshold, knee), inp=d_in.data_ptr(), out=d_out.data_ptr(),
                     out_bloom=d_b.data_ptr() if second else None, scratch=d_scratch.data_ptr(), scratch_bytes=size)
    bl.check("rtb_apply", lib.rtb_apply(a, stream.cuda_stream))
    stream.synchronize()
    assert d_in.cpu().numpy().tobytes() == img.tobytes(), "the input changed"
    outs = []
    for d in (d_out, d_b):
        if d is None:
            outs.append(None)
            continue
        h = d.cpu().numpy()
        assert (h[img.size:] == SENTINEL).all(), "written past an output"
        assert not (h[:img.size] == SENTINEL).any(), "an output was not written everywhere"
        outs.append(h[:img.size].reshape(img.shape))
    s = d_scratch.cpu().numpy()
    assert (s[size:] == 0xA5).all(), "written past the scratch"
    levels_ = {}
    for k, (shape, at) in enumerate(zip(bnp.level_shapes((R, W), levels)[1:], offsets), 1):
        levels_[k] = s[at:at + shape[0] * shape[1] * 12].view(f32).reshape(*shape, 3)
    return outs[0], outs[1], levels_, s[:size]

def same_as_restatement(lib, stream, img, levels, what, **kw):
    # both forms against the restatement and against each other; the levels a form writes, and the ones the tail keeps on chip
    want_out, want_b, want_U = bnp.bloom(img, levels, **kw)
    tf = bnp.tail_from(img.shape[:2], levels)
    got = {}
    for form in FORMS:
        out, b, U, _ = device_apply(lib, stream, img, levels, form, **kw)
        xp.same(out, want_out, (what, form, "out"))
        if b is not None:
            xp.same(b, want_b, (what, form, "bloom"))
        for k in range(1, levels + 1):
            if form == bnp.LEVELS or tf > levels or k <= tf:
                xp.same(U[k], want_U[k], (what, form, "U", k))
            else:
                assert (U[k].view(np.uint8) == 0xA5).all(), (what, "the tail wrote level", k)
        got[form] = (out, b)
    assert got[bnp.LEVELS][0].tobytes() == got[bnp.TAIL][0].tobytes(), (what, "the forms differ")
    if got[bnp.LEVELS][1] is not None:
        assert got[bnp.LEVELS][1].tobytes() == got[bnp.TAIL][1].tobytes(), (what, "the forms differ in the bloom")
    return want_out, want_b
"""


def _child(body, *args, timeout=600):
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body, *map(str, args)], capture_output=True, text=True, cwd=ROOT,
                       timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    return r.stdout


# ------------------------------------------------------------------------------------------- 1. the library, no scene

_CONSTANT_CHILD = r"""
lib = bl.load()
stream = torch.cuda.Stream(device=dev)
assert bnp.norm_of(1.0, 4) == f32(0.25)
for shape, _ in bnp.SHAPES:
    img = np.full((*shape, 3), 0.75, f32)
    for form in FORMS:
        out, b, U, _ = device_apply(lib, stream, img, 4, form, spread=1.0, strength=0.25)
        assert (out == f32(0.75)).all() and (b == f32(0.75)).all(), (shape, form)
        assert (U[1] == f32(3.0)).all()                                  # 0.75 (1 + 1 + 1 + 1)
print("ok")
"""

_IMPULSE_CHILD = r"""
lib = bl.load()
stream = torch.cuda.Stream(device=dev)
# a corner, the centre, and the pixel whose level-1 pixel is the first of the second tile both ways (row 16, column 64)
cases = [((75, 283), 4, (0, 0)), ((75, 283), 4, (74, 282)), ((75, 283), 4, (37, 141)), ((75, 283), 4, (16, 64)), ((75, 283), 4, (15, 63)),
         ((200, 260), 6, (16, 64)), ((200, 260), 6, (199, 0)), ((5, 37), 3, (2, 18)), ((67, 9), 6, (66, 8)), ((2, 3), 2, (1, 2)), ((1, 1), 8, (0, 0))]
for shape, levels, at in cases:
    out, b = same_as_restatement(lib, stream, bnp.impulse(shape, at), levels, (shape, levels, at))
    assert b[at].min() > 0 and out[at][0] > 900 and (b >= 0).all()
print("ok")
"""

_NOISE_CHILD = r"""
lib = bl.load()
stream = torch.cuda.Stream(device=dev)
for j, (shape, levels) in enumerate(bnp.SHAPES):
    out, b = same_as_restatement(lib, stream, bnp.log_uniform(shape, 40 + j), levels, (shape, levels))
    assert not np.isnan(out).any() and (b >= 0).all() and (shape[0] * shape[1] < 4 or (b > 0).any())
print("ok")
"""

_EXTREME_CHILD = r"""
lib = bl.load()
stream = torch.cuda.Stream(device=dev)
kept = {}
for tier in xp.TIERS:
    for j, (shape, levels) in enumerate((((5, 37), 3), ((67, 9), 6), ((75, 283), 4), ((200, 260), 6))):
        img = bnp.extreme(shape, tier, 70 + j)
        for kw in (dict(), dict(mode=bnp.ADD, strength=3.0, threshold=1.0), dict(cap=2.0 ** 62, threshold=2.0 ** 61, knee=1.0)):
            out, b = same_as_restatement(lib, stream, img, levels, (tier, shape, levels, kw), **kw)
            assert not np.isnan(out).any() and not np.isnan(b).any() and (out >= 0).all() and (b >= 0).all()
            assert (out[np.isposinf(img)] == np.inf).all()
            kept[tier] = kept.get(tier, False) or bool(((out > 0) & (out < xp.TINY)).any() and ((b > 0) & (b < xp.TINY)).any())
        if tier == "nonfinite":
            assert np.isnan(img).any() and np.isposinf(img).any() and np.isneginf(img).any()
assert kept["small"]             # subnormals are kept: where the tier's block of subnormal pixels is wider than the pyramid's reach
print("ok")
"""

_INSTANCES_CHILD = r"""
lib = bl.load()
stream = torch.cuda.Stream(device=dev)
for j, (shape, levels) in enumerate((((67, 9), 6), ((75, 283), 4), ((200, 260), 6))):
    img = bnp.log_uniform(shape, 90 + j, -6.0, 6.0)
    for threshold in (0.0, 1.0):
        for mode, strength in ((bnp.MIX, 0.3), (bnp.ADD, 1.5)):
            kw = dict(mode=mode, strength=strength, threshold=threshold, knee=0.5, spread=0.85)
            want_out, want_b = same_as_restatement(lib, stream, img, levels, (shape, kw, "two outputs"), **kw)
            for form in FORMS:
                out, none, _, _ = device_apply(lib, stream, img, levels, form, second=False, **kw)
                assert none is None
                xp.same(out, want_out, (shape, kw, form, "one output"))
    # the threshold does something, and so does the mode
    assert not np.array_equal(bnp.bloom(img, levels, threshold=1.0)[1], bnp.bloom(img, levels)[1])
print("ok")
"""


def test_a_constant_image_stays_exactly_what_it_is(ndev):
    _child(_CONSTANT_CHILD)


def test_single_impulses(ndev):
    _child(_IMPULSE_CHILD)


def test_log_uniform_noise_on_every_shape(ndev):
    _child(_NOISE_CHILD)


def test_the_extreme_tiers(ndev):
    _child(_EXTREME_CHILD)


def test_every_instance(ndev):
    _child(_INSTANCES_CHILD)


# ------------------------------------------------------------------------------------------- 2. end to end

_FILM_CHILD = r"""
import _display_np as dnp
W, H, DIV, SPP = 64, 36, 3, 8
sph, rq = scenes.config("c2")
strips = lambda s=1: [rt.default_request(width=s * W, height=s * H, divisions=DIV, division_no=k, spp=SPP, max_bounces=rq.max_bounces,
                                         seed=rq.seed) for k in range(DIV)]

def host(film, t):
    film.sync()
    return t.cpu().numpy()

with rt.Scene(0, rt.World(sph)) as scene:
    kw = dict(integrator="nee", mode=rt.RT_NEE_MIS, moments=True)
    with rt.Film(scene, strips(), **kw) as plain:
        plain.render_pass(0, SPP)
        accum0, moments0 = host(plain, plain.accum).copy(), host(plain, plain.moments).copy()
    with rt.Film(scene, strips(), **kw) as film:
        film.render_pass(0, SPP)
        linear = film.preview(("linear",))["linear"]
        lin = host(film, linear).copy()
        assert lin.shape == (H, W, 3) and (lin > 1).any()                       # the lamp is above 1.0
        for form in ("levels", "tail"):
            with rt.FilmBloom(film) as bloom, rt.FilmDisplay(film) as disp:
                assert bloom.settings == ((H, W), 5, 0.7, 0.05, "mix", 0.0, 0.5, 65536.0) and bloom.form == fb.FORM
                bloom.form = form
                out = bloom.apply(linear, ("linear", "bloom"))
                assert set(out) == {"linear", "bloom"} and all(t.dtype == torch.float32 and tuple(t.shape) == (H, W, 3) for t in out.values())
                want_out, want_b, _ = bnp.bloom(lin, 5)
                xp.same(host(film, out["linear"]), want_out, (form, "linear"))
                xp.same(host(film, out["bloom"]), want_b, (form, "bloom"))
                again = bloom.apply(linear)
                assert set(again) == {"linear"} and again["linear"].data_ptr() != out["linear"].data_ptr()      # new tensors a call
                xp.same(host(film, again["linear"]), want_out, (form, "again"))
                # the bloomed frame through the display
                rgb = disp.display(out["linear"])["rgb"]
                rec = dnp.expose(dnp.histogram(want_out), dnp.record0())
                xp.same(host(film, rgb), dnp.apply(want_out, rec, dnp.FILMIC)[1], (form, "rgb"))
                assert host(film, rgb).std() > 1.0
        xp.identical(host(film, linear), lin, "the linear image after the blooms")
        # other settings
        with rt.FilmBloom(film, levels=3, spread=1.0, strength=2.0, mode="add", threshold=1.0, knee=0.25, cap=1000.0) as bloom:
            out = bloom.apply(linear, ("linear", "bloom"))
            want_out, want_b, _ = bnp.bloom(lin, 3, spread=1.0, strength=2.0, mode=bnp.ADD, threshold=1.0, knee=0.25, cap=1000.0)
            xp.same(host(film, out["linear"]), want_out, "add: linear")
            xp.same(host(film, out["bloom"]), want_b, "add: bloom")
        # the film's sums are what they are without a bloom
        xp.identical(host(film, film.accum), accum0, "accum")
        xp.identical(host(film, film.moments), moments0, "moments")
        # an upsampled frame through a bloom of its own shape
        with rt.FilmUpsampler(film, strips(2)) as up, rt.FilmBloom(film, shape=(2 * H, 2 * W)) as big, rt.FilmBloom(film) as small:
            hi = up.upsample(linear, planes_lo={}, planes_hi={}, outputs=("linear",))["linear"]
            img = host(film, hi).copy()
            assert img.shape == (2 * H, 2 * W, 3) and big.settings.levels == 6
            xp.same(host(film, big.apply(hi)["linear"]), bnp.bloom(img, 6)[0], "the upsampled frame")
            xp.identical(host(film, hi), img, "the upsampled frame after its bloom")
            # the refusals: shape, dtype, device, contiguity, outputs
            assert refused(big.apply, linear) and refused(small.apply, hi) and not refused(small.apply, linear)
            assert refused(small.apply, linear.double()) and refused(small.apply, linear.cpu()) and refused(small.apply, lin)
            assert refused(small.apply, linear.permute(1, 0, 2)) and refused(small.apply, hi[::2, ::2]) and refused(small.apply, None)
            assert refused(small.apply, linear, ()) and refused(small.apply, linear, ("bloom",)) and refused(small.apply, linear, ("linear", "rgb"))
            small.close()
            assert refused(small.apply, linear)
            small.close()
        late = rt.FilmBloom(film)
    assert refused(late.apply, linear) and refused(rt.FilmBloom, film)           # a closed film
print("ok")
"""


def test_a_film_through_its_bloom_and_its_display(ndev):
    _child(_FILM_CHILD)
