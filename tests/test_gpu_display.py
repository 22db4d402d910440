"""The display on the GPU (ray_tracer_s8_amd/film_display.py, display_csrc/), whole tensors compared bit for bit (NaN
where NaN) with the restatement tests/_display_np.py, and inputs read back unchanged:
1. rtd_meter with no scene, both histogram forms: 37 x 5 pixels (two full waves and a ragged third), 67 x 9 (ten waves of
   a block, the last ragged, and six with nothing), 131 x 71 (three blocks of 4 096 pixels, the last ragged) and 1030 x 1024 (258 chunks
   under a grid capped at 256 blocks: the stride loop runs twice); a constant image (every
   pixel in one bin, the count exactly R W), the bin edges tiled, log-uniform noise and the three extreme tiers; the histogram
   prefilled with a pattern, so that the clear is the call's; a second call on another image leaves that image's counts;
2. rtd_expose on the histograms of the host test, uploaded as they are, from a first and from a later record; a five-frame adaptation
   at rate 0.25 with its reset; manual values;
3. rtd_apply on 67 x 9 and 37 x 5 pixels, all six instances, the corpora of the host test at four scales and three whites, the record
   written by rtd_expose; each output alone into sentinel-filled tensors, and both together;
4. end to end on c2 at 64 x 36 in 3 strips, 8 samples: display() of the film's linear image; the identity with the film's rgb; three
   poses at rate 0.25; reset(); an upsampled frame through a display made with shape=; the refusals; the film's sums untouched.
Every body runs in a child process that imports torch first.  Without the feature every test here fails: there is no rt.FilmDisplay
and no librt_display.so.  No timing is asserted."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

_PRELUDE = r"""
import math
import sys
import numpy as np
import torch                                                      # first: the libraries then bind to torch's HIP runtime
sys.path.insert(0, "tests")
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, _display_lib as dl, film_display as fd, scenes
import _extreme_planes as xp
import _display_np as dnp

f32, u32 = np.float32, np.uint32
dev = torch.device("cuda", 0)

def refused(call, *a, **kw):
    try:
        call(*a, **kw)
    except ValueError:
        return True
    return False

def upload(stream, a):
    # an array's bytes on the device: uint32 words travel as int32
    a = np.ascontiguousarray(a)
    with torch.cuda.stream(stream):
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)

def words(t):
    return t.cpu().numpy().view(np.uint32)

def expose(lib, stream, d_H, d_rec, mode=dnp.AUTO, scale=1.0, white=np.inf, **kw):
    a = dict(dnp.DEFAULTS)
    a.update(kw)
    args = dl.ExposeArgs(mode=mode, key=a["key"], key_q16=a["key_q16"], white_q16=a["white_q16"], rate=a["rate"], scale_min=a["scale_min"],
                         scale_max=a["scale_max"], scale=scale, white=white, hist=None if d_H is None else d_H.data_ptr(),
                         record=d_rec.data_ptr())
    dl.check("rtd_expose", lib.rtd_expose(args, stream.cuda_stream))
"""


def _child(body, *args, timeout=600):
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body, *map(str, args)], capture_output=True, text=True, cwd=ROOT,
                       timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    return r.stdout


# ------------------------------------------------------------------------------------------- 1. the histogram, no scene

_METER_CHILD = r"""
W, R = (int(v) for v in sys.argv[1:3])
lib = dl.load()
stream = torch.cuda.Stream(device=dev)
images = dnp.meter_images(R, W)
pattern = (np.arange(dnp.WORDS, dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(1)
for form in dl.FORMS.values():
    d_H = upload(stream, pattern)
    for name, img in images.items():
        d_img = upload(stream, img)
        a = dl.MeterArgs(W=W, R=R, form=form, linear=d_img.data_ptr(), hist=d_H.data_ptr())
        dl.check("rtd_meter", lib.rtd_meter(a, stream.cuda_stream))
        stream.synchronize()
        H = words(d_H)
        want = dnp.histogram(img)
        assert (H == want).all(), (form, name, np.flatnonzero(H != want)[:8], H[H != want][:8], want[H != want][:8])
        assert int(H.astype(np.uint64).sum()) == R * W, (form, name)
        xp.identical(d_img.cpu().numpy(), img, ("the image", form, name))
        if name == "constant":
            assert H[120] == R * W                                 # every pixel in one bin: the worst contention
    # (every call above but the first ran over the counts of the image before it)
    assert len({dnp.histogram(i).tobytes() for i in images.values()}) == len(images)
print("ok")
"""


@pytest.mark.parametrize("W,R", [(37, 5), (67, 9), (131, 71), (1030, 1024)])
def test_the_meter_kernel(ndev, W, R):
    _child(_METER_CHILD, W, R)


# ------------------------------------------------------------------------------------------- 2. the exposure record

_EXPOSE_CHILD = r"""
lib = dl.load()
stream = torch.cuda.Stream(device=dev)

def run(H, rec, **kw):
    d_H = None if H is None else upload(stream, H)
    d_rec = upload(stream, dnp.record_words(rec))
    expose(lib, stream, d_H, d_rec, **kw)
    stream.synchronize()
    if H is not None:
        assert (words(d_H) == H).all()
    return dnp.record_of(words(d_rec))

for name, H, kw in dnp.expose_histograms():
    for frames in (0, 3):
        rec = dict(dnp.record0(), frames=frames, scale=f32(0.8))
        dnp.same_record(run(H, rec, **kw), dnp.expose(H, rec, **kw), (name, frames))
empty = np.zeros(dnp.WORDS, u32)
empty[256] = 630
for rec in (dict(dnp.record0(), scale=f32(5), white=f32(2), target=f32(6)),
            dict(dnp.record0(), scale=f32(5), white=f32(2), target=f32(6), frames=9, bin_key=4, bin_white=7),
            dict(dnp.record0(), frames=0xFFFFFFFF)):
    dnp.same_record(run(empty, rec), dnp.expose(empty, rec), ("empty", rec["frames"]))
# five frames at rate 0.25 on one record that stays on the device, then a reset as FilmDisplay.reset() does it
d_rec = upload(stream, dnp.record_words(dnp.record0()))
want = dnp.record0()
for k, H in enumerate(dnp.adaptation_histograms() + [None] + dnp.adaptation_histograms()[1::3]):
    if H is None:
        with torch.cuda.stream(stream):
            d_rec[7:].zero_()
        want = dict(want, frames=0)
        continue
    expose(lib, stream, upload(stream, H), d_rec, rate=0.25)
    stream.synchronize()
    want = dnp.expose(H, want, rate=0.25)
    dnp.same_record(dnp.record_of(words(d_rec)), want, ("frame", k))
    if k == 6:
        assert want["scale"] == want["target"] and want["frames"] == 1     # the first frame after the reset
assert want["frames"] == 2 and want["scale"] != want["target"]
# manual values: no histogram is read
rec = dict(dnp.record0(), counted=77, excluded=5, frames=2, bin_key=9, bin_white=11)
for scale, white in ((0.37, 4.0), (1.0, np.inf), (np.inf, np.inf), (2.0 ** -100, 1.0)):
    dnp.same_record(run(None, rec, mode=dnp.MANUAL, scale=scale, white=white), dnp.expose(None, rec, dnp.MANUAL, scale=scale, white=white),
                    ("manual", scale, white))
print("ok")
"""


def test_the_expose_kernel(ndev):
    _child(_EXPOSE_CHILD)


# ------------------------------------------------------------------------------------------- 3. the curves

_APPLY_CHILD = r"""
curve = int(sys.argv[1])
lib = dl.load()
stream = torch.cuda.Stream(device=dev)
SENTINEL = 7
cols = dnp.apply_colours()
calls = 0
for W, R in ((67, 9), (37, 5)):
    n = W * R
    if (W, R) == (67, 9):
        images = [dnp.tiled(cols, R, W, k * n) for k in range(-(-len(cols) // n))]          # every colour of the corpus
    else:
        images = [dnp.tiled(cols, R, W), dnp.tiled(cols[-n:], R, W)]
    images += [dnp.extreme_image(R, W, tier) for tier in xp.TIERS]
    d_rec = upload(stream, dnp.record_words(dnp.record0()))
    for scale in dnp.APPLY_SCALES:
        for white in dnp.APPLY_WHITES:
            expose(lib, stream, None, d_rec, mode=dnp.MANUAL, scale=scale, white=white)          # the record is rtd_expose's
            rec = dict(dnp.record0(), scale=f32(scale), white=f32(white))
            for k, img in enumerate(images):
                d_img = upload(stream, img)
                for dither in (0, 1):
                    want = dict(zip(("f32", "rgb"), dnp.apply(img, rec, curve, bool(dither))))
                    # both outputs on every image; each alone on the first and on the extreme ones
                    for asked in ((("f32", "rgb"),) + ((("f32",), ("rgb",)) if k == 0 or k >= len(images) - 3 else ())):
                        with torch.cuda.stream(stream):
                            out = dict(f32=torch.full((R, W, 3), SENTINEL, dtype=torch.float32, device=dev),
                                       rgb=torch.full((R, W, 3), SENTINEL, dtype=torch.uint8, device=dev))
                        a = dl.ApplyArgs(W=W, R=R, curve=curve, dither=dither, linear=d_img.data_ptr(), record=d_rec.data_ptr(),
                                         **{"out_" + o: out[o].data_ptr() for o in asked})
                        dl.check("rtd_apply", lib.rtd_apply(a, stream.cuda_stream))
                        stream.synchronize()
                        calls += 1
                        for o in ("f32", "rgb"):
                            got = out[o].cpu().numpy()
                            if o in asked:
                                xp.same(got, want[o], (W, R, curve, dither, scale, white, k, asked, o))
                            else:
                                assert (got == SENTINEL).all(), (W, R, curve, dither, scale, white, k, asked, o, "the sentinel")
                xp.identical(d_img.cpu().numpy(), img, ("the image", k))
            assert (words(d_rec)[:2] == np.array([scale, white], f32).view(u32)).all()
assert calls == 12 * (46 + 26)                                        # per size: 2 dithers x (3 calls on four images, 1 on the others)
print("ok")
"""


@pytest.mark.parametrize("curve", (0, 1, 2))
def test_the_apply_kernel(ndev, curve):
    _child(_APPLY_CHILD, curve)


# ------------------------------------------------------------------------------------------- 4. end to end

_FILM_CHILD = r"""
W, H, DIV, SPP = 64, 36, 3, 8
sph, rq = scenes.config("c2")
strips = lambda s=1: [rt.default_request(width=s * W, height=s * H, divisions=DIV, division_no=k, spp=SPP, max_bounces=rq.max_bounces,
                                         seed=rq.seed) for k in range(DIV)]

def orbit_camera(i, n=96):
    a = 2.0 * math.pi * i / n
    return rt.Camera.look_at((1.2 * math.sin(a), 0.3 + 0.4 * math.cos(a), 0.2), (0.0, -0.8, -4.0))

def host(film, t):
    film.sync()
    return t.cpu().numpy()

def record(disp):
    e = disp.exposure()
    assert tuple(e) == dnp.FIELDS
    return e

CURVE = dict(none=dnp.NONE, reinhard=dnp.REINHARD, filmic=dnp.FILMIC)

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
        # display() with the defaults, and every curve with and without dither
        for curve in fd.CURVES:
            for dither in (False, True):
                with rt.FilmDisplay(film, curve=curve, dither=dither) as disp:
                    assert record(disp) == dict(dnp.record0(), scale=1.0, white=math.inf, target=1.0)
                    out = disp.display(linear, ("rgb", "f32"))
                    assert out["rgb"].dtype == torch.uint8 and out["f32"].dtype == torch.float32 and tuple(out["rgb"].shape) == (H, W, 3)
                    Hist = dnp.histogram(lin)
                    assert disp.histogram.dtype == torch.int32 and tuple(disp.histogram.shape) == (257,)
                    assert (words(disp.histogram) == Hist).all() and int(Hist.sum()) == H * W
                    want = dnp.expose(Hist, dnp.record0())
                    dnp.same_record(record(disp), want, ("the record", curve, dither))
                    f, rgb = dnp.apply(lin, want, CURVE[curve], dither)
                    xp.same(host(film, out["f32"]), f, (curve, dither, "f32"))
                    xp.same(host(film, out["rgb"]), rgb, (curve, dither, "rgb"))
                    assert set(disp.display(linear)) == {"rgb"} and set(disp.apply(linear, ("f32",))) == {"f32"}
                    assert rgb.std() > 1.0
        # the film's sums are what they are without a display
        xp.identical(host(film, film.accum), accum0, "accum")
        xp.identical(host(film, film.moments), moments0, "moments")
        # curve "none", scale 1, no dither: the film's own rgb, byte for byte
        with rt.FilmDisplay(film, curve="none") as disp:
            disp.set_exposure(1.0)
            a = host(film, disp.apply(linear)["rgb"]).copy()
            b = host(film, film.preview(("rgb",))["rgb"])
            assert a.tobytes() == b.tobytes() and a.std() > 1.0
            assert host(film, disp.display(linear)["rgb"]).tobytes() == b.tobytes()      # metering keeps the manual values
            e = record(disp)
            assert (e["scale"], e["white"], e["target"], e["frames"]) == (1.0, math.inf, 1.0, 2)
            disp.set_exposure(0.37, 4.0)
            dnp.same_record(record(disp), dict(e, scale=f32(0.37), white=f32(4), target=f32(0.37), frames=3), "manual")
            disp.auto()
            assert record(disp)["frames"] == 0
            assert refused(disp.set_exposure, 0.0) and refused(disp.set_exposure, 1.0, 0.5) and refused(disp.set_exposure, math.nan)
        xp.identical(host(film, linear), lin, "the linear image after the displays")
        # three poses of the orbit at rate 0.25, then a reset
        with rt.FilmDisplay(film, rate=0.25, curve="reinhard", dither=True) as disp:
            want = dnp.record0()
            scales = []
            for i in (0, 8, 16, None, 24):
                if i is None:
                    disp.reset()
                    want = dict(want, frames=0)
                    assert record(disp)["frames"] == 0
                    continue
                scene.set_camera(orbit_camera(i))
                film.reset(seed=rq.seed + i)
                film.render_pass(0, SPP)
                frame = film.preview(("linear",))["linear"]
                rgb = disp.display(frame)["rgb"]
                img = host(film, frame).copy()
                want = dnp.expose(dnp.histogram(img), want, rate=0.25)
                dnp.same_record(record(disp), want, ("pose", i))
                xp.same(host(film, rgb), dnp.apply(img, want, dnp.REINHARD, True)[1], ("pose", i, "rgb"))
                scales.append((want["scale"], want["target"]))
            assert scales[0][0] == scales[0][1] and scales[3][0] == scales[3][1] and want["frames"] == 1
            assert all(s == f32(p + f32(f32(0.25) * f32(t - p))) for (p, _), (s, t) in zip(scales[:2], scales[1:3]))
        # an upsampled frame through a display of its own shape
        with rt.FilmUpsampler(film, strips(2)) as up, rt.FilmDisplay(film, shape=(2 * H, 2 * W)) as big, rt.FilmDisplay(film) as small:
            frame = film.preview(("linear",))["linear"]
            hi = up.upsample(frame, planes_lo={}, planes_hi={}, outputs=("linear",))["linear"]
            rgb = big.display(hi)["rgb"]
            img = host(film, hi).copy()
            assert img.shape == (2 * H, 2 * W, 3)
            want = dnp.expose(dnp.histogram(img), dnp.record0())
            dnp.same_record(record(big), want, "the upsampled frame")
            xp.same(host(film, rgb), dnp.apply(img, want, dnp.FILMIC)[1], "the upsampled frame: rgb")
            # the refusals: shape, dtype, device, contiguity, outputs
            for call in (big.meter, big.apply, big.display):
                assert refused(call, frame)                                    # the film's shape, not the display's
            assert refused(small.display, hi) and not refused(small.display, frame)
            assert refused(small.display, frame.double()) and refused(small.display, frame.cpu()) and refused(small.display, host(film, frame))
            assert refused(small.display, frame.permute(1, 0, 2)) and refused(small.display, hi[::2, ::2]) and refused(small.display, None)
            assert refused(small.display, frame, ()) and refused(small.apply, frame, ("linear",)) and refused(small.apply, frame, ("rgb", "rgb"))
            small.close()
            assert refused(small.display, frame) and refused(small.exposure) and refused(small.reset) and refused(lambda: small.histogram)
            small.close()
        late = rt.FilmDisplay(film)
    assert refused(late.display, linear) and refused(late.exposure) and refused(rt.FilmDisplay, film)        # a closed film
print("ok")
"""


def test_a_film_through_its_display(ndev):
    _child(_FILM_CHILD)
