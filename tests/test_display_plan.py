"""The display without a GPU (ray_tracer_s8_amd/film_display.py, _display_lib.py, build.py):
1. check_display, check_exposure, check_outputs and percentile_q16 refuse, with ValueError, everything FilmDisplay refuses; FilmDisplay
   is in rt.__all__;
2. film_display.py and _display_lib.py import without torch and without loading the library;
3. the binding has the version, the status table, the modes, the curves, the forms and the sizes of this library's header;
4. every refusal of the library's calls comes back as a status, with no device bound and addresses that are never read.
What holds of every private library (a library of its own, its record, its exports, who builds it) is tests/test_private_libraries.py's.
Without the feature every test here fails: there is no film_display, no _display_lib and no build.DISPLAY."""
import ctypes as C
import math
import re
import subprocess
import sys
import types
from pathlib import Path

import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import build

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rtd_version", "rtd_meter", "rtd_expose", "rtd_apply")


def test_check_display():
    from ray_tracer_s8_amd import film_display as fd
    assert rt.FilmDisplay is fd.FilmDisplay and "FilmDisplay" in rt.__all__
    assert fd.CURVES == ("none", "reinhard", "filmic") and fd.OUTPUTS == ("rgb", "f32")
    s = fd.check_display((36, 64))
    assert s == ((36, 64), "filmic", 0.54, 32768, 64880, 1.0, 2.0 ** -8, 2.0 ** 8, False)
    assert (s.shape, s.curve, s.key_q16, s.white_q16, s.dither) == ((36, 64), "filmic", 32768, 64880, False)
    for curve in fd.CURVES:
        assert fd.check_display([9, 70], curve, dither=True).curve == curve
    assert fd.check_display((1, 1), key=1, rate=0.25, key_percentile=0, white_percentile=1, scale_range=(1, 1))[2:8] == \
        (1.0, 0, 65535, 0.25, 1.0, 1.0)
    assert fd.check_display((1 << 15, (1 << 16) - 2)).shape == (1 << 15, (1 << 16) - 2)
    bad = {
        "no shape": dict(shape=None), "a flat shape": dict(shape=(64,)), "three": dict(shape=(36, 64, 3)), "zero rows": dict(shape=(0, 64)),
        "negative": dict(shape=(36, -1)), "float sizes": dict(shape=(36.0, 64)), "bool sizes": dict(shape=(True, 64)),
        "2^31 pixels": dict(shape=(1 << 15, 1 << 16)),
        "an unknown curve": dict(curve="aces"), "curve None": dict(curve=None), "curve 2": dict(curve=2),
        "key 0": dict(key=0.0), "key < 0": dict(key=-0.5), "key inf": dict(key=math.inf), "key nan": dict(key=math.nan),
        "key a string": dict(key="0.5"), "key True": dict(key=True), "key below f32": dict(key=1e-50), "key above f32": dict(key=1e39),
        "rate 0": dict(rate=0.0), "rate > 1": dict(rate=1.25), "rate nan": dict(rate=math.nan), "rate < 0": dict(rate=-0.5),
        "rate None": dict(rate=None),
        "range of one": dict(scale_range=(1.0,)), "range None": dict(scale_range=None), "range descending": dict(scale_range=(4.0, 0.25)),
        "range from 0": dict(scale_range=(0.0, 4.0)), "range to inf": dict(scale_range=(0.25, math.inf)),
        "range nan": dict(scale_range=(math.nan, 4.0)),
        "percentile > 1": dict(white_percentile=1.5), "percentile < 0": dict(key_percentile=-0.1), "percentile nan": dict(key_percentile=math.nan),
        "percentile None": dict(white_percentile=None), "white below key": dict(key_percentile=0.75, white_percentile=0.5),
        "dither 1": dict(dither=1), "dither None": dict(dither=None),
    }
    for what, kw in bad.items():
        args = dict(shape=(36, 64))
        args.update(kw)
        with pytest.raises(ValueError):
            fd.check_display(**args)
            pytest.fail(what)


def test_percentiles_exposures_and_outputs():
    from ray_tracer_s8_amd import film_display as fd
    q = fd.percentile_q16
    assert (q(0), q(0.0), q(0.5), q(0.99), q(1), q(1.0), q(1 / 65536), q(0.999999)) == (0, 0, 32768, 64880, 65535, 65535, 1, 65535)
    assert all(q(k / 65536) == k for k in range(0, 65536, 257))
    for p in (-1e-9, 1.0000001, math.nan, math.inf, None, "0.5", True):
        with pytest.raises(ValueError):
            q(p)
    assert fd.check_exposure(1.0) == (1.0, math.inf) and fd.check_exposure(0.37, 4) == (0.37, 4.0)
    assert fd.check_exposure(math.inf, math.inf) == (math.inf, math.inf) and fd.check_exposure(2.0 ** -100, 1.0) == (2.0 ** -100, 1.0)
    for scale, white in ((0.0, 2.0), (-1.0, 2.0), (math.nan, 2.0), (None, 2.0), (1.0, 0.5), (1.0, math.nan), (1.0, -math.inf),
                         (1e-50, 2.0), (1e39, 2.0), ("1", 2.0), (True, 2.0), (1.0, None)):
        with pytest.raises(ValueError):
            fd.check_exposure(scale, white)
            pytest.fail(repr((scale, white)))
    assert fd.check_outputs() == ("rgb",) and fd.check_outputs(["f32", "rgb"]) == ("f32", "rgb")
    for outs in ((), ("linear",), ("rgb", "rgb"), ("rgb", "hdr")):
        with pytest.raises(ValueError, match="outputs"):
            fd.check_outputs(outs)


def test_film_display_runs_its_checks_before_anything_else():
    """Bad arguments: ValueError before the film, torch or the library is touched."""
    from ray_tracer_s8_amd import _display_lib
    loaded = _display_lib.BINDING.loaded
    film = types.SimpleNamespace(rows=36, width=64)                     # (no _check_open, no _torch: touching either would raise)
    for kw in (dict(curve="aces"), dict(key=0), dict(rate=2.0), dict(shape=(0, 3)), dict(key_percentile=0.9, white_percentile=0.1),
               dict(dither="yes"), dict(scale_range=(2.0, 1.0))):
        with pytest.raises(ValueError):
            rt.FilmDisplay(film, **kw)
    with pytest.raises(ValueError):
        rt.FilmDisplay(types.SimpleNamespace())                        # no shape to take from the film
    assert _display_lib.BINDING.loaded is loaded


_IMPORT_CHILD = r"""
import sys
import ray_tracer_s8_amd as rt
import ray_tracer_s8_amd.film_display as fd
import ray_tracer_s8_amd._display_lib as dl
assert "torch" not in sys.modules
assert not dl.BINDING.loaded                            # importing loads nothing
assert callable(fd.check_display) and callable(fd.percentile_q16) and rt.FilmDisplay is fd.FilmDisplay
assert all(callable(getattr(fd.FilmDisplay, n)) for n in ("meter", "apply", "display", "set_exposure", "auto", "exposure", "reset", "close"))
assert isinstance(fd.FilmDisplay.histogram, property)
assert sorted(dl.SIGNATURES) == sorted(%r)
assert fd.check_display((9, 70), "reinhard").curve == "reinhard"
assert "torch" not in sys.modules and not dl.BINDING.loaded
print("ok")
""" % (NAMES,)


def test_film_display_and_its_binding_import_without_torch():
    r = subprocess.run([sys.executable, "-c", _IMPORT_CHILD], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_the_bindings_own_constants():
    from ray_tracer_s8_amd import _display_lib
    assert _display_lib.RTD_VERSION == 1 and set(_display_lib.SIGNATURES) == set(NAMES)
    assert _display_lib.STATUS == {1: "RTD_ERR_BAD_ARG", 2: "RTD_ERR_LIMIT", 3: "RTD_ERR_HIP", 4: "RTD_ERR_INTERNAL"}
    text = (build.DISPLAY.src_dir / "rt_display.h").read_text()
    named = lambda names: dict((n.lower(), int(v)) for n, v in re.findall(rf"^#define RTD_({names}) (\d+)u", text, re.M))
    assert named("AUTO|MANUAL") == _display_lib.MODES and named("NONE|REINHARD|FILMIC") == _display_lib.CURVES
    assert named("HIST_WAVE|HIST_MATCH") == {"hist_" + k: v for k, v in _display_lib.FORMS.items()}
    assert named("HIST_WORDS|RECORD_WORDS") == dict(hist_words=_display_lib.HIST_WORDS, record_words=_display_lib.RECORD_WORDS)


def test_the_binding_loads_the_library_and_refusals_are_statuses():
    """Loading binds no device: rtd_version is host arithmetic, and rtd_meter, rtd_expose and rtd_apply refuse before any launch."""
    from ray_tracer_s8_amd import _display_lib as dl
    lib = dl.load()
    assert lib.rtd_version(None) == 1
    v = C.c_uint32(0)
    assert lib.rtd_version(C.byref(v)) == 0 and v.value == dl.RTD_VERSION
    assert lib.rtd_meter(None, None) == 1 and lib.rtd_expose(None, None) == 1 and lib.rtd_apply(None, None) == 1
    MB = 1 << 20
    at = lambda k: C.c_void_p(k * MB)                                 # (addresses never read: every call here is refused)

    def meter(**kw):
        # 67 x 9 pixels: the image 7 236 bytes, the histogram 1 028
        good = dict(W=67, R=9, form=0, linear=at(1), hist=at(2))
        good.update(kw)
        return lib.rtd_meter(dl.MeterArgs(**good), None)

    bad = [dict(W=0), dict(R=0), dict(form=2), dict(form=255), dict(reserved=1), dict(linear=None), dict(hist=None),
           dict(linear=C.c_void_p(MB + 2)), dict(hist=C.c_void_p(2 * MB + 1)),
           # the histogram inside the image, at its last float, the image inside the histogram
           dict(hist=at(1)), dict(hist=C.c_void_p(MB + 7232)), dict(hist=C.c_void_p(MB - 1024)), dict(linear=C.c_void_p(2 * MB + 1024))]
    for kw in bad:
        assert meter(**kw) == 1, kw
    assert meter(W=1 << 16, R=1 << 15) == 2                          # 2^31 pixels
    assert meter(W=1 << 31, R=1 << 31) == 2

    def expose(**kw):
        good = dict(mode=0, key=0.54, key_q16=32768, white_q16=64880, rate=0.25, scale_min=2.0 ** -8, scale_max=2.0 ** 8, hist=at(1), record=at(2))
        good.update(kw)
        return lib.rtd_expose(dl.ExposeArgs(**good), None)

    inf, nan = math.inf, math.nan
    bad = [dict(mode=2), dict(mode=255), dict(reserved=7), dict(hist=None), dict(record=None),
           dict(hist=C.c_void_p(MB + 2)), dict(record=C.c_void_p(2 * MB + 3)),
           dict(record=at(1)), dict(record=C.c_void_p(MB + 1024)), dict(record=C.c_void_p(MB - 28)),
           dict(key=0.0), dict(key=-0.54), dict(key=inf), dict(key=nan), dict(rate=0.0), dict(rate=-1.0), dict(rate=1.0000001), dict(rate=nan),
           dict(rate=inf), dict(scale_min=0.0), dict(scale_min=nan), dict(scale_min=inf), dict(scale_max=inf), dict(scale_max=-1.0),
           dict(scale_min=2.0, scale_max=1.0), dict(key_q16=65536), dict(white_q16=65536), dict(white_q16=32767),
           dict(key_q16=50000, white_q16=49999),
           dict(mode=1, scale=0.0, white=1.0), dict(mode=1, scale=-2.0, white=1.0), dict(mode=1, scale=nan, white=1.0),
           dict(mode=1, scale=1.0, white=0.999), dict(mode=1, scale=1.0, white=nan), dict(mode=1, scale=1.0, white=-inf),
           dict(mode=1, scale=1.0, white=2.0, record=None), dict(mode=1, scale=1.0, white=2.0, record=C.c_void_p(2 * MB + 2))]
    for kw in bad:
        assert expose(**kw) == 1, kw

    def apply(**kw):
        # 67 x 9 pixels: the image and out_f32 7 236 bytes, out_rgb 1 809, the record 32
        good = dict(W=67, R=9, curve=2, dither=0, linear=at(1), record=at(2), out_f32=at(3), out_rgb=at(4))
        good.update(kw)
        return lib.rtd_apply(dl.ApplyArgs(**good), None)

    bad = [dict(W=0), dict(R=0), dict(curve=3), dict(curve=255), dict(dither=2), dict(linear=None), dict(record=None),
           dict(out_f32=None, out_rgb=None),
           dict(linear=C.c_void_p(MB + 4)), dict(linear=C.c_void_p(MB + 8)), dict(out_f32=C.c_void_p(3 * MB + 4)),
           dict(out_rgb=C.c_void_p(4 * MB + 1)), dict(out_rgb=C.c_void_p(4 * MB + 2)), dict(record=C.c_void_p(2 * MB + 2)),
           # an output that is the image, ends inside it, begins at its last float; the record inside an output; two outputs that overlap
           dict(out_f32=at(1)), dict(out_rgb=at(1)), dict(out_f32=C.c_void_p(MB - 16)), dict(out_rgb=C.c_void_p(MB + 7232)),
           dict(record=C.c_void_p(MB + 7232)), dict(record=C.c_void_p(3 * MB + 64)), dict(record=C.c_void_p(4 * MB + 1808)),
           dict(out_rgb=at(3)), dict(out_rgb=C.c_void_p(3 * MB + 7232)), dict(out_f32=C.c_void_p(4 * MB - 7232 + 16))]
    for kw in bad:
        assert apply(**kw) == 1, kw
    assert apply(W=1 << 16, R=1 << 15) == 2                          # 2^31 pixels
    with pytest.raises(dl.RtdError):
        dl.check("rtd_apply", 2)
    assert isinstance(dl.RtdError("x", 1), RuntimeError) and "RTD_ERR_BAD_ARG" in str(dl.RtdError("x", 1))
