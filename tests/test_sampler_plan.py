"""The film sampler without a GPU (ray_tracer_s8_amd/film_sampler.py, _sampler_lib.py, build.py):
1. check_sampler refuses, with ValueError, everything FilmSampler refuses, and accepts the rest;
2. film_sampler.py and _sampler_lib.py import without torch and without loading the sampler library;
3. every refusal of the library's calls comes back as a status, with no device bound.
What holds of every private library (a library of its own, its record, its exports, who builds it) is tests/test_private_libraries.py's.
Without the feature every test here fails: there is no film_sampler, no _sampler_lib and no build.SAMPLER."""
import ctypes as C
import subprocess
import sys
import types
from pathlib import Path

import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rts_version", "rts_scratch_bytes", "rts_select", "rts_gather", "rts_fold", "rts_normalise")


def test_check_sampler_accepts():
    from ray_tracer_s8_amd import film_sampler as fs
    assert fs.check_sampler(True) == (fs.THRESHOLD, 1, fs.EPS)
    assert fs.check_sampler(True, 0, 0, 1e-9) == (0.0, 0, 1e-9)
    assert fs.check_sampler(True, 0.25, 1, 2) == (0.25, 1, 2.0)
    assert fs.check_sampler(True, float("inf")) == (float("inf"), 1, fs.EPS)        # a sampler that never finds a noisy pixel
    assert fs.THRESHOLD >= 0 and fs.EPS > 0 and fs.DILATE == 1
    assert rt.FilmSampler is fs.FilmSampler and "FilmSampler" in rt.__all__


def test_check_sampler_refuses():
    from ray_tracer_s8_amd import film_sampler as fs
    inf, nan = float("inf"), float("nan")
    bad = {
        "no moments": dict(moments=False),
        "threshold < 0": dict(threshold=-0.1),
        "threshold -inf": dict(threshold=-inf),
        "threshold nan": dict(threshold=nan),
        "threshold a string": dict(threshold="0.1"),
        "threshold True": dict(threshold=True),
        "threshold None": dict(threshold=None),
        "dilate 2": dict(dilate=2),
        "dilate -1": dict(dilate=-1),
        "dilate 1.0": dict(dilate=1.0),
        "dilate True": dict(dilate=True),
        "dilate None": dict(dilate=None),
        "eps 0": dict(eps=0.0),
        "eps < 0": dict(eps=-1e-3),
        "eps inf": dict(eps=inf),
        "eps nan": dict(eps=nan),
        "eps a string": dict(eps="1e-3"),
        "eps True": dict(eps=True),
    }
    for what, kw in bad.items():
        args = dict(moments=True)
        args.update(kw)
        with pytest.raises(ValueError):
            fs.check_sampler(**args)
            pytest.fail(what)


def test_film_sampler_runs_its_checks_before_anything_else():
    """No film, a film without moments, bad constants: ValueError before torch or the library is touched."""
    plain = types.SimpleNamespace(moments=None)
    with_moments = types.SimpleNamespace(moments=object())
    for film, kw in ((None, {}), (plain, {}), (with_moments, dict(threshold=-1.0)), (with_moments, dict(dilate=2)),
                     (with_moments, dict(eps=0.0))):
        with pytest.raises(ValueError):
            rt.FilmSampler(film, **kw)


_IMPORT_CHILD = r"""
import sys
import ray_tracer_s8_amd as rt
import ray_tracer_s8_amd.film_sampler as fs
import ray_tracer_s8_amd._sampler_lib as sl
assert "torch" not in sys.modules
assert not sl.BINDING.loaded                            # importing loads nothing
assert callable(fs.check_sampler) and callable(fs.FilmSampler.begin) and callable(fs.FilmSampler.render_pass)
assert callable(fs.FilmSampler.render) and callable(fs.FilmSampler.resolve_guided) and callable(fs.FilmSampler.variance)
assert sorted(sl.SIGNATURES) == sorted(%r)
fs.check_sampler(True)
assert "torch" not in sys.modules and not sl.BINDING.loaded
print("ok")
""" % (NAMES,)


def test_film_sampler_and_its_binding_import_without_torch():
    r = subprocess.run([sys.executable, "-c", _IMPORT_CHILD], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_abi_module_holds_nothing_of_the_sampler_library():
    names = [n for n in dir(_abi) if "rts_" in n.lower() or "sampler" in n.lower()]
    assert names == [], names


def test_the_binding_loads_the_library_and_refusals_are_statuses():
    """Loading binds no device: rts_version and rts_scratch_bytes are host arithmetic, and the others refuse before any launch."""
    from ray_tracer_s8_amd import _sampler_lib as sl
    lib = sl.load()
    inf, nan = float("inf"), float("nan")
    assert lib.rts_version(None) == 1
    v = C.c_uint32(0)
    assert lib.rts_version(C.byref(v)) == 0 and v.value == sl.RTS_VERSION
    # the scratch: two bytes a pixel, then one uint32 a workgroup of 256 strip indices, 8-byte aligned between
    n = C.c_uint64(0)
    assert lib.rts_scratch_bytes(50, 48, 16, C.byref(n)) == 0 and n.value == 2 * 50 * 48 + 4 * 3 * 4
    assert lib.rts_scratch_bytes(1, 1, 1, C.byref(n)) == 0 and n.value == 8 + 4
    assert sl.scratch_bytes(130, 70, 35) == 2 * 130 * 70 + 4 * 2 * 18
    for bad in ((0, 4, 2), (4, 0, 2), (4, 4, 0), (4, 4, 3), (4, 3, 4)):
        assert lib.rts_scratch_bytes(*bad, C.byref(n)) == 1, bad
    assert lib.rts_scratch_bytes(4, 4, 2, None) == 1
    assert lib.rts_scratch_bytes(1 << 16, 1 << 16, 1 << 16, C.byref(n)) == 2
    assert lib.rts_scratch_bytes(1, 1 << 20, 1, C.byref(n)) == 2                           # more strips than a grid has rows

    one, odd4, odd8 = C.c_void_p(64), C.c_void_p(66), C.c_void_p(68)     # (addresses never read: every call here is refused)
    need = sl.scratch_bytes(8, 4, 2)
    good = dict(W=8, R=4, Hs=2, dilate=1, threshold=0.1, eps=0.01, moments=one, counts=one, err=one, active=one, strip_counts=one,
                scratch=one, scratch_bytes=need)
    bad = [dict(W=0), dict(R=0), dict(Hs=0), dict(Hs=3), dict(R=3), dict(dilate=2), dict(reserved=1), dict(reserved2=1),
           dict(threshold=nan), dict(threshold=-0.5), dict(threshold=-inf), dict(eps=0.0), dict(eps=-1.0), dict(eps=inf), dict(eps=nan),
           dict(moments=None), dict(counts=None), dict(err=None), dict(active=None), dict(strip_counts=None), dict(scratch=None),
           dict(moments=odd8), dict(counts=odd4), dict(err=odd4), dict(active=odd4), dict(strip_counts=odd4), dict(scratch=odd8),
           dict(scratch_bytes=need - 1), dict(scratch_bytes=0), dict(W=1 << 16, R=1 << 16, Hs=1 << 16)]
    assert lib.rts_select(None, None) == 1
    for kw in bad:
        assert lib.rts_select(sl.SelectArgs(**{**good, **kw}), None) in (1, 2, 5), kw
    assert lib.rts_select(sl.SelectArgs(**{**good, "scratch_bytes": need - 1}), None) == 5

    a, b, c, d, e = (C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20), C.c_void_p(5 << 20))
    good = dict(n_active=3, k=2, pixels=16, active=a, rays=b, states=c, out_rays=d, out_states=e)
    bad = [dict(k=0), dict(pixels=0), dict(n_active=17), dict(reserved=1), dict(active=None), dict(active=odd4), dict(rays=None),
           dict(states=None), dict(out_rays=None), dict(out_states=None), dict(rays=C.c_void_p((2 << 20) + 8)),
           dict(out_states=C.c_void_p((5 << 20) + 4)),
           dict(out_rays=b), dict(out_states=c), dict(out_rays=c), dict(out_states=d),          # in place, or one buffer twice
           dict(out_rays=C.c_void_p((2 << 20) + 16 * 2 * 32 - 32)),                            # the last input record
           dict(pixels=1 << 30, k=2)]
    assert lib.rts_gather(None, None) == 1
    for kw in bad:
        assert lib.rts_gather(sl.GatherArgs(**{**good, **kw}), None) in (1, 2), kw
    assert lib.rts_gather(sl.GatherArgs(**{**good, "n_active": 0}), None) == 0                 # nothing to do: OK, and no launch

    good = dict(n_active=3, k=2, pixels=16, active=a, rgb=b, accum=c, moments=d, counts=e)
    bad = [dict(k=0), dict(pixels=0), dict(n_active=17), dict(reserved=1), dict(active=None), dict(rgb=None), dict(accum=None),
           dict(moments=None), dict(counts=None), dict(moments=C.c_void_p((4 << 20) + 4)), dict(accum=C.c_void_p((3 << 20) + 2)),
           dict(pixels=1 << 30, k=2)]
    assert lib.rts_fold(None, None) == 1
    for kw in bad:
        assert lib.rts_fold(sl.FoldArgs(**{**good, **kw}), None) in (1, 2), kw
    assert lib.rts_fold(sl.FoldArgs(**{**good, "n_active": 0}), None) == 0

    good = dict(W=8, R=4, e0=4, accum=a, moments=b, counts=c, out_accum=d, out_moments=e)
    bad = [dict(W=0), dict(R=0), dict(e0=0), dict(e0=1), dict(e0=(1 << 24) + 1), dict(reserved=1), dict(accum=None), dict(moments=None),
           dict(counts=None), dict(out_accum=None), dict(out_moments=None), dict(moments=C.c_void_p((2 << 20) + 4)),
           dict(out_moments=C.c_void_p((5 << 20) + 4)), dict(out_accum=a), dict(out_moments=b), dict(W=1 << 16, R=1 << 16)]
    assert lib.rts_normalise(None, None) == 1
    for kw in bad:
        assert lib.rts_normalise(sl.NormaliseArgs(**{**good, **kw}), None) in (1, 2), kw
    with pytest.raises(sl.RtsError):
        sl.check("rts_select", 5)
