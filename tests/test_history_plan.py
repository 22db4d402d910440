"""The film history without a GPU (ray_tracer_s8_amd/film_history.py, _history_lib.py, build.py):
1. check_history refuses, with ValueError, everything FilmHistory refuses, and accepts the rest;
2. film_history.py and _history_lib.py import without torch and without loading the history library;
3. rth_accumulate refuses bad arguments with a status, before any launch;
4. Film.reset(seed=...) sets the seed of the film's own requests, not the caller's.
What holds of every private library (a library of its own, its record, its exports, who builds it) is tests/test_private_libraries.py's.
Without the feature every test here fails: there is no film_history, no _history_lib and no build.HISTORY."""
import contextlib
import ctypes as C
import subprocess
import sys
import types
from pathlib import Path

import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

ROOT = Path(__file__).resolve().parent.parent


def test_check_history_accepts():
    from ray_tracer_s8_amd import film_history as fh
    assert fh.check_history(True) == (fh.ALPHA, float(fh.N_MAX), fh.K_DEPTH, None)
    assert fh.check_history(True, 1, 1, 0, 0) == (1.0, 1.0, 0.0, 0.0)
    assert fh.check_history(True, 0.05, 64, 0.5, 0.95) == (0.05, 64.0, 0.5, 0.95)
    assert 0 < fh.ALPHA <= 1 and fh.N_MAX >= 1 and fh.K_DEPTH >= 0
    assert rt.FilmHistory is fh.FilmHistory and "FilmHistory" in rt.__all__


def test_check_history_refuses():
    from ray_tracer_s8_amd import film_history as fh
    inf, nan = float("inf"), float("nan")
    bad = {
        "no moments": dict(moments=False),
        "alpha 0": dict(alpha=0.0),
        "alpha < 0": dict(alpha=-0.1),
        "alpha > 1": dict(alpha=1.5),
        "alpha nan": dict(alpha=nan),
        "alpha inf": dict(alpha=inf),
        "alpha a string": dict(alpha="0.2"),
        "alpha True": dict(alpha=True),
        "n_max 0": dict(n_max=0),
        "n_max 0.5": dict(n_max=0.5),
        "n_max inf": dict(n_max=inf),
        "n_max nan": dict(n_max=nan),
        "n_max None": dict(n_max=None),
        "k_depth < 0": dict(k_depth=-1.0),
        "k_depth nan": dict(k_depth=nan),
        "k_depth inf": dict(k_depth=inf),
        "k_normal < 0": dict(k_normal=-0.5),
        "k_normal nan": dict(k_normal=nan),
        "k_normal inf": dict(k_normal=inf),
        "k_normal a string": dict(k_normal="0.9"),
    }
    for what, kw in bad.items():
        args = dict(moments=True)
        args.update(kw)
        with pytest.raises(ValueError):
            fh.check_history(**args)
            pytest.fail(what)


def test_film_history_runs_its_checks_before_anything_else():
    """No film, a film without moments, bad constants: ValueError before torch or the library is touched."""
    plain = types.SimpleNamespace(moments=None)
    for film, kw in ((None, {}), (plain, {}), (types.SimpleNamespace(moments=object()), dict(alpha=0.0)),
                     (types.SimpleNamespace(moments=object()), dict(n_max=0))):
        with pytest.raises(ValueError):
            rt.FilmHistory(film, **kw)


_IMPORT_CHILD = r"""
import sys
import ray_tracer_s8_amd as rt
import ray_tracer_s8_amd.film_history as fh
import ray_tracer_s8_amd._history_lib as hl
assert "torch" not in sys.modules
assert not hl.BINDING.loaded                            # importing loads nothing
assert callable(fh.check_history) and callable(fh.FilmHistory.accumulate) and callable(fh.FilmHistory.resolve_guided)
assert sorted(hl.SIGNATURES) == ["rth_accumulate", "rth_version"]
fh.check_history(True)
assert "torch" not in sys.modules and not hl.BINDING.loaded
print("ok")
"""


def test_film_history_and_its_binding_import_without_torch():
    r = subprocess.run([sys.executable, "-c", _IMPORT_CHILD], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_abi_module_holds_nothing_of_the_history_library():
    names = [n for n in dir(_abi) if "rth" in n.lower() or "history" in n.lower()]
    assert names == [], names


def test_the_binding_loads_the_library_and_refusals_are_statuses():
    """Loading binds no device: rth_version is host arithmetic, and rth_accumulate refuses before any launch."""
    from ray_tracer_s8_amd import _history_lib as hl
    lib = hl.load()
    assert lib.rth_version(None) == 1
    assert lib.rth_accumulate(None, None) == 1
    rq = _abi.default_request(width=8, height=6, divisions=3, division_no=1, spp=4)
    one = C.c_void_p(8)                                   # (a non-null, 8-byte aligned address that is never read: every call is refused)
    planes = dict(accum=one, moments=one, depth=one, hits=one, index=one)
    state = hl.State(accum=one, moments=one, length=one, depth=one, index=one)
    good = dict(W=8, R=4, alpha=0.2, n_max=8.0, k_depth=0.1, request=C.pointer(rq), next=state, **planes)
    bad = [dict(W=0), dict(R=0), dict(R=3), dict(R=6), dict(W=7), dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float("nan")),
           dict(n_max=0.5), dict(n_max=float("inf")), dict(k_depth=-1.0), dict(k_normal=float("nan")), dict(reserved=1),
           dict(request=None), dict(accum=None), dict(hits=None), dict(moments=C.c_void_p(4)), dict(next=hl.State()),
           dict(normal=one),                                                      # with normals, the state needs a normal plane
           dict(have_prev=1),                                                     # no previous state or request
           dict(have_prev=1, prev=state, prev_request=C.pointer(rq)),             # reads what it writes
           dict(W=1 << 24, R=2)]
    for kw in bad:
        a = hl.AccumulateArgs(**{**good, **kw})
        assert lib.rth_accumulate(a, None) in (1, 2), kw
    cam = _abi.Camera.look_at((0, 0, 0), (0, 0, 0))                               # a pose make_pose refuses
    a = hl.AccumulateArgs(**good)
    a.camera = C.pointer(cam)
    assert lib.rth_accumulate(a, None) == 1
    with pytest.raises(hl.RthError):
        hl.check("rth_accumulate", 1)


def test_film_reset_with_a_seed_sets_the_films_requests_and_not_the_callers():
    """On a film put together without a device: reset() reads accum, moments, the stream and torch.cuda.stream only."""
    from ray_tracer_s8_amd import film as film_mod

    class Plane:
        zeroed = 0

        def zero_(self):
            self.zeroed += 1

    mine = [_abi.default_request(width=8, height=6, divisions=3, division_no=k, spp=4, seed=7) for k in range(3)]
    plan = film_mod.check_job(mine)
    film = film_mod.Film.__new__(film_mod.Film)
    film.accum, film.moments, film.stream, film.samples, film.reqs = Plane(), Plane(), None, 3, plan.reqs
    film._torch = types.SimpleNamespace(cuda=types.SimpleNamespace(stream=lambda s: contextlib.nullcontext()))
    film.reset()
    assert [r.seed for r in film.reqs] == [7, 7, 7] and film.samples == 0 and film.accum.zeroed == 1 and film.moments.zeroed == 1
    film.samples = 2
    film.reset(seed=0xDEADBEEF12345678)
    assert [r.seed for r in film.reqs] == [0xDEADBEEF12345678] * 3 and film.samples == 0 and film.accum.zeroed == 2
    assert [r.seed for r in mine] == [7, 7, 7]
    assert [r.division_no for r in film.reqs] == [0, 1, 2]
    for seed in (-1, 1 << 64, 1.5, "7", True):
        with pytest.raises(ValueError):
            film.reset(seed=seed)
        assert [r.seed for r in film.reqs] == [0xDEADBEEF12345678] * 3 and film.accum.zeroed == 2
