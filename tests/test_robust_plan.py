"""The robust film without a GPU (ray_tracer_s8_amd/film_robust.py, _robust_lib.py, build.py, film.py):
1. check_robust and check_estimate refuse, with ValueError, everything FilmRobust refuses; FilmRobust is in rt.__all__;
2. film_robust.py and _robust_lib.py import without torch and without loading the library;
3. the binding has the version, the status table and the modes of this library's header;
4. every refusal of the library's calls comes back as a status, with no device bound;
5. the film's tap: a film with no tap makes the calls it made before and no other, and a tap is shown every strip's sub-range after
   its fold, in order, and the reset after the film's own zeroing.
What holds of every private library (a library of its own, its record, its exports, who builds it) is tests/test_private_libraries.py's.
Without the feature every test here fails: there is no film_robust, no _robust_lib, no build.ROBUST and no Film._taps."""
import ctypes as C
import re
import subprocess
import sys
import types
from contextlib import contextmanager
from pathlib import Path

import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, build

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rtr_version", "rtr_fold", "rtr_resolve")


def test_check_robust():
    from ray_tracer_s8_amd import film_robust as fr
    assert rt.FilmRobust is fr.FilmRobust and "FilmRobust" in rt.__all__
    assert fr.check_robust(0) == (5, "gini", 0) and fr.BUCKETS == 5 and fr.MODES == ("gini", "trim")
    for K in (3, 5, 7, 9, 11, 13, 15):
        h = (K - 1) // 2
        assert fr.check_robust(0, K) == (K, "gini", 0)
        for c in range(h + 1):
            assert fr.check_robust(0, K, "trim", c) == (K, "trim", c)
    bad = {
        "even": dict(buckets=8), "1": dict(buckets=1), "17": dict(buckets=17), "0": dict(buckets=0), "-3": dict(buckets=-3),
        "a float": dict(buckets=9.0), "True": dict(buckets=True), "None": dict(buckets=None),
        "an unknown mode": dict(mode="median"), "mode None": dict(mode=None), "mode 0": dict(mode=0),
        "trim without c": dict(mode="trim"), "trim c = h + 1": dict(mode="trim", c=3), "trim c < 0": dict(mode="trim", c=-1),
        "trim c a float": dict(mode="trim", c=1.0), "trim c True": dict(mode="trim", c=True),
        "trim c beyond a small K": dict(buckets=3, mode="trim", c=2),
        "gini with c": dict(mode="gini", c=0), "gini with c = 2": dict(c=2), "trim c beyond K = 9": dict(buckets=9, mode="trim", c=5),
        "a film that holds samples": dict(samples=4), "samples None": dict(samples=None),
    }
    for what, kw in bad.items():
        args = dict(samples=0)
        args.update(kw)
        with pytest.raises(ValueError):
            fr.check_robust(**args)
            pytest.fail(what)


def test_check_estimate():
    from ray_tracer_s8_amd import film_robust as fr
    assert fr.OUTPUTS == ("linear", "gini", "kept", "variance")
    assert fr.check_estimate(9, 9, 9) == ("linear",)
    assert fr.check_estimate(20, 20, 9, ["kept", "gini"]) == ("kept", "gini")
    with pytest.raises(ValueError, match="needs one in each"):
        fr.check_estimate(8, 8, 9)
    with pytest.raises(ValueError, match="advanced while"):
        fr.check_estimate(12, 9, 9)
    for outs in ((), ("rgb",), ("linear", "linear"), ("accum",)):
        with pytest.raises(ValueError, match="outputs"):
            fr.check_estimate(9, 9, 9, outs)


def test_film_robust_runs_its_checks_before_anything_else():
    """Bad arguments, a film that holds samples: ValueError before torch or the library is touched."""
    from ray_tracer_s8_amd import _robust_lib
    loaded = _robust_lib.BINDING.loaded
    fresh, used = types.SimpleNamespace(samples=0), types.SimpleNamespace(samples=3)
    for film, kw in ((fresh, dict(buckets=4)), (fresh, dict(mode="trim")), (fresh, dict(c=1)), (fresh, dict(mode="x")),
                     (used, {}), (None, {})):
        with pytest.raises(ValueError):
            rt.FilmRobust(film, **kw)
    assert _robust_lib.BINDING.loaded is loaded


_IMPORT_CHILD = r"""
import sys
import ray_tracer_s8_amd as rt
import ray_tracer_s8_amd.film_robust as fr
import ray_tracer_s8_amd._robust_lib as rl
assert "torch" not in sys.modules
assert not rl.BINDING.loaded                            # importing loads nothing
assert callable(fr.check_robust) and callable(fr.FilmRobust.estimate) and callable(fr.FilmRobust.state)
assert all(callable(getattr(fr.FilmRobust, n)) for n in ("preview", "resolve", "resolve_guided", "variance", "close"))
assert sorted(rl.SIGNATURES) == sorted(%r)
assert fr.check_robust(0, 5, "trim", 2) == (5, "trim", 2)
assert "torch" not in sys.modules and not rl.BINDING.loaded
print("ok")
""" % (NAMES,)


def test_film_robust_and_its_binding_import_without_torch():
    r = subprocess.run([sys.executable, "-c", _IMPORT_CHILD], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_the_bindings_own_constants():
    from ray_tracer_s8_amd import _robust_lib
    assert _robust_lib.RTR_VERSION == 1 and set(_robust_lib.SIGNATURES) == set(NAMES)
    assert _robust_lib.STATUS == {1: "RTR_ERR_BAD_ARG", 2: "RTR_ERR_LIMIT", 3: "RTR_ERR_HIP", 4: "RTR_ERR_INTERNAL"}
    text = (build.ROBUST.src_dir / "rt_robust.h").read_text()
    modes = dict((n.lower(), int(v)) for n, v in re.findall(r"^#define RTR_(GINI|TRIM) (\d+)u", text, re.M))
    assert modes == _robust_lib.MODES
    assert (_robust_lib.MIN_BUCKETS, _robust_lib.MAX_BUCKETS) == (3, 15)


def test_the_binding_loads_the_library_and_refusals_are_statuses():
    """Loading binds no device: rtr_version is host arithmetic, and rtr_fold and rtr_resolve refuse before any launch."""
    from ray_tracer_s8_amd import _robust_lib as rl
    lib = rl.load()
    assert lib.rtr_version(None) == 1
    v = C.c_uint32(0)
    assert lib.rtr_version(C.byref(v)) == 0 and v.value == rl.RTR_VERSION
    assert lib.rtr_fold(None, None) == 1 and lib.rtr_resolve(None, None) == 1
    MB = 1 << 20
    at = lambda k: C.c_void_p(k * MB)                                 # (addresses never read: every call here is refused)

    def fold(**kw):
        # 185 pixels, 20 records each (44 400 bytes), into strip parts of 2 220 bytes 64 KB apart
        good = dict(pixels=185, n=20, first=3, K=9, bucket_stride=16384, records=at(1), buckets=at(2))
        good.update(kw)
        return lib.rtr_fold(rl.FoldArgs(**good), None)

    bad = [dict(pixels=0), dict(n=0), dict(K=0), dict(K=1), dict(K=2), dict(K=4), dict(K=8), dict(K=16), dict(K=17), dict(K=255),
           dict(records=None), dict(buckets=None), dict(records=C.c_void_p(MB + 2)), dict(buckets=C.c_void_p(2 * MB + 1)),
           dict(bucket_stride=0), dict(bucket_stride=3 * 185 - 1),
           # the records inside bucket 0's part, at its last byte, inside bucket 8's part; the buckets inside the records
           dict(records=at(2)), dict(records=C.c_void_p(2 * MB + 2216)), dict(records=C.c_void_p(2 * MB + 8 * 65536)),
           dict(buckets=C.c_void_p(MB + 44396)), dict(buckets=C.c_void_p(MB - 65536 * 3)), dict(records=C.c_void_p(2 * MB - 4))]
    for kw in bad:
        assert fold(**kw) == 1, kw
    # sizes beyond what the kernel indexes: more than 2^31 - 1 records, a stride beyond 2^40 floats
    assert fold(pixels=1 << 20, n=1 << 11, bucket_stride=3 << 20, records=at(1), buckets=C.c_void_p(1 << 44)) == 2
    assert fold(bucket_stride=(1 << 40) + 1) == 2

    def resolve(**kw):
        # 67 x 9 pixels: the buckets 65 124 bytes at K = 9, a three-float output 7 236
        good = dict(W=67, R=9, K=9, samples=20, mode=0, c=0, buckets=at(1), out_linear=at(2), out_gini=at(3), out_kept=at(4),
                    out_variance=at(5), out_accum=at(6), out_moments=at(7))
        good.update(kw)
        return lib.rtr_resolve(rl.ResolveArgs(**good), None)

    none = dict(out_linear=None, out_gini=None, out_kept=None, out_variance=None, out_accum=None, out_moments=None)
    bad = [dict(W=0), dict(R=0), dict(K=2), dict(K=4), dict(K=1), dict(K=17), dict(samples=8), dict(samples=0), dict(mode=2),
           dict(mode=0, c=1), dict(mode=1, c=5), dict(K=3, samples=3, mode=1, c=2), dict(buckets=None), none,
           dict(buckets=C.c_void_p(MB + 1)), dict(out_gini=C.c_void_p(3 * MB + 2)), dict(out_kept=C.c_void_p(4 * MB + 3)),
           # an output that is the buckets, ends inside them, begins at their last float; two outputs that overlap
           dict(out_linear=at(1)), dict(out_gini=C.c_void_p(MB - 4)), dict(out_moments=C.c_void_p(MB + 65120)),
           dict(out_accum=at(2)), dict(out_variance=C.c_void_p(2 * MB + 7232)), dict(out_kept=C.c_void_p(5 * MB - 2408))]
    for kw in bad:
        assert resolve(**kw) == 1, kw
    assert resolve(W=1 << 16, R=1 << 15) == 2                        # 2^31 pixels
    with pytest.raises(rl.RtrError):
        rl.check("rtr_resolve", 2)
    assert isinstance(rl.RtrError("x", 1), RuntimeError) and "RTR_ERR_BAD_ARG" in str(rl.RtrError("x", 1))


# ---- the tap, with stand-ins for torch, the scene and the tensors ---------------------------------------------------------------------
class _Tensor:
    """What render_pass and reset do with a tensor, logged: slices and views are tensors of the same name, and every call that would
    enqueue work is an entry of the log."""

    def __init__(self, log, name, shape=()):
        self.log, self.name, self.shape = log, name, tuple(shape)

    def __getitem__(self, key):
        return _Tensor(self.log, self.name, self.shape)

    def view(self, *shape):
        return _Tensor(self.log, self.name, shape)

    def data_ptr(self):
        return hash(self.name) & 0xFFFF0

    def add_(self, other):
        self.log.append(("add_", self.name, other.name))

    def zero_(self):
        self.log.append(("zero_", self.name))


def _fake_film(log, strips=2, moments=False):
    from ray_tracer_s8_amd.film import Film

    @contextmanager
    def on_stream(s):
        log.append(("stream", "enter"))
        yield
        log.append(("stream", "exit"))

    reqs = [_abi.default_request(width=8, height=6, divisions=3, division_no=k, spp=12) for k in range(strips)]
    scene = types.SimpleNamespace(
        camera_rays_device=lambda rq, b, e, rays, states, stream: log.append(("camera", rq.division_no, b, e)),
        trace_nee_device=lambda rays, n, rgb, **kw: log.append(("trace", n)),
        collect=lambda: log.append(("collect",)) or _abi.TileStats())
    film = Film.__new__(Film)
    film._torch = types.SimpleNamespace(cuda=types.SimpleNamespace(stream=on_stream))
    film.scene, film.reqs, film.integrator, film.mode, film.flags = scene, tuple(reqs), "nee", _abi.RT_NEE_MIS, 0
    film.hs, film.width, film.rows, film.spp, film.max_records = 2, 8, 2 * strips, 12, 16 * 5       # sub-ranges of 5 samples
    film.stream = types.SimpleNamespace(cuda_stream=0x1234)
    film._collect_at, film._uncollected, film._stats = 8192, 0, _abi.TileStats()
    film.samples = 0
    film.accum, film.moments = _Tensor(log, "accum"), (_Tensor(log, "moments") if moments else None)
    film._rays, film._states, film._rgb = _Tensor(log, "rays"), _Tensor(log, "states"), _Tensor(log, "rgb")
    film._fold_moments = lambda acc, mom, records: log.append(("fold_moments", records.shape))
    film._taps = []
    return film


class _Tap:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def _on_records(self, i, b, e, records):
        self.log.append(("tap", self.name, i, b, e, records.name, records.shape))

    def _on_reset(self):
        self.log.append(("tap reset", self.name))


@pytest.mark.parametrize("moments", (False, True))
def test_a_film_with_no_tap_makes_no_extra_call_and_a_tap_sees_every_sub_range_in_order(moments):
    from ray_tracer_s8_amd.film import Film
    assert Film.__init__.__code__.co_names.count("_taps") == 1                  # made by the constructor, empty
    plain, tapped = [], []
    film = _fake_film(plain, moments=moments)
    assert film._taps == []
    film.render_pass(0, 7)
    film.render_pass(7, 12)
    film.reset()
    # what the film did before the tap existed: per strip and sub-range the camera, the trace and the fold, and nothing else
    chunks = [(0, 5), (5, 7), (7, 12)]
    want = []
    for lo, hi in ((0, 7), (7, 12)):
        want.append(("stream", "enter"))
        for i in range(2):
            for b, e in (c for c in chunks if lo <= c[0] < hi):
                want += [("camera", i, b, e), ("trace", 16 * (e - b))]
                want += [("fold_moments", (16, e - b, 3))] if moments else [("add_", "accum", "rgb")] * (e - b)
        want.append(("stream", "exit"))
    want += [("stream", "enter"), ("zero_", "accum")] + ([("zero_", "moments")] if moments else []) + [("stream", "exit")]
    assert plain == want
    # with two taps: the same calls, and after every fold both taps in their order; after the film's zeroing both resets
    film = _fake_film(tapped, moments=moments)
    film._taps += [_Tap(tapped, "a"), _Tap(tapped, "b")]
    film.render_pass(0, 7)
    film.render_pass(7, 12)
    film.reset()
    assert [x for x in tapped if not x[0].startswith("tap")] == plain
    seen = [x for x in tapped if x[0] == "tap"]
    order = [(i, b, e) for lo, hi in ((0, 7), (7, 12)) for i in range(2) for b, e in chunks if lo <= b < hi]
    assert seen == [("tap", n, i, b, e, "rgb", (16, e - b, 3)) for i, b, e in order for n in "ab"]
    fold = ("fold_moments",) if moments else ("add_", "accum", "rgb")
    for k, x in enumerate(tapped):
        if x[0] == "tap" and x[1] == "a":
            assert tapped[k - 1][:len(fold)] == fold and tapped[k + 1][:2] == ("tap", "b")      # directly after the fold
    tail = tapped[-4:] if not moments else tapped[-5:]
    assert tail[-3:] == [("tap reset", "a"), ("tap reset", "b"), ("stream", "exit")] and tail[0][0] == "zero_"
    assert film.samples == 0
