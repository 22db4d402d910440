"""The film's regression resolve without a GPU (ray_tracer_s8_amd/film.py, _film_lib.py, film_csrc/rt_film.h):
1. check_regression refuses, with ValueError, everything resolve_regression refuses, and accepts the rest; regression_nodes;
2. film.py and _film_lib.py import without torch and without loading the film library;
3. the film library is version 2 in the header and in the binding, and the binding's ResolveArgs has the header's fields in the
   header's order;
4. with a NULL stream and no device, every refusal of a kind-1 call comes back as its status, a kind-0 call with an appended field
   set is refused, and an unknown kind is.
Without the feature every test here fails: there is no check_regression, and rtf_resolve_args has no kind."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "ray_tracer_s8_amd" / "film_csrc" / "rt_film.h"


def test_check_regression_accepts():
    from ray_tracer_s8_amd import film
    assert film.check_regression(1) == ((), ("rgb",))
    assert film.check_regression(8, ("hits", "index", "normal", "depth", "albedo"), ("f32", "rgb", "linear"), 1e-4, 0.5) == \
        (("albedo", "normal", "depth", "hits"), ("f32", "rgb", "linear"))
    assert film.check_regression(2, ["albedo"], ["linear"], ridge=1)[0] == ("albedo",)
    assert film.check_regression(2, ("hits",), albedo_eps=None)[0] == ("hits",)
    assert film.REGRESSION_OUTPUTS == ("rgb", "linear", "f32") and film.REGRESSION_RECORD == 32
    assert isinstance(film.RIDGE, float) and film.check_regression(1, ridge=film.RIDGE)


def test_check_regression_refuses():
    from ray_tracer_s8_amd import film
    inf, nan = float("inf"), float("nan")
    bad = {
        "no samples": dict(samples=0),
        "samples -1": dict(samples=-1),
        "samples 2.0": dict(samples=2.0),
        "unknown output": dict(outputs=("rgb", "png")),
        "variance": dict(outputs=("variance",)),
        "no output": dict(outputs=()),
        "repeated output": dict(outputs=("rgb", "rgb")),
        "unknown plane": dict(planes=("colour",)),
        "depth without hits": dict(planes=("normal", "depth")),
        "ridge 0": dict(ridge=0.0),
        "ridge < 0": dict(ridge=-1e-3),
        "ridge inf": dict(ridge=inf),
        "ridge nan": dict(ridge=nan),
        "ridge 0 as f32": dict(ridge=1e-60),
        "ridge inf as f32": dict(ridge=1e39),
        "ridge a string": dict(ridge="1e-3"),
        "ridge None": dict(ridge=None),
        "ridge True": dict(ridge=True),
        "albedo_eps 0": dict(albedo_eps=0.0),
        "albedo_eps < 0": dict(albedo_eps=-1.0),
        "albedo_eps nan": dict(albedo_eps=nan),
        "albedo_eps inf": dict(albedo_eps=inf),
    }
    for what, kw in bad.items():
        args = dict(samples=8)
        args.update(kw)
        with pytest.raises(ValueError):
            film.check_regression(**args)
            pytest.fail(what)


def test_regression_nodes():
    from ray_tracer_s8_amd import film
    want = {1: 2, 16: 2, 17: 3, 32: 3, 33: 4, 3840: 241}
    for W, nx in want.items():
        assert film.regression_nodes(W, 1) == (2, nx) and film.regression_nodes(1, W) == (nx, 2), W
    assert film.regression_nodes(1920, 1080) == (69, 121)
    for W, R in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError):
            film.regression_nodes(W, R)


_IMPORT_CHILD = r"""
import sys
import ray_tracer_s8_amd as rt
import ray_tracer_s8_amd.film as film
import ray_tracer_s8_amd._film_lib as fl
assert "torch" not in sys.modules
assert not fl.BINDING.loaded                            # importing loads nothing
assert callable(film.check_regression) and callable(film.regression_nodes) and callable(film.Film.resolve_regression)
assert fl.RTF_VERSION == 2 and (fl.RESOLVE_ATROUS, fl.RESOLVE_REGRESS) == (0, 1) and fl.REGRESS_RECORD == 32
film.check_regression(1)
assert "torch" not in sys.modules and not fl.BINDING.loaded
print("ok")
"""


def test_film_and_its_binding_import_without_torch():
    r = subprocess.run([sys.executable, "-c", _IMPORT_CHILD], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_version_two_in_the_header_and_the_binding():
    from ray_tracer_s8_amd import _film_lib
    text = HEADER.read_text()
    assert re.search(r"^#define RTF_VERSION 2u$", text, re.M) and _film_lib.RTF_VERSION == 2 and _film_lib.BINDING.version == 2
    assert re.search(r"^#define RTF_RESOLVE_ATROUS 0u", text, re.M) and re.search(r"^#define RTF_RESOLVE_REGRESS 1u", text, re.M)
    assert re.search(r"^#define RTF_REGRESS_RECORD 32u", text, re.M)
    v = C.c_uint32(0)
    assert _film_lib.load().rtf_version(C.byref(v)) == 0 and v.value == 2


_CTYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}


def test_the_struct_mirror_follows_the_header():
    from ray_tracer_s8_amd import _film_lib
    text = HEADER.read_text()
    body = re.search(r"typedef struct rtf_resolve_args \{(.*?)\} rtf_resolve_args;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.fullmatch(r"(const\s+)?(\w+)(\s*\*)?\s+([\w\s,]+)", decl)
        assert m, decl
        ctype = C.c_void_p if m.group(3) else _CTYPES[m.group(2)]
        fields += [(n.strip(), ctype) for n in m.group(4).split(",")]
    assert fields == list(_film_lib.ResolveArgs._fields_)
    names = [n for n, _ in fields]
    assert names[5] == "kind" and names[names.index("out_variance") + 1:] == ["albedo", "aov_samples", "albedo_eps", "ridge", "reserved",
                                                                             "model", "model_bytes"]


def _kind1(**kw):
    """A kind-1 call that passes every check (the pointers are never followed: a refusal comes before any launch, and the one call
    that would launch is not made)."""
    from ray_tracer_s8_amd import _film_lib
    args = dict(W=33, R=47, samples=1, kind=_film_lib.RESOLVE_REGRESS, accum=0x1000, out_rgb=0x2000, ridge=1e-3, model=0x3000,
                model_bytes=4 * 4 * 128)
    args.update(kw)
    return _film_lib.ResolveArgs(**args)


def test_refusals_of_a_kind_1_call_are_statuses():
    from ray_tracer_s8_amd import _film_lib
    lib = _film_lib.load()
    inf, nan = float("inf"), float("nan")
    BAD, SCRATCH = 1, 3
    cases = {
        "no samples": (dict(samples=0), BAD),
        "iterations": (dict(iterations=1), BAD),
        "out_variance": (dict(out_variance=0x4000), BAD),
        "no output": (dict(out_rgb=None), BAD),
        "no accum": (dict(accum=None), BAD),
        "no model": (dict(model=None), BAD),
        "model misaligned": (dict(model=0x3008), BAD),
        "model_bytes short": (dict(model_bytes=4 * 4 * 128 - 1), SCRATCH),
        "model_bytes 0": (dict(model_bytes=0), SCRATCH),
        "ridge 0": (dict(ridge=0.0), BAD),
        "ridge < 0": (dict(ridge=-1.0), BAD),
        "ridge inf": (dict(ridge=inf), BAD),
        "ridge nan": (dict(ridge=nan), BAD),
        "depth without hits": (dict(depth=0x5000, aov_samples=1), BAD),
        "albedo without aov_samples": (dict(albedo=0x5000, albedo_eps=0.5), BAD),
        "albedo with albedo_eps 0": (dict(albedo=0x5000, aov_samples=1), BAD),
        "albedo with albedo_eps inf": (dict(albedo=0x5000, aov_samples=1, albedo_eps=inf), BAD),
        "albedo with albedo_eps nan": (dict(albedo=0x5000, aov_samples=1, albedo_eps=nan), BAD),
        "normal without aov_samples": (dict(normal=0x5000), BAD),
        "hits without aov_samples": (dict(hits=0x5000), BAD),
        "reserved": (dict(reserved=1), BAD),
        "W 0": (dict(W=0), BAD),
        "an image beyond the limit": (dict(W=1 << 30, R=1), 2),
    }
    for what, (kw, status) in cases.items():
        assert lib.rtf_resolve(_kind1(**kw), None) == status, what
    # other outputs alone pass the output check: the next refusal is reached
    for o in ("out_f32", "out_linear"):
        assert lib.rtf_resolve(_kind1(out_rgb=None, model_bytes=0, **{o: 0x2000}), None) == SCRATCH, o
    assert lib.rtf_resolve(_kind1(kind=2), None) == BAD and lib.rtf_resolve(_kind1(kind=0xFFFFFFFF), None) == BAD
    with pytest.raises(_film_lib.RtfError):
        _film_lib.check("rtf_resolve", lib.rtf_resolve(_kind1(model_bytes=0), None))


def test_a_kind_0_call_takes_no_appended_field():
    from ray_tracer_s8_amd import _film_lib
    lib = _film_lib.load()
    # a kind-0 call that is refused only for its scratch: every check before it passes
    base = dict(W=4, R=4, samples=2, var_eps=2.0 ** -8, accum=0x1000, moments=0x2000, scratch=0x3000, scratch_bytes=0, out_rgb=0x4000)
    assert lib.rtf_resolve(_film_lib.ResolveArgs(**base), None) == 3
    appended = dict(albedo=0x5000, aov_samples=1, albedo_eps=0.5, ridge=1e-3, reserved=1, model=0x6000, model_bytes=128)
    for name, v in appended.items():
        assert lib.rtf_resolve(_film_lib.ResolveArgs(**base, **{name: v}), None) == 1, name
    # ... and what the existing callers pass still gets what it got
    assert lib.rtf_resolve(_film_lib.ResolveArgs(W=4, R=4, samples=1), None) == 1
    assert lib.rtf_resolve(None, None) == 1
