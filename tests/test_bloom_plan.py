"""The bloom without a GPU (ray_tracer_s8_amd/film_bloom.py, _bloom_lib.py, build.py):
1. check_bloom refuses, with ValueError, everything FilmBloom refuses; FilmBloom is in rt.__all__ and runs its checks first;
   level_shapes, default_levels and the scratch layout, which is the library's rtb_scratch_bytes and the restatement's;
2. what tests/test_private_libraries.py states of the six members of build.PRIVATE, stated of build.BLOOM, which is held beside them as
   build.JPEG is: a library of its own, its dependencies exactly, the golden record, exports equal to SIGNATURES and all rtb_*, the
   header declaring exactly those functions, the prefix in no other source directory and no other library's prefix in this one, who
   builds it, and a binding that imports without torch and loads nothing;
3. every refusal of the library's calls comes back as a status, with no device bound and addresses that are never read.
Without the feature every test here fails at the import of _bloom_lib."""
import ctypes as C
import re
import subprocess
import sys
import types
from pathlib import Path

import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, _bloom_lib as bl, build

import _bloom_np as bnp
import _surface

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden" / "build_records"
NAMES = ("rtb_version", "rtb_scratch_bytes", "rtb_apply")
OTHERS = {"s8": build.PRODUCT, "s8_dbg": build.DEBUG, **build.PRIVATE, "jpeg": build.JPEG}


# ---- 1. the checks ---------------------------------------------------------------------------------------------------------------------
def test_check_bloom():
    from ray_tracer_s8_amd import film_bloom as fb
    assert rt.FilmBloom is fb.FilmBloom and "FilmBloom" in rt.__all__
    assert fb.check_bloom((1080, 1920)) == ((1080, 1920), 8, 0.7, 0.05, "mix", 0.0, 0.5, 65536.0)
    assert fb.check_bloom([19, 67], 2, 1.0, 7.5, "add", 2.0, 1.0, 2.0) == ((19, 67), 2, 1.0, 7.5, "add", 2.0, 1.0, 2.0)
    assert fb.check_bloom((36, 64), cap=2.0 ** 62).cap == 2.0 ** 62 and fb.check_bloom((36, 64), knee=0).knee == 0.0
    assert fb.FORM in bl.FORMS and fb.MODES == tuple(bl.MODES) and fb.OUTPUTS == ("linear", "bloom")
    bad = {
        "no shape": dict(shape=None), "a flat shape": dict(shape=(64,)), "three": dict(shape=(36, 64, 3)), "zero rows": dict(shape=(0, 64)),
        "negative": dict(shape=(36, -1)), "float sizes": dict(shape=(36.0, 64)), "bool sizes": dict(shape=(True, 64)),
        "2^31 pixels": dict(shape=(65536, 32768)),
        "levels 0": dict(levels=0), "levels 9": dict(levels=9), "levels 2.0": dict(levels=2.0), "levels True": dict(levels=True),
        "levels a string": dict(levels="8"),
        "spread 0": dict(spread=0.0), "spread 1.5": dict(spread=1.5), "spread nan": dict(spread=float("nan")), "spread None": dict(spread=None),
        "spread negative": dict(spread=-0.5), "spread a string": dict(spread="0.7"), "spread 1e-60": dict(spread=1e-60),
        "strength 0": dict(strength=0.0), "strength 1 under mix": dict(strength=1.0), "strength 2 under mix": dict(strength=2.0),
        "strength inf under add": dict(mode="add", strength=float("inf")), "strength 1e39 under add": dict(mode="add", strength=1e39),
        "strength nan": dict(strength=float("nan")), "strength True": dict(strength=True), "strength negative": dict(mode="add", strength=-1.0),
        "mode": dict(mode="screen"), "mode 0": dict(mode=0), "mode None": dict(mode=None),
        "threshold negative": dict(threshold=-0.1), "threshold inf": dict(threshold=float("inf")), "threshold nan": dict(threshold=float("nan")),
        "threshold above the cap": dict(threshold=2.0, cap=1.0), "threshold None": dict(threshold=None),
        "knee negative": dict(knee=-0.1), "knee 1.5": dict(knee=1.5), "knee nan": dict(knee=float("nan")), "knee a string": dict(knee="0.5"),
        "cap 0": dict(cap=0.0), "cap negative": dict(cap=-1.0), "cap inf": dict(cap=float("inf")), "cap nan": dict(cap=float("nan")),
        "cap 2^63": dict(cap=2.0 ** 63), "cap None": dict(cap=None),
    }
    for what, kw in bad.items():
        args = dict(shape=(36, 64))
        args.update(kw)
        with pytest.raises(ValueError):
            fb.check_bloom(**args)
            pytest.fail(what)
    assert fb.check_outputs() == ("linear",) and fb.check_outputs(["linear", "bloom"]) == ("linear", "bloom")
    for outs in ((), ("bloom",), ("linear", "linear"), ("linear", "rgb")):
        with pytest.raises(ValueError):
            fb.check_outputs(outs)


def test_film_bloom_runs_its_checks_before_anything_else():
    """Bad arguments: ValueError before the film, torch or the library is touched."""
    loaded = bl.BINDING.loaded
    film = types.SimpleNamespace(rows=36, width=64)                     # (no _check_open, no _torch: touching either would raise)
    for kw in (dict(levels=0), dict(spread=0.0), dict(shape=(0, 3)), dict(strength=1.0), dict(mode="screen"), dict(cap=0.0), dict(knee=2.0),
               dict(threshold=-1.0)):
        with pytest.raises(ValueError):
            rt.FilmBloom(film, **kw)
    with pytest.raises(ValueError):
        rt.FilmBloom(types.SimpleNamespace())                          # no shape to take from the film
    assert bl.BINDING.loaded is loaded


def test_level_shapes_and_the_scratch():
    from ray_tracer_s8_amd import film_bloom as fb
    assert fb.level_shapes((1080, 1920), 8) == ((1080, 1920), (540, 960), (270, 480), (135, 240), (68, 120), (34, 60), (17, 30), (9, 15), (5, 8))
    assert fb.level_shapes((1, 1), 8) == ((1, 1),) * 9 and fb.level_shapes((2, 3), 2) == ((2, 3), (1, 2), (1, 1))
    assert fb.level_shapes([5, 37], 3) == ((5, 37), (3, 19), (2, 10), (1, 5))
    for shape, want in (((1, 1), 1), ((1, 500), 1), ((2, 3), 1), ((3, 2), 1), ((4, 4), 2), ((5, 37), 2), ((36, 64), 5), ((255, 999), 7),
                        ((256, 999), 8), ((1080, 1920), 8), ((2160, 3840), 8)):
        assert fb.default_levels(shape) == want == bnp.default_levels(shape) and fb.check_bloom(shape).levels == want, shape
    for bad in (0, 9, 1.0, None, True):
        with pytest.raises(ValueError):
            fb.level_shapes((36, 64), bad)
    with pytest.raises(ValueError):
        fb.level_shapes((36, 0), 2)
    lib = bl.load()
    n = C.c_uint64(0)
    for shape, _ in bnp.SHAPES + [((1080, 1920), 8), ((7, 1), 1)]:
        for levels in range(1, 9):
            assert list(fb.level_shapes(shape, levels)) == bnp.level_shapes(shape, levels)
            offsets, size = fb.scratch_layout(shape, levels)
            assert (list(offsets), size) == bnp.scratch_layout(shape, levels) and all(o % 16 == 0 for o in offsets)
            assert lib.rtb_scratch_bytes(shape[1], shape[0], levels, C.byref(n)) == 0 and n.value == size, (shape, levels)
    assert fb.scratch_layout((1080, 1920), 8)[1] == 8295440
    # norm and K are the restatement's
    for spread in (0.7, 1.0, 0.3, 1e-3):
        for levels in range(1, 9):
            assert bl.norm_of(spread, levels) == float(bnp.norm_of(spread, levels))
    assert bl.norm_of(1.0, 4) == 0.25 and bl.norm_of(0.5, 1) == 1.0
    assert bl.knee_of(0.3, 0.7) == float(bnp.knee_of(0.3, 0.7)) and bl.knee_of(1.0, 0.5) == 0.5


# ---- 2. the registry -------------------------------------------------------------------------------------------------------------------
def test_a_library_of_its_own_beside_the_registry():
    lib = build.BLOOM
    assert isinstance(lib, build.Library) and lib not in build.PRIVATE.values() and "bloom" not in build.PRIVATE and lib is not build.JPEG
    assert bl.BINDING.library is lib and bl.BINDING.prefix == "rtb"
    assert lib.path == build.LIB_DIR / "librt_bloom.so" and lib.obj_dir == build.LIB_DIR / "obj_bloom"
    assert lib.units == (("rt_bloom.hip", ()),) and (lib.src_dir / "rt_bloom.hip").is_file() and lib.extra == ("-fno-slp-vectorize",)
    own = {"rt_bloom.h", "rt_bloom_math.h", "rt_bloom.hip.h"}
    assert own == {f.name for f in lib.src_dir.iterdir() if f.suffix == ".h"}
    assert lib.src_dir == build.PKG / "bloom_csrc" and lib.src_dir.is_dir() and build.CSRC not in lib.src_dir.parents
    assert lib.include_dirs == (build.INCLUDE, build.CSRC, lib.src_dir, build.PRIVATE_CSRC)
    for other in OTHERS.values():
        assert other.path != lib.path and other.obj_dir != lib.obj_dir and other.src_dir != lib.src_dir and other.record_path != lib.record_path
    # its dependencies, exactly: no csrc/ header
    deps = build.dep_files(lib)
    assert len(deps) == len(set(deps)) and all(d.is_file() for d in deps)
    assert set(deps) == {*(f for f in lib.src_dir.rglob("*") if f.is_file()), build.PRIVATE_CSRC / "rt_private_host.h",
                         build.ROOT / "include" / "rt_tile.h", Path(build.__file__)}
    assert not [d for d in deps if build.CSRC in d.parents]
    # ... are what its sources include
    included = set()
    for f in lib.src_dir.iterdir():
        included |= set(re.findall(r'^#include "([\w.]+)"', f.read_text(), re.M))
    assert included == own | {"rt_private_host.h"}
    # no other library depends on its directory or is named in its record, and it on no other private directory
    for name, other in OTHERS.items():
        assert not [f for f in build.dep_files(other) if lib.src_dir in f.parents], name
        assert "rt_bloom" not in build.record(other), name
        if other.src_dir != build.CSRC:
            assert not [f for f in deps if other.src_dir in f.parents], name
            assert f"rt_{name}" not in build.record(lib)
    assert "rt_bloom" not in build.flags_record()


def test_the_record_is_the_golden_one_and_the_products_flags(monkeypatch):
    lib = build.BLOOM
    golden = (GOLDEN / "bloom.flags").read_text()
    assert build.record(lib) == golden and golden.startswith("rt_bloom.hip: ") and golden.count("\n") == 1
    flags = golden.split(": ", 1)[1].split()
    assert flags == [f for f in build.HIPCC_FLAGS if f != "-shared"] + ["-fno-slp-vectorize"]
    monkeypatch.setenv("RT_EXTRA_HIPCC_FLAGS", "-DRT_PROFILE_TIME")      # never the experiments' flags, which are the product's
    assert "-DRT_PROFILE_TIME" in build.flags_record() and build.record(lib) == golden
    monkeypatch.delenv("RT_EXTRA_HIPCC_FLAGS")
    path = build.ensure(lib)
    assert path == lib.path and path.exists() and not build.stale(lib) and lib.record_path.read_text() == golden


def test_exports():
    _abi.load()
    _abi.load_debug()
    mine = {s for s in _surface.all_exported(build.ensure(build.BLOOM)) if not s.startswith("_")}
    assert mine == set(bl.SIGNATURES) == set(NAMES) and all(s.startswith("rtb_") for s in mine), mine
    assert not _surface.exported(build.BLOOM.path)                      # nothing of the tile ABI
    for name, other in OTHERS.items():
        symbols = _surface.all_exported(build.ensure(other) if name in build.PRIVATE or name == "jpeg" else other.path)
        assert not [s for s in symbols if "rtb_" in s], name
    # the private header declares exactly the functions the binding names, the version and the statuses the binding expects
    text = (build.BLOOM.src_dir / "rt_bloom.h").read_text()
    assert set(re.findall(r"^int (rtb_\w+)\(", text, re.M)) == set(bl.SIGNATURES)
    assert re.search(r"^#define RTB_VERSION (\d+)u$", text, re.M).group(1) == str(bl.RTB_VERSION) == "1" and bl.BINDING.version == 1
    assert re.search(r"^#define RTB_OK 0$", text, re.M) and bl.RTB_OK == 0
    status = dict((int(v), n) for n, v in re.findall(r"^#define (RTB_ERR_\w+) (\d+)", text, re.M))
    assert status == bl.STATUS == {1: "RTB_ERR_BAD_ARG", 2: "RTB_ERR_LIMIT", 3: "RTB_ERR_HIP", 4: "RTB_ERR_INTERNAL"}
    assert bl.RtbError is bl.BINDING.Error and bl.RtbError.STATUS == bl.STATUS and issubclass(bl.RtbError, RuntimeError)
    named = dict((n, int(v)) for n, v in re.findall(r"^#define RTB_(MAX_LEVELS|MIX|ADD|FORM_LEVELS|FORM_TAIL) (\d+)u", text, re.M))
    assert named == dict(MAX_LEVELS=bl.MAX_LEVELS, MIX=bl.MODES["mix"], ADD=bl.MODES["add"], FORM_LEVELS=bl.FORMS["levels"],
                         FORM_TAIL=bl.FORMS["tail"])
    assert (bnp.MIX, bnp.ADD, bnp.LEVELS, bnp.TAIL, bnp.MAX_LEVELS) == (0, 1, 0, 1, 8)
    # the struct is the header's, field for field
    body = re.search(r"typedef struct rtb_apply_args \{(.*?)\} rtb_apply_args;", text, re.S).group(1)
    fields = [n for line in body.splitlines() for n in re.findall(r"(\w+)[,;]", line.split("/*")[0])]
    assert fields == [{"inp": "in"}.get(n, n) for n, _ in bl.ApplyArgs._fields_] and C.sizeof(bl.ApplyArgs) == 88
    assert not (ROOT / "include" / "rt_bloom.h").exists()


def test_the_prefix_is_in_no_other_source_directory():
    dirs = [build.CSRC, build.PRIVATE_CSRC, ROOT / "include", build.JPEG.src_dir, *(lib.src_dir for lib in build.PRIVATE.values())]
    assert not {f for d in dirs for f in d.rglob("*") if f.is_file() and "rtb_" in f.read_text().lower()}
    # and the other prefixes are not in this one
    for prefix in ("rtf", "rth", "rts", "rtu", "rtr", "rtd", "rtj"):
        assert not {f for f in build.BLOOM.src_dir.rglob("*") if f.is_file() and prefix + "_" in f.read_text().lower()}, prefix


def test_who_builds(monkeypatch):
    """build() is the six and the product, as before; the driver's build() forces the bloom library after the JPEG library and before
    the oracle; `python -m ray_tracer_s8_amd.build` names it; the binding builds a missing one."""
    asked = []
    monkeypatch.setattr(build, "ensure", lambda lib, force=False, verbose=False: asked.append(lib.path) or lib.path)
    build.build()
    assert asked == [*(lib.path for lib in build.PRIVATE.values()), build.LIB_PATH] and build.BLOOM.path not in asked
    monkeypatch.undo()
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert entry.index("hip_build.build(force=True)") < entry.index("hip_build.build_debug(force=True)") \
        < entry.index("hip_build.ensure(hip_build.JPEG, force=True)") < entry.index("hip_build.ensure(hip_build.BLOOM, force=True)") \
        < entry.index("orc.build(")
    lines = entry.splitlines()
    at = lambda text: next(i for i, line in enumerate(lines) if text in line)
    assert at("hip_build.JPEG") < at("hip_build.BLOOM") < at("orc.build(")
    main = Path(build.__file__).read_text().split('if __name__ == "__main__":')[1]
    assert "BLOOM" in main and "JPEG" in main
    from ray_tracer_s8_amd import _private_lib
    assert "_bloom_lib.py" in _private_lib.__doc__
    path = build.ensure(build.BLOOM)
    missing = types.SimpleNamespace(path=ROOT / "no_such_dir" / "librt_bloom.so")
    built = []
    monkeypatch.setattr(build, "ensure", lambda lib, force=False, verbose=False: built.append(lib) or path)
    b = _private_lib.Binding(missing, "rtb", bl.RTB_VERSION, bl.STATUS, bl.SIGNATURES)
    b.load()
    assert built == [missing] and b.loaded


_IMPORT_CHILD = r"""
import sys
import ray_tracer_s8_amd as rt
import ray_tracer_s8_amd.film_bloom as fb
import ray_tracer_s8_amd._bloom_lib as m
assert "torch" not in sys.modules
assert m.BINDING.loaded is False                        # importing loads nothing
assert callable(m.load) and callable(m.check) and issubclass(m.RtbError, RuntimeError)
assert sorted(m.SIGNATURES) == sorted(%r) and "rtb_version" in m.SIGNATURES
try:
    m.check("x", 1)
except m.RtbError as e:
    assert e.status == 1 and str(e) == "x: " + m.STATUS[1]
else:
    raise AssertionError("check(1) did not raise")
m.check("x", 0)
assert rt.FilmBloom is fb.FilmBloom and fb.check_bloom((19, 67)).levels == 4 and fb.level_shapes((19, 67), 1) == ((19, 67), (10, 34))
assert all(callable(getattr(fb.FilmBloom, n)) for n in ("apply", "close"))
assert "defaults are aesthetic settings, not tuned results" in fb.FilmBloom.__doc__
assert "torch" not in sys.modules and m.BINDING.loaded is False
print("ok")
""" % (NAMES,)


def test_the_binding_and_the_module_import_without_torch_and_load_nothing():
    r = subprocess.run([sys.executable, "-c", _IMPORT_CHILD], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_are_statuses():
    """Loading binds no device: rtb_version and rtb_scratch_bytes are host arithmetic, and rtb_apply refuses before any launch."""
    lib = bl.load()
    assert lib.rtb_version(None) == 1
    v = C.c_uint32(0)
    assert lib.rtb_version(C.byref(v)) == 0 and v.value == bl.RTB_VERSION
    n = C.c_uint64(0)
    assert lib.rtb_scratch_bytes(67, 19, 3, None) == 1
    for W, R, levels in ((0, 19, 3), (67, 0, 3), (67, 19, 0), (67, 19, 9)):
        assert lib.rtb_scratch_bytes(W, R, levels, C.byref(n)) == 1, (W, R, levels)
    assert lib.rtb_scratch_bytes(65536, 32768, 3, C.byref(n)) == 2           # 2^31 pixels
    assert lib.rtb_scratch_bytes(65536, 32767, 8, C.byref(n)) == 0 and n.value == bnp.scratch_layout((32767, 65536), 8)[1]
    assert lib.rtb_scratch_bytes(67, 19, 3, C.byref(n)) == 0
    need = n.value
    assert need == bnp.scratch_layout((19, 67), 3)[1] == 4080 + 1024 + 336

    MB = 1 << 20
    at = lambda k: k * MB                                            # (addresses never read: every call here is refused)

    def apply(**kw):
        # 67 x 19: an image is 15 276 bytes, the scratch 5 440
        good = dict(W=67, R=19, levels=3, mode=0, form=0, spread=0.7, strength=0.05, norm=0.4, cap=65536.0, T=0.0, K=0.0, inp=at(1), out=at(2),
                    out_bloom=at(3), scratch=at(4), scratch_bytes=need)
        good.update(kw)
        return lib.rtb_apply(bl.ApplyArgs(**good), None)

    assert lib.rtb_apply(None, None) == 1
    inf, nan = float("inf"), float("nan")
    bad = [dict(W=0), dict(R=0), dict(levels=0), dict(levels=9), dict(mode=2), dict(form=2), dict(reserved=1),
           dict(spread=0.0), dict(spread=1.5), dict(spread=nan), dict(spread=-1.0),
           dict(strength=0.0), dict(strength=1.0), dict(strength=nan), dict(mode=1, strength=inf), dict(mode=1, strength=0.0), dict(mode=1, strength=-2.0),
           dict(norm=0.0), dict(norm=inf), dict(norm=nan),
           dict(cap=0.0), dict(cap=-1.0), dict(cap=inf), dict(cap=nan), dict(cap=2.0 ** 63),
           dict(T=-1.0), dict(T=inf), dict(T=nan), dict(T=1.0, K=2.0), dict(T=1.0, K=nan), dict(T=1.0, K=-0.5), dict(cap=1.0, T=2.0),
           dict(inp=None), dict(out=None), dict(scratch=None),
           dict(inp=at(1) + 4), dict(out=at(2) + 8), dict(out_bloom=at(3) + 4), dict(scratch=at(4) + 12),
           dict(scratch_bytes=need - 1), dict(scratch_bytes=0),
           # the output in the input, at its last bytes; the bloom in the output; the scratch in each; each reaching the next
           dict(out=at(1)), dict(out=at(1) + 15264), dict(out_bloom=at(2)), dict(out_bloom=at(1) + 16), dict(scratch=at(1)), dict(scratch=at(2) + 1024),
           dict(scratch=at(3) + 15264), dict(inp=at(4) + need - 16), dict(out=at(4) - 15264), dict(scratch=at(1) - need + 16)]
    for kw in bad:
        assert apply(**kw) == 1, kw
    assert apply(W=65536, R=32768) == 2
    with pytest.raises(bl.RtbError):
        bl.check("rtb_apply", 2)
    assert isinstance(bl.RtbError("x", 1), RuntimeError) and "RTB_ERR_BAD_ARG" in str(bl.RtbError("x", 1))
