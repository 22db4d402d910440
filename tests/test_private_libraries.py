"""What holds of every private library (ray_tracer_s8_amd/build.py PRIVATE, _private_lib.Binding, <name>_csrc/), stated
once over all of them, without a GPU:
1. a library of its own: a path, an object directory and a source directory no other library has, one unit, its headers; its
   dependencies are exactly its directory, private_csrc/, the csrc/ headers build.py names, the C header and the recipe, and those
   csrc/ headers are exactly the ones its sources include; no library's dependencies reach into another private directory;
2. the record: the golden one, the product's flags plus -fno-slp-vectorize whatever RT_EXTRA_HIPCC_FLAGS says, and what the built
   library was compiled with;
3. exports: the built library exports exactly its binding's SIGNATURES, all with its prefix, and nothing of the tile ABI; no other
   library exports a name with its prefix; the private header declares exactly those functions, the binding's version and statuses,
   and there is no public header;
4. its prefix occurs in no other source directory (the exceptions are a table);
5. build() makes every private library, in order, then the product, and the driver's build() forces it;
6. every binding imports without torch and loads nothing.
What only one library has (its check_* function, constants, status table, refusals, class surface) is that library's plan test's."""
import importlib
import re
import subprocess
import sys
from pathlib import Path

import pytest

from ray_tracer_s8_amd import _abi, build

import _surface

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden" / "build_records"
PREFIX = {"film": "rtf", "history": "rth", "sampler": "rts", "upsample": "rtu", "robust": "rtr", "display": "rtd"}
# the csrc/ headers each library includes, as build.py names them
CSRC_HEADERS = {"film": {"rt_denoise_math.h", "rt_consts.h", "rt_plan.h"}, "history": {"rt_consts.h", "rt_plan.h"}, "sampler": set(),
                "upsample": {"rt_denoise_math.h", "rt_consts.h"}, "robust": set(), "display": set()}
EVERY = {"s8": build.PRODUCT, "s8_dbg": build.DEBUG, **build.PRIVATE}
# Files outside a library's directory that mention its prefix, in comments: the film's functions where the history and the upsampler
# say what they take from a film, and a word of the product's comments that happens to hold the letters ("north_star").
MENTIONS = {
    "rtf": {build.HISTORY.src_dir / "rt_history.h", build.UPSAMPLE.src_dir / "rt_upsample.h"},
    "rth": {build.CSRC / "rt_kernel.hip.h", build.CSRC / "rt_consts.h"},
}


def binding(name):
    return importlib.import_module(f"ray_tracer_s8_amd._{name}_lib")


def under(d, files):
    return [f for f in files if d in f.parents]


def test_the_registry():
    assert list(build.PRIVATE) == list(PREFIX) == list(CSRC_HEADERS)
    assert (build.FILM, build.HISTORY, build.SAMPLER, build.UPSAMPLE, build.ROBUST, build.DISPLAY) == tuple(build.PRIVATE.values())
    assert all(isinstance(lib, build.Library) for lib in build.PRIVATE.values())
    assert build.PRODUCT not in build.PRIVATE.values() and build.DEBUG not in build.PRIVATE.values()
    for name in build.PRIVATE:
        b = binding(name).BINDING
        assert b.library is build.PRIVATE[name] and b.prefix == PREFIX[name]


def test_every_library_has_a_path_and_an_object_directory_of_its_own():
    libs = list(EVERY.values())
    assert len({lib.path for lib in libs}) == len({lib.obj_dir for lib in libs}) == len({lib.record_path for lib in libs}) == 8
    assert all(lib.path.parent == lib.obj_dir.parent == build.LIB_DIR for lib in libs)
    assert len({lib.src_dir for lib in libs}) == 7 and build.PRODUCT.src_dir == build.DEBUG.src_dir == build.CSRC


@pytest.mark.parametrize("name", build.PRIVATE)
def test_a_library_of_its_own(name):
    lib = build.PRIVATE[name]
    assert lib.path == build.LIB_DIR / f"librt_{name}.so" and lib.obj_dir == build.LIB_DIR / f"obj_{name}"
    assert lib.units == ((f"rt_{name}.hip", ()),) and (lib.src_dir / f"rt_{name}.hip").is_file()
    own = {f"rt_{name}.h", f"rt_{name}_math.h", f"rt_{name}.hip.h"}
    assert own == {f.name for f in lib.src_dir.iterdir() if f.suffix == ".h"}
    # beside csrc/, not under it, and the shared host header likewise
    assert lib.src_dir == build.PKG / f"{name}_csrc" and lib.src_dir.is_dir() and build.CSRC not in lib.src_dir.parents
    assert build.PRIVATE_CSRC == build.PKG / "private_csrc" and [f.name for f in build.PRIVATE_CSRC.iterdir()] == ["rt_private_host.h"]
    assert lib.include_dirs == (build.INCLUDE, build.CSRC, lib.src_dir, build.PRIVATE_CSRC)
    # its dependencies, exactly
    deps = build.dep_files(lib)
    assert len(deps) == len(set(deps)) and all(d.is_file() for d in deps)
    assert set(deps) == {*(f for f in lib.src_dir.rglob("*") if f.is_file()), build.PRIVATE_CSRC / "rt_private_host.h",
                         *(build.CSRC / h for h in CSRC_HEADERS[name]), build.ROOT / "include" / "rt_tile.h", Path(build.__file__)}
    assert {d.name for d in under(build.CSRC, deps)} == CSRC_HEADERS[name]
    # ... are what its sources include
    included = set()
    for f in lib.src_dir.iterdir():
        included |= set(re.findall(r'^#include "([\w.]+)"', f.read_text(), re.M))
    assert included - {"rt_tile.h"} == own | {"rt_private_host.h"} | CSRC_HEADERS[name]
    assert {n for n in included if (build.CSRC / n).exists()} == CSRC_HEADERS[name]
    # no other library depends on its directory or is named in its record, and it on no other private directory
    for other_name, other in EVERY.items():
        if other is lib:
            continue
        assert not under(lib.src_dir, build.dep_files(other)), other.path
        assert f"rt_{name}" not in build.record(other), other.path
        if other.src_dir != build.CSRC:
            assert not under(other.src_dir, deps), other.path
    assert f"rt_{name}" not in build.flags_record()


@pytest.mark.parametrize("name", build.PRIVATE)
def test_the_record_is_the_golden_one_and_the_products_flags(name, monkeypatch):
    lib = build.PRIVATE[name]
    golden = (GOLDEN / f"{name}.flags").read_text()
    assert build.record(lib) == golden and golden.startswith(f"rt_{name}.hip: ") and golden.count("\n") == 1
    flags = golden.split(": ", 1)[1].split()
    assert flags == [f for f in build.HIPCC_FLAGS if f != "-shared"] + ["-fno-slp-vectorize"]
    assert "-ffp-contract=off" in flags and "-fno-unroll-loops" in flags and "--offload-arch=gfx950" in flags
    assert not any("correctly-rounded" in f or "fast-math" in f for f in flags)          # correctly rounded div / sqrt: the default
    # never the experiments' flags, which are the product's
    others = [build.record(o) for o in EVERY.values() if o is not build.PRODUCT]
    monkeypatch.setenv("RT_EXTRA_HIPCC_FLAGS", "-DRT_PROFILE_TIME")
    assert "-DRT_PROFILE_TIME" in build.flags_record() and build.record(lib) == golden
    assert [build.record(o) for o in EVERY.values() if o is not build.PRODUCT] == others
    monkeypatch.delenv("RT_EXTRA_HIPCC_FLAGS")
    path = build.ensure(lib)
    assert path == lib.path and path.exists() and not build.stale(lib) and lib.record_path.read_text() == golden


@pytest.fixture(scope="module")
def exports():
    """{name: every symbol the built library defines}, of all eight."""
    _abi.load()
    _abi.load_debug()
    return {name: _surface.all_exported(build.ensure(lib) if name in build.PRIVATE else lib.path) for name, lib in EVERY.items()}


def test_the_product_exports_exactly_the_header(exports):
    declared = set(_surface.parse()["functions"])
    assert len(declared) == 51 and _surface.exported(build.LIB_PATH) == declared
    assert declared <= exports["s8"] and declared <= exports["s8_dbg"]


@pytest.mark.parametrize("name", build.PRIVATE)
def test_exports(name, exports):
    b, prefix = binding(name), PREFIX[name]
    mine = {s for s in exports[name] if not s.startswith("_")}
    assert mine == set(b.SIGNATURES) and all(s.startswith(prefix + "_") for s in mine), mine
    assert f"{prefix}_version" in mine
    assert not _surface.exported(build.PRIVATE[name].path)            # nothing of the tile ABI
    for other, symbols in exports.items():
        if other != name:
            assert not [s for s in symbols if prefix + "_" in s], other
    # the private header declares exactly the functions the binding names, the version and the statuses the binding expects
    text = (build.PRIVATE[name].src_dir / f"rt_{name}.h").read_text()
    P = prefix.upper()
    assert set(re.findall(rf"^int ({prefix}_\w+)\(", text, re.M)) == set(b.SIGNATURES)
    version = getattr(b, f"{P}_VERSION")
    assert re.search(rf"^#define {P}_VERSION (\d+)u$", text, re.M).group(1) == str(version) and b.BINDING.version == version
    assert re.search(rf"^#define {P}_OK 0$", text, re.M) and getattr(b, f"{P}_OK") == 0
    status = dict((int(v), n) for n, v in re.findall(rf"^#define ({P}_ERR_\w+) (\d+)", text, re.M))
    assert status == b.STATUS and sorted(status) == list(range(1, len(status) + 1))
    error = getattr(b, f"{prefix.capitalize()}Error")
    assert error is b.BINDING.Error and error.STATUS == b.STATUS and issubclass(error, RuntimeError)
    assert not (ROOT / "include" / f"rt_{name}.h").exists()


@pytest.mark.parametrize("name", build.PRIVATE)
def test_the_prefix_is_in_no_other_source_directory(name):
    prefix = PREFIX[name]
    dirs = [build.CSRC, build.PRIVATE_CSRC, ROOT / "include", *(lib.src_dir for n, lib in build.PRIVATE.items() if n != name)]
    found = {f for d in dirs for f in d.rglob("*") if f.is_file() and prefix + "_" in f.read_text().lower()}
    assert found == MENTIONS.get(prefix, set())


def test_who_builds(monkeypatch):
    """build() with the recipe's steps replaced by recorders: every private library in PRIVATE's order, then the product, each
    compiled if it is stale or the build forced and left alone otherwise; the driver's build() forces it."""
    assert not build.VARIANT
    paths = [*(lib.path for lib in build.PRIVATE.values()), build.LIB_PATH]
    for is_stale, force, compiled in ((True, False, True), (False, False, False), (False, True, True)):
        asked = []
        monkeypatch.setattr(build, "stale", lambda lib: asked.append(("stale", lib.path)) or is_stale)
        monkeypatch.setattr(build, "compile_and_link", lambda lib, verbose=False: asked.append(("compile", lib.path)) or lib.path)
        assert build.build(force=force) == build.LIB_PATH
        if force:
            assert asked == [("compile", p) for p in paths]
        else:
            assert [p for w, p in asked if w == "stale"] == paths
            assert [p for w, p in asked if w == "compile"] == (paths if compiled else [])
        asked.clear()
        for lib in build.PRIVATE.values():                              # and one library alone
            assert build.ensure(lib, force) == lib.path
            assert asked == ([("compile", lib.path)] if force else [("stale", lib.path)] + [("compile", lib.path)] * compiled)
            asked.clear()
        assert build.build_debug(force) == build.DEBUG_LIB_PATH and asked[-1][1] == build.DEBUG_LIB_PATH
    monkeypatch.undo()
    asked = []
    monkeypatch.setattr(build, "ensure", lambda lib, force=False, verbose=False: asked.append(lib.path) or lib.path)
    build.build()
    assert asked == paths
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert entry.index("hip_build.build(force=True)") < entry.index("hip_build.build_debug(force=True)") < entry.index("orc.build(")
    assert not re.search(r"build_(film|history|sampler|upsample|robust|display)\b", entry)


_IMPORT_CHILD = r"""
import sys
import ray_tracer_s8_amd as rt
import ray_tracer_s8_amd._%(name)s_lib as m
assert "torch" not in sys.modules
assert m.BINDING.loaded is False                        # importing loads nothing
assert callable(m.load) and callable(m.check) and issubclass(m.%(error)s, RuntimeError)
assert all(n.startswith("%(prefix)s_") for n in m.SIGNATURES) and "%(prefix)s_version" in m.SIGNATURES
try:
    m.check("x", 1)
except m.%(error)s as e:
    assert e.status == 1 and str(e) == "x: " + m.STATUS[1]
else:
    raise AssertionError("check(1) did not raise")
m.check("x", 0)
assert "torch" not in sys.modules and m.BINDING.loaded is False
print("ok")
"""


@pytest.mark.parametrize("name", build.PRIVATE)
def test_the_binding_imports_without_torch_and_loads_nothing(name):
    child = _IMPORT_CHILD % dict(name=name, prefix=PREFIX[name], error=PREFIX[name].capitalize() + "Error")
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
