"""The build recipe without a GPU (ray_tracer_s8_amd/build.py): the four libraries are build.Library values, and the record, the
staleness rule and the build are functions of one.
1. every library is stale when missing, when its record names other flags and when it is older than a dependency, and fresh
   otherwise; none of that changes the record or the staleness of any other library;
2. the libraries have paths of their own under lib/, the private libraries' sources lie beside csrc/ and are a dependency of their
   own library only, and the product's record names the product's units only;
3. the private libraries are compiled with the product's flags plus -fno-slp-vectorize, and keep a record of their own;
4. the records are those of tests/golden/build_records/, byte for byte: what the libraries were compiled with before the recipe was
   written once.  An edit of the recipe that moves a flag shows here."""
import dataclasses
import os
from pathlib import Path

import pytest

from ray_tracer_s8_amd import build

GOLDEN = Path(__file__).resolve().parent / "golden" / "build_records"
NAMES = {"s8": build.PRODUCT, "s8_dbg": build.DEBUG, "film": build.FILM, "history": build.HISTORY}
PRIVATE = {"film": build.FILM, "history": build.HISTORY}


def test_the_libraries_are_the_four_descriptors():
    assert build.LIBRARIES == tuple(NAMES.values())
    assert (build.PRODUCT.path, build.DEBUG.path) == (build.LIB_PATH, build.DEBUG_LIB_PATH)
    assert tuple(build.PRODUCT.units) == tuple(build.UNITS) == tuple(build.DEBUG.units)
    assert list(build.DEBUG.extra) == build.DEBUG_FLAGS and not build.PRODUCT.extra
    for lib in build.LIBRARIES:
        assert lib.record_path == lib.path.with_suffix(".flags")
        with pytest.raises(dataclasses.FrozenInstanceError):
            lib.path = lib.path


@pytest.mark.parametrize("name", NAMES)
def test_staleness_is_each_librarys_own(name, tmp_path):
    """On a copy of the descriptor under tmp_path (nothing of build is patched): missing, other flags, older than its sources, fresh.
    Through every step the record and the staleness of every other library, and what needs_build() and flags_record() say of the
    product, are what they were."""
    real = NAMES[name]
    others = [o for o in build.LIBRARIES if o is not real]
    state = lambda: ([(build.record(o), build.stale(o)) for o in others], build.flags_record(), build.needs_build())
    before = state()
    lib = dataclasses.replace(real, path=tmp_path / real.path.name, obj_dir=tmp_path / real.obj_dir.name)
    assert lib.record_path.parent == tmp_path and build.record(lib) == build.record(real)
    assert build.stale(lib) and state() == before
    # present, with a record of other flags: stale, and nothing to the others
    lib.path.write_bytes(b"")
    lib.record_path.write_text("".join(f"{unit}: -O0\n" for unit, _ in lib.units))
    assert build.stale(lib) and state() == before
    # present with the right record, but older than its sources: stale again
    lib.record_path.write_text(build.record(lib))
    os.utime(lib.path, (1, 1))
    assert build.stale(lib) and state() == before
    os.utime(lib.path, None)
    assert not build.stale(lib) and state() == before
    assert build.ensure(lib) == lib.path and lib.path.read_bytes() == b""             # fresh: nothing is compiled
    # used as it was built (a prebuilt experiment variant): only a missing file or record makes it stale
    kept = dataclasses.replace(lib, as_built=True, extra=("-DRT_OTHER",))
    os.utime(lib.path, (1, 1))
    assert not build.stale(kept) and build.stale(dataclasses.replace(kept, as_built=False))
    lib.record_path.unlink()
    assert build.stale(kept) and state() == before


def test_the_libraries_are_apart():
    paths = [lib.path for lib in build.LIBRARIES]
    assert len(set(paths)) == 4 and all(p.parent == build.LIB_DIR for p in paths)
    assert len({lib.obj_dir for lib in build.LIBRARIES}) == 4 and all(lib.obj_dir.parent == build.LIB_DIR for lib in build.LIBRARIES)
    assert build.FILM.path == build.LIB_DIR / "librt_film.so" and build.HISTORY.path == build.LIB_DIR / "librt_history.so"
    if "RT_LIB_VARIANT" not in os.environ:
        assert build.LIB_PATH.name == "librt_s8.so"
    assert build.PRODUCT.src_dir == build.DEBUG.src_dir == build.CSRC
    for lib in PRIVATE.values():
        # beside csrc/, not under it: a dependency of its own library and of no other
        assert lib.src_dir.parent == build.CSRC.parent and lib.src_dir != build.CSRC and build.CSRC not in lib.src_dir.parents
        assert lib.src_dir.is_dir() and (lib.src_dir / lib.units[0][0]).is_file()
        assert any(lib.src_dir in d.parents for d in build.dep_files(lib))
        for other in build.LIBRARIES:
            if other is not lib:
                assert not any(lib.src_dir in d.parents for d in build.dep_files(other)), other.path
    assert build.FILM.src_dir != build.HISTORY.src_dir
    for lib in build.LIBRARIES:
        deps = build.dep_files(lib)
        assert all(d.is_file() for d in deps) and Path(build.__file__) in deps and build.ROOT / "include" / "rt_tile.h" in deps
        assert all(lib.src_dir / unit in deps for unit, _ in lib.units)
    # the product's and the test library's: everything under csrc/
    for lib in (build.PRODUCT, build.DEBUG):
        assert {f for f in build.CSRC.rglob("*") if f.is_file()} <= set(build.dep_files(lib))
    # a private library's: of csrc/, only the headers named
    assert {d.name for d in build.dep_files(build.FILM) if d.parent == build.CSRC} == {"rt_denoise_math.h", "rt_consts.h", "rt_plan.h"}
    assert {d.name for d in build.dep_files(build.HISTORY) if d.parent == build.CSRC} == {"rt_consts.h", "rt_plan.h"}
    for record in (build.flags_record(), build.record(build.PRODUCT), build.record(build.DEBUG)):
        assert "rt_film" not in record and "rt_history" not in record and len(record.splitlines()) == len(build.UNITS)
    assert "rt_history" not in build.record(build.FILM) and "rt_film" not in build.record(build.HISTORY)


def test_the_private_libraries_never_take_the_experiments_flags(monkeypatch):
    before = [build.record(lib) for lib in PRIVATE.values()], build.record(build.DEBUG)
    monkeypatch.setenv("RT_EXTRA_HIPCC_FLAGS", "-DRT_PROFILE_TIME")
    assert "-DRT_PROFILE_TIME" in build.flags_record()
    assert ([build.record(lib) for lib in PRIVATE.values()], build.record(build.DEBUG)) == before
    assert "-DRT_PROFILE_TIME" not in "".join(before[0]) + before[1]


@pytest.mark.parametrize("name", PRIVATE)
def test_a_private_library_is_compiled_with_the_products_flags(name):
    lib = PRIVATE[name]
    path = {"film": build.build_film, "history": build.build_history}[name]()
    assert path == lib.path and path.exists() and not build.stale(lib)
    line = lib.record_path.read_text()
    assert line == build.record(lib) and line.startswith(f"rt_{name}.hip: ")
    flags = line.split(": ", 1)[1].split()
    assert flags == [f for f in build.HIPCC_FLAGS if f != "-shared"] + ["-fno-slp-vectorize"]
    assert "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags
    assert not any("correctly-rounded" in f or "fast-math" in f for f in flags)          # correctly rounded div / sqrt: the default


@pytest.mark.parametrize("name", NAMES)
def test_the_records_are_the_golden_ones(name, monkeypatch):
    golden = (GOLDEN / f"{name}.flags").read_text()
    assert build.record(NAMES[name]) == golden
    if name == "s8":
        monkeypatch.delenv("RT_EXTRA_HIPCC_FLAGS", raising=False)
        assert build.flags_record() == build.flags_record([]) == golden
    if name == "s8_dbg":
        assert build.flags_record(build.DEBUG_FLAGS) == golden
