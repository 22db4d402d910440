"""The build recipe without a GPU (ray_tracer_s8_amd/build.py): the product, the test library and every member of build.PRIVATE are
build.Library values, and the record, the staleness rule and the build are functions of one.
1. every library is stale when missing, when its record names other flags and when it is older than a dependency, and fresh
   otherwise; none of that changes the record or the staleness of any other library;
2. every library depends on its units, the C header and the recipe, the product and the test library on everything under csrc/,
   and their records name the product's units only;
3. no library but the product takes the experiments' flags;
4. the records are those of tests/golden/build_records/, byte for byte: what the libraries were compiled with before the recipe was
   written once.  An edit of the recipe that moves a flag shows here.
What makes a private library one of its own (paths, sources, dependencies, flags, exports) is tests/test_private_libraries.py's."""
import dataclasses
import os
from pathlib import Path

import pytest

from ray_tracer_s8_amd import build

GOLDEN = Path(__file__).resolve().parent / "golden" / "build_records"
NAMES = {"s8": build.PRODUCT, "s8_dbg": build.DEBUG, **build.PRIVATE}
EVERY = tuple(NAMES.values())


def test_the_libraries_are_descriptors():
    assert list(build.PRIVATE) == ["film", "history", "sampler", "upsample", "robust", "display"] and len({lib.path for lib in EVERY}) == 8
    assert (build.PRODUCT.path, build.DEBUG.path) == (build.LIB_PATH, build.DEBUG_LIB_PATH)
    assert tuple(build.PRODUCT.units) == tuple(build.UNITS) == tuple(build.DEBUG.units)
    assert list(build.DEBUG.extra) == build.DEBUG_FLAGS and not build.PRODUCT.extra
    for lib in EVERY:
        assert lib.record_path == lib.path.with_suffix(".flags")
        with pytest.raises(dataclasses.FrozenInstanceError):
            lib.path = lib.path


@pytest.mark.parametrize("name", NAMES)
def test_staleness_is_each_librarys_own(name, tmp_path):
    """On a copy of the descriptor under tmp_path (nothing of build is patched): missing, other flags, older than its sources, fresh.
    Through every step the record and the staleness of every other library, and what needs_build() and flags_record() say of the
    product, are what they were."""
    real = NAMES[name]
    others = [o for o in EVERY if o is not real]
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
    if "RT_LIB_VARIANT" not in os.environ:
        assert build.LIB_PATH.name == "librt_s8.so"
    assert build.PRODUCT.src_dir == build.DEBUG.src_dir == build.CSRC
    for lib in EVERY:
        deps = build.dep_files(lib)
        assert all(d.is_file() for d in deps) and Path(build.__file__) in deps and build.ROOT / "include" / "rt_tile.h" in deps
        assert all(lib.src_dir / unit in deps for unit, _ in lib.units)
    # the product's and the test library's: everything under csrc/, and nothing of a private library
    for lib in (build.PRODUCT, build.DEBUG):
        deps = set(build.dep_files(lib))
        assert {f for f in build.CSRC.rglob("*") if f.is_file()} <= deps
        assert not [d for d in deps if build.CSRC not in d.parents and d.parent != build.ROOT / "include" and d != Path(build.__file__)]
    for record in (build.flags_record(), build.record(build.PRODUCT), build.record(build.DEBUG)):
        assert not [n for n in build.PRIVATE if f"rt_{n}" in record] and len(record.splitlines()) == len(build.UNITS)


def test_the_private_libraries_never_take_the_experiments_flags(monkeypatch):
    before = [build.record(lib) for lib in build.PRIVATE.values()], build.record(build.DEBUG)
    monkeypatch.setenv("RT_EXTRA_HIPCC_FLAGS", "-DRT_PROFILE_TIME")
    assert "-DRT_PROFILE_TIME" in build.flags_record()
    assert ([build.record(lib) for lib in build.PRIVATE.values()], build.record(build.DEBUG)) == before
    assert "-DRT_PROFILE_TIME" not in "".join(before[0]) + before[1]


@pytest.mark.parametrize("name", NAMES)
def test_the_records_are_the_golden_ones(name, monkeypatch):
    golden = (GOLDEN / f"{name}.flags").read_text()
    assert build.record(NAMES[name]) == golden
    if name == "s8":
        monkeypatch.delenv("RT_EXTRA_HIPCC_FLAGS", raising=False)
        assert build.flags_record() == build.flags_record([]) == golden
    if name == "s8_dbg":
        assert build.flags_record(build.DEBUG_FLAGS) == golden
