"""The frame encoder without a GPU (ray_tracer_s8_amd/frame_encoder.py, _jpeg_lib.py, build.py):
1. check_encoder refuses, with ValueError, everything FrameEncoder refuses; FrameEncoder is in rt.__all__ and runs its checks first;
2. what tests/test_private_libraries.py states of the six members of build.PRIVATE, stated of build.JPEG, which is held beside them:
   a library of its own, its dependencies exactly, the golden record, exports equal to SIGNATURES and all rtj_*, the header declaring
   exactly those functions, the prefix in no other source directory and in no other library's exports, who builds it, and a binding
   that imports without torch and loads nothing;
3. every refusal of the library's calls comes back as a status, with no device bound and addresses that are never read;
4. rtj_header is the restatement's header and rtj_bound is at least the restatement's file on the whole corpus.
Without the feature every test here fails at the import of _jpeg_lib."""
import ctypes as C
import re
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, _jpeg_lib as jl, build

import _jpeg_np as jnp
import _surface

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden" / "build_records"
NAMES = ("rtj_version", "rtj_header", "rtj_bound", "rtj_scratch_bytes", "rtj_encode")
OTHERS = {"s8": build.PRODUCT, "s8_dbg": build.DEBUG, **build.PRIVATE}


# ---- 1. the checks ---------------------------------------------------------------------------------------------------------------------
def test_check_encoder():
    from ray_tracer_s8_amd import frame_encoder as fe
    assert rt.FrameEncoder is fe.FrameEncoder and "FrameEncoder" in rt.__all__
    assert fe.check_encoder((1080, 1920)) == ((1080, 1920), 90, 16, 629 + 1080 * 1920 * 3)
    assert fe.check_encoder([19, 67], 1, 1, 630) == ((19, 67), 1, 1, 630)
    assert fe.check_encoder((65535, 1), 100, 65535).interval == 65535 and fe.check_encoder((8, 9)).interval == fe.INTERVAL == 16
    bad = {
        "no shape": dict(shape=None), "a flat shape": dict(shape=(64,)), "three": dict(shape=(36, 64, 3)), "zero rows": dict(shape=(0, 64)),
        "negative": dict(shape=(36, -1)), "float sizes": dict(shape=(36.0, 64)), "bool sizes": dict(shape=(True, 64)),
        "a side of 2^16": dict(shape=(36, 65536)),
        "quality 0": dict(quality=0), "quality 101": dict(quality=101), "quality 90.0": dict(quality=90.0), "quality None": dict(quality=None),
        "quality True": dict(quality=True), "quality a string": dict(quality="90"),
        "interval 0": dict(interval=0), "interval 2^16": dict(interval=65536), "interval 2.0": dict(interval=2.0), "interval True": dict(interval=True),
        "capacity the header": dict(capacity=629), "capacity 0": dict(capacity=0), "capacity 2^32": dict(capacity=1 << 32),
        "capacity 1e6": dict(capacity=1e6),
    }
    for what, kw in bad.items():
        args = dict(shape=(36, 64))
        args.update(kw)
        with pytest.raises(ValueError):
            fe.check_encoder(**args)
            pytest.fail(what)


def test_frame_encoder_runs_its_checks_before_anything_else():
    """Bad arguments: ValueError before the film, torch or the library is touched."""
    loaded = jl.BINDING.loaded
    film = types.SimpleNamespace(rows=36, width=64)                     # (no _check_open, no _torch: touching either would raise)
    for kw in (dict(quality=0), dict(interval=0), dict(shape=(0, 3)), dict(capacity=10), dict(quality="best")):
        with pytest.raises(ValueError):
            rt.FrameEncoder(film, **kw)
    with pytest.raises(ValueError):
        rt.FrameEncoder(types.SimpleNamespace())                       # no shape to take from the film
    assert jl.BINDING.loaded is loaded


# ---- 2. the registry -------------------------------------------------------------------------------------------------------------------
def test_a_library_of_its_own_beside_the_registry():
    lib = build.JPEG
    assert isinstance(lib, build.Library) and lib not in build.PRIVATE.values() and "jpeg" not in build.PRIVATE
    assert jl.BINDING.library is lib and jl.BINDING.prefix == "rtj"
    assert lib.path == build.LIB_DIR / "librt_jpeg.so" and lib.obj_dir == build.LIB_DIR / "obj_jpeg"
    assert lib.units == (("rt_jpeg.hip", ()),) and (lib.src_dir / "rt_jpeg.hip").is_file() and lib.extra == ("-fno-slp-vectorize",)
    own = {"rt_jpeg.h", "rt_jpeg_math.h", "rt_jpeg.hip.h"}
    assert own == {f.name for f in lib.src_dir.iterdir() if f.suffix == ".h"}
    assert lib.src_dir == build.PKG / "jpeg_csrc" and lib.src_dir.is_dir() and build.CSRC not in lib.src_dir.parents
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
        assert "rt_jpeg" not in build.record(other), name
        if other.src_dir != build.CSRC:
            assert not [f for f in deps if other.src_dir in f.parents], name
            assert f"rt_{name}" not in build.record(lib)
    assert "rt_jpeg" not in build.flags_record()


def test_the_record_is_the_golden_one_and_the_products_flags(monkeypatch):
    lib = build.JPEG
    golden = (GOLDEN / "jpeg.flags").read_text()
    assert build.record(lib) == golden and golden.startswith("rt_jpeg.hip: ") and golden.count("\n") == 1
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
    mine = {s for s in _surface.all_exported(build.ensure(build.JPEG)) if not s.startswith("_")}
    assert mine == set(jl.SIGNATURES) == set(NAMES) and all(s.startswith("rtj_") for s in mine), mine
    assert not _surface.exported(build.JPEG.path)                       # nothing of the tile ABI
    for name, other in OTHERS.items():
        symbols = _surface.all_exported(build.ensure(other) if name in build.PRIVATE else other.path)
        assert not [s for s in symbols if "rtj_" in s], name
    # the private header declares exactly the functions the binding names, the version and the statuses the binding expects
    text = (build.JPEG.src_dir / "rt_jpeg.h").read_text()
    assert set(re.findall(r"^int (rtj_\w+)\(", text, re.M)) == set(jl.SIGNATURES)
    assert re.search(r"^#define RTJ_VERSION (\d+)u$", text, re.M).group(1) == str(jl.RTJ_VERSION) == "1" and jl.BINDING.version == 1
    assert re.search(r"^#define RTJ_OK 0$", text, re.M) and jl.RTJ_OK == 0
    status = dict((int(v), n) for n, v in re.findall(r"^#define (RTJ_ERR_\w+) (\d+)", text, re.M))
    assert status == jl.STATUS == {1: "RTJ_ERR_BAD_ARG", 2: "RTJ_ERR_LIMIT", 3: "RTJ_ERR_HIP", 4: "RTJ_ERR_INTERNAL"}
    assert jl.RtjError is jl.BINDING.Error and jl.RtjError.STATUS == jl.STATUS and issubclass(jl.RtjError, RuntimeError)
    named = dict((n, int(v)) for n, v in re.findall(r"^#define RTJ_(HEADER_LEN|RECORD_WORDS|MAX_INTERVAL|MAX_SIDE) (\d+)u", text, re.M))
    assert named == dict(HEADER_LEN=jl.HEADER_LEN, RECORD_WORDS=jl.RECORD_WORDS, MAX_INTERVAL=jl.MAX_INTERVAL, MAX_SIDE=jl.MAX_SIDE)
    assert not (ROOT / "include" / "rt_jpeg.h").exists()


def test_the_prefix_is_in_no_other_source_directory():
    dirs = [build.CSRC, build.PRIVATE_CSRC, ROOT / "include", *(lib.src_dir for lib in build.PRIVATE.values())]
    assert not {f for d in dirs for f in d.rglob("*") if f.is_file() and "rtj_" in f.read_text().lower()}
    # and the six prefixes are not in this one
    for prefix in ("rtf", "rth", "rts", "rtu", "rtr", "rtd"):
        assert not {f for f in build.JPEG.src_dir.rglob("*") if f.is_file() and prefix + "_" in f.read_text().lower()}, prefix


def test_who_builds(monkeypatch):
    """build() is the six and the product, as before; the driver's build() forces the JPEG library after the test library and before
    the oracle; `python -m ray_tracer_s8_amd.build` names it; the binding builds a missing one."""
    asked = []
    monkeypatch.setattr(build, "ensure", lambda lib, force=False, verbose=False: asked.append(lib.path) or lib.path)
    build.build()
    assert asked == [*(lib.path for lib in build.PRIVATE.values()), build.LIB_PATH] and build.JPEG.path not in asked
    monkeypatch.undo()
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert entry.index("hip_build.build(force=True)") < entry.index("hip_build.build_debug(force=True)") \
        < entry.index("hip_build.ensure(hip_build.JPEG, force=True)") < entry.index("orc.build(")
    main = Path(build.__file__).read_text().split('if __name__ == "__main__":')[1]
    assert "JPEG" in main
    from ray_tracer_s8_amd import _private_lib
    path = build.ensure(build.JPEG)
    missing = types.SimpleNamespace(path=ROOT / "no_such_dir" / "librt_jpeg.so")
    built = []
    monkeypatch.setattr(build, "ensure", lambda lib, force=False, verbose=False: built.append(lib) or path)
    b = _private_lib.Binding(missing, "rtj", jl.RTJ_VERSION, jl.STATUS, jl.SIGNATURES)
    b.load()
    assert built == [missing] and b.loaded


_IMPORT_CHILD = r"""
import sys
import ray_tracer_s8_amd as rt
import ray_tracer_s8_amd.frame_encoder as fe
import ray_tracer_s8_amd._jpeg_lib as m
assert "torch" not in sys.modules
assert m.BINDING.loaded is False                        # importing loads nothing
assert callable(m.load) and callable(m.check) and issubclass(m.RtjError, RuntimeError)
assert sorted(m.SIGNATURES) == sorted(%r) and "rtj_version" in m.SIGNATURES
try:
    m.check("x", 1)
except m.RtjError as e:
    assert e.status == 1 and str(e) == "x: " + m.STATUS[1]
else:
    raise AssertionError("check(1) did not raise")
m.check("x", 0)
assert rt.FrameEncoder is fe.FrameEncoder and fe.check_encoder((19, 67)).interval == 16
assert all(callable(getattr(fe.FrameEncoder, n)) for n in ("encode", "encode_device", "record", "close"))
assert all(isinstance(getattr(fe.FrameEncoder, n), property) for n in ("header", "tables", "bound"))
assert "torch" not in sys.modules and m.BINDING.loaded is False
print("ok")
""" % (NAMES,)


def test_the_binding_and_the_module_import_without_torch_and_load_nothing():
    r = subprocess.run([sys.executable, "-c", _IMPORT_CHILD], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_are_statuses():
    """Loading binds no device: rtj_version, rtj_header, rtj_bound and rtj_scratch_bytes are host arithmetic, and rtj_encode refuses
    before any launch."""
    lib = jl.load()
    assert lib.rtj_version(None) == 1
    v = C.c_uint32(0)
    assert lib.rtj_version(C.byref(v)) == 0 and v.value == jl.RTJ_VERSION
    n = C.c_uint64(0)
    for fn in (lib.rtj_bound, lib.rtj_scratch_bytes):
        assert fn(67, 19, 3, None) == 1
        for W, R, interval in ((0, 19, 3), (67, 0, 3), (67, 19, 0), (65536, 19, 3), (67, 65536, 3), (67, 19, 65536)):
            assert fn(W, R, interval, C.byref(n)) == 1, (W, R, interval)
        assert fn(67, 19, 3, C.byref(n)) == 0 and n.value > 0
        assert fn(8192, 8192, 1024, C.byref(n)) == 2                 # 1 048 576 MCUs: the raw stream's bits pass 2^32
        assert fn(7680, 4320, 960, C.byref(n)) == 0
    assert lib.rtj_scratch_bytes(67, 19, 3, C.byref(n)) == 0
    scratch_bytes = n.value
    assert scratch_bytes % 256 == 0 and scratch_bytes >= 27 * 384 + jnp.bound(67, 19, 3) // 2 - 400

    head = (C.c_uint8 * 700)()
    tables = (C.c_uint8 * 128)(*([3] * 128))
    zero = (C.c_uint8 * 128)(*([3] * 127 + [0]))
    hdr = lambda cap=700, out=head, length=n, **kw: lib.rtj_header(jl.EncodeArgs(**{**dict(W=67, R=19, quality=90, interval=3), **kw}), out, cap, C.byref(length) if length is not None else None)
    assert hdr() == 0 and n.value == jl.HEADER_LEN
    assert hdr(cap=628) == 2 and hdr(out=None) == 1 and hdr(length=None) == 1 and lib.rtj_header(None, head, 700, C.byref(n)) == 1
    for kw in (dict(W=0), dict(R=0), dict(W=65536), dict(interval=0), dict(interval=65536), dict(quality=101), dict(quality=0),
               dict(quality=90, tables=C.addressof(tables)), dict(quality=0, tables=C.addressof(zero))):
        assert hdr(**kw) == 1, kw
    assert hdr(quality=0, tables=C.addressof(tables)) == 0 and bytes(head[25:89]) == bytes([3] * 64)

    MB = 1 << 20
    at = lambda k: k * MB                                            # (addresses never read: every call here is refused)

    def encode(**kw):
        # 67 x 19: the frame 3 819 bytes, the record 32
        good = dict(W=67, R=19, quality=90, interval=3, rgb=at(1), scratch=at(2), scratch_bytes=scratch_bytes, out=at(4), capacity=4448,
                    header_len=jl.HEADER_LEN, record=at(5))
        good.update(kw)
        return lib.rtj_encode(jl.EncodeArgs(**good), None)

    assert lib.rtj_encode(None, None) == 1
    bad = [dict(W=0), dict(R=0), dict(W=65536), dict(R=65536), dict(interval=0), dict(interval=65536), dict(quality=0), dict(quality=101),
           dict(tables=C.addressof(tables)), dict(quality=0, tables=C.addressof(zero)), dict(reserved=1),
           dict(rgb=None), dict(scratch=None), dict(out=None), dict(record=None),
           dict(rgb=at(1) + 2), dict(scratch=at(2) + 128), dict(scratch=at(2) + 4), dict(record=at(5) + 2),
           dict(header_len=0), dict(header_len=628), dict(header_len=630), dict(capacity=629), dict(capacity=0),
           dict(scratch_bytes=scratch_bytes - 1), dict(scratch_bytes=0),
           # the output in the frame, at its last byte, the frame in the scratch, the record in the output and in the scratch, the output
           # reaching the record
           dict(out=at(1)), dict(out=at(1) + 3818), dict(rgb=at(2) + 256), dict(record=at(4) + 4444), dict(record=at(2) + scratch_bytes - 4),
           dict(out=at(5) - 4447), dict(scratch=at(1) - scratch_bytes + 256), dict(out=at(2) + 1)]
    for kw in bad:
        assert encode(**kw) == 1, kw
    assert encode(W=8192, R=8192, interval=1024) == 2
    with pytest.raises(jl.RtjError):
        jl.check("rtj_encode", 2)
    assert isinstance(jl.RtjError("x", 1), RuntimeError) and "RTJ_ERR_BAD_ARG" in str(jl.RtjError("x", 1))


# ---- 4. the header and the bound -------------------------------------------------------------------------------------------------------
def test_the_header_and_the_bound_on_the_corpus():
    lib = jl.load()
    n, got = C.c_uint64(0), C.c_uint64(0)
    head = (C.c_uint8 * jl.HEADER_LEN)()
    for name, rgb, quality, interval in jnp.corpus():
        R, W = rgb.shape[:2]
        interval = (W + 7) // 8 if interval is None else interval
        want = jnp.encode(rgb, quality, interval)
        assert lib.rtj_header(jl.EncodeArgs(W=W, R=R, quality=quality, interval=interval), head, jl.HEADER_LEN, C.byref(got)) == 0
        assert got.value == jl.HEADER_LEN and bytes(head) == want["header"] == want["file"][:jl.HEADER_LEN], name
        assert lib.rtj_bound(W, R, interval, C.byref(n)) == 0 and n.value == jnp.bound(W, R, interval) >= want["record"]["total"], name
    # the caller's tables, and the extremes of every field
    tables = np.arange(1, 129, dtype=np.uint8)
    for W, R, interval in ((1, 1, 1), (65535, 65535, 65535), (1920, 1080, 240)):
        a = jl.EncodeArgs(W=W, R=R, quality=0, interval=interval, tables=tables.ctypes.data)
        assert lib.rtj_header(a, head, jl.HEADER_LEN, C.byref(got)) == 0
        assert bytes(head) == jnp.header(W, R, 0, interval, tables), (W, R, interval)
    for quality in range(1, 101):
        assert lib.rtj_header(jl.EncodeArgs(W=8, R=8, quality=quality, interval=1), head, jl.HEADER_LEN, C.byref(got)) == 0
        assert bytes(head) == jnp.header(8, 8, quality, 1), quality
