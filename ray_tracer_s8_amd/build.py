"""Build recipe for the HIP libraries (gfx950 only): each library is a `Library` value, and the recipe (record, staleness, compile
and link, build if stale) is written once over it.

`hipcc --offload-arch=gfx950` cross-compiles without a GPU, so this runs in the CPU
container too.  The .so files are built in-tree (ray_tracer_s8_amd/lib/) so they travel to the
GPU box with a snapshot of the working tree; git ignores them.
"""
from __future__ import annotations

import os
import subprocess
from dataclasses import dataclass, replace
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
LIB_DIR = PKG / "lib"
# RT_LIB_VARIANT=<name> (experiments): build and load lib/librt_s8_<name>.so with RT_EXTRA_HIPCC_FLAGS, objects in their own
# directory — the product library lib/librt_s8.so is never rebuilt in place by an A/B run (round-2 advisor)
VARIANT = os.environ.get("RT_LIB_VARIANT", "")
LIB_PATH = LIB_DIR / (f"librt_s8_{VARIANT}.so" if VARIANT else "librt_s8.so")
DEBUG_LIB_PATH = LIB_DIR / "librt_s8_dbg.so"

# -ffp-contract=off: the kernel must perform the reference's IEEE binary32 operations one
# by one (Rust never contracts a*b+c); FMA appears only where written as __builtin_fmaf.
# Correctly rounded f32 sqrt/div is hipcc's default (-fhip-fp32-correctly-rounded-divide-sqrt).
# -fno-unroll-loops: only the loops marked `#pragma unroll` are unrolled; the heuristic unrolling of the divergent
# loops (samplers, root tests, path product) cost c3 3 % (tools/variants_all.sh).
HIPCC_FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-ffp-contract=off",
    "-fno-unroll-loops",
    "-fPIC",
    "-shared",
    "-fvisibility=hidden",
]


# translation units and the flags each one adds: the host side, the linear-scan kernels, the traversal kernels
# (SLP-vectorised packed FP32 pairs: linear kernels +3 %, traversal kernels -1.5 %, tools/variants_all.sh), the ray-query kernels,
# the kernels that path-trace caller rays, the kernels of their single path steps, the kernels of their direct lighting, the kernel of their next-event-estimation integrator, the kernels of the feature buffers, the kernels of the denoiser, the camera-ray kernel
UNITS = [
    ("rt_api.hip", []),
    ("rt_kernels_lin.hip", []),
    ("rt_kernels_trav.hip", ["-fno-slp-vectorize"]),
    ("rt_kernels_query.hip", ["-fno-slp-vectorize"]),
    ("rt_kernels_trace.hip", ["-fno-slp-vectorize"]),
    ("rt_kernels_bounce.hip", ["-fno-slp-vectorize"]),
    ("rt_kernels_direct.hip", ["-fno-slp-vectorize"]),
    ("rt_kernels_nee.hip", ["-fno-slp-vectorize"]),
    ("rt_kernels_aov.hip", ["-fno-slp-vectorize"]),
    ("rt_kernels_denoise.hip", ["-fno-slp-vectorize"]),
    ("rt_kernels_camera.hip", ["-fno-slp-vectorize"]),
]


@dataclass(frozen=True)
class Library:
    """One shared library as data.  Every function of the recipe below reads its argument only, so a test hands them a copy
    (dataclasses.replace(lib, path=...)) instead of patching this module."""
    path: Path                     # the .so; its record, the exact compile lines it was built with, is path.with_suffix(".flags")
    obj_dir: Path
    src_dir: Path
    units: tuple                   # (file under src_dir, the flags that unit adds after the include directories)
    extra: tuple = ()              # flags of every unit, ahead of the include directories
    include_dirs: tuple = ()
    deps: tuple = ()               # what staleness looks at: files, and directories taken with every file under them
    as_built: bool = False         # used as it was built: only a missing file or record makes it stale

    @property
    def record_path(self) -> Path:
        return self.path.with_suffix(".flags")


INCLUDE = ROOT / "include"
# The product and the test library are compiled from everything under csrc/, subdirectories included (a new header cannot be
# forgotten; a stray file there costs a rebuild, never a stale library), the C header and this recipe.
_CSRC_DEPS = (CSRC, INCLUDE / "rt_tile.h", Path(__file__))

# The PRODUCT with the default flags: it exports exactly include/rt_tile.h (tests/test_surface.py).  _product() is the product as
# asked for now, RT_EXTRA_HIPCC_FLAGS included.
PRODUCT = Library(LIB_PATH, LIB_DIR / (f"obj_{VARIANT}" if VARIANT else "obj"), CSRC, tuple(UNITS), include_dirs=(INCLUDE, CSRC),
                  deps=_CSRC_DEPS)

# The TEST library: the product sources plus -DRT_DEBUG_HOOKS, which compiles the rt_debug_* entry points (launch-path knobs,
# counter read-back, a throwing body, the sqrt self-test, the unit kernels of rt_unit.hip.h and rt_unit_sampling.hip.h) that tests
# and tools use.
DEBUG_FLAGS = ["-DRT_DEBUG_HOOKS"]
DEBUG = replace(PRODUCT, path=DEBUG_LIB_PATH, obj_dir=LIB_DIR / "obj_dbg", extra=tuple(DEBUG_FLAGS))


# What the host files of the private libraries share (rt_private_host.h): beside csrc/, so a library that includes no csrc/ header
# depends on nothing under csrc/.
PRIVATE_CSRC = PKG / "private_csrc"


def _private(name: str, headers: tuple) -> Library:
    """A private library: lib/librt_<name>.so from the one unit <name>_csrc/rt_<name>.hip, loaded by a binding module of its own
    (_private_lib.Binding) and no part of the tile ABI.  Its sources lie beside csrc/, not under it, so they are no dependency of
    any other library; its own dependencies are its directory, private_csrc/, the csrc/ headers it includes (named here), the C
    header and this recipe.  The product's flags plus -fno-slp-vectorize, and never RT_EXTRA_HIPCC_FLAGS: experiments are the
    product library's."""
    src = PKG / f"{name}_csrc"
    return Library(LIB_DIR / f"librt_{name}.so", LIB_DIR / f"obj_{name}", src, ((f"rt_{name}.hip", ()),), extra=("-fno-slp-vectorize",),
                   include_dirs=(INCLUDE, CSRC, src, PRIVATE_CSRC),
                   deps=(src, PRIVATE_CSRC, *(CSRC / h for h in headers), INCLUDE / "rt_tile.h", Path(__file__)))


# The PRIVATE libraries, in the order build() makes them: name -> Library, with the csrc/ headers each one includes.  A further
# library is one entry here, its directory, its binding module and its golden record.
PRIVATE = {
    "film": _private("film", ("rt_denoise_math.h", "rt_consts.h", "rt_plan.h")),    # moments fold, guided resolve; rtf_*
    "history": _private("history", ("rt_consts.h", "rt_plan.h")),                   # temporal accumulation (4.24); rth_*
    "sampler": _private("sampler", ()),                                             # adaptive sampling (4.25); rts_*
    "upsample": _private("upsample", ("rt_denoise_math.h", "rt_consts.h")),         # joint-bilateral upsampling (4.27); rtu_*
    "robust": _private("robust", ()),                                               # median of means (4.29); rtr_*
    "display": _private("display", ()),                                             # metered exposure, tone curves (4.30); rtd_*
}
FILM, HISTORY, SAMPLER, UPSAMPLE, ROBUST, DISPLAY = PRIVATE.values()

# The JPEG library (baseline JPEG encoding of a device frame, 4.32; rtj_*): a private library by the same recipe, held beside PRIVATE:
# build() leaves it to its binding (_jpeg_lib.py builds a missing one on load), the driver's build() and `python -m` make it.
JPEG = _private("jpeg", ())

# The bloom library (pyramid bloom of a linear frame, 4.33; rtb_*): held beside PRIVATE in the same way, and built by the same three
# (_bloom_lib.py on load, the driver's build(), `python -m`).
BLOOM = _private("bloom", ())


def _product(extra: list[str] | None = None) -> Library:
    """The product as asked for NOW: RT_EXTRA_HIPCC_FLAGS (experiments only, e.g. -DRT_MAXC=12) is read at every call.  A prebuilt
    experiment variant (RT_LIB_VARIANT set, RT_EXTRA_HIPCC_FLAGS not) is used as it was built: its flags are in its record."""
    env = os.environ.get("RT_EXTRA_HIPCC_FLAGS")
    return replace(PRODUCT, extra=tuple((env or "").split() if extra is None else extra), as_built=bool(VARIANT) and env is None)


def record(lib: Library) -> str:
    """What the library was (or would be) compiled with: one line per translation unit.  A library whose record differs
    from the flags asked for NOW is stale whatever its mtime — an A/B script that died before restoring the default
    build (tools/ab*.sh, phase_time.py: -DRT_PROFILE_TIME, experimental -D knobs) would otherwise leave a variant that
    looks fresh, travels to the GPU box and gets benchmarked."""
    common = [f for f in HIPCC_FLAGS if f != "-shared"] + list(lib.extra)
    return "".join(f"{unit}: {' '.join(common + list(flags))}\n" for unit, flags in lib.units)


def dep_files(lib: Library) -> list[Path]:
    """lib.deps as files, the directories read now: a file added to one is a dependency from then on."""
    return [f for d in lib.deps for f in (sorted(p for p in d.rglob("*") if p.is_file()) if d.is_dir() else [d])]


def stale(lib: Library) -> bool:
    """Missing, built with other flags than record(lib), or older than one of its dependencies."""
    if not lib.path.exists() or not lib.record_path.exists():
        return True
    if lib.as_built:
        return False
    if lib.record_path.read_text() != record(lib):
        return True
    t = lib.path.stat().st_mtime
    return any(d.stat().st_mtime > t for d in dep_files(lib))


def compile_and_link(lib: Library, verbose: bool = False) -> Path:
    """Compile the units side by side (they are independent), then link.  Raises on failure (no fallback)."""
    hipcc = os.environ.get("HIPCC", "hipcc")
    lib.path.parent.mkdir(parents=True, exist_ok=True)
    lib.record_path.unlink(missing_ok=True)           # no record while the objects are in flux
    lib.obj_dir.mkdir(parents=True, exist_ok=True)
    common = [f for f in HIPCC_FLAGS if f != "-shared"] + list(lib.extra) + [f"-I{d}" for d in lib.include_dirs]
    objs = [str(lib.obj_dir / (Path(unit).stem + ".o")) for unit, _ in lib.units]
    cmds = [[hipcc, *common, *flags, "-c", str(lib.src_dir / unit), "-o", obj] for (unit, flags), obj in zip(lib.units, objs)]
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(lib.path), *objs]
    procs = []
    for cmd in cmds:
        if verbose:
            print(" ".join(cmd))
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for cmd, pr in zip(cmds, procs):
        so, se = pr.communicate()
        if pr.returncode != 0:
            raise RuntimeError(f"hipcc failed ({pr.returncode}): {' '.join(cmd)}\n{so}\n{se}")
    if verbose:
        print(" ".join(link))
    proc = subprocess.run(link, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"hipcc link failed ({proc.returncode}):\n{proc.stdout}\n{proc.stderr}")
    lib.record_path.write_text(record(lib))
    return lib.path


def ensure(lib: Library, force: bool = False, verbose: bool = False) -> Path:
    """Build the library if it is missing or stale, or if forced."""
    return compile_and_link(lib, verbose) if force or stale(lib) else lib.path


def flags_record(extra: list[str] | None = None) -> str:
    """The product's record with `extra` in the place of RT_EXTRA_HIPCC_FLAGS."""
    return record(_product(extra))


def built_with_default_flags() -> bool:
    """True iff the library on disk was compiled with exactly HIPCC_FLAGS (no RT_EXTRA_HIPCC_FLAGS)."""
    return LIB_PATH.exists() and PRODUCT.record_path.exists() and PRODUCT.record_path.read_text() == record(PRODUCT)


def needs_build() -> bool:
    return stale(_product())


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile librt_s8.so (or the RT_LIB_VARIANT named) if missing or stale, and with no variant named every private library
    first."""
    for lib in () if VARIANT else PRIVATE.values():
        ensure(lib, force, verbose)
    return ensure(_product(), force, verbose)


def build_debug(force: bool = False, verbose: bool = False) -> Path:
    return ensure(DEBUG, force, verbose)


if __name__ == "__main__":
    print(build(force=True, verbose=True))
    if not VARIANT:
        for lib in (DEBUG, JPEG, BLOOM, *PRIVATE.values()):    # (the private ones were forced by build())
            print(ensure(lib, force=lib in (DEBUG, JPEG, BLOOM), verbose=True))
