"""Build recipe for the HIP C-ABI library (gfx950 only).

`hipcc --offload-arch=gfx950` cross-compiles without a GPU, so this runs in the CPU
container too.  The .so is built in-tree (ray_tracer_s8_amd/lib/) so it travels to the
GPU box with the repo snapshot; it is git-ignored, not gpurun-ignored.
"""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
LIB_DIR = PKG / "lib"
# RT_LIB_VARIANT=<name> (experiments): build and load lib/librt_s8_<name>.so with RT_EXTRA_HIPCC_FLAGS, objects in their own
# directory — the product library lib/librt_s8.so is never rebuilt in place by an A/B run (round-2 advisor)
VARIANT = os.environ.get("RT_LIB_VARIANT", "")
LIB_PATH = LIB_DIR / (f"librt_s8_{VARIANT}.so" if VARIANT else "librt_s8.so")

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


def _deps() -> list[Path]:
    """Everything a library is compiled from: every file under csrc/, subdirectories included (a new header cannot be forgotten; a
    stray file there costs a rebuild, never a stale library), the C header, this recipe."""
    return sorted(f for f in CSRC.rglob("*") if f.is_file()) + [ROOT / "include" / "rt_tile.h", Path(__file__)]


FLAGS_PATH = LIB_PATH.with_suffix(".flags")      # the exact compile lines of the library next to it

# The TEST library: the product sources plus -DRT_DEBUG_HOOKS, which compiles the rt_debug_* entry points (launch-path knobs,
# counter read-back, a throwing body, the sqrt self-test, the unit kernels of rt_unit.hip.h and rt_unit_sampling.hip.h) that tests
# and tools use.
# The product library exports exactly include/rt_tile.h (tests/test_surface.py checks both).
DEBUG_VARIANT = "dbg"
DEBUG_FLAGS = ["-DRT_DEBUG_HOOKS"]
DEBUG_LIB_PATH = LIB_DIR / f"librt_s8_{DEBUG_VARIANT}.so"


# The FILM library: the moments fold and the variance-guided resolve of film.py, a second, private library that
# only ray_tracer_s8_amd/_film_lib.py loads.  Its sources lie beside csrc/, not under it (_deps() globs csrc/ for the libraries
# above), it exports only rtf_* names, and it takes no RT_EXTRA_HIPCC_FLAGS: experiments are the product library's.
FILM_CSRC = PKG / "film_csrc"
FILM_UNIT = "rt_film.hip"
FILM_FLAGS = ["-fno-slp-vectorize"]
FILM_LIB_PATH = LIB_DIR / "librt_film.so"
FILM_FLAGS_PATH = FILM_LIB_PATH.with_suffix(".flags")


def _film_deps() -> list[Path]:
    """What the film library is compiled from: film_csrc/, the three csrc/ headers it includes (and the C header rt_plan.h reads),
    this recipe."""
    return sorted(f for f in FILM_CSRC.rglob("*") if f.is_file()) + [CSRC / "rt_denoise_math.h", CSRC / "rt_consts.h", CSRC / "rt_plan.h",
                                                                    ROOT / "include" / "rt_tile.h", Path(__file__)]


# The HISTORY library: the temporal accumulation of film_history.py, a third, private library that only
# ray_tracer_s8_amd/_history_lib.py loads.  Built like the film library: sources beside csrc/, rth_* exports only, the product's flags
# plus -fno-slp-vectorize, no RT_EXTRA_HIPCC_FLAGS, a record and a staleness check of its own.
HISTORY_CSRC = PKG / "history_csrc"
HISTORY_UNIT = "rt_history.hip"
HISTORY_FLAGS = ["-fno-slp-vectorize"]
HISTORY_LIB_PATH = LIB_DIR / "librt_history.so"
HISTORY_FLAGS_PATH = HISTORY_LIB_PATH.with_suffix(".flags")


def _history_deps() -> list[Path]:
    """What the history library is compiled from: history_csrc/, the two csrc/ headers it includes (and the C header they read), this
    recipe."""
    return sorted(f for f in HISTORY_CSRC.rglob("*") if f.is_file()) + [CSRC / "rt_consts.h", CSRC / "rt_plan.h",
                                                                       ROOT / "include" / "rt_tile.h", Path(__file__)]


def _extra_flags() -> list[str]:
    return os.environ.get("RT_EXTRA_HIPCC_FLAGS", "").split()          # experiments only (e.g. -DRT_MAXC=12)


def flags_record(extra: list[str] | None = None) -> str:
    """What the library was (or would be) compiled with: one line per translation unit.  A library whose record differs
    from the flags asked for NOW is stale whatever its mtime — an A/B script that died before restoring the default
    build (tools/ab*.sh, phase_time.py: -DRT_PROFILE_TIME, experimental -D knobs) would otherwise leave a variant that
    looks fresh, travels to the GPU box and gets benchmarked."""
    extra = _extra_flags() if extra is None else extra
    common = [f for f in HIPCC_FLAGS if f != "-shared"] + extra
    return "".join(f"{unit}: {' '.join(common + flags)}\n" for unit, flags in UNITS)


def built_with_default_flags() -> bool:
    """True iff the library on disk was compiled with exactly HIPCC_FLAGS (no RT_EXTRA_HIPCC_FLAGS)."""
    return LIB_PATH.exists() and FLAGS_PATH.exists() and FLAGS_PATH.read_text() == flags_record([])


def needs_build() -> bool:
    if not LIB_PATH.exists() or not FLAGS_PATH.exists():
        return True
    if VARIANT and "RT_EXTRA_HIPCC_FLAGS" not in os.environ:
        return False          # a prebuilt experiment variant is used as it was built (its flags are in its record)
    if FLAGS_PATH.read_text() != flags_record():
        return True
    t = LIB_PATH.stat().st_mtime
    return any(d.stat().st_mtime > t for d in _deps())


def _compile(lib_path: Path, flags_path: Path, obj_dir: Path, extra: list[str], verbose: bool) -> Path:
    LIB_DIR.mkdir(parents=True, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "hipcc")
    if flags_path.exists():
        flags_path.unlink()                       # no record while the objects are in flux
    obj_dir.mkdir(exist_ok=True)
    common = [f for f in HIPCC_FLAGS if f != "-shared"] + extra + [f"-I{ROOT / 'include'}", f"-I{CSRC}"]
    cmds, objs = [], []
    for unit, flags in UNITS:
        obj = obj_dir / (Path(unit).stem + ".o")
        objs.append(str(obj))
        cmds.append([hipcc, *common, *flags, "-c", str(CSRC / unit), "-o", str(obj)])
    cmds.append([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(lib_path), *objs])
    # the compiles are independent: run them side by side, then link
    procs = []
    for cmd in cmds[:-1]:
        if verbose:
            print(" ".join(cmd))
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for cmd, pr in zip(cmds[:-1], procs):
        so, se = pr.communicate()
        if pr.returncode != 0:
            raise RuntimeError(f"hipcc failed ({pr.returncode}): {' '.join(cmd)}\n{so}\n{se}")
    if verbose:
        print(" ".join(cmds[-1]))
    proc = subprocess.run(cmds[-1], capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"hipcc link failed ({proc.returncode}):\n{proc.stdout}\n{proc.stderr}")
    flags_path.write_text(flags_record(extra))
    return lib_path


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile librt_s8.so (or the RT_LIB_VARIANT named) if missing or stale, and with no variant named the film library and the
    history library next to it.  Raises on failure (no fallback)."""
    if not VARIANT:
        build_film(force, verbose)
        build_history(force, verbose)
    if not force and not needs_build():
        return LIB_PATH
    return _compile(LIB_PATH, FLAGS_PATH, LIB_DIR / (f"obj_{VARIANT}" if VARIANT else "obj"), _extra_flags(), verbose)


def build_debug(force: bool = False, verbose: bool = False) -> Path:
    """Compile the test library lib/librt_s8_dbg.so (product sources + -DRT_DEBUG_HOOKS) if missing or stale."""
    fp = DEBUG_LIB_PATH.with_suffix(".flags")
    stale = (not DEBUG_LIB_PATH.exists() or not fp.exists() or fp.read_text() != flags_record(DEBUG_FLAGS)
             or any(d.stat().st_mtime > DEBUG_LIB_PATH.stat().st_mtime for d in _deps()))
    if not force and not stale:
        return DEBUG_LIB_PATH
    return _compile(DEBUG_LIB_PATH, fp, LIB_DIR / f"obj_{DEBUG_VARIANT}", DEBUG_FLAGS, verbose)


def film_flags_record() -> str:
    """The compile line of the film library's one translation unit (its own record, lib/librt_film.flags)."""
    return f"{FILM_UNIT}: {' '.join([f for f in HIPCC_FLAGS if f != '-shared'] + FILM_FLAGS)}\n"


def film_needs_build() -> bool:
    if not FILM_LIB_PATH.exists() or not FILM_FLAGS_PATH.exists() or FILM_FLAGS_PATH.read_text() != film_flags_record():
        return True
    t = FILM_LIB_PATH.stat().st_mtime
    return any(d.stat().st_mtime > t for d in _film_deps())


def build_film(force: bool = False, verbose: bool = False) -> Path:
    """Compile lib/librt_film.so (film_csrc/) if missing or stale: the product's flags, linked like the product
    library, with a flags record and a staleness check of its own.  Raises on failure (no fallback)."""
    if not force and not film_needs_build():
        return FILM_LIB_PATH
    LIB_DIR.mkdir(parents=True, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "hipcc")
    if FILM_FLAGS_PATH.exists():
        FILM_FLAGS_PATH.unlink()
    obj_dir = LIB_DIR / "obj_film"
    obj_dir.mkdir(exist_ok=True)
    obj = obj_dir / (Path(FILM_UNIT).stem + ".o")
    common = [f for f in HIPCC_FLAGS if f != "-shared"] + FILM_FLAGS
    cmds = [[hipcc, *common, f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-I{FILM_CSRC}", "-c", str(FILM_CSRC / FILM_UNIT), "-o", str(obj)],
            [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(FILM_LIB_PATH), str(obj)]]
    for cmd in cmds:
        if verbose:
            print(" ".join(cmd))
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError(f"hipcc failed ({proc.returncode}): {' '.join(cmd)}\n{proc.stdout}\n{proc.stderr}")
    FILM_FLAGS_PATH.write_text(film_flags_record())
    return FILM_LIB_PATH


def history_flags_record() -> str:
    """The compile line of the history library's one translation unit (its own record, lib/librt_history.flags)."""
    return f"{HISTORY_UNIT}: {' '.join([f for f in HIPCC_FLAGS if f != '-shared'] + HISTORY_FLAGS)}\n"


def history_needs_build() -> bool:
    if (not HISTORY_LIB_PATH.exists() or not HISTORY_FLAGS_PATH.exists()
            or HISTORY_FLAGS_PATH.read_text() != history_flags_record()):
        return True
    t = HISTORY_LIB_PATH.stat().st_mtime
    return any(d.stat().st_mtime > t for d in _history_deps())


def build_history(force: bool = False, verbose: bool = False) -> Path:
    """Compile lib/librt_history.so (history_csrc/) if missing or stale, as build_film compiles the film library.
    Raises on failure (no fallback)."""
    if not force and not history_needs_build():
        return HISTORY_LIB_PATH
    LIB_DIR.mkdir(parents=True, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "hipcc")
    if HISTORY_FLAGS_PATH.exists():
        HISTORY_FLAGS_PATH.unlink()
    obj_dir = LIB_DIR / "obj_history"
    obj_dir.mkdir(exist_ok=True)
    obj = obj_dir / (Path(HISTORY_UNIT).stem + ".o")
    common = [f for f in HIPCC_FLAGS if f != "-shared"] + HISTORY_FLAGS
    cmds = [[hipcc, *common, f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-I{HISTORY_CSRC}", "-c", str(HISTORY_CSRC / HISTORY_UNIT),
             "-o", str(obj)],
            [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(HISTORY_LIB_PATH), str(obj)]]
    for cmd in cmds:
        if verbose:
            print(" ".join(cmd))
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError(f"hipcc failed ({proc.returncode}): {' '.join(cmd)}\n{proc.stdout}\n{proc.stderr}")
    HISTORY_FLAGS_PATH.write_text(history_flags_record())
    return HISTORY_LIB_PATH


if __name__ == "__main__":
    print(build(force=True, verbose=True))
    if not VARIANT:
        print(build_debug(force=True, verbose=True))
        print(build_film(force=True, verbose=True))
        print(build_history(force=True, verbose=True))
