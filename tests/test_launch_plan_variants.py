"""The launch plan's choice of a variant of the LDS-tree kernels (csrc/rt_plan.h through a g++ harness, as tests/test_launch_plan.py):
Plan::tris, the sphere-only instantiation for worlds without triangles, and plain_frame, the launches that may commit through the
copy of the commit without the launch-uniform tests.  What the variants render is tests/test_gpu_ltree_variants.py's business."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
SRC = ROOT / "tests" / "host" / "plan_variants_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "libplan_variants_host.so"
DEPS = [SRC, CSRC / "rt_plan.h", CSRC / "rt_consts.h", ROOT / "include" / "rt_tile.h"]

F_LINEAR_SCAN, F_NO_LDS_TREE, F_CULL_WALK, F_NO_CULL_WALK = 1 << 5, 1 << 8, 1 << 10, 1 << 11


@pytest.fixture(scope="module")
def lib():
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                        "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    l.plan_variants.argtypes = [C.c_uint32] * 9 + [C.c_int] * 4 + [C.c_void_p]
    l.sphere_only_max_tris.restype = C.c_uint32
    return l


def plan(lib, n_sph=1024, n_tri=0, depth=12, flags=0, width=3840, height=2160, spp=8, passes=None, ltree_general=0, plain_frame=1,
         lds_tree=1):
    out = np.zeros(6, np.int32)
    b, e = passes if passes else (0, spp)
    lib.plan_variants(n_sph, n_tri, depth, flags, width, height, spp, b, e, 1 if passes else 0, ltree_general, plain_frame, lds_tree,
                      out.ctypes.data)
    return dict(zip(["engine", "tris", "plain_shape", "plain", "plain_with_f32", "plain_with_cost"], out.tolist()))


def test_sphere_only_kernel_only_without_triangles(lib):
    assert lib.sphere_only_max_tris() == 0
    for flags, engine in ((0, 4), (F_NO_CULL_WALK, 4), (F_CULL_WALK, 7)):
        assert plan(lib, flags=flags) == dict(engine=engine, tris=0, plain_shape=1, plain=1, plain_with_f32=0, plain_with_cost=0)
        assert plan(lib, n_sph=40, depth=7, flags=flags)["tris"] == 0
        for n_sph, n_tri in ((1023, 1), (20, 12), (0, 500)):                       # one triangle is enough
            r = plan(lib, n_sph=n_sph, n_tri=n_tri, flags=flags)
            assert r["engine"] == engine and r["tris"] == 1, (n_sph, n_tri, r)
        assert plan(lib, flags=flags, ltree_general=1)["tris"] == 1                # the knob forces the general kernel
    assert plan(lib, n_sph=2)["engine"] == 4 and plan(lib, n_sph=2)["tris"] == 0


def test_other_engines_have_one_kernel(lib):
    for kw in (dict(flags=F_LINEAR_SCAN), dict(flags=F_NO_LDS_TREE), dict(lds_tree=0), dict(n_sph=9000, depth=15), dict(n_sph=1)):
        r = plan(lib, **kw)
        assert r["engine"] not in (4, 7) and r["tris"] == 1 and r["plain_shape"] == 0 and r["plain"] == 0, (kw, r)


def test_plain_frame_is_the_flagship_shape(lib):
    assert plan(lib)["plain"] == 1                                                 # c3: 8 spp in one pass
    for spp in (8, 16, 64, 4096):                                                  # a power of two from 8 up: one pixel per slot, the mean a product
        assert plan(lib, spp=spp)["plain"] == 1, spp
    for spp in (1, 2, 3, 4, 7):                                                    # below 8: several pixels per slot
        assert plan(lib, spp=spp)["plain_shape"] == 0, spp
    for spp in (9, 24, 100):                                                       # the mean is a division
        assert plan(lib, spp=spp)["plain_shape"] == 0, spp
    assert plan(lib, passes=(0, 8))["plain_shape"] == 0                            # a pass stores its running sum
    assert plan(lib, passes=(0, 3))["plain_shape"] == 0 and plan(lib, passes=(3, 8))["plain_shape"] == 0
    assert plan(lib, spp=16, passes=(8, 16))["plain_shape"] == 0                   # (8 units, a power-of-two end: still a pass)
    r = plan(lib)
    assert r["plain_with_f32"] == 0 and r["plain_with_cost"] == 0                  # what the strips and the caller ask for
    assert plan(lib, plain_frame=0) == dict(r, plain_shape=0, plain=0)             # the knob
    assert plan(lib, n_sph=20, n_tri=12)["plain"] == 1                             # the commit does not care what the world holds
    assert plan(lib, ltree_general=1)["plain"] == 1
