"""The plan of path tracing of caller rays (csrc/rt_plan.h plan_trace, through a g++ harness): the engine and scan semantics (the
query path's), the slab test, the workgroup size and the LDS layout of the walk stack and the path stack, from the scene's shape, the
request flags and the bounce count.  That the kernels give the oracle's colours is tests/test_gpu_trace.py's business; here: that the
rule says what rt_tile.h says and stays inside a CU's LDS, on the CPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
SRC = ROOT / "tests" / "host" / "trace_plan_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "libtrace_plan_host.so"
DEPS = [SRC, CSRC / "rt_plan.h", CSRC / "rt_consts.h", ROOT / "include" / "rt_tile.h"]

# include/rt_tile.h
F_EXACT_SCAN, F_NO_BVH_CULL, F_OC_BROAD_PHASE, F_FULL_CHAIN = 1 << 0, 1 << 1, 1 << 2, 1 << 3
F_BVH_TRAVERSE, F_LINEAR_SCAN, F_EXACT_NODES, F_QUANT_NODES = 1 << 4, 1 << 5, 1 << 6, 1 << 7
F_NO_LDS_TREE, F_COUNT_STEPS, F_CULL_WALK, F_NO_CULL_WALK = 1 << 8, 1 << 9, 1 << 10, 1 << 11
F_FRAME = (1 << 12) | (1 << 13) | (1 << 14)
IGNORED = [F_OC_BROAD_PHASE, F_EXACT_NODES, F_QUANT_NODES, F_COUNT_STEPS, F_CULL_WALK, F_NO_CULL_WALK, F_FRAME, F_BVH_TRAVERSE,
           F_NO_LDS_TREE]
WALK, SCAN = 2, 1
LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                        "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    l.trace_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    l.trace_trav_stack.restype = C.c_uint32
    l.trace_max_bounces.restype = C.c_uint32
    return l


def plan(lib, n_sph=1024, n_tri=0, depth=20, inverted=False, flags=0, bounces=10):
    sh = np.array([n_sph, n_tri, depth, int(inverted)], np.uint32)
    out = np.zeros(7, np.uint64)
    lib.trace_plan(sh.ctypes.data, flags, bounces, out.ctypes.data)
    return dict(engine=int(out[0]), scan_mode=int(out[1]), full_chain=bool(out[2]), block=int(out[3]), path32=bool(out[4]),
                path_off=int(out[5]), lds=int(out[6]))


def _layout_ok(p, depth, bounces):
    stack = (depth + 1) * 4 if p["engine"] == WALK else 0
    path = (bounces + 1) * (4 if p["path32"] else 2)
    assert p["path_off"] == stack * p["block"]
    assert p["lds"] == (stack + path) * p["block"]
    assert p["block"] in (64, 128, 256)
    assert p["lds"] <= LDS_CU


def test_engine_and_scan_mode_for_every_flag(lib):
    assert plan(lib)["engine"] == WALK and plan(lib)["scan_mode"] == 2 and not plan(lib)["full_chain"]
    p = plan(lib, flags=F_NO_BVH_CULL)
    assert (p["engine"], p["scan_mode"], p["full_chain"]) == (SCAN, 0, False)
    for f in (F_EXACT_SCAN, F_LINEAR_SCAN, F_EXACT_SCAN | F_LINEAR_SCAN, F_LINEAR_SCAN | F_BVH_TRAVERSE):
        p = plan(lib, flags=f)
        assert (p["engine"], p["scan_mode"]) == (SCAN, 2), f
    assert plan(lib, flags=F_NO_BVH_CULL | F_BVH_TRAVERSE)["scan_mode"] == 0
    p = plan(lib, flags=F_FULL_CHAIN)
    assert p["full_chain"] and p["engine"] == WALK
    assert plan(lib, inverted=True)["full_chain"]
    for base in (0, F_NO_BVH_CULL, F_EXACT_SCAN, F_FULL_CHAIN):
        ref = plan(lib, flags=base)
        for f in IGNORED:
            assert plan(lib, flags=base | f) == ref, (base, f)


def test_a_tree_deeper_than_the_stack_takes_the_scan(lib):
    top = lib.trace_trav_stack()
    p = plan(lib, depth=top - 1)
    assert p["engine"] == WALK
    _layout_ok(p, top - 1, 10)
    deep = plan(lib, depth=top)
    assert deep["engine"] == SCAN and deep["scan_mode"] == 2 and deep["path_off"] == 0    # BVH semantics kept, no walk stack
    _layout_ok(deep, top, 10)
    assert plan(lib, n_sph=0, n_tri=0, depth=0)["engine"] == SCAN                          # empty world: nothing to walk


@pytest.mark.parametrize("flags", [0, F_NO_BVH_CULL, F_EXACT_SCAN])
def test_lds_fits_a_cu_at_the_extremes(lib, flags):
    top, mb = lib.trace_trav_stack(), lib.trace_max_bounces()
    for n_sph, n_tri in ((1, 0), (65536, 0), (65537, 0), (0, 100352)):
        for depth in (0, 1, 20, top - 1, top):
            for bounces in (0, 1, 10, mb):
                p = plan(lib, n_sph, n_tri, depth=depth, flags=flags, bounces=bounces)
                _layout_ok(p, depth, bounces)
                assert 2 * p["lds"] <= LDS_CU, (n_sph, n_tri, depth, bounces, p)      # two workgroups a CU, always possible here
    # the largest legal input does not fit two 256-lane workgroups: a smaller block keeps two
    big = plan(lib, 0, 100352, depth=top - 1, bounces=mb)
    assert big["block"] == 128 and big["lds"] == (top + mb + 1) * 4 * 128
    assert plan(lib, 1024, 0, depth=20, bounces=10)["block"] == 256


def test_path_entries_are_u16_up_to_65536_primitives(lib):
    for n_sph, n_tri, wide in ((65536, 0, False), (65535, 1, False), (65537, 0, True), (0, 65537, True), (1, 65536, True),
                               (0, 100352, True), (16, 0, False)):
        p = plan(lib, n_sph, n_tri, depth=12, bounces=8)
        assert p["path32"] == wide, (n_sph, n_tri)
        assert p["lds"] - p["path_off"] == 9 * (4 if wide else 2) * p["block"]
