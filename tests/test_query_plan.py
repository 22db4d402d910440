"""The ray-query engine choice (csrc/rt_plan.h plan_query, through a g++ harness): which engine serves a query, with which scan
semantics, slab test and LDS stack, from the scene's shape and the request flags.  That each engine gives the oracle's hits is
tests/test_gpu_query.py's business; here: that the rule says what rt_tile.h says, on the CPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
SRC = ROOT / "tests" / "host" / "query_plan_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "libquery_plan_host.so"
DEPS = [SRC, CSRC / "rt_plan.h", CSRC / "rt_consts.h", ROOT / "include" / "rt_tile.h"]

# include/rt_tile.h
F_EXACT_SCAN, F_NO_BVH_CULL, F_OC_BROAD_PHASE, F_FULL_CHAIN = 1 << 0, 1 << 1, 1 << 2, 1 << 3
F_BVH_TRAVERSE, F_LINEAR_SCAN, F_EXACT_NODES, F_QUANT_NODES = 1 << 4, 1 << 5, 1 << 6, 1 << 7
F_NO_LDS_TREE, F_COUNT_STEPS, F_CULL_WALK, F_NO_CULL_WALK = 1 << 8, 1 << 9, 1 << 10, 1 << 11
F_FRAME = (1 << 12) | (1 << 13) | (1 << 14)
IGNORED = [F_OC_BROAD_PHASE, F_EXACT_NODES, F_QUANT_NODES, F_COUNT_STEPS, F_CULL_WALK, F_NO_CULL_WALK, F_FRAME, F_BVH_TRAVERSE,
           F_NO_LDS_TREE]
WALK, SCAN = 2, 1


@pytest.fixture(scope="module")
def lib():
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                        "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    l.query_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    l.query_trav_stack.restype = C.c_uint32
    l.query_block.restype = C.c_uint32
    return l


def plan(lib, n_sph=1024, n_tri=0, depth=20, inverted=False, flags=0):
    sh = np.array([n_sph, n_tri, depth, int(inverted)], np.uint32)
    out = np.zeros(4, np.uint64)
    lib.query_plan(sh.ctypes.data, flags, out.ctypes.data)
    return dict(engine=int(out[0]), scan_mode=int(out[1]), full_chain=bool(out[2]), lds=int(out[3]))


def test_default_is_the_exact_node_walk_for_every_scene(lib):
    for n_sph, n_tri in [(1, 0), (2, 0), (16, 0), (1024, 0), (65536, 0), (0, 1), (0, 100352), (5, 7)]:
        p = plan(lib, n_sph, n_tri, depth=12)
        assert p["engine"] == WALK and not p["full_chain"], (n_sph, n_tri)
        assert p["lds"] == 13 * lib.query_block() * 4


def test_scan_semantics_follow_the_flags(lib):
    assert plan(lib, flags=F_NO_BVH_CULL) == dict(engine=SCAN, scan_mode=0, full_chain=False, lds=0)
    for f in (F_EXACT_SCAN, F_LINEAR_SCAN, F_EXACT_SCAN | F_LINEAR_SCAN, F_LINEAR_SCAN | F_BVH_TRAVERSE):
        assert plan(lib, flags=f) == dict(engine=SCAN, scan_mode=2, full_chain=False, lds=0), f
    # plain linear semantics win over every engine flag, as in the tile entry points
    assert plan(lib, flags=F_NO_BVH_CULL | F_BVH_TRAVERSE)["scan_mode"] == 0


def test_the_walk_needs_a_tree_that_fits_its_stack(lib):
    top = lib.query_trav_stack()
    assert plan(lib, depth=top - 1)["engine"] == WALK
    assert plan(lib, depth=top - 1)["lds"] == top * lib.query_block() * 4
    deep = plan(lib, depth=top)
    assert deep["engine"] == SCAN and deep["scan_mode"] == 2 and deep["lds"] == 0     # BVH semantics kept
    assert plan(lib, n_sph=0, n_tri=0, depth=0)["engine"] == SCAN                     # empty world: nothing to walk


def test_full_chain_from_the_flag_or_inverted_boxes(lib):
    assert plan(lib, flags=F_FULL_CHAIN)["full_chain"] and plan(lib, flags=F_FULL_CHAIN)["engine"] == WALK
    assert plan(lib, inverted=True)["full_chain"]
    assert plan(lib, inverted=True, flags=F_NO_BVH_CULL)["full_chain"]
    assert not plan(lib)["full_chain"]


@pytest.mark.parametrize("base", [0, F_NO_BVH_CULL, F_EXACT_SCAN, F_FULL_CHAIN])
def test_flags_of_engines_the_query_path_lacks_change_nothing(lib, base):
    ref = plan(lib, flags=base)
    for f in IGNORED:
        assert plan(lib, flags=base | f) == ref, (base, f)
