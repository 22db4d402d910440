"""The launch plan (csrc/rt_plan.h, the product's plan_launch / plan_queue through a g++ harness): which engine renders a launch, its
LDS layout, its sample units and its queue, at the rules' boundaries and as invariants over a seeded grid of scene shapes, requests
and knobs; and the layout of the host forms' staging buffer (stage_layout, the denoiser's list).  What each engine costs on real scenes is tests/test_gpu_engine_rules.py's business; here: that the rules say what they
say, on the CPU."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _knob_matrix as M

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
SRC = ROOT / "tests" / "host" / "plan_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "libplan_host.so"
DEPS = [SRC, CSRC / "rt_plan.h", CSRC / "rt_consts.h", ROOT / "include" / "rt_tile.h"]

# include/rt_tile.h
F_EXACT_SCAN, F_NO_BVH_CULL, F_OC_BROAD_PHASE, F_FULL_CHAIN = 1 << 0, 1 << 1, 1 << 2, 1 << 3
F_BVH_TRAVERSE, F_LINEAR_SCAN, F_EXACT_NODES, F_QUANT_NODES = 1 << 4, 1 << 5, 1 << 6, 1 << 7
F_NO_LDS_TREE, F_COUNT_STEPS, F_CULL_WALK, F_NO_CULL_WALK = 1 << 8, 1 << 9, 1 << 10, 1 << 11
RT_OK, RT_ERR_LIMIT = 0, -8
LEAF_BIT = 0x80000000
NONE = 0xFFFFFFFF

SHAPE_FIELDS = ["n_sph", "n_sph_pad", "n_tri", "bvh_depth", "n_internal", "root_ref", "cull_density", "cull_pays", "xcull_pays",
                "quant_ok", "tri_ok", "r_slack", "inverted_boxes", "expanded", "leaf_density"]
KNOBS = dict(lds_tree=1, cull_walk=-1, no_stage=0, slots=0, commit_slots=0, force_capped=0, stack_lds=0, compact=1,
             refill_eighths=0, tail_tiles=-1)


@pytest.fixture(scope="module")
def lib():
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                        "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    l.plan_field_names.restype = C.c_char_p
    l.plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    l.plan_engine.argtypes = [C.c_int, C.c_void_p]
    l.plan_const.restype = C.c_double
    l.plan_const.argtypes = [C.c_char_p]
    l.names = l.plan_field_names().decode().split(",")
    return l


def K(lib, name):
    v = lib.plan_const(name.encode())
    assert not math.isnan(v), name
    return v


def scene(n_sph, n_tri=0, **kw):
    """A scene shape as build_host_scene would give it, roughly: a balanced tree, spheres of moderate density."""
    n = n_sph + n_tri
    sh = dict(n_sph=n_sph, n_sph_pad=(n_sph + 7) // 8 * 8, n_tri=n_tri, bvh_depth=max(1, math.ceil(math.log2(max(n, 1)))) + 1,
              n_internal=max(n - 1, 0), root_ref=0 if n > 1 else LEAF_BIT, cull_density=1.0, cull_pays=0, xcull_pays=0, quant_ok=1,
              tri_ok=1 if n_tri else 0, r_slack=0.5, inverted_boxes=0, expanded=1, leaf_density=1.0)
    sh.update(kw)
    return sh


def plan(lib, sh, flags=0, width=256, height=64, divisions=1, spp=4, max_bounces=10, n_strips=1, pass_range=None, grid=0, **knobs):
    kn = dict(KNOBS, **knobs)
    shape = np.array([sh[f] for f in SHAPE_FIELDS], np.float64)
    rq = np.array([width, height, divisions, spp, max_bounces, flags, 0.1, 1.0, math.pi / 2, 1.0, 0.001, 1000.0], np.float64)
    kv = np.array([kn[k] for k in KNOBS], np.int32)
    out = np.zeros(len(lib.names), np.float64)
    begin, end = pass_range if pass_range else (0, spp)
    lib.plan(shape.ctypes.data, rq.ctypes.data, n_strips, begin, end, 1 if pass_range else 0, kv.ctypes.data, grid, out.ctypes.data)
    r = dict(zip(lib.names, out.tolist()))
    return {k: (v if k in ("lens_radius", "focus_distance", "u_den", "v_den", "t_min", "t_max", "spp_f", "spp_rcp") or k[:3] in
                ("org", "llc", "hor", "ver") else int(v)) for k, v in r.items()}


def engine(lib, sh, **kw):
    r = plan(lib, sh, **kw)
    assert r["status"] == RT_OK
    return r["engine"]


# ---------------------------------------------------------------------------------------------------- engine choice


def test_scan_below_two_primitives_tree_from_two(lib):
    assert K(lib, "TRAVERSE_MIN_PRIMS") == 2
    assert engine(lib, scene(1)) == 0
    assert engine(lib, scene(2)) == 4
    assert engine(lib, scene(1), flags=F_BVH_TRAVERSE) >= 2             # the flag forces the walk whatever the size
    assert engine(lib, scene(0, 1)) == 0 and engine(lib, scene(0, 2)) == 4


def test_dense_pile_keeps_the_scan(lib):
    assert K(lib, "DENSE_SCAN_MAX_PRIMS") == 192
    assert engine(lib, scene(192, cull_density=3.0)) == 0
    assert engine(lib, scene(193, cull_density=3.0)) == 7               # (culled LDS tree: density >= 2.2)
    assert engine(lib, scene(192, cull_density=np.float32(2.99))) == 7
    assert engine(lib, scene(192, cull_density=3.0), flags=F_BVH_TRAVERSE) == 7
    assert engine(lib, scene(100, 92, cull_density=3.0)) == 7           # triangles: never a pile


def test_tree_depth_must_fit_the_traversal_stack(lib):
    ts = int(K(lib, "TRAV_STACK"))
    assert engine(lib, scene(1000, bvh_depth=ts - 1)) >= 2
    assert engine(lib, scene(1000, bvh_depth=ts)) == 0
    assert engine(lib, scene(1000, bvh_depth=ts), flags=F_BVH_TRAVERSE) == 0
    assert engine(lib, scene(3000, bvh_depth=ts)) == 1                  # (streamed: more spheres than one LDS chunk)


def _lds_tree_bytes(lib, n_internal, n_prims, bvh_depth, max_bounces):
    lane = (K(lib, "MAXL_LTREE") + max_bounces + 1 + bvh_depth + 2) * 2
    return int(((n_internal + 2) * K(lib, "LNODE_DW") + n_prims) * 4 + 16 + lane * K(lib, "LTREE_BLOCK"))


def test_lds_tree_fits_to_the_byte(lib):
    limit = int(K(lib, "LDS_LIMIT"))
    depth, mb, n_internal = 10, 10, 1000
    n_prims = (limit - _lds_tree_bytes(lib, n_internal, 0, depth, mb)) // 4
    assert _lds_tree_bytes(lib, n_internal, n_prims, depth, mb) == limit          # (the sizes are whole dwords: limit, limit + 4)
    base = dict(bvh_depth=depth, n_internal=n_internal, quant_ok=0, cull_density=1.0)
    r = plan(lib, scene(n_prims, **base), max_bounces=mb)
    assert r["engine"] == 4 and r["block"] == K(lib, "LTREE_BLOCK") and r["lds"] <= limit
    assert engine(lib, scene(n_prims + 1, **base), max_bounces=mb) == 2
    assert engine(lib, scene(n_prims, **dict(base, n_internal=n_internal + 1)), max_bounces=mb) == 2
    assert engine(lib, scene(n_prims, **base), max_bounces=mb + 1) == 2
    assert engine(lib, scene(n_prims, **base), max_bounces=mb, flags=F_NO_LDS_TREE) == 2
    assert engine(lib, scene(n_prims, **base), max_bounces=mb, lds_tree=0) == 2


def test_quantised_nodes(lib):
    qmin = int(K(lib, "RT_QNODES_MIN_PRIMS"))
    assert qmin == 4096
    sparse = dict(cull_density=0.1)                                      # (below the field rule)
    assert engine(lib, scene(qmin - 1, **sparse)) == 2
    assert engine(lib, scene(qmin, **sparse)) == 3
    assert engine(lib, scene(qmin, **sparse, quant_ok=0)) == 2
    assert engine(lib, scene(qmin, **sparse), flags=F_EXACT_NODES) == 2
    # triangles > spheres: the exact nodes
    assert engine(lib, scene(qmin // 2, qmin // 2 + 1, **sparse)) == 2
    assert engine(lib, scene(qmin // 2 + 1, qmin // 2, **sparse)) == 3
    # field_mid: a sphere field whose tree does not fit LDS, from a box density of 0.15
    deep = dict(bvh_depth=40)
    assert K(lib, "FIELD_MID_MIN_DENSITY") == np.float32(0.15)
    assert engine(lib, scene(1000, cull_density=np.float32(0.15), **deep)) == 3
    assert engine(lib, scene(1000, cull_density=np.float32(0.149), **deep)) == 2
    assert engine(lib, scene(1000, cull_density=np.float32(0.15))) == 4         # (the tree fits LDS: the LDS tree)
    # dense_mid: cull_pays, density 2.5, 512 primitives, tree not in LDS (with triangles, where field_mid does not apply)
    assert K(lib, "DENSE_MID_MIN_DENSITY") == 2.5 and K(lib, "DENSE_MID_MIN_PRIMS") == 512
    dm = dict(cull_pays=1, cull_density=2.5, **deep)
    assert engine(lib, scene(100, 412, **dm)) == 3
    assert engine(lib, scene(100, 411, **dm)) == 2
    assert engine(lib, scene(100, 412, **dict(dm, cull_density=np.float32(2.49)))) == 2
    assert engine(lib, scene(100, 412, **dict(dm, cull_pays=0))) == 2
    assert engine(lib, scene(100, 412, **dm), flags=F_NO_CULL_WALK) == 2
    assert engine(lib, scene(100, 412, **dm), flags=F_QUANT_NODES) == 3


def test_lds_tree_culls_from_density_2_2(lib):
    assert K(lib, "LT_CULL_MIN_DENSITY") == np.float32(2.2)
    assert engine(lib, scene(100, cull_density=np.float32(2.2))) == 7
    assert engine(lib, scene(100, cull_density=np.float32(2.19))) == 4
    assert engine(lib, scene(100, 50, cull_density=np.float32(2.2))) == 7
    assert engine(lib, scene(100, 50, cull_density=np.float32(2.2), tri_ok=0)) == 4


# ---------------------------------------------------------------------------------------------------- premises and flags


def test_scan_forcing_flags(lib):
    for f in (F_LINEAR_SCAN, F_EXACT_SCAN, F_NO_BVH_CULL):
        assert engine(lib, scene(100), flags=f) == 0
        assert engine(lib, scene(5000), flags=f | F_BVH_TRAVERSE) == 1


def test_node_format_flags(lib):
    assert engine(lib, scene(100), flags=F_NO_LDS_TREE) == 3                  # (field_mid)
    assert engine(lib, scene(100, quant_ok=0), flags=F_NO_LDS_TREE) == 2
    assert engine(lib, scene(100, cull_density=0.1), flags=F_NO_LDS_TREE | F_QUANT_NODES) == 3
    assert engine(lib, scene(100, cull_density=0.1, quant_ok=0), flags=F_NO_LDS_TREE | F_QUANT_NODES) == 2
    assert engine(lib, scene(100), flags=F_QUANT_NODES) == 3                  # (a quantised walk is never the LDS tree)
    assert engine(lib, scene(100), flags=F_EXACT_NODES) == 4
    assert engine(lib, scene(5000), flags=F_EXACT_NODES | F_QUANT_NODES) == 2


@pytest.mark.parametrize("kind", ["quant", "exact", "ltree"])
def test_cull_walk_precedence(lib, kind):
    """Request flag over the RT_CULL_WALK knob over the host rule, for each of the three culled walks."""
    if kind == "quant":
        rule_on, rule_off, culled, plain = scene(5000, cull_pays=1), scene(5000, cull_pays=0), 5, 3
    elif kind == "exact":
        rule_on, rule_off, culled, plain = (scene(100, 5000, xcull_pays=1), scene(100, 5000, xcull_pays=0), 6, 2)
    else:
        rule_on, rule_off, culled, plain = scene(300, cull_density=3.0), scene(300, cull_density=1.0), 7, 4
    assert engine(lib, rule_on) == culled and engine(lib, rule_off) == plain
    assert engine(lib, rule_off, cull_walk=1) == culled and engine(lib, rule_on, cull_walk=0) == plain
    for knob in (-1, 0, 1):
        for sh in (rule_on, rule_off):
            assert engine(lib, sh, flags=F_CULL_WALK, cull_walk=knob) == culled
            assert engine(lib, sh, flags=F_NO_CULL_WALK, cull_walk=knob) == plain
            assert engine(lib, sh, flags=F_CULL_WALK | F_NO_CULL_WALK, cull_walk=knob) == plain


def test_culling_premises(lib):
    for bad in (math.inf, math.nan):
        assert engine(lib, scene(5000, r_slack=bad), flags=F_CULL_WALK) == 3
        assert engine(lib, scene(100, 5000, r_slack=bad), flags=F_CULL_WALK) == 2
        assert engine(lib, scene(100, r_slack=bad), flags=F_CULL_WALK) == 4
    assert engine(lib, scene(100, 5000, tri_ok=0), flags=F_CULL_WALK) == 2
    assert engine(lib, scene(5000, 100), flags=F_CULL_WALK) == 3               # the quantised culled walk: spheres only
    # inverted boxes: no culled exact-node or LDS-tree walk, and the whole box chain throughout
    for sh, eng in ((scene(100, 5000, inverted_boxes=1), 2), (scene(100, inverted_boxes=1), 4), (scene(5000, inverted_boxes=1), 5)):
        r = plan(lib, sh, flags=F_CULL_WALK)
        assert r["engine"] == eng and r["flags"] == F_CULL_WALK | F_FULL_CHAIN
    assert plan(lib, scene(100), flags=F_CULL_WALK)["flags"] == F_CULL_WALK


def test_force_capped_takes_the_capped_kernel(lib):
    rows = {e: _engine_row(lib, e) for e in range(8)}
    for sh, e in ((scene(5000, bvh_depth=12), 3), (scene(5000, bvh_depth=12, cull_pays=1), 5)):   # (13 stack entries per lane)
        r = plan(lib, sh)
        assert r["engine"] == e and not r["capped"] and r["isect"] == rows[e][0] and r["stack_lds"] == 13
        r = plan(lib, sh, force_capped=1)
        assert r["engine"] == e and r["capped"] and r["isect"] == rows[e][1]
        assert r["stack_lds"] == K(lib, "STACK_LDS_MAX") == 12 and r["ovf_entries"] == 1
        r = plan(lib, sh, force_capped=1, stack_lds=5, grid=256)
        assert r["capped"] and r["stack_lds"] == 5 and r["ovf_words"] == 8 * r["ovf_stride"] > 0
        r = plan(lib, sh, force_capped=1, stack_lds=13)                        # the whole stack fits: not capped
        assert not r["capped"] and r["isect"] == rows[e][0] and r["stack_lds"] == 13 and r["ovf_entries"] == 0
    r = plan(lib, scene(5000, bvh_depth=20))                                   # a deep tree is capped without the knob
    assert r["capped"] and r["isect"] == rows[3][1]


# ---------------------------------------------------------------------------------------------------- engine table


def _engine_row(lib, e):
    out = np.zeros(3, np.int32)
    lib.plan_engine(e, out.ctypes.data)
    return out.tolist()


def _kernel_cases(unit):
    src = (CSRC / unit).read_text()
    return {int(c) for c in re.findall(r"case (\d+):", src)}


def test_engine_table(lib):
    rows = [_engine_row(lib, e) for e in range(8)]
    isects = [r[0] for r in rows] + [r[1] for r in rows if r[1] >= 0]
    assert len(set(isects)) == len(isects) == 10 == K(lib, "N_ISECT")
    linear, trav = _kernel_cases("rt_kernels_lin.hip"), _kernel_cases("rt_kernels_trav.hip")
    assert linear == {0, 1} and trav == set(range(2, 10))
    for e, (isect, capped, block) in enumerate(rows):
        assert isect in (linear if e < 2 else trav)
        assert capped == -1 or capped in trav
        assert block == (K(lib, "LTREE_BLOCK") if e in (4, 7) else K(lib, "BLOCK"))
    assert [e for e in range(8) if rows[e][1] >= 0] == [3, 5]


# ---------------------------------------------------------------------------------------------------- invariants


def _regions(lib, r):
    """LDS regions [start, end) of the plan, sized from its own parameters."""
    block, depth = r["block"], r["depth"]
    if r["engine"] in (4, 7):
        nodes = ((r["n_internal"] + 2) * K(lib, "LNODE_DW") + r["n_sph"] + r["n_tri"]) * 4
        stack = r["lds"] - r["lds_stack_off"]
        assert stack % (2 * block) == 0
        regs = [(0, nodes), (r["lds_cand_off"], r["lds_cand_off"] + r["maxl"] * block * 2),
                (r["lds_path_off"], r["lds_path_off"] + depth * block * 2), (r["lds_stack_off"], r["lds"])]
        assert r["lds_cand_off"] % 16 == 0
        return regs
    trav = r["engine"] >= 2
    geom = 0 if trav else r["chunk"] * 16
    cand = r["maxl"] * block * (2 if r["list16"] else 4) if trav else K(lib, "MAXC") * block * 2
    path = depth * block * (4 if r["path32"] else 2)
    rr = r["chunk"] * 4 if r["expanded"] else 0
    stack = r["stack_lds"] * block * 4 if trav else 0
    regs = [(0, geom), (r["lds_cand_off"], r["lds_cand_off"] + cand), (r["lds_path_off"], r["lds_path_off"] + path),
            (r["lds_rr_off"], r["lds_rr_off"] + rr), (r["lds_stack_off"], r["lds_stack_off"] + stack)]
    if r["lds_cmp_off"] != NONE:
        regs.append((r["lds_cmp_off"], r["lds_cmp_off"] + 1024 * block // 64))
    if r["lds_stage_off"] != NONE:
        regs.append((r["lds_stage_off"], r["lds_stage_off"] + K(lib, "STAGE_TILES") * K(lib, "STAGE_TILE_BYTES") * block // 64))
    for off in (r["lds_cmp_off"], r["lds_stage_off"]):
        assert off == NONE or off % 16 == 0
    return regs


def _random_case(rng):
    n_sph = int(rng.choice([0, 1, 2, rng.integers(3, 200), rng.integers(200, 5000), rng.integers(5000, 100000)]))
    n_tri = int(rng.choice([0, 0, rng.integers(1, 500), rng.integers(500, 200000)]))
    if n_sph + n_tri == 0:
        n_sph = 1
    sh = scene(n_sph, n_tri, bvh_depth=int(rng.integers(1, 70)), cull_density=float(rng.choice([0.05, 0.15, 1.0, 2.2, 2.5, 3.0, 8.0])),
               cull_pays=int(rng.integers(2)), xcull_pays=int(rng.integers(2)), quant_ok=int(rng.integers(2)), tri_ok=int(rng.integers(2)),
               r_slack=float(rng.choice([0.5, math.inf])), inverted_boxes=int(rng.random() < 0.1), expanded=int(rng.integers(2)))
    flags = 0
    for f in (F_EXACT_SCAN, F_NO_BVH_CULL, F_OC_BROAD_PHASE, F_BVH_TRAVERSE, F_LINEAR_SCAN, F_EXACT_NODES, F_QUANT_NODES, F_NO_LDS_TREE,
              F_COUNT_STEPS, F_CULL_WALK, F_NO_CULL_WALK):
        if rng.random() < 0.12:
            flags |= f
    spp = int(rng.choice([1, 3, 4, 16, 17, 33, 100, 4096]))
    kw = dict(flags=flags, width=int(rng.integers(1, 4000)), height=int(rng.integers(1, 2200)), divisions=1, spp=spp,
              max_bounces=int(rng.choice([0, 4, 10, 63])), n_strips=int(rng.integers(1, 65)), grid=int(rng.integers(1, 2000)))
    kw["divisions"] = int(rng.integers(1, kw["height"] + 1))
    if rng.random() < 0.3:
        b = int(rng.integers(0, spp))
        kw["pass_range"] = (b, int(rng.integers(b + 1, spp + 1)))
    if rng.random() < 0.3:
        kw.update(lds_tree=int(rng.integers(2)), cull_walk=int(rng.integers(-1, 2)), no_stage=int(rng.integers(2)),
                  force_capped=int(rng.integers(2)), stack_lds=int(rng.integers(0, 20)), compact=int(rng.integers(2)))
    return sh, kw


def test_plan_invariants_over_a_seeded_grid(lib):
    rng = np.random.default_rng(20261016)
    limit = K(lib, "LDS_LIMIT")
    seen = set()
    for _ in range(4000):
        sh, kw = _random_case(rng)
        r = plan(lib, sh, **kw)
        if r["status"] != RT_OK:
            assert r["status"] == RT_ERR_LIMIT and (r["lds"] > limit or r["tiles_per_strip"] * kw["n_strips"] > 0x1FFFFFFF)
            continue
        seen.add(r["engine"])
        assert r["lds"] <= limit
        regs = sorted((a, b) for a, b in _regions(lib, r) if b > a)
        assert all(b <= r["lds"] for _, b in regs), (sh, kw, r)
        assert all(b1 <= a2 for (_, b1), (a2, _) in zip(regs, regs[1:])), (sh, kw, r)
        assert r["isect"] == _engine_row(lib, r["engine"])[1 if r["capped"] else 0]
        # the queue
        waves = r["blocks"] * r["block"] // 64
        assert 1 <= r["blocks"] <= kw["grid"] and (r["blocks"] == kw["grid"] or r["blocks"] * r["block"] // 64 <= r["tiles_total"] + 63)
        conv = r["tiles_total"] - r["tiles_big"]
        assert r["n_tiles"] == r["tiles_big"] + (conv << r["sub_shift"]) < 2 ** 31
        assert r["ovf_stride"] == r["blocks"] * r["block"]
        assert r["ring_bytes"] == waves * r["n_slots"] * r["slot_stride"] * 12
    assert seen == set(range(8))


# ---------------------------------------------------------------------------------------------------- sample units


def test_sample_units_for_every_upp(lib):
    slots_max = int(K(lib, "SLOTS_MAX"))
    sh = scene(100)
    for upp in range(1, 4097):
        r = plan(lib, sh, spp=upp)
        grp = r["grp"]
        assert grp * upp >= 8 and (grp == 1 or (grp - 1) * upp < 8)
        u = grp * upp
        fewest = 16 if u <= 256 else 8 if u <= 1024 else 4
        assert r["n_slots"] == min(slots_max, max(fewest, 384 // u))
        assert r["slot_stride"] == 1 + u
        assert 1 <= r["commit_slots"] == max(1, r["n_slots"] // 4) <= r["n_slots"]
        assert r["spp_magic"] == (0 if upp == 1 else (1 << 32) // upp + 1)
        assert r["slotu_magic"] == (1 << 32) // u + 1
        assert r["grp_magic"] == (0 if grp == 1 else (1 << 32) // grp + 1)
    assert plan(lib, sh, spp=4, slots=40)["n_slots"] == slots_max
    assert plan(lib, sh, spp=4, slots=5, commit_slots=9)["commit_slots"] == 5


def _magic_divides(d, magic):
    q = np.arange(65 * d, dtype=np.uint64)
    return bool(np.array_equal((q * np.uint64(magic)) >> np.uint64(32), q // np.uint64(d)))


def test_magic_divisors_are_exact(lib):
    """q / d == mulhi(q, magic) for every q < 65 d: every unit count of a pixel (spp_magic) and of a slot (slotu_magic)."""
    sh = scene(100)
    checked = set()
    for upp in range(1, 4097):
        r = plan(lib, sh, spp=upp)
        if upp > 1:
            assert _magic_divides(upp, r["spp_magic"]), upp
        u = r["grp"] * upp
        if u not in checked:
            assert _magic_divides(u, r["slotu_magic"]), u
            checked.add(u)


def test_pass_range(lib):
    r = plan(lib, scene(100), spp=100, pass_range=(40, 64))
    assert (r["upp"], r["spp_all"], r["s_begin"], r["gap"], r["acc_out"], r["spp_f"], r["spp_rcp"]) == (24, 100, 40, 76, 1, 64.0, 1 / 64)
    r = plan(lib, scene(100), spp=100)
    assert (r["upp"], r["s_begin"], r["gap"], r["acc_out"], r["spp_f"], r["spp_rcp"]) == (100, 0, 0, 0, 100.0, 0.0)


# ---------------------------------------------------------------------------------------------------- queue parts


def test_all_parts_below_16_tiles_per_wave_or_above_16_spp(lib):
    sh = scene(1)                                                         # (the scan: 4 waves per workgroup)
    kw = dict(width=256, height=64)                                       # 4 x 64 = 256 tiles
    r = plan(lib, sh, spp=4, grid=4, **kw)                                # 16 waves: 16 tiles each -> whole tiles, the last 2 per wave in quarters
    assert (r["tiles_total"], r["tiles_big"], r["sub_shift"], r["n_tiles"]) == (256, 224, 2, 224 + (32 << 2))
    r = plan(lib, sh, spp=4, grid=5, **kw)                                # 20 waves: fewer than 16 tiles each -> all in parts
    assert (r["tiles_big"], r["n_tiles"]) == (0, 256 << 2)
    assert plan(lib, sh, spp=16, grid=4, **kw)["tiles_big"] == 224
    assert plan(lib, sh, spp=17, grid=4, **kw)["tiles_big"] == 0
    r = plan(lib, sh, spp=4, grid=4, tail_tiles=10, **kw)
    assert (r["tiles_big"], r["n_tiles"]) == (246, 246 + (10 << 2))
    r = plan(lib, sh, spp=4, grid=5, tail_tiles=0, **kw)
    assert (r["tiles_big"], r["n_tiles"]) == (256, 256)


def test_sixteenths_from_33_spp_and_the_31_bit_limit(lib):
    sh = scene(1)
    assert plan(lib, sh, spp=32, grid=4)["sub_shift"] == 2
    assert plan(lib, sh, spp=33, grid=4)["sub_shift"] == 4
    # one tile per row: tiles_total = rows; every tile in sixteenths while 16 x tiles fits 31 bits
    r = plan(lib, sh, spp=33, width=64, height=2 ** 27 - 1, grid=1000)
    assert (r["sub_shift"], r["n_tiles"]) == (4, (2 ** 27 - 1) << 4)
    r = plan(lib, sh, spp=33, width=64, height=2 ** 27, grid=1000)
    assert (r["sub_shift"], r["n_tiles"]) == (2, 2 ** 27 << 2)


def test_too_many_tiles(lib):
    assert plan(lib, scene(1), width=64, height=2 ** 29 - 1)["status"] == RT_OK
    assert plan(lib, scene(1), width=64, height=2 ** 29)["status"] == RT_ERR_LIMIT


# ---------------------------------------------------------------------------------------------------- the GPU knob matrix


@pytest.mark.parametrize("rq_name", list(M.REQUESTS))
def test_knob_matrix_tuples_stay_inside_the_kernels_domain(lib, rq_name):
    """Every (request, strips, setting) tests/test_gpu_knobs.py launches (tests/_knob_matrix.py), as the 256-thread kernels and as the
    1024-thread LDS-tree kernels plan it, on a grid of one workgroup and on a full chip's, the progressive passes included: the
    slots and the queue stay inside what the kernel supports, the sample units are the ones the matrix says each request
    reaches, and the queue has whole-tile entries exactly where the matrix claims them (RT_TAIL_TILES 0 and 1)."""
    slots_max = int(K(lib, "SLOTS_MAX"))
    w, h, spp, grp, units = M.REQUESTS[rq_name]
    pw, ph, pspp, passes = M.PASS_JOB
    launches = [(w, h, spp, n, None) for n in (M.DIVISIONS, 1)]
    if rq_name == list(M.REQUESTS)[0]:
        launches += [(pw, ph, pspp, 1, p) for p in passes]
    seen_big = set()
    for sh, block in ((scene(1), "BLOCK"), (scene(1000, cull_density=0.1), "LTREE_BLOCK")):
        for grid in (1, 256 * 8):
            for (fw, fh, fspp, n_strips, pass_range), setting in ((l, s) for l in launches for s in M.SETTINGS):
                kn = M.plan_knobs(setting)
                r = plan(lib, sh, width=fw, height=fh, divisions=M.DIVISIONS, spp=fspp, max_bounces=M.MAX_BOUNCES, n_strips=n_strips,
                         pass_range=pass_range, grid=grid, **kn)
                what = (rq_name, n_strips, pass_range, setting, block, grid)
                assert r["status"] == RT_OK and r["block"] == K(lib, block), what
                assert 1 <= r["commit_slots"] <= r["n_slots"] <= slots_max, what
                assert r["n_slots"] == kn.get("slots", r["n_slots"]) and r["commit_slots"] == min(kn.get("commit_slots", r["commit_slots"]), r["n_slots"]), what
                assert 1 <= r["refill_eighths"] <= 8, what
                total = r["tiles_total"]
                assert total == (fw + 63) // 64 * (fh // M.DIVISIONS) * n_strips, what
                assert r["n_tiles"] == r["tiles_big"] + ((total - r["tiles_big"]) << r["sub_shift"]), what
                assert r["tiles_big"] == {"none": 0, "all": total, "all_but_one": total - 1}[M.SETTINGS[setting][2]], what
                assert r["sub_shift"] == (4 if r["upp"] > 32 else 2), what
                seen_big.add(r["tiles_big"] > 0)
                if pass_range is None:
                    assert (r["upp"], r["grp"], r["slot_stride"] - 1) == (spp, grp, units), what
                else:
                    assert (r["upp"], r["s_begin"], r["gap"], r["acc_out"]) == (pass_range[1] - pass_range[0], pass_range[0],
                                                                                 fspp - r["upp"], 1), what
    assert seen_big == {False, True}


def test_knob_matrix_covers_every_kernel_family():
    """Every setting runs on at least one engine of every kernel family it applies to: the ones every engine takes (slots, commit
    threshold, queue split, strip costs, the two combined ones) on all seven families, the refill threshold on every walk, output
    staging on every kernel it is compiled into, the compacted root tests on the exact-node L2 walks."""
    families = set(M.FAMILY.values())
    assert len(families) == 7 and set(M.FAMILY) == set(M.ENGINE_KEYS)
    walks = families - {"resident scan", "streamed scan"}
    staging = families - {"resident scan", "LDS tree", "LDS tree culled"}
    for name, (knobs, engines, _) in M.SETTINGS.items():
        assert set(knobs) <= set(M.PLAN_KNOB) | {"RT_STRIP_COST"}, name
        want = families
        if name not in ("starved", "wide"):
            want = {"L2 exact"} if "RT_COMPACT" in knobs else staging if "RT_NO_STAGE" in knobs else walks if "RT_REFILL_EIGHTHS" in knobs else families
        assert {M.FAMILY[e] for e in engines} == want, name
    assert M.settings_for(0)[0] == "default" and M.SLOTS_MIN == 1


# ---------------------------------------------------------------------------------------------------- staging layout
ALIGN = 256


def _align(b):
    return (b + ALIGN - 1) // ALIGN * ALIGN


def _stage_lib(lib):
    lib.stage_layout.restype = C.c_uint64
    lib.stage_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.stage_denoise.restype = C.c_uint64
    lib.stage_denoise.argtypes = [C.c_uint32] * 6 + [C.c_void_p] * 3
    lib.stage_scratch_bytes.restype = C.c_double
    lib.stage_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
    return lib


def _check_layout(nbytes, present, off, total, what):
    """Every present entry at a multiple of 256, behind the one before it and inside the total; returns the aligned sizes' sum."""
    top = 0
    for k in np.nonzero(present)[0]:
        assert off[k] % ALIGN == 0 and off[k] >= top, (what, k)
        top = int(off[k]) + int(nbytes[k])
    assert top <= total, what
    return sum(_align(int(b)) for b in nbytes[present != 0])


def test_staging_layout_of_random_lists(lib):
    """rtplan::stage_layout against the arithmetic: an entry is present when it has a host side or is device-only, absent ones take no
    room, present ones lie in list order at multiples of 256 without overlap, zero-byte ones included, and the total covers the last."""
    _stage_lib(lib)
    assert K(lib, "DN_ALIGN") == ALIGN
    g = np.random.default_rng(0x57A6E)
    for _ in range(300):
        n = int(g.integers(0, 40))
        nbytes = np.where(g.random(n) < 0.25, 0, g.integers(0, 5000, n)).astype(np.uint64)
        host = (g.random(n) < 0.6).astype(np.uint8)
        dev = (g.random(n) < 0.25).astype(np.uint8)
        off, present = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
        total = lib.stage_layout(nbytes.ctypes.data, host.ctypes.data, dev.ctypes.data, n, off.ctypes.data, present.ctypes.data)
        assert np.array_equal(present != 0, (host | dev) != 0)
        assert _check_layout(nbytes, present, off, total, (n, nbytes, host, dev)) == total      # ... and no more than that
        want = np.concatenate([[0], np.cumsum([_align(int(b)) if p else 0 for b, p in zip(nbytes, present)])])
        assert np.array_equal(off, want[:-1].astype(np.uint64))


@pytest.mark.parametrize("n", [1, 3, 66])
def test_staging_list_of_the_denoiser(lib, n):
    """rtplan::dn_stage_list for every plane set of tests/test_gpu_denoise.py: the scratch first, at offset 0 and device-only, then per
    strip the sum, the guide planes it has and the outputs asked for, each aligned; the total holds the scratch and every aligned size."""
    from test_gpu_denoise import PLANE_SETS
    _stage_lib(lib)
    W, Hs = 40, 2
    per = lib.stage_per_strip()
    assert per == 8
    v3, s1, u8 = Hs * W * 12, Hs * W * 4, Hs * W * 3
    scratch = int(lib.stage_scratch_bytes(W, Hs * n))
    assert scratch >= 3 * 16 * W * Hs * n
    order = ("albedo", "normal", "depth", "hits")
    for names in PLANE_SETS:
        planes = sum(1 << order.index(k) for k in names)
        for outs in (1, 4, 7):                                  # rgb only, linear only, all three
            m = 1 + per * n
            nbytes, off, present = np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.uint8)
            total = lib.stage_denoise(W, Hs * 66, 66, n, planes, outs, nbytes.ctypes.data, off.ctypes.data, present.ctypes.data)
            what = (n, names, outs)
            assert present[0] and off[0] == 0 and nbytes[0] == scratch, what
            strip = [1] + [1 if k in names else 0 for k in order] + [outs & 1, outs >> 1 & 1, outs >> 2 & 1]
            assert np.array_equal(present[1:].reshape(n, per), np.tile(np.array(strip, np.uint8), (n, 1))), what
            assert np.array_equal(nbytes[1:].reshape(n, per), np.tile(np.array([v3, v3, v3, s1, s1, u8, v3, v3], np.uint64), (n, 1))), what
            aligned = _check_layout(nbytes, present, off, total, what)
            assert aligned == _align(scratch) + n * sum(_align(b) for b, p in zip([v3, v3, v3, s1, s1, u8, v3, v3], strip) if p), what
            assert total >= aligned, what


def test_staging_harness_under_the_sanitizers(tmp_path):
    """The harness source once more as a program with its own main, built with -fsanitize=address,undefined: the same lists, run to the
    end with no report."""
    exe = tmp_path / "plan_host_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DPLAN_HOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "staging ok" and not r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
