"""Direct lighting off the GPU, through the g++ harness tests/host/direct_host.cpp:
(a) the product's sampling arithmetic (csrc/rt_direct_math.h: the pick, the point on the light, the cosines, the weight, the radiance)
    equals the numpy restatement of rt_tile.h (tests/_direct_np.py) bit for bit on seeded records, sphere and triangle lights, M from
    1 to 5, with the awkward cases constructed: the u1 + u2 > 1 fold, hit points on the light's plane, d2 == 0, zero normals, a
    degenerate triangle, huge and tiny radii;
(b) the emitter list of the host's scene derivation (csrc/rt_scene_host.h emitter_list): the emitters in ascending world position,
    with and without a world_index, below and above the storage-reorder threshold, M = 0;
(c) the plan (csrc/rt_plan.h plan_direct): the query plan's engines and the limit of 2^23 emitters."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _direct_np as D
import _ray_cases as R
from ray_tracer_s8_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
SRC = ROOT / "tests" / "host" / "direct_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "libdirect_host.so"
DEPS = [SRC, CSRC / "rt_direct_math.h", CSRC / "rt_scene_host.h", CSRC / "rt_plan.h", CSRC / "rt_bvh.h", CSRC / "rt_consts.h",
        ROOT / "include" / "rt_tile.h"]
F32 = np.float32
IN_WORDS, OUT_WORDS = 28, 16


@pytest.fixture(scope="module")
def lib():
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", f"-I{CSRC}",
                        f"-I{ROOT / 'include'}", "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    vp, u32 = C.c_void_p, C.c_uint32
    l.direct_math.argtypes = [u32, vp, vp]
    l.direct_emitters.argtypes = [vp, u32, vp, u32, vp, C.c_int, u32, vp, vp, vp]
    l.direct_emitters.restype = u32
    l.direct_plan.argtypes = [vp, u32, u32, vp]
    l.direct_max_lights.restype = u32
    l.direct_math_max_lights.restype = u32
    return l


# ---------------------------------------------------------------- (a) the arithmetic
def _records(seed, n):
    """n seeded records (a list of dicts of float32 values), the constructed cases first."""
    g = np.random.default_rng(seed)
    recs = []

    def rec(kind, M, **kw):
        r = dict(kind=kind, M=M, u=F32(g.random()), P=g.uniform(-3, 3, 3).astype(F32), n=R._unit(g, 1)[0],
                 albedo=g.uniform(0, 1, 3).astype(F32), emission=F32(g.uniform(0.5, 8)))
        if kind == 0:
            r.update(c=g.uniform(-3, 3, 3).astype(F32), r=F32(g.uniform(0.05, 2)), us=R._unit(g, 1)[0])
        else:
            a = g.uniform(-3, 3, 3).astype(F32)
            r.update(a=a, b=(a + g.normal(0, 1, 3)).astype(F32), c=(a + g.normal(0, 1, 3)).astype(F32),
                     u1=F32(g.random()), u2=F32(g.random()))
        r.update(kw)
        if kind == 1:
            r["nl"] = D.normalize_or_zero(D.cross(r["a"] - r["b"], r["a"] - r["c"]))
        recs.append(r)
        return r

    z3 = np.zeros(3, F32)
    for M in range(1, 6):
        # the pick at its ends: u = 0, the largest u01, and the u whose product rounds up to M
        for u in (F32(0), F32(1) - F32(2.0 ** -24), F32(0.5)):
            rec(0, M, u=u)
            rec(1, M, u=u)
        rec(1, M, u1=F32(0.75), u2=F32(0.5))                               # the fold
        rec(1, M, u1=F32(0.5), u2=F32(0.5))                                # u1 + u2 == 1: no fold
        rec(1, M, u1=F32(1) - F32(2.0 ** -24), u2=F32(2.0 ** -24))
        t = rec(1, M)                                                      # the hit point on the triangle's plane: cl is 0 or rounding
        t["P"] = (t["a"] + F32(2) * (t["b"] - t["a"]) + F32(3) * (t["c"] - t["a"])).astype(F32)
        s = rec(0, M)                                                      # d2 == 0: the hit point is the light point
        s["P"] = D.sphere_point(s["c"], s["r"], s["us"])
        t = rec(1, M, u1=F32(0), u2=F32(0))
        t["P"] = t["a"].copy()
        rec(0, M, n=z3)                                                    # zero normals
        rec(1, M, n=z3)
        a = g.uniform(-1, 1, 3).astype(F32)
        rec(1, M, a=a, b=(a + F32(1)).astype(F32), c=(a + F32(2)).astype(F32))   # a degenerate triangle: area 0, normal 0
        rec(1, M, a=a, b=a.copy(), c=a.copy())
        for r in (1e-30, 1e-20, 1e-6, 1e6, 1e18, 1e19, 3e19, 1e30):        # tiny and huge radii (4 r^2 M and d2 overflow)
            rec(0, M, r=F32(r))
        L = F32(1e10)
        rec(1, M, a=np.array([-L, -L, -5], F32), b=np.array([L, -L, -5], F32), c=np.array([0, L, -5], F32))   # area and normal overflow
    while len(recs) < n:
        rec(int(g.integers(0, 2)), int(g.integers(1, 6)))
    return recs


def _pack(recs):
    a = np.zeros((len(recs), IN_WORDS), np.uint32)
    f = a.view(F32)
    for i, r in enumerate(recs):
        a[i, 0], a[i, 1] = r["kind"], r["M"]
        f[i, 2], f[i, 3:6], f[i, 6:9] = r["u"], r["P"], r["n"]
        if r["kind"] == 0:
            f[i, 9:12], f[i, 12], f[i, 13:16] = r["c"], r["r"], r["us"]
        else:
            f[i, 9:12], f[i, 12:15], f[i, 15:18], f[i, 18], f[i, 19], f[i, 20:23] = r["a"], r["b"], r["c"], r["u1"], r["u2"], r["nl"]
        f[i, 23:26], f[i, 26] = r["albedo"], r["emission"]
    return a


def _restate(r):
    """One record through tests/_direct_np.py, as the OUT_WORDS float32 / uint32 values of the harness."""
    sphere = r["kind"] == 0
    M = r["M"]
    with np.errstate(all="ignore"):
        if sphere:
            L, nl, A = D.sphere_point(r["c"], r["r"], r["us"]), r["us"], F32(0)
        else:
            u1, u2 = D.fold_pair(r["u1"], r["u2"])
            L, nl, A = D.triangle_point(r["a"], r["b"], r["c"], u1, u2), r["nl"], D.triangle_area(r["a"], r["b"], r["c"])
        v, d2, w, cs, cl, facing = D.geometry(r["P"], r["n"], L, nl, sphere)
        W = D.sphere_weight(cs, cl, r["r"], M, d2) if sphere else D.triangle_weight(cs, cl, A, M, d2)
        rgb = D.radiance(r["albedo"], r["emission"], W)
    return D.pick(r["u"], M), np.array([*L, d2, cs, cl], F32), facing, np.array([W, *rgb, *w, A], F32)


def test_math_header_equals_the_restatement(lib):
    recs = _records(2024, 1500)
    packed = _pack(recs)
    out = np.zeros((len(recs), OUT_WORDS), np.uint32)
    lib.direct_math(len(recs), packed.ctypes.data, out.ctypes.data)
    outf = out.view(F32)
    seen = dict(fold=0, facing=0, away=0, d2_zero=0, nan=0, inf=0)
    for i, r in enumerate(recs):
        k, head, facing, tail = _restate(r)
        assert out[i, 0] == k and k < r["M"], (i, "pick")
        assert D.B.same_bits(outf[i, 1:7], head).all(), (i, r, outf[i, 1:7], head)
        assert bool(out[i, 7]) == facing, (i, "facing")
        assert D.B.same_bits(outf[i, 8:16], tail).all(), (i, r, outf[i, 8:16], tail)
        seen["fold"] += r["kind"] == 1 and r["u1"] + r["u2"] > 1
        seen["facing" if facing else "away"] += 1
        seen["d2_zero"] += head[3] == 0
        seen["nan"] += bool(np.isnan(tail[0]))
        seen["inf"] += bool(np.isinf(head[3]))
        if facing:                                                         # what the kernel relies on: a traced sample has a finite,
            assert np.isfinite(head[3]) and head[3] > 0 and np.all(np.isfinite(tail[4:7]))   # positive d2 and a finite direction
    assert seen["fold"] > 100 and seen["facing"] > 100 and seen["away"] > 100 and seen["d2_zero"] >= 5 and seen["inf"] >= 5, seen


def test_pick_is_uniform_and_in_range(lib):
    """Every u01 (a multiple of 2^-24) picks k < M, at M up to the limit; the limit of the header is the plan's."""
    assert lib.direct_max_lights() == lib.direct_math_max_lights() == D.MAX_LIGHTS
    g = np.random.default_rng(3)
    for M in (1, 2, 3, 5, 1000, D.MAX_LIGHTS - 1, D.MAX_LIGHTS):
        us = np.concatenate([[0.0, 1 - 2.0 ** -24, 0.5], g.integers(0, 1 << 24, 200) / float(1 << 24)]).astype(F32)
        packed = np.zeros((len(us), IN_WORDS), np.uint32)
        packed[:, 1] = M
        packed.view(F32)[:, 2] = us
        out = np.zeros((len(us), OUT_WORDS), np.uint32)
        lib.direct_math(len(us), packed.ctypes.data, out.ctypes.data)
        assert [D.pick(u, M) for u in us] == out[:, 0].tolist() and out[:, 0].max() == M - 1 and out[0, 0] == 0


# ---------------------------------------------------------------- (b) the emitter list
def _host_emitters(lib, sph, tri, wi, reorder=1):
    ns, nt = len(sph), len(tri)
    cap = ns + nt + 1
    pos, is_sph, em = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    sp, tr = np.ascontiguousarray(sph), np.ascontiguousarray(tri)
    w = None if wi is None else np.ascontiguousarray(wi, np.uint32)
    m = lib.direct_emitters(sp.ctypes.data if ns else None, ns, tr.ctypes.data if nt else None, nt,
                            None if w is None else w.ctypes.data, reorder, cap, pos.ctypes.data, is_sph.ctypes.data, em.ctypes.data)
    assert m <= ns + nt
    return [(int(pos[k]), "sphere" if is_sph[k] else "triangle", em.view(F32)[k]) for k in range(m)]


def _world(seed, ns, nt, share):
    g = np.random.default_rng(seed)
    sph, tri = np.zeros(ns, _abi.SPHERE_DTYPE), np.zeros(nt, _abi.TRIANGLE_DTYPE)
    sph["cx"], sph["cy"], sph["cz"] = g.uniform(-8, 8, (3, ns))
    sph["radius"] = g.uniform(0.1, 0.6, ns)
    sph["emission"] = np.where(g.random(ns) < share, g.uniform(0.5, 4, ns), 0.0)
    p = g.uniform(-8, 8, (nt, 3))
    tri["a"], tri["b"], tri["c"] = p, p + g.normal(0, 0.4, (nt, 3)), p + g.normal(0, 0.4, (nt, 3))
    tri["emission"] = np.where(g.random(nt) < share, g.uniform(0.5, 4, nt), 0.0)
    return sph, tri, g.permutation(ns + nt).astype(np.uint32)


@pytest.mark.parametrize("ns,nt", [(1, 0), (0, 1), (7, 5), (40, 23), (50, 14), (300, 200)])
def test_emitter_list_is_in_world_order(lib, ns, nt):
    """Below and above REORDER_MIN_PRIMS = 64 (storage in depth-first leaf order), with the caller's world_index and without, with
    the reorder switched off: the list is the restatement's — the emitters by ascending world position, each with its own kind and
    emission."""
    for share in (0.0, 0.3, 1.0):
        sph, tri, wi = _world(ns * 1000 + nt, ns, nt, share)
        if share == 0.3 and ns:
            sph["emission"][0] = np.nan                                    # a NaN emits nothing; nor does a negative emission
        if share == 0.3 and nt:
            tri["emission"][0] = -1.0
        for w in (None, wi):
            want = [(pos, kind, F32(rec["emission"])) for pos, kind, rec in D.emitters(sph, tri, w)]
            for reorder in (1, 0):
                got = _host_emitters(lib, sph, tri, w, reorder)
                assert got == want, (ns, nt, share, w is not None, reorder)
            assert [p for p, _, _ in want] == sorted(p for p, _, _ in want)
            if share == 0.0:
                assert want == []
            if share == 1.0:
                assert len(want) == ns + nt


def test_empty_world_has_no_emitters(lib):
    assert _host_emitters(lib, D.B.NO_SPH, D.B.NO_TRI, None) == []


# ---------------------------------------------------------------- (c) the plan
def test_plan_is_the_query_plan_with_the_light_limit(lib):
    flags = [0, _abi.RT_FLAG_NO_BVH_CULL, _abi.RT_FLAG_EXACT_SCAN, _abi.RT_FLAG_LINEAR_SCAN, _abi.RT_FLAG_FULL_CHAIN,
             _abi.RT_FLAG_QUANT_NODES | _abi.RT_FLAG_CULL_WALK]
    for shape in ((16, 0, 5, 0), (0, 900, 14, 0), (30, 40, R.trav_stack(), 0), (0, 0, 0, 0), (10, 0, 4, 1)):
        for f in flags:
            for m, too_many in ((0, 0), (1, 0), (D.MAX_LIGHTS, 0), (D.MAX_LIGHTS + 1, 1), (0xFFFFFFFF, 1)):
                out = np.zeros(5, np.uint64)
                lib.direct_plan(np.array(shape, np.uint32).ctypes.data, m, f, out.ctypes.data)
                q = R.query_plan(*shape, f)
                assert (int(out[0]), int(out[1]), bool(out[2]), int(out[3])) == (q["engine"], q["scan_mode"], q["full_chain"], q["lds"]), (shape, f, m)
                assert int(out[4]) == too_many, (shape, f, m)
