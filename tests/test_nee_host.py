"""The next-event-estimation integrator off the GPU, through the g++ harness tests/host/nee_host.cpp:
(a) the product's MIS weights (csrc/rt_nee_math.h light_weight, bounce_weight) equal the numpy restatement of rt_tile.h
    (tests/_nee_np.py) bit for bit on seeded W and on W = 0, subnormal, 1, large and +inf: wl runs from 1 to 0, wb from 0 to 1, and
    neither is a NaN for any W >= 0;
(b) the light strategy's view of an emitter the bounce reached (emitter_view, view_weight): cs', cl', d2', the samplable test and W'
    on seeded records, with cs', cl' and d2' at and around 0, a sphere hit from inside, zero normals and a degenerate triangle
    constructed;
(c) the plan (csrc/rt_plan.h plan_nee) is the query plan with the limit of 2^23 emitters, over the legal range;
(d) the harness as a stand-alone program under -fsanitize=address,undefined."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _direct_np as D
import _nee_np as N
import _ray_cases as R
from ray_tracer_s8_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
SRC = ROOT / "tests" / "host" / "nee_host.cpp"
BUILD = ROOT / "tests" / "host" / "_build"
OUT = BUILD / "libnee_host.so"
DEPS = [SRC, CSRC / "rt_nee_math.h", CSRC / "rt_direct_math.h", CSRC / "rt_scene_host.h", CSRC / "rt_plan.h", CSRC / "rt_bvh.h",
        CSRC / "rt_consts.h", ROOT / "include" / "rt_tile.h"]
F32 = np.float32
IN_WORDS, OUT_WORDS = 13, 6
GXX = ["g++", "-std=c++17", "-ffp-contract=off", "-pthread", f"-I{CSRC}", f"-I{ROOT / 'include'}"]


@pytest.fixture(scope="module")
def lib():
    BUILD.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(GXX + ["-O2", "-fPIC", "-shared", "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    vp, u32 = C.c_void_p, C.c_uint32
    l.nee_weights.argtypes = [u32, vp, vp]
    l.nee_view.argtypes = [u32, vp, vp]
    l.nee_plan.argtypes = [vp, u32, u32, vp]
    return l


# ---------------------------------------------------------------- (a) the two weights
CONSTRUCTED_W = [0.0, 2.0 ** -149, 1e-40, 2.0 ** -126, 2.0 ** -25, 2.0 ** -24, 1e-3, 0.5, 1.0, 2.0, 3.0, 2.0 ** 24, 2.0 ** 25, 1e30,
                 3.4028234663852886e38, np.inf]


def test_weights_equal_the_restatement(lib):
    g = np.random.default_rng(11)
    W = np.concatenate([np.array(CONSTRUCTED_W), np.exp(g.uniform(-100, 88, 3000)), g.uniform(0, 4, 1000)]).astype(F32)
    assert np.all(W >= 0)
    out = np.zeros((len(W), 2), np.uint32)
    lib.nee_weights(len(W), W.ctypes.data, out.ctypes.data)
    got = out.view(F32)
    want = np.array([[N.light_weight(w), N.bounce_weight(w)] for w in W], F32)
    assert D.B.same_bits(got, want).all()
    assert not np.isnan(got).any() and np.all((got >= 0) & (got <= 1))
    assert tuple(got[0]) == (1.0, 0.0) and tuple(got[len(CONSTRUCTED_W) - 1]) == (0.0, 1.0)       # W = 0 and W = +inf
    assert tuple(got[CONSTRUCTED_W.index(1.0)]) == (0.5, 0.5)
    assert tuple(got[1]) == (1.0, 0.0)                                                          # a subnormal W is absorbed by 1 + W
    order = np.argsort(W, kind="stable")
    assert np.all(np.diff(got[order, 0]) <= 0) and np.all(np.diff(got[order, 1]) >= 0)         # wl falls, wb rises


# ---------------------------------------------------------------- (b) the view of an emitter the bounce reached
def _records(seed, n):
    g = np.random.default_rng(seed)
    recs = []

    def rec(kind, **kw):
        r = dict(kind=kind, M=int(g.integers(1, 6)), n=R._unit(g, 1)[0], d=R._unit(g, 1)[0], nh=R._unit(g, 1)[0],
                 distance=F32(g.uniform(0.01, 30)), size=F32(g.uniform(0.05, 3)))
        r.update(kw)
        recs.append(r)

    z3 = np.zeros(3, F32)
    ez = np.array([0, 0, 1], F32)
    tiny = F32(2.0 ** -149)
    for kind in (0, 1):
        # cs' at and around 0: the previous normal perpendicular to the segment, and one ulp either side
        for c in (F32(0), tiny, -tiny, F32(1e-30), F32(-1e-30)):
            rec(kind, n=np.array([1, 0, c], F32), d=ez, nh=-ez)
        # cl' at and around 0
        for c in (F32(0), tiny, -tiny, F32(1e-30), F32(-1e-30)):
            rec(kind, n=ez, d=ez, nh=np.array([1, 0, c], F32))
        # d2' at and around 0, its underflow, its overflow
        for dist in (0.0, 2.0 ** -149, 2.0 ** -75, 2.0 ** -74, 1e-19, 1e19, 1.8446743e19, 1.8446744e19, 3e19, np.inf):
            rec(kind, n=ez, d=ez, nh=-ez, distance=F32(dist))
        rec(kind, n=ez, d=ez, nh=ez)                                       # the emitter hit from inside (sphere) / from behind (triangle)
        rec(kind, n=ez, d=ez, nh=-ez)                                      # ... and from outside
        rec(kind, n=z3, d=ez, nh=-ez)                                      # zero normals
        rec(kind, n=ez, d=ez, nh=z3)                                       # (a degenerate triangle reports the zero normal)
        rec(kind, n=ez, d=ez, nh=-ez, size=F32(0))                         # ... and has area 0
        rec(kind, n=ez, d=ez, nh=-ez, size=F32(1e30))
        rec(kind, n=ez, d=ez, nh=-ez, size=F32(np.inf))
    while len(recs) < n:
        rec(int(g.integers(0, 2)))
    return recs


def _pack(recs):
    a = np.zeros((len(recs), IN_WORDS), np.uint32)
    f = a.view(F32)
    for i, r in enumerate(recs):
        a[i, 0], a[i, 1] = r["kind"], r["M"]
        f[i, 2:5], f[i, 5:8], f[i, 8:11], f[i, 11], f[i, 12] = r["n"], r["d"], r["nh"], r["distance"], r["size"]
    return a


def test_view_equals_the_restatement(lib):
    recs = _records(7, 2000)
    packed = _pack(recs)
    out = np.zeros((len(recs), OUT_WORDS), np.uint32)
    lib.nee_view(len(recs), packed.ctypes.data, out.ctypes.data)
    outf = out.view(F32)
    seen = dict(samplable=0, not_samplable=0, inside=0)
    for i, r in enumerate(recs):
        sphere = r["kind"] == 0
        cs, cl, d2, samplable = N.emitter_view(r["n"], r["d"], r["nh"], r["distance"], sphere)
        W = N.view_weight(cs, cl, d2, sphere, r["size"], r["M"])
        want = np.array([cs, cl, d2], F32)
        assert D.B.same_bits(outf[i, 0:3], want).all(), (i, r, outf[i, 0:3], want)
        assert bool(out[i, 3]) == samplable, (i, r)
        assert D.B.same_bits(outf[i, 4:6], np.array([W, N.bounce_weight(W)], F32)).all(), (i, r, outf[i, 4:6], W)
        seen["samplable" if samplable else "not_samplable"] += 1
        if samplable:                                                      # what the kernel relies on: then W' >= 0 and wb is in [0, 1]
            assert W >= 0 and 0 <= outf[i, 5] <= 1, (i, r)
        if sphere and cs > 0 and cl < 0:
            seen["inside"] += 1
            assert not samplable
    assert seen["samplable"] > 100 and seen["not_samplable"] > 100 and seen["inside"] > 50, seen
    # the constructed cases one by one (per kind: 5 cs', 5 cl', 10 d2', then inside, outside, two zero normals, three sizes)
    per = 27
    for base in (0, per):
        flag = out[base:base + per, 3].tolist()
        assert flag[0:5] == [0, 1, 0, 1, 0], "cs' == 0 is not samplable, one subnormal above is"
        assert flag[5:10] == ([0, 0, 1, 0, 1] if base == 0 else [0, 1, 1, 1, 1]), "cl': -(nh.d) for a sphere, |nh.d| for a triangle"
        assert flag[10:20] == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0], "d2' == 0 (also by underflow) and d2' == inf (also by overflow) are not samplable"
        assert flag[20:22] == ([0, 1] if base == 0 else [1, 1]), "a sphere from inside is not samplable; a triangle is, from both sides"
        assert flag[22:24] == [0, 0], "zero normals"
        assert flag[24:27] == [1, 1, 1] and outf[base + 24, 5] == 0 and outf[base + 26, 5] == 1, "size 0: wb = 0; size inf: wb = 1"


# ---------------------------------------------------------------- (c) the plan
def test_plan_is_the_query_plan_with_the_light_limit(lib):
    flags = [0, _abi.RT_FLAG_NO_BVH_CULL, _abi.RT_FLAG_EXACT_SCAN, _abi.RT_FLAG_LINEAR_SCAN, _abi.RT_FLAG_FULL_CHAIN,
             _abi.RT_FLAG_QUANT_NODES | _abi.RT_FLAG_CULL_WALK]
    for shape in ((16, 0, 5, 0), (0, 900, 14, 0), (30, 40, R.trav_stack() - 1, 0), (30, 40, R.trav_stack(), 0), (0, 0, 0, 0), (10, 0, 4, 1)):
        for f in flags:
            for m, too_many in ((0, 0), (1, 0), (D.MAX_LIGHTS, 0), (D.MAX_LIGHTS + 1, 1), (0xFFFFFFFF, 1)):
                out = np.zeros(5, np.uint64)
                lib.nee_plan(np.array(shape, np.uint32).ctypes.data, m, f, out.ctypes.data)
                q = R.query_plan(*shape, f)
                assert (int(out[0]), int(out[1]), bool(out[2]), int(out[3])) == (q["engine"], q["scan_mode"], q["full_chain"], q["lds"]), (shape, f, m)
                assert int(out[4]) == too_many, (shape, f, m)
                assert int(out[3]) <= 64 * 1024                            # the walk's stack alone: never more than TRAV_STACK x 256 x 4 bytes


# ---------------------------------------------------------------- (d) under a sanitizer, stand-alone
def test_host_program_under_sanitizers(tmp_path):
    exe = tmp_path / "nee_host_san"
    r = subprocess.run(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DNEE_HOST_MAIN", "-o", str(exe),
                              str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "NEE_HOST_OK" in run.stdout and not run.stderr, run.stdout + run.stderr
