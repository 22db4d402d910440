"""The a-trous denoiser off the GPU: the product's per-pixel lines (csrc/rt_denoise_math.h, through the g++ harness
tests/host/denoise_host.cpp) equal the numpy restatement of rt_tile.h (tests/_denoise_np.py) bit for bit on seeded random images, the
plan (csrc/rt_plan.h plan_denoise) stays inside a CU's LDS with aligned, disjoint scratch regions, and properties of the contract hold
on the restatement: sky and geometry do not mix, a strong normal edge has zero weight, and no iteration is the preview."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _denoise_np as dn

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
SRC = ROOT / "tests" / "host" / "denoise_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "libdenoise_host.so"
DEPS = [SRC, CSRC / "rt_denoise_math.h", CSRC / "rt_plan.h", CSRC / "rt_consts.h", ROOT / "include" / "rt_tile.h"]
f32 = np.float32
MAX_ITER = 8
TILE_ABI_MAX_PIXELS = 0x7FFFFFFF


def load_lib():
    """The harness as a library, built if it is missing or older than its sources (tests/test_extreme_planes_host.py loads it too)."""
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                        "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    vp = C.c_void_p
    l.dn_host.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    l.dn_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, vp]
    l.dn_lds_max_step_default.restype = C.c_uint32
    l.dn_lds_cu.restype = C.c_uint64
    return l


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _p(a):
    return None if a is None else a.ctypes.data


def host_denoise(lib, C_, e, *, A=None, k=1, N=None, D=None, hits=None, iterations=5, k_color=0.01, color_step_scale=4.0,
                 k_normal=1.0, k_depth=4.0, albedo_eps=2.0 ** -8):
    R, W = C_.shape[:2]
    fp = np.array([e, k, albedo_eps, k_color, color_step_scale, k_normal, k_depth], f32)
    lin = np.empty((R, W, 3), f32)
    ff = np.empty((R, W, 3), f32)
    rgb = np.empty((R, W, 3), np.uint8)
    args = [np.ascontiguousarray(a) if a is not None else None for a in (C_, A, N, D, hits)]
    lib.dn_host(W, R, iterations, fp.ctypes.data, *[_p(a) for a in args], lin.ctypes.data, ff.ctypes.data, rgb.ctypes.data)
    return dict(linear=lin, f32=ff, rgb=rgb)


def synthetic(rng, R, W, e=8, k=4):
    """Sums as a renderer writes them after e colour and k feature samples, with the awkward parts: pixels no sample hit (a sky
    region and scattered ones), partial hits, zero normal sums, zero albedo channels, heavy-tailed colours, two depth layers."""
    hits = rng.integers(0, k + 1, (R, W)).astype(np.uint32)
    hits[: max(1, R // 3)] = 0                                            # a sky band
    hits[rng.random((R, W)) < 0.1] = k                                     # full hits
    geo = hits > 0
    col = rng.random((R, W, 3)).astype(f32) * f32(e)
    tail = rng.random((R, W)) < 0.05
    col[tail] *= rng.pareto(1.2, (int(tail.sum()), 1)).astype(f32) * f32(50) + f32(1)     # fireflies
    alb = (rng.random((R, W, 3)).astype(f32) * f32(k))
    alb[rng.random((R, W)) < 0.1, 1] = 0                                   # zero albedo channels
    nrm = rng.normal(size=(R, W, 3)).astype(f32) * hits[..., None].astype(f32)
    nrm[rng.random((R, W)) < 0.05] = 0                                      # zero normal sums
    nrm[~geo] = 0
    layer = np.where(rng.random((R, W)) < 0.5, f32(2), f32(9))
    dep = (layer * hits.astype(f32) * (f32(1) + rng.random((R, W)).astype(f32) * f32(0.05))).astype(f32)
    dep[~geo] = 0
    return dict(C=col.astype(f32), A=alb, N=nrm, D=dep, hits=hits)


def _eq(a, b, what):
    if a.dtype == np.uint8:
        bad = np.argwhere(a != b)
    else:
        bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert len(bad) == 0, (what, len(bad), bad[:4], a[tuple(bad[0])], b[tuple(bad[0])])


SIZES = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (5, 67), (13, 9)]
COMBOS = list(itertools.product([False, True], [False, True], [False, True]))      # albedo, normal, depth+hits


@pytest.mark.parametrize("R,W", SIZES)
@pytest.mark.parametrize("albedo,normal,depth", COMBOS)
def test_host_lines_equal_the_restatement(lib, R, W, albedo, normal, depth):
    rng = np.random.default_rng(R * 1000 + W * 10 + albedo * 4 + normal * 2 + depth)
    s = synthetic(rng, R, W)
    kw = dict(A=s["A"] if albedo else None, k=4, N=s["N"] if normal else None, D=s["D"] if depth else None,
              hits=s["hits"] if depth else None)
    for it, kc, kn, kd in [(0, 1.0, 4.0, 16.0), (1, 1.0, 4.0, 16.0), (3, 0.5, 2.0, 8.0), (5, 1.0, 4.0, 16.0), (8, 1.0, 4.0, 16.0),
                           (3, 0.0, 0.0, 0.0), (2, 1e6, 1e6, 1e6)]:
        want = dn.denoise(s["C"], 8, iterations=it, k_color=f32(kc), k_normal=f32(kn), k_depth=f32(kd), **kw)
        got = host_denoise(lib, s["C"], 8, iterations=it, k_color=kc, k_normal=kn, k_depth=kd, **kw)
        for o in ("linear", "f32", "rgb"):
            _eq(got[o], want[o], (R, W, albedo, normal, depth, it, kc, o))


def test_hits_without_depth_and_normal_without_hits(lib):
    rng = np.random.default_rng(5)
    s = synthetic(rng, 11, 23)
    for kw in (dict(hits=s["hits"]), dict(N=s["N"]), dict(A=s["A"], hits=s["hits"], N=s["N"])):
        want = dn.denoise(s["C"], 8, k=4, iterations=4, **kw)
        got = host_denoise(lib, s["C"], 8, k=4, iterations=4, **kw)
        for o in ("linear", "f32", "rgb"):
            _eq(got[o], want[o], (sorted(kw), o))


def test_plain_b3_atrous_with_zero_k(lib):
    """k = 0: every tap takes its full B3 weight (inside the image), so a constant image stays constant."""
    Cc = np.full((9, 10, 3), 3.0, f32)
    out = dn.denoise(Cc, 4, iterations=3, k_color=f32(0), k_normal=f32(0), k_depth=f32(0))
    assert np.array_equal(out["linear"], np.full((9, 10, 3), 0.75, f32))
    _eq(host_denoise(lib, Cc, 4, iterations=3, k_color=0.0)["linear"], out["linear"], "const")


def _plan(lib, W, R, I, guided, lds_max_step):
    out = np.zeros(6 + 3 * MAX_ITER, np.uint64)
    lib.dn_plan(W, R, I, int(guided), lds_max_step, out.ctypes.data)
    return dict(npix=int(out[0]), tiles_x=int(out[1]), off_guide=int(out[2]), off_c0=int(out[3]), off_c1=int(out[4]),
                scratch=int(out[5]), step=[int(v) for v in out[6::3]], lds=[int(v) for v in out[7::3]],
                wg=[int(v) for v in out[8::3]])


@pytest.mark.parametrize("W,R", [(1, 1), (63, 5), (64, 4), (65, 3), (3840, 2160), (1, TILE_ABI_MAX_PIXELS),
                                 (TILE_ABI_MAX_PIXELS, 1), (46340, 46340)])
def test_plan_boundaries(lib, W, R):
    lds_cu = int(lib.dn_lds_cu())
    for I, guided, lstep in itertools.product([0, 1, 5, 8], [False, True], [0, 1, 2, 4, 8, 128]):
        p = _plan(lib, W, R, I, guided, lstep)
        n = W * R
        assert p["npix"] == n and p["tiles_x"] == (W + 63) // 64
        regions = sorted([(p["off_guide"], 16 * n), (p["off_c0"], 16 * n), (p["off_c1"], 16 * n)])
        for (o, b), (o2, _) in zip(regions, regions[1:]):
            assert o + b <= o2
        assert all(o % 256 == 0 for o, _ in regions)
        assert regions[-1][0] + regions[-1][1] <= p["scratch"] and p["scratch"] % 256 == 0
        assert p["scratch"] == _plan(lib, W, R, 0, False, 0)["scratch"]          # what rt_denoise_scratch_bytes returns
        assert p["scratch"] >= 48 * n and p["scratch"] < 48 * n + 3 * 256            # (no wrap-around at the largest frame)
        for i in range(MAX_ITER):
            if i >= I:
                assert p["lds"][i] == 0 and p["step"][i] == 0
                continue
            s = 1 << i
            assert p["step"][i] == s
            win = (64 + 4 * s) * (4 + 4 * s) * 16 * (2 if guided else 1)
            if p["lds"][i]:
                assert s <= lstep and p["lds"][i] == win
                assert p["lds"][i] * p["wg"][i] <= lds_cu and 1 <= p["wg"][i] <= 8
            else:
                assert s > lstep or win > lds_cu
                assert p["wg"][i] == 8


@pytest.mark.parametrize("W,R", [(67, 12), (129, 40)])
def test_plan_of_every_lds_step_the_gpu_sweep_sets(lib, W, R):
    """RT_DENOISE_LDS_STEP as tests/test_gpu_knobs.py sweeps it, five iterations: steps up to the knob are staged in LDS wherever the
    window fits a CU's 160 KiB, larger ones gather through L2; the guided window of step 16 (278 528 bytes) never fits."""
    lds_cu = int(lib.dn_lds_cu())
    assert lds_cu == 160 * 1024 and lib.dn_lds_max_step_default() == 2
    for guided in (False, True):
        win = [(64 + 4 * s) * (4 + 4 * s) * 16 * (2 if guided else 1) for s in (1, 2, 4, 8, 16)]
        assert win[4] == (278528 if guided else 139264)
        for knob in (0, 1, 4, 8, 16):
            p = _plan(lib, W, R, 5, guided, knob)
            assert p["step"][:5] == [1, 2, 4, 8, 16]
            for i, s in enumerate(p["step"][:5]):
                assert p["lds"][i] == (win[i] if s <= knob and win[i] <= lds_cu else 0), (guided, knob, s)
        assert _plan(lib, W, R, 5, guided, 16)["lds"][4] == (0 if guided else 139264)
        assert _plan(lib, W, R, 5, guided, 8)["lds"][:5] == win[:4] + [0]
        assert not any(_plan(lib, W, R, 5, guided, 0)["lds"])


def test_scratch_bytes_of_the_library_match_the_plan(lib):
    from ray_tracer_s8_amd import _abi
    l = _abi.load()
    for W, R in [(1, 1), (65, 3), (3840, 2160), (1, TILE_ABI_MAX_PIXELS)]:
        assert l.rt_denoise_scratch_bytes(W, R) == _plan(lib, W, R, 0, False, 0)["scratch"]


# ---- properties of the contract, on the restatement -------------------------------------------------------------------------------
def test_sky_and_geometry_do_not_mix():
    rng = np.random.default_rng(11)
    s = synthetic(rng, 24, 31)
    kw = dict(A=s["A"], k=4, N=s["N"], D=s["D"], hits=s["hits"], iterations=5)
    base = dn.denoise(s["C"], 8, **kw)["linear"]
    geo = s["hits"] > 0
    C2 = s["C"].copy()
    C2[geo] = C2[geo] * f32(3) + f32(1)
    out = dn.denoise(C2, 8, **kw)["linear"]
    assert np.array_equal(out[~geo].view(np.uint32), base[~geo].view(np.uint32))
    C3 = s["C"].copy()
    C3[~geo] = C3[~geo] * f32(5) + f32(2)
    out = dn.denoise(C3, 8, **kw)["linear"]
    assert np.array_equal(out[geo].view(np.uint32), base[geo].view(np.uint32))


def test_a_normal_edge_has_zero_weight():
    rng = np.random.default_rng(12)
    R, W = 16, 32
    Cc = rng.random((R, W, 3)).astype(f32)
    N = np.zeros((R, W, 3), f32)
    N[:, :16, 2] = 1
    N[:, 16:, 0] = 1                                                        # dot = 0 across the edge
    base = dn.denoise(Cc, 1, N=N, iterations=4, k_normal=f32(1))["linear"]
    C2 = Cc.copy()
    C2[:, 16:] = rng.random((R, 16, 3)).astype(f32) * f32(9)
    out = dn.denoise(C2, 1, N=N, iterations=4, k_normal=f32(1))["linear"]
    assert np.array_equal(out[:, :16].view(np.uint32), base[:, :16].view(np.uint32))


def test_no_iteration_is_the_preview():
    rng = np.random.default_rng(13)
    Cc = (rng.random((5, 9, 3)) * 7).astype(f32)
    out = dn.denoise(Cc, 7, iterations=0)
    prev = np.sqrt(Cc / f32(7))
    assert np.array_equal(out["f32"].view(np.uint32), prev.view(np.uint32))
    assert np.array_equal(out["rgb"], dn.as_u8(prev * f32(255.999)))
