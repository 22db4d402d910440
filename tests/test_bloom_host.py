"""The bloom off the GPU: the product's lines (bloom_csrc/rt_bloom_math.h, through the g++ harness
tests/host/bloom_host.cpp) equal the numpy restatement of bloom_csrc/rt_bloom.h (tests/_bloom_np.py) bit for bit, NaN where NaN: the
sanitised input and the threshold over the three extreme tiers of tests/_extreme_planes.py and log-uniform colours, with m on, just
below and just above T - K, T and T + K, at K = 0 and with tiny m; the down and the up taps at every clamp case (first and last row and
column, sides of 1 and 2) against a second writing of their definitions, and whole levels down and up; the whole call with its scratch
layout, both mixes, with and without the threshold, at the shapes the GPU test runs; no NaN out and +inf kept over the extreme tiers;
a constant image kept exactly; tail_from over a grid of shapes and levels, with "everything fits", "nothing fits" and the 1920 x 1080
case; what the host refuses of the settings; the harness as a stand-alone program runs clean under the address and
undefined-behaviour sanitizers.  Without the feature every test here fails: there is no bloom_csrc."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _bloom_np as bnp
import _extreme_planes as xp

ROOT = Path(__file__).resolve().parents[1]
BLOOM_CSRC = ROOT / "ray_tracer_s8_amd" / "bloom_csrc"
SRC = ROOT / "tests" / "host" / "bloom_host.cpp"
BUILD = ROOT / "tests" / "host" / "_build"
OUT = BUILD / "libbloom_host.so"
DEPS = [SRC, BLOOM_CSRC / "rt_bloom_math.h"]
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-I{BLOOM_CSRC}"]
f32, u32 = np.float32, np.uint32


def load_lib():
    BUILD.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run([*GXX, "-fPIC", "-shared", "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    l.bloom_source_host.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p]
    l.bloom_factor_host.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_void_p]
    l.bloom_down_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    l.bloom_up_host.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p]
    l.bloom_taps_host.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    l.bloom_tail_from_host.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]
    l.bloom_tail_from_host.restype = C.c_uint32
    l.bloom_lds_budget_host.restype = C.c_uint64
    l.bloom_scratch_host.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    l.bloom_scratch_host.restype = C.c_uint64
    l.bloom_settings_ok_host.argtypes = [C.c_uint32, C.c_uint32] + [C.c_float] * 6
    l.bloom_apply_host.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.c_float] * 6 + [C.c_void_p] * 4
    return l


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def host_source(lib, img, cap, T=0.0, K=0.0):
    img = np.ascontiguousarray(img, f32)
    before = img.tobytes()
    out = np.full(img.shape, 7, f32)
    lib.bloom_source_host(img.ctypes.data, img.size // 3, cap, T, K, out.ctypes.data)
    assert img.tobytes() == before
    return out


def host_down(lib, S):
    S = np.ascontiguousarray(S, f32)
    R, W = S.shape[:2]
    out = np.full(((R + 1) >> 1, (W + 1) >> 1, 3), 7, f32)
    lib.bloom_down_host(S.ctypes.data, W, R, out.ctypes.data)
    return out


def host_up(lib, X, shape):
    X = np.ascontiguousarray(X, f32)
    out = np.full((*shape, 3), 7, f32)
    lib.bloom_up_host(X.ctypes.data, X.shape[1], X.shape[0], shape[1], shape[0], out.ctypes.data)
    return out


def host_apply(lib, img, levels, mode=bnp.MIX, spread=0.7, strength=0.05, threshold=0.0, knee=0.5, cap=65536.0, second=True):
    """(status, out, bloom, {k: U_k}) with the scratch exactly its size and guard bytes behind it."""
    img = np.ascontiguousarray(img, f32)
    R, W = img.shape[:2]
    before = img.tobytes()
    offsets, size = bnp.scratch_layout((R, W), levels)
    scratch = np.full(size + 64, 0xA5, np.uint8)
    first, out, b = (np.full(img.shape, 7, f32) for _ in range(3))
    status = lib.bloom_apply_host(img.ctypes.data, W, R, levels, mode, spread, strength, bnp.norm_of(spread, levels), cap, threshold,
                                  bnp.knee_of(threshold, knee), first.ctypes.data, scratch.ctypes.data, out.ctypes.data,
                                  b.ctypes.data if second else None)
    assert img.tobytes() == before and (scratch[size:] == 0xA5).all()
    U = {}
    for k, (shape, at) in enumerate(zip(bnp.level_shapes((R, W), levels)[1:], offsets), 1):
        U[k] = scratch[at:at + shape[0] * shape[1] * 12].view(f32).reshape(*shape, 3)
    return status, out, b, U


def colours():
    """Pixels [n][3]: log-uniform ones and the three extreme tiers."""
    px = [bnp.log_uniform((9, 70), 1).reshape(-1, 3), bnp.log_uniform((9, 70), 2, -40, 40).reshape(-1, 3)]
    px += [bnp.extreme((9, 70), tier, 3 + j).reshape(-1, 3) for j, tier in enumerate(xp.TIERS)]
    vals = np.concatenate([xp.SMALL, xp.HUGE, xp.NONFINITE])
    px.append(np.stack(np.meshgrid(vals, vals[::3], vals[::5], indexing="ij"), -1).reshape(-1, 3))
    return np.concatenate(px).astype(f32)


# ---- the input and the threshold ---------------------------------------------------------------------------------------------------------
def test_the_sanitised_input(lib):
    px = colours()
    for cap in (65536.0, 1.0, 1e-40, 2.0 ** 62):
        got = host_source(lib, px, cap)
        assert got.tobytes() == bnp.sanitise(px, cap).tobytes()
        assert not np.isnan(got).any() and not np.signbit(got).any() and (got <= f32(cap)).all()
        assert (got[np.isposinf(px)] == f32(cap)).all() and (got[np.isnan(px) | (px <= 0)] == 0).all()
    q = bnp.positive(px)
    assert (q[np.isposinf(px)] == np.inf).all() and not np.isnan(q).any() and not np.signbit(q).any()


def test_the_threshold(lib):
    for T, K in bnp.THRESHOLDS:
        K = float(f32(K))
        for px in (bnp.threshold_pixels(T, K), colours()):
            p = bnp.sanitise(px, 65536.0)
            f = np.full(len(p), 7, f32)
            lib.bloom_factor_host(p.ctypes.data, len(p), T, K, f.ctypes.data)
            want = bnp.threshold_factor(p, T, K)
            assert f.tobytes() == want.tobytes(), (T, K)
            assert not np.isnan(f).any() and (f >= 0).all() and (f <= f32(1.0001)).all()
            got = host_source(lib, px, 65536.0, T, K)
            xp.same(got, bnp.source(px, 65536.0, T, K), (T, K))
            m = p.max(-1)
            assert (got[m <= f32(f32(T) - f32(K))] == 0).all()                # below the knee nothing passes
            assert not np.isnan(got).any() and (got <= p).all()
    # a hard threshold (K = 0): what passes is m - T of m
    p = np.array([[2, 1, 0.5], [1, 1, 1], [0.5, 2, 0]], f32)
    assert bnp.threshold_factor(p, 1.0, 0.0).tolist() == [0.5, 0.0, 0.5]
    # without one the pixel is the sanitised one
    assert host_source(lib, p, 65536.0, 0.0, 0.0).tobytes() == p.tobytes()


# ---- the taps ----------------------------------------------------------------------------------------------------------------------------
def test_the_taps_at_every_clamp_case(lib):
    down, up, w = np.zeros(4, u32), np.zeros(2, u32), np.zeros(2, f32)
    for n in (1, 2, 3, 4, 5, 8, 9, 37):
        for i in range(2 * n + 2):
            lib.bloom_taps_host(i, n, down.ctypes.data, up.ctypes.data, w.ctypes.data)
            assert down.tolist() == [min(max(2 * i - 1 + a, 0), n - 1) for a in range(4)], (n, i)
            ya = (i + 1) // 2 - 1
            assert up.tolist() == [min(max(ya, 0), n - 1), min(ya + 1, n - 1)] and w.tolist() == ([3, 1] if i & 1 else [1, 3]), (n, i)
        assert [t.tolist() for t in bnp.down_taps((n + 1) >> 1, n)] == \
            [[min(max(2 * i - 1 + a, 0), n - 1) for i in range((n + 1) >> 1)] for a in range(4)]
    # the first and the last pixel of a side of 5 from a side of 3, and a side of 1 from a side of 1
    assert [bnp.up_taps(5, 3)[k].tolist() for k in range(4)] == [[0, 0, 0, 1, 1], [0, 1, 1, 2, 2], [1, 3, 1, 3, 1], [3, 1, 3, 1, 3]]
    assert [bnp.up_taps(1, 1)[k].tolist() for k in range(4)] == [[0], [0], [1], [3]]


def test_whole_levels_down_and_up(lib):
    for R, W in ((1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (3, 3), (5, 37), (9, 70), (34, 5)):
        for name, S in (("noise", np.abs(bnp.log_uniform((R, W), R * 100 + W))), ("huge", bnp.sanitise(bnp.extreme((R, W), "huge", 5), 3.4e38)),
                        ("small", bnp.sanitise(bnp.extreme((R, W), "small", 6), 65536.0))):
            D = host_down(lib, S)
            xp.same(D, bnp.down(S), (R, W, name, "down"))
            assert D.shape == ((R + 1) >> 1, (W + 1) >> 1, 3) and not np.isnan(D).any()
            for shape in ((R, W), (2 * D.shape[0], 2 * D.shape[1]), (max(1, 2 * D.shape[0] - 1), max(1, 2 * D.shape[1] - 1))):
                xp.same(host_up(lib, D, shape), bnp.up(D, shape), (R, W, name, "up", shape))
    # the weights sum to 64 and to 16: a constant level stays what it is, exactly, at every clamp case
    for R, W in ((1, 1), (2, 3), (5, 37)):
        S = np.full((R, W, 3), 0.75, f32)
        D = host_down(lib, S)
        assert (D == f32(0.75)).all() and (host_up(lib, D, (R, W)) == f32(0.75)).all()
    # a single pixel of a level of 4 x 4 reaches the output pixels the definition says, with the 1 3 3 1 weights
    S = np.zeros((4, 4, 3), f32)
    S[1, 2] = 64
    assert bnp.down(S)[:, :, 0].tolist() == [[3, 9], [1, 3]] and host_down(lib, S)[:, :, 0].tolist() == [[3, 9], [1, 3]]


# ---- the whole call ----------------------------------------------------------------------------------------------------------------------
def _same_call(lib, img, levels, what, **kw):
    status, out, b, U = host_apply(lib, img, levels, **kw)
    want_out, want_b, want_U = bnp.bloom(img, levels, **kw)
    assert status == 0
    xp.same(out, want_out, (what, "out"))
    xp.same(b, want_b, (what, "bloom"))
    for k in U:
        xp.same(U[k], want_U[k], (what, "U", k))
    return out, b


def test_the_call_on_the_shapes_of_the_gpu_test(lib):
    for j, (shape, levels) in enumerate(bnp.SHAPES):
        img = bnp.log_uniform(shape, 40 + j)
        _same_call(lib, img, levels, (shape, levels))
        if shape[0] * shape[1] <= 10000:
            _same_call(lib, img, levels, (shape, levels, "add, threshold"), mode=bnp.ADD, strength=1.5, threshold=1.0, knee=0.5, spread=1.0)
            _same_call(lib, img, levels, (shape, levels, "mix, hard threshold"), threshold=0.25, knee=0.0, spread=0.3, strength=0.9)
    # without the second output the first is the same
    img = bnp.log_uniform((5, 37), 3)
    assert host_apply(lib, img, 3, second=False)[1].tobytes() == host_apply(lib, img, 3)[1].tobytes()


def test_a_constant_image_is_kept_exactly(lib):
    """0.75 everywhere with spread 1, four levels and strength 0.25: every level is 0.75, U_k = (5 - k) 0.75, norm = 0.25, b = 0.75 and
    out = 0.75 0.75 + 0.25 0.75, every one of them exact."""
    for shape, _ in bnp.SHAPES:
        if shape[0] * shape[1] > 10000:
            continue
        img = np.full((*shape, 3), 0.75, f32)
        status, out, b, U = host_apply(lib, img, 4, spread=1.0, strength=0.25)
        assert status == 0 and (out == f32(0.75)).all() and (b == f32(0.75)).all(), shape
        assert all((U[k] == f32(0.75 * (5 - k))).all() for k in U)
        assert bnp.norm_of(1.0, 4) == f32(0.25)
        assert (bnp.bloom(img, 4, spread=1.0, strength=0.25)[0] == f32(0.75)).all()


def test_impulses(lib):
    for shape, at in (((9, 70), (0, 0)), ((9, 70), (4, 35)), ((9, 70), (8, 69)), ((37, 5), (36, 0)), ((40, 130), (16, 64))):
        out, b = _same_call(lib, bnp.impulse(shape, at), 3, (shape, at))
        assert b[at].min() > 0 and (b >= 0).all() and out[at][0] > 900
        # the bloom falls off from the impulse along its row
        row = b[at[0], :, 0]
        assert row[at[1]] == row.max()


def test_no_nan_leaves_and_an_infinity_stays(lib):
    for tier in xp.TIERS:
        for j, (shape, levels) in enumerate((((9, 70), 3), ((22, 70), 5), ((5, 37), 8))):
            img = bnp.extreme(shape, tier, 70 + j)
            for kw in (dict(), dict(mode=bnp.ADD, strength=3.0), dict(threshold=1.0), dict(cap=2.0 ** 62), dict(cap=2.0 ** 62, threshold=2.0 ** 61, knee=1.0)):
                out, b = _same_call(lib, img, levels, (tier, shape, levels, kw), **kw)
                assert not np.isnan(out).any() and not np.isnan(b).any() and (out >= 0).all() and (b >= 0).all()
                assert (out[np.isposinf(img)] == np.inf).all()
                if kw.get("cap", 65536.0) == 65536.0:
                    assert np.isfinite(b).all() and (b <= f32(65536 * 1.0001)).all()
        if tier == "nonfinite":
            assert np.isnan(img).any() and np.isposinf(img).any() and np.isneginf(img).any()


# ---- the tail's place ----------------------------------------------------------------------------------------------------------------------
def test_tail_from(lib):
    budget = lib.bloom_lds_budget_host()
    assert budget == bnp.LDS_BUDGET == 160 * 1024
    shapes = [(1, 1), (2, 3), (5, 37), (67, 9), (131, 71), (200, 260), (240, 260), (75, 283), (1080, 1920), (2160, 3840), (4320, 7680), (1, 100000),
              (30000, 30000)]
    for R, W in shapes:
        for levels in range(1, 9):
            for b in (budget, 12, 11, 0, 1 << 40, 5000):
                assert lib.bloom_tail_from_host(W, R, levels, b) == bnp.tail_from((R, W), levels, b), (R, W, levels, b)
    tf = lambda shape, levels, b=budget: lib.bloom_tail_from_host(shape[1], shape[0], levels, b)
    assert tf((1080, 1920), 8) == 4 and bnp.level_shapes((1080, 1920), 8)[4] == (68, 120)
    assert bnp.launches((1080, 1920), 8, bnp.TAIL) == 8 and bnp.launches((1080, 1920), 8, bnp.LEVELS) == 16
    assert tf((2160, 3840), 8) == 5 and tf((67, 9), 6) == 1 and tf((131, 71), 8) == 1              # everything fits
    assert tf((200, 260), 6) == 2 and tf((200, 260), 1) == 1 and tf((240, 260), 1) == 2            # mid-pyramid; no tail at all
    assert tf((30000, 30000), 3) == 4 and tf((1, 1), 1, 11) == 2 and tf((1, 1), 8, 12) == 8         # nothing fits
    assert tf((1, 1), 8, 96) == 1
    # the layout of the scratch
    offsets = (C.c_uint64 * 8)()
    for R, W in shapes[:-1]:
        for levels in (1, 3, 8):
            size = lib.bloom_scratch_host(W, R, levels, offsets)
            want = bnp.scratch_layout((R, W), levels)
            assert (list(offsets[:levels]), size) == (want[0], want[1]) and all(o % 16 == 0 for o in want[0]) and size % 16 == 0


def test_what_the_host_refuses(lib):
    ok = lambda levels=8, mode=0, spread=0.7, strength=0.05, norm=0.3, cap=65536.0, T=0.0, K=0.0: \
        lib.bloom_settings_ok_host(levels, mode, spread, strength, norm, cap, T, K)
    assert ok() == 1 and ok(levels=1) == 1 and ok(spread=1.0) == 1 and ok(mode=1, strength=100.0) == 1 and ok(T=1.0, K=1.0) == 1
    assert ok(cap=2.0 ** 62, T=2.0 ** 62, K=2.0 ** 61) == 1
    inf, nan = np.inf, np.nan
    bad = [dict(levels=0), dict(levels=9), dict(mode=2), dict(spread=0.0), dict(spread=-0.5), dict(spread=1.0001), dict(spread=nan),
           dict(strength=0.0), dict(strength=1.0), dict(strength=nan), dict(strength=-1.0), dict(mode=1, strength=inf), dict(mode=1, strength=0.0),
           dict(mode=1, strength=nan), dict(norm=0.0), dict(norm=inf), dict(norm=nan), dict(cap=0.0), dict(cap=-1.0), dict(cap=inf),
           dict(cap=nan), dict(cap=2.0 ** 63), dict(T=-1.0), dict(T=nan), dict(T=inf), dict(T=1.0, K=1.5), dict(T=1.0, K=nan),
           dict(T=1.0, K=-0.5), dict(T=1.0, K=inf), dict(cap=1.0, T=2.0), dict(K=1.0)]
    for kw in bad:
        assert ok(**kw) == 0, kw


def test_the_stand_alone_harness_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "bloom_host"
    r = subprocess.run([*GXX, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBLOOM_HOST_MAIN",
                        "-o", str(exe), str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pixels bloomed" in r.stdout, r.stdout + r.stderr
