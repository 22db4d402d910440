"""The film sampler off the GPU: the product's per-pixel lines (sampler_csrc/rt_sampler_math.h, through the g++ harness
tests/host/sampler_host.cpp) equal the numpy restatement of sampler_csrc/rt_sampler.h (tests/_sampler_np.py) bit for bit: the metric,
the noisy rule and the dilation, the ascending lists, the gather, the fold and the normalisation, on seeded adversarial inputs; the
fold equals the film's (tests/_film_np.py); a pixel at the film's count normalises to its own bytes; the film's variance on the
normalised sums is within the bound the header derives of the variance at the true count; the harness as a stand-alone program runs
clean under the address and undefined-behaviour sanitizers.  Without the feature every test here fails: there is no sampler_csrc."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _film_np as fnp
import _sampler_np as snp

ROOT = Path(__file__).resolve().parents[1]
SAMPLER_CSRC = ROOT / "ray_tracer_s8_amd" / "sampler_csrc"
SRC = ROOT / "tests" / "host" / "sampler_host.cpp"
BUILD = ROOT / "tests" / "host" / "_build"
OUT = BUILD / "libsampler_host.so"
DEPS = [SRC, SAMPLER_CSRC / "rt_sampler_math.h"]
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-I{SAMPLER_CSRC}"]
f32 = np.float32
# (W, R, Hs): one pixel; one strip; three strips of 800 pixels; two strips of 4 550 (the shapes of tests/test_gpu_sampler.py)
SIZES = [(1, 1, 1), (70, 9, 9), (50, 48, 16), (130, 70, 35)]
PATTERNS = ("none", "all", "first", "last", "random")


@pytest.fixture(scope="module")
def lib():
    BUILD.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run([*GXX, "-fPIC", "-shared", "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    vp, u32 = C.c_void_p, C.c_uint32
    l.sampler_select_host.argtypes = [u32, u32, u32, u32, C.c_float, C.c_float] + [vp] * 5
    l.sampler_gather_host.argtypes = [u32, u32, u32, vp, vp, vp]
    l.sampler_fold_host.argtypes = [u32, u32, u32] + [vp] * 5
    l.sampler_normalise_host.argtypes = [C.c_uint64, u32] + [vp] * 5
    return l


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def host_select(lib, M, counts, hs, threshold, dilate, eps):
    R, W = counts.shape
    M, counts = np.ascontiguousarray(M, f32), np.ascontiguousarray(counts, np.int32)
    err = np.full((R, W), 7, f32)
    active = np.full(R * W, 0xFFFFFFFF, np.uint32)
    sc = np.zeros(R // hs, np.uint32)
    assert lib.sampler_select_host(W, R, hs, dilate, f32(threshold), f32(eps), M.ctypes.data, counts.ctypes.data, err.ctypes.data,
                                   active.ctypes.data, sc.ctypes.data) == 0
    P = hs * W
    lists = [active[i * P:i * P + sc[i]].copy() for i in range(R // hs)]
    for i, l in enumerate(lists):                                    # the elements behind a list are not written
        assert (active[i * P + sc[i]:(i + 1) * P] == 0xFFFFFFFF).all()
    return err, lists, sc


def check_select(lib, M, counts, hs, threshold, dilate, eps, what):
    err, lists, sc = host_select(lib, M, counts, hs, threshold, dilate, eps)
    werr, wlists, wsc = snp.select(M, counts, hs, threshold, dilate, eps)
    same(err, werr, (what, "err"))
    same(sc, wsc, (what, "strip counts"))
    for i, (g, w) in enumerate(zip(lists, wlists)):
        same(g, w, (what, "list", i))
        assert (np.diff(g.astype(np.int64)) > 0).all()               # strictly ascending
    return err, lists


@pytest.mark.parametrize("W,R,hs", SIZES)
def test_select_equals_the_restatement_on_every_pattern(lib, W, R, hs):
    rng = np.random.default_rng(1000 * R + W)
    for name in PATTERNS:
        flags = snp.pattern(name, rng, R, W)
        M, counts, thr, eps = snp.moments_for(flags)
        for dilate in (0, 1):
            err, lists = check_select(lib, M, counts, hs, thr, dilate, eps, (name, dilate))
            n = sum(len(l) for l in lists)
            if dilate == 0:
                assert n == int(flags.sum())
            if name == "none":
                assert n == 0
            if name == "all":
                assert n == R * W
    # seeded sums at mixed counts, around a threshold that is the median of their error
    counts = rng.integers(2, 30, (R, W)).astype(np.int32)
    M = snp.moments_of(rng, R, W, counts)
    thr = np.median(snp.pixel_error(M, counts, 2.0 ** -6))
    for dilate in (0, 1):
        check_select(lib, M, counts, hs, thr, dilate, 2.0 ** -6, ("seeded", dilate))


def test_the_metric_on_adversarial_sums(lib):
    M, counts, eps = snp.adversarial()
    for thr in (0.0, 0.05, 1.0, np.inf):
        for dilate in (0, 1):
            for hs in (6, 2, 1):
                err, lists = check_select(lib, M, counts, hs, thr, dilate, eps, ("adversarial", thr, dilate, hs))
    err = snp.pixel_error(M, counts, eps)
    flat, n, m = err.reshape(-1), counts.reshape(-1), M.reshape(-1, 2)
    assert (bits(flat[n < 2]) == 0x7FC00000).all() and (n < 2).sum() == 3                  # refused: the quiet NaN, never noisy
    assert (bits(flat[np.isnan(flat)]) == 0x7FC00000).all() and np.isnan(flat).sum() > 3     # NaN sums too
    assert not snp.noisy(flat[np.isnan(flat)], 0.0).any()
    cancel = (m[:, 0] == f32(3.0000002)) & (n == 3)                                          # d < 0 from cancellation: clamped, err +0
    assert cancel.sum() == 1 and bits(flat[cancel])[0] == 0
    both_inf = np.isinf(m[:, 0]) & np.isinf(m[:, 1]) & (m[:, 0] > 0)                         # inf - inf is not > 0: d = 0, err = 0
    assert both_inf.sum() == 1 and flat[both_inf][0] == 0
    assert np.isinf(flat[(m[:, 0] == 1) & np.isinf(m[:, 1])]).all()                          # S2 alone infinite: err = inf, noisy
    zero_mean = (m[:, 0] == 0) & (m[:, 1] == 4) & (n == 6)                                   # m = 0: the eps alone divides
    assert flat[zero_mean][0] == np.sqrt(f32(f32(4) / f32(6)) / f32(5)).astype(f32) / f32(eps)
    big = n == 1 << 24
    assert big.sum() == 1 and np.isfinite(flat[big]).all() and flat[big][0] > 0
    assert np.isfinite(flat[n == 2]).all() and (n == 2).sum() >= 2
    # +inf as the threshold: nothing is noisy, not even an infinite err
    assert sum(len(l) for l in snp.select(M, counts, 6, np.inf, 1, eps)[1]) == 0


def test_err_equal_to_the_threshold_is_not_noisy(lib):
    rng = np.random.default_rng(5)
    R, W = 4, 5
    counts = rng.integers(2, 20, (R, W)).astype(np.int32)
    M = snp.moments_of(rng, R, W, counts)
    err = snp.pixel_error(M, counts, 2.0 ** -6)
    for e in np.unique(err[err > 0]):
        _, lists = check_select(lib, M, counts, R, e, 0, 2.0 ** -6, ("equal", e))
        at = set(np.flatnonzero(err.reshape(-1) > e).tolist())
        assert set(lists[0].tolist()) == at and int(np.flatnonzero(err.reshape(-1) == e)[0]) not in at
        _, lists = check_select(lib, M, counts, R, np.nextafter(e, f32(0)), 0, 2.0 ** -6, ("below", e))
        assert set(np.flatnonzero(err.reshape(-1) == e).tolist()) <= set(lists[0].tolist())


def test_active_pixels_at_the_ends_of_strips_and_dilation_across_them(lib):
    W, R, hs = 7, 9, 3
    P = hs * W
    for spots in ([(0, 0)], [(2, 6)], [(3, 0)], [(5, 6)], [(2, 6), (3, 0)], [(0, 0), (0, 6), (8, 0), (8, 6)], [(2, 3)], [(3, 3)]):
        flags = np.zeros((R, W), bool)
        for y, x in spots:
            flags[y, x] = True
        M, counts, thr, eps = snp.moments_for(flags)
        _, lists = check_select(lib, M, counts, hs, thr, 0, eps, (spots, 0))
        assert sorted((i * hs + int(q) // W, int(q) % W) for i, l in enumerate(lists) for q in l) == sorted(spots)
        _, lists = check_select(lib, M, counts, hs, thr, 1, eps, (spots, 1))
        got = {(i * hs + int(q) // W, int(q) % W) for i, l in enumerate(lists) for q in l}
        want = {(y + dy, x + dx) for y, x in spots for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 0 <= y + dy < R and 0 <= x + dx < W}
        assert got == want
    # a strip's first and last index alone
    flags = np.zeros((R, W), bool)
    flags[3, 0] = flags[5, 6] = True
    M, counts, thr, eps = snp.moments_for(flags)
    _, lists = check_select(lib, M, counts, hs, thr, 0, eps, "ends")
    assert [l.tolist() for l in lists] == [[], [0, P - 1], []]
    # the noisy pixel of row 2 reaches into strip 1 and the corner's window is clipped
    flags = np.zeros((R, W), bool)
    flags[2, 6] = True
    M, counts, thr, eps = snp.moments_for(flags)
    _, lists = check_select(lib, M, counts, hs, thr, 1, eps, "across")
    assert lists[0].tolist() == [W + 5, W + 6, 2 * W + 5, 2 * W + 6] and lists[1].tolist() == [5, 6] and not len(lists[2])


@pytest.mark.parametrize("P,k", [(1, 1), (63, 3), (257, 7)])
def test_gather_and_fold_equal_the_restatement_and_the_films_fold(lib, P, k):
    rng = np.random.default_rng(P * 10 + k)
    for n_active in sorted({0, 1, P // 2, P}):
        active = np.sort(rng.permutation(P)[:n_active]).astype(np.uint32)
        rays = rng.integers(0, 256, (P * k, 32)).astype(np.uint8)
        out = np.full((n_active * k + 1, 32), 0xAB, np.uint8)
        assert lib.sampler_gather_host(n_active, k, P, active.ctypes.data, rays.ctypes.data, out.ctypes.data) == 0
        same(out[:-1], snp.gather(active, k, rays), ("gather", n_active))
        assert (out[-1] == 0xAB).all()
        for a in range(n_active):
            for j in range(k):
                assert (out[a * k + j] == rays[int(active[a]) * k + j]).all()
        rgb = fnp.adversarial_records(max(n_active, 1), k)[:n_active]
        acc0 = fnp.adversarial_records(P, 1, seed=3)[:, 0].copy()
        mom0 = rng.standard_normal((P, 2)).astype(f32)
        cnt0 = rng.integers(2, 50, P).astype(np.int32)
        acc, mom, cnt = acc0.copy(), mom0.copy(), cnt0.copy()
        assert lib.sampler_fold_host(n_active, k, P, active.ctypes.data, np.ascontiguousarray(rgb).ctypes.data, acc.ctypes.data,
                                     mom.ctypes.data, cnt.ctypes.data) == 0
        wa, wm, wc = snp.fold(acc0, mom0, cnt0, active, rgb.reshape(-1, 3), k)
        same(acc, wa, ("fold accum", n_active))
        same(mom, wm, ("fold moments", n_active))
        same(cnt, wc, ("fold counts", n_active))
        idle = np.setdiff1d(np.arange(P), active)
        same(acc[idle], acc0[idle], "untouched accum")
        same(mom[idle], mom0[idle], "untouched moments")
        assert (cnt[idle] == cnt0[idle]).all() and (cnt[active.astype(int)] == cnt0[active.astype(int)] + k).all()


@pytest.mark.parametrize("P,K", [(1, 1), (3, 7), (63, 7), (257, 7)])
def test_the_fold_is_the_films_fold(lib, P, K):
    """Every pixel active: rts_fold's lines on _film_np.adversarial_records have the bytes of _film_np.fold."""
    v = fnp.adversarial_records(P, K)
    want_acc, want_mom = fnp.fold(np.zeros((P, 3), f32), np.zeros((P, 2), f32), v)
    acc, mom, cnt = np.zeros((P, 3), f32), np.zeros((P, 2), f32), np.zeros(P, np.int32)
    active = np.arange(P, dtype=np.uint32)
    assert lib.sampler_fold_host(P, K, P, active.ctypes.data, v.ctypes.data, acc.ctypes.data, mom.ctypes.data, cnt.ctypes.data) == 0
    same(acc, want_acc, "accum")
    same(mom, want_mom, "moments")
    assert (cnt == K).all()
    # cut into sub-ranges, the sums carried: the same bytes
    if K > 2:
        acc, mom, cnt = np.zeros((P, 3), f32), np.zeros((P, 2), f32), np.zeros(P, np.int32)
        for b, e in ((0, 1), (1, K - 1), (K - 1, K)):
            part = np.ascontiguousarray(v[:, b:e])
            lib.sampler_fold_host(P, e - b, P, active.ctypes.data, part.ctypes.data, acc.ctypes.data, mom.ctypes.data, cnt.ctypes.data)
        same(acc, want_acc, "accum cut")
        same(mom, want_mom, "moments cut")
    a2, m2, _ = snp.fold(np.zeros((P, 3), f32), np.zeros((P, 2), f32), np.zeros(P, np.int32), active, v.reshape(-1, 3), K)
    same(a2, want_acc, "restated accum")
    same(m2, want_mom, "restated moments")


def host_normalise(lib, A, M, counts, e0):
    A, M, counts = np.ascontiguousarray(A, f32), np.ascontiguousarray(M, f32), np.ascontiguousarray(counts, np.int32)
    oA, oM = np.full_like(A, 9), np.full_like(M, 9)
    assert lib.sampler_normalise_host(counts.size, e0, A.ctypes.data, M.ctypes.data, counts.ctypes.data, oA.ctypes.data,
                                      oM.ctypes.data) == 0
    return oA, oM


def test_normalise_equals_the_restatement_and_copies_a_pixel_at_the_films_count(lib):
    M, counts, _ = snp.adversarial()
    rng = np.random.default_rng(11)
    A = fnp.adversarial_records(counts.size, 1, seed=9)[:, 0].reshape(*counts.shape, 3)
    for e0 in (2, 4, 5, 1 << 24):
        oA, oM = host_normalise(lib, A, M, counts, e0)
        wA, wM = snp.normalise(A, M, counts, e0)
        same(oA, wA, ("accum", e0))
        same(oM, wM, ("moments", e0))
        at = counts == e0
        same(oA[at], A[at], "a pixel at the film's count")
        same(oM[at], M[at], "a pixel at the film's count")
    # every pixel at the film's count, whatever its bytes: NaN payloads, -0, subnormals
    raw = rng.integers(0, 1 << 32, (64, 5), dtype=np.uint64).astype(np.uint32)
    raw[:8, 0] = [0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000]
    A, M = raw[:, :3].copy().view(f32), raw[:, 3:].copy().view(f32)
    oA, oM = host_normalise(lib, A, M, np.full(64, 6, np.int32), 6)
    assert oA.tobytes() == A.tobytes() and oM.tobytes() == M.tobytes()
    wA, wM = snp.normalise(A, M, np.full(64, 6, np.int32), 6)
    assert wA.tobytes() == A.tobytes() and wM.tobytes() == M.tobytes()


@pytest.mark.parametrize("e0", [2, 4, 16, 1000])
def test_the_films_variance_on_normalised_sums_is_the_true_count_variance_within_the_bound(lib, e0):
    """rt_sampler.h "THE BOUND": |v0' - v| <= 6u v + 4u a' / (e0 - 1), asserted as the header derives it."""
    rng = np.random.default_rng(e0)
    R, W = 40, 50
    counts = (e0 + rng.integers(0, 6, (R, W)) * rng.integers(1, 40, (R, W))).astype(np.int32)
    counts[0, :5] = [e0, e0 + 1, 1 << 20, 1 << 24, max(2, e0)]
    M = snp.moments_of(rng, R, W, counts)
    assert (counts == e0).any() and (counts > e0).any()
    _, Mp = host_normalise(lib, np.zeros((R, W, 3), f32), M, counts, e0)
    same(Mp, snp.normalise(np.zeros((R, W, 3), f32), M, counts, e0)[1], "moments")
    v0 = fnp.entry_variance(Mp, e0)                                    # what the film's resolve makes of the primed sums
    v = snp.true_variance(M, counts)
    bound = snp.variance_bound(v, Mp, e0)
    diff = np.abs(v0.astype(np.float64) - v.astype(np.float64))
    assert np.isfinite(diff).all() and (v > 0).sum() > R * W // 2
    worst = np.argmax(diff - bound)
    assert (diff <= bound).all(), (diff.reshape(-1)[worst], bound.reshape(-1)[worst], counts.reshape(-1)[worst])
    at = counts == e0
    same(v0[at], v[at], "at the film's count the variance is the film's")
    # not at e0's scale: without the g factor the film would divide the spread by e0 - 1, off by (n - 1) / (e0 - 1)
    far = (counts > e0) & (v > 1e-6)
    naive = snp.spread(M[..., 0], M[..., 1], counts.astype(f32)) / f32(e0 - 1)
    assert far.any() and (np.abs(naive[far] - v[far]) > bound[far]).all()


def test_the_stand_alone_harness_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "sampler_host"
    r = subprocess.run([*GXX, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSAMPLER_HOST_MAIN",
                        "-o", str(exe), str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pixels sampled" in r.stdout, r.stdout + r.stderr
