"""The regression resolve off the GPU: the product's per-pixel and per-node lines (film_csrc/rt_film_math.h, through
the g++ harness tests/host/film_regress_host.cpp) equal the numpy restatement of film_csrc/rt_film.h (tests/_film_regress_np.py) bit
for bit, model and outputs, on seeded synthetic images of five sizes under five plane subsets and on the awkward windows (no valid
pixel, one valid pixel, constant depth, zero normals, a flat wall, a failed pivot); and properties of the contract hold on the
restatement.  Without the feature every test here fails: rt_film_math.h has no rg_* function."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _film_regress_np as rnp

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
FILM_CSRC = ROOT / "ray_tracer_s8_amd" / "film_csrc"
SRC = ROOT / "tests" / "host" / "film_regress_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "libfilm_regress_host.so"
DEPS = [SRC, FILM_CSRC / "rt_film_math.h", CSRC / "rt_denoise_math.h", CSRC / "rt_consts.h"]
f32 = np.float32
OUTPUTS = ("linear", "f32", "rgb")
SIZES = [(1, 1), (16, 16), (17, 16), (33, 47), (70, 9)]                       # (W, R)
E, K = 8, 4
RIDGE, EPS = f32(1e-3), f32(2.0 ** -8)
# The exact-colour test's tolerance on |f32 - float64| of the linear output, of colours between 0.4 and 1.5.  Measured on the committed
# cases of test_exact_colours_come_back (the five sizes at ridge 1e-3 and 1e-5, printed by the test): the largest deviation is 5.61e-6
# (70 x 9 at ridge 1e-5; 5.20e-6 at ridge 1e-3; 3.0e-8 on 1 x 1).  Times 4, because the error of an f32 Cholesky solve grows with the
# conditioning of the normal equations, which the cases vary.
EXACT_TOL = 4 * 5.61e-6


def load_lib():
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", f"-I{FILM_CSRC}",
                        "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    l.film_regress_host.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 10
    l.film_regress_host.restype = None
    return l


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def host_resolve(lib, C_, e, *, A=None, k=K, albedo_eps=EPS, N=None, D=None, hits=None, ridge=RIDGE):
    R, W = C_.shape[:2]
    NY, NX = rnp.nodes(W, R)
    fp = np.array([e, k, albedo_eps, ridge], f32)
    model = np.full((NY, NX, rnp.RECORD), 7.0, f32)
    lin, ff, rgb = np.empty((R, W, 3), f32), np.empty((R, W, 3), f32), np.empty((R, W, 3), np.uint8)
    args = [np.ascontiguousarray(a) if a is not None else None for a in (C_, A, N, D, hits)]
    lib.film_regress_host(W, R, fp.ctypes.data, *[None if a is None else a.ctypes.data for a in args], model.ctypes.data,
                          lin.ctypes.data, ff.ctypes.data, rgb.ctypes.data)
    return dict(model=model, linear=lin, f32=ff, rgb=rgb)


def _eq(a, b, what):
    """Bit-equal, but a NaN for a NaN (the text leaves its payload open)."""
    if a.dtype == np.uint8:
        bad = np.argwhere(a != b)
    else:
        an, bn = np.isnan(a), np.isnan(b)
        bad = np.argwhere((an != bn) | (~an & ~bn & (a.view(np.uint32) != b.view(np.uint32))))
    assert len(bad) == 0, (what, len(bad), bad[:4], a[tuple(bad[0])], b[tuple(bad[0])])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32).tobytes()


@pytest.fixture(scope="module")
def images():
    return {(W, R): rnp.synthetic(np.random.default_rng(R * 1000 + W), R, W, E, K) for W, R in SIZES}


# ---- the host lines against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,R", SIZES)
@pytest.mark.parametrize("names", rnp.SUBSETS, ids=lambda n: "+".join(n) or "none")
def test_host_lines_equal_the_restatement(lib, images, W, R, names):
    s = images[(W, R)]
    kw = rnp.np_planes(s, names)
    for ridge in (RIDGE, f32(1e-1)):
        want = rnp.resolve(s["C"], E, k=K, albedo_eps=EPS, ridge=ridge, **kw)
        got = host_resolve(lib, s["C"], E, ridge=ridge, **kw)
        for o in ("model",) + OUTPUTS:
            _eq(got[o], want[o], (W, R, names, float(ridge), o))
    assert (want["model"][..., 27] == 1).any() or W * R == 1 or not s["hits"].any()


def special(kind):
    """The awkward windows, on 70 x 9 (five nodes across, two down), all planes given."""
    s = rnp.synthetic(np.random.default_rng(31), 9, 70, E, K)
    hits = s["hits"]
    if kind in ("no valid pixel", "one valid pixel"):
        hits[:, :32] = 0                                       # nodes 0 and 1 of both rows see no valid pixel
        if kind == "one valid pixel":
            hits[5, 3] = K
    elif kind == "constant depth":
        hits[:] = np.maximum(hits, 1)
        s["D"] = (f32(3) * hits.astype(f32)).astype(f32)
    elif kind == "zero normals":
        s["N"][:] = 0
    elif kind == "flat wall":
        s["N"] = (np.array([0.0, 0.6, 0.8], f32) * hits[..., None].astype(f32)).astype(f32)
    elif kind == "failed pivot":
        hits[:] = np.maximum(hits, 1)
        s["D"] = (f32(3) * hits.astype(f32)).astype(f32)
        s["D"][4, 40] = np.inf                                 # zeta = inf / inf: a NaN in A, no pivot > 0
    geo = hits > 0
    for k in ("A", "N", "D"):
        s[k][~geo] = 0
    return s


KINDS = ("no valid pixel", "one valid pixel", "constant depth", "zero normals", "flat wall", "failed pivot")


@pytest.mark.parametrize("kind", KINDS)
def test_awkward_windows(lib, kind):
    s = special(kind)
    names = rnp.SUBSETS[-1]
    kw = rnp.np_planes(s, names)
    want = rnp.resolve(s["C"], E, k=K, albedo_eps=EPS, ridge=RIDGE, **kw)
    got = host_resolve(lib, s["C"], E, **kw)
    for o in ("model",) + OUTPUTS:
        _eq(got[o], want[o], (kind, o))
    m = want["model"]
    n, flag = m[..., 26], m[..., 27]
    if kind == "no valid pixel":
        assert (n[:, :2] == 0).all() and not m[:, :2, :26].any() and (flag[:, :2] == 0).all() and (flag[:, 3:] == 1).all()
    if kind == "one valid pixel":
        assert (n[:, :2] == 1).all() and (flag[:, :2] == 1).all()
    if kind == "constant depth":
        assert not m[..., 25].any() and (m[..., 24] == 3).all() and (flag == 1).all() and not m[..., 12:18].any()
    if kind == "zero normals":
        assert (flag[n > 0] == 1).all() and not m[..., 3:12].any()
    if kind == "flat wall":
        assert (flag[n > 0] == 1).all() and np.isfinite(m).all()
    if kind == "failed pivot":
        failed = (flag == 0) & (n > 0)
        assert failed.any() and (flag == 1).any() and not m[failed][:, 3:24].any() and (m[failed][:, :3] > 0).all()
        assert np.isfinite(want["linear"]).all()


def test_a_pivot_lost_to_rounding_falls_back(lib):
    """A flat wall under a ridge below the rounding of A: the normal's columns are collinear with phi0, and where the pivot of one
    comes out not above zero the node takes the constant fallback; host and restatement agree on which."""
    s = special("flat wall")
    kw = rnp.np_planes(s, ("normal", "hits"))
    want = rnp.resolve(s["C"], E, k=K, ridge=f32(1e-12), **kw)
    got = host_resolve(lib, s["C"], E, ridge=f32(1e-12), **kw)
    for o in ("model",) + OUTPUTS:
        _eq(got[o], want[o], o)
    m = want["model"]
    failed = (m[..., 27] == 0) & (m[..., 26] > 0)
    assert failed.any() and not m[failed][:, 3:24].any() and np.isfinite(want["linear"]).all()


@pytest.mark.parametrize("tier", ("small", "huge", "nonfinite"))
def test_extreme_planes(lib, tier):
    """The cases tests/test_gpu_film_regress.py runs on the device (tests/_extreme_planes.py's values), under its rule: a NaN where
    the restatement has one, the same bits elsewhere."""
    import _extreme_planes as xp
    calls = nans = fallback = subnormal = 0
    for name, names, s in rnp.extreme_cases(tier, EPS):
        for ridge in (RIDGE, f32(1e-1)):
            kw = rnp.np_planes(s, names)
            want = rnp.resolve(s["C"], xp.E, k=xp.K, albedo_eps=EPS, ridge=ridge, **kw)
            got = host_resolve(lib, s["C"], xp.E, k=xp.K, ridge=ridge, **kw)
            for o in ("model",) + OUTPUTS:
                xp.same(got[o], want[o], (tier, name, names, float(ridge), o))
            calls += 1
            nans += int(np.isnan(want["linear"]).sum())
            fallback += int(((want["model"][..., 27] == 0) & (want["model"][..., 26] > 0)).sum())
            mag = np.abs(want["linear"])
            subnormal += int(((mag > 0) & (mag < xp.TINY)).sum())
    print(tier, calls, "calls,", nans, "NaNs,", fallback, "fallbacks,", subnormal, "subnormal outputs")
    assert calls >= 6
    if tier == "nonfinite":
        assert nans > 0 and fallback > 0
    if tier == "small":
        assert nans == 0 and subnormal > 0


# ---- properties of the contract, on the restatement -------------------------------------------------------------------------------
def linear_image(rng, W, R):
    """Planes with every pixel hit, and a colour that is an exact linear function of the eight features over the whole frame: of 1,
    the unit normal, z, z^2, x and y (z and z^2 are linear in a window's zeta and zeta^2, x and y in its phi6 and phi7).  In a
    window's own features the weights but the constant's have a norm below 0.4."""
    yy, xx = np.mgrid[0:R, 0:W].astype(np.float64)
    N = rng.normal(size=(R, W, 3)) * 0.3 + np.array([0.2, 0.4, 0.8])
    N = N.astype(f32)
    hits = np.full((R, W), K, np.uint32)
    z = (2.0 + 2.0 * rng.random((R, W))).astype(f32)
    D = (z * f32(K)).astype(f32)
    # the features as the resolve will see them, in double
    _, _, n, zp, _ = rnp.entry(np.zeros((R, W, 3), f32), 1, None, 1, EPS, N, D, hits, np.float64)
    col = 0.5 + n @ np.array([0.1, -0.1, 0.1]) + 0.05 * zp + 0.01 * zp * zp + 0.005 * xx / max(W / 16, 1) + 0.005 * yy / max(R / 16, 1)
    col = np.stack([col, 0.5 * col, 0.25 + 0.25 * col], -1)
    return dict(C=(col * E).astype(f32), N=N, D=D, hits=hits), col


@pytest.mark.parametrize("W,R", SIZES)
def test_exact_colours_come_back(W, R):
    s, col = linear_image(np.random.default_rng(77 + W), W, R)
    kw = dict(N=s["N"], D=s["D"], hits=s["hits"])
    # in double under a ridge of 1e-9 the fit is the colour: the ridge objective at its minimum is at most its value at the true
    # weights, lambda n |w'|^2, so no residual exceeds sqrt(1024 lambda) |w'| < 1e-3 * 0.4; the colours were rounded to f32 (1e-7)
    d = rnp.resolve(s["C"], E, ridge=f32(1e-9), dtype=np.float64, **kw)
    assert np.abs(d["linear"] - col).max() < 4e-4, np.abs(d["linear"] - col).max()
    # ... and f32 follows the double evaluation of the same text on the same inputs
    worst = 0.0
    for ridge in (RIDGE, f32(1e-5)):
        a = rnp.resolve(s["C"], E, ridge=ridge, **kw)
        b = rnp.resolve(s["C"], E, ridge=ridge, dtype=np.float64, **kw)
        assert (a["model"][..., 27] == 1).all()
        dev = np.abs(a["linear"].astype(np.float64) - b["linear"]).max()
        print(f"exact colours {W} x {R}, ridge {float(ridge):g}: max |f32 - f64| = {dev:.3g}")
        worst = max(worst, dev)
    assert worst <= EXACT_TOL, worst


def test_invalid_pixels_pass_through(images):
    s = images[(33, 47)]
    for names in (("hits",), rnp.SUBSETS[-1]):
        out = rnp.resolve(s["C"], E, k=K, **rnp.np_planes(s, names))
        inv = ~out["valid"]
        assert inv.any() and (s["hits"][inv] == 0).all() and out["valid"].any()
        assert _bits(out["fitted"][inv]) == _bits(out["r"][inv])
        if names == ("hits",):
            assert _bits(out["linear"][inv]) == _bits((s["C"] / f32(E))[inv])
        assert _bits(out["fitted"][~inv]) != _bits(out["r"][~inv])


def test_the_weights_sum_to_one():
    """Four identical node models give that model's value, up to the four roundings of the blend: 4 * 2^-24 relative."""
    R, W = 40, 40
    yy, xx = np.mgrid[0:R, 0:W]
    fx = (((xx & 15).astype(f32) + f32(0.5)) / f32(16)).astype(f32)
    fy = (((yy & 15).astype(f32) + f32(0.5)) / f32(16)).astype(f32)
    wts = [(f32(1) - fx) * (f32(1) - fy), fx * (f32(1) - fy), (f32(1) - fx) * fy, fx * fy]
    assert all(w.dtype == f32 for w in wts)
    total = sum(w.astype(np.float64) for w in wts)
    assert (total == 1.0).all()                                 # exactly: every weight is a multiple of 2^-10
    assert all(((w.astype(np.float64) * 1024) % 1 == 0).all() for w in wts)
    # one model in every node, with no weight on the window position (the only features that differ between a pixel's four nodes)
    rng = np.random.default_rng(5)
    rec = np.zeros(rnp.RECORD, f32)
    rec[:18] = rng.random(18).astype(f32) * f32(0.2)
    rec[24:28] = [1.0, 2.0, 1024.0, 1.0]
    NY, NX = rnp.nodes(W, R)
    model = np.broadcast_to(rec, (NY, NX, rnp.RECORD)).copy()
    nrm = rng.normal(size=(R, W, 3)).astype(f32)
    z = (f32(1) + f32(2) * rng.random((R, W)).astype(f32)).astype(f32)
    valid = np.ones((R, W), bool)
    got = rnp.apply(np.zeros((R, W, 3), f32), nrm, z, valid, model, f32)
    phi = rnp.features(nrm, z, f32(1), f32(2), xx, yy, f32)
    for c in range(3):
        m = np.zeros((R, W), f32)
        for k in range(6):
            m = (m + rec[3 * k + c] * phi[k]).astype(f32)
        m = np.where(m > 0, m, f32(0))
        assert (m > 0).any() and np.abs(got[..., c].astype(np.float64) - m).max() <= 4 * 2.0 ** -24 * m.max(), c


def test_outputs_are_never_negative(images):
    for (W, R), s in images.items():
        for names in rnp.SUBSETS:
            out = rnp.resolve(s["C"], E, k=K, **rnp.np_planes(s, names))
            for o in ("linear", "f32"):
                assert (out[o] >= 0).all() and not np.signbit(out[o][out["valid"]]).any(), (W, R, names, o)
            assert np.array_equal(out["rgb"], rnp.dn.as_u8(out["f32"] * f32(255.999)))
    # a colour far below what the planes explain: the fit undershoots somewhere and is clamped at +0
    s = images[(33, 47)]
    Cn = s["C"].copy()
    Cn[::3, ::2] = 0
    Cn[1::3, 1::2] *= f32(40)
    out = rnp.resolve(Cn, E, k=K, **rnp.np_planes(s, ("normal", "depth", "hits")))
    assert (out["linear"] >= 0).all() and (out["linear"][out["valid"]] == 0).any()
