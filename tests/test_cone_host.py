"""Cone sampling of sphere lights off the GPU, through the g++ harness tests/host/cone_host.cpp:
(a) the regime test (csrc/rt_direct_math.h cone_regime) at 2^-10, at 1 and at their two f32 neighbours each, and at 0, inf and NaN;
(b) the cone sample, its geometry, weight and point equal the numpy restatement of rt_tile.h (tests/_cone_np.py) bit for bit, on
    structured operands — q at the regime's ends, r = 0 and a subnormal radius, dc2 = 0, inf and NaN, s = 0, the smallest positive s
    and the largest s below 1, the axis along +-x, +-y, +-z exactly with w.z = -0.0 among them — and on 2^16 seeded ones; on every
    in-regime operand no NaN, 0 <= W <= 2 ip and |v.v - 1| <= 2^-18;
(c) the cone view of an emitter the bounce reached (csrc/rt_nee_math.h emitter_view_cone) equals the restatement;
(d) unbiased against the closed form: for a cone wholly above the hit's horizon E[cs * 2 omc] = q (n.w) exactly, and the mean of 2^20
    samples is within 5 sample standard errors of it, on three geometries;
(e) the rim share: with the light alone in the scene, the share of cone samples whose shadow ray (oracle.intersect_batch) does not hit
    the emitter is at most 2^-14 at r/dc = 0.9, 0.3, 1/16 and 1/32, 2^19 samples each;
(f) the restatement's drivers (tests/_lights_np.py) with cone=False give the bytes recorded from the drivers of tests/_lightpick_np.py
    that they replaced (tests/test_light_restatement.py), and with cone=True leave the same states and segments;
(g) the harness as a stand-alone program under -fsanitize=address,undefined."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _bounce_np as B
import _cone_np as CN
import _direct_np as D
import _lightpick_np as LP
import _lights_np as LN
from ray_tracer_s8_amd import _abi
from test_light_restatement import recorded

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
SRC = ROOT / "tests" / "host" / "cone_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "libcone_host.so"
DEPS = [SRC, CSRC / "rt_direct_math.h", CSRC / "rt_nee_math.h", CSRC / "rt_consts.h"]
GXX = ["g++", "-std=c++17", "-ffp-contract=off", "-pthread", f"-I{CSRC}", f"-I{ROOT / 'include'}"]
F32 = np.float32
CONE_IN, CONE_OUT, VIEW_IN, VIEW_OUT = 16, 20, 14, 5
R = B.R


@pytest.fixture(scope="module")
def lib():
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(GXX + ["-O2", "-fPIC", "-shared", "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    vp, u32 = C.c_void_p, C.c_uint32
    l.cone_regimes.argtypes = [u32, vp, vp]
    l.cone_samples.argtypes = [u32, vp, vp]
    l.cone_views.argtypes = [u32, vp, vp]
    return l


def _nb(x, up):
    return np.nextafter(F32(x), F32(np.inf if up else -np.inf))


# ---------------------------------------------------------------- (a) the regime
def test_regime_at_its_ends(lib):
    lo, hi = F32(2.0 ** -10), F32(1)
    qs = np.array([_nb(lo, False), lo, _nb(lo, True), _nb(hi, False), hi, _nb(hi, True), 0.0, -0.0, np.inf, -np.inf, np.nan, 0.5,
                   1e-45, -0.5], F32)
    want = [0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    out = np.zeros(len(qs), np.uint32)
    lib.cone_regimes(len(qs), qs.ctypes.data, out.ctypes.data)
    assert out.tolist() == want
    assert [int(CN.cone_regime(q)) for q in qs] == want
    assert CN.Q_MIN == lo and float(lo) == 1 / 1024


# ---------------------------------------------------------------- (b) the sample
def _host_samples(lib, P, c, r, x1, x2, s, n, ip):
    """cone_samples on arrays (vectors (m, 3)); returns the (m, CONE_OUT) words."""
    m = len(r)
    rec = np.zeros((m, CONE_IN), F32)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 7], rec[:, 8], rec[:, 9], rec[:, 10:13], rec[:, 13] = P, c, r, x1, x2, s, n, ip
    out = np.zeros((m, CONE_OUT), np.uint32)
    lib.cone_samples(m, rec.ctypes.data, out.ctypes.data)
    return out


def _restated(P, c, r, x1, x2, s, n, ip):
    """The restatement on the same arrays, in the harness's output layout (float32; columns 1 and 14 are flags)."""
    PT, cT, nT = P.T.astype(F32), c.T.astype(F32), n.T.astype(F32)
    q = CN.cone_axis(PT, cT, r)[3]
    reg = CN.cone_regime(q)
    k = CN.cone_sample(PT, cT, r, x1, x2, s)
    wn, cs, facing = CN.cone_geometry(nT, k["v"])
    W = CN.cone_weight(cs, k["omc"], ip)
    L = CN.cone_point(PT, wn, k)
    with np.errstate(all="ignore"):
        vv = D.dot(k["v"], k["v"])
    cols = [q, reg, *k["v"], k["omc"], k["dc2"], k["dc"], k["ct"], k["st"], *wn, cs, facing, W, *L, vv]
    return np.stack([np.asarray(x, F32) for x in cols], 1), reg


def _assert_samples(lib, P, c, r, x1, x2, s, n, ip, what):
    got = _host_samples(lib, P, c, r, x1, x2, s, n, ip)
    want, reg = _restated(P, c, r, x1, x2, s, n, ip)
    assert np.array_equal(got[:, 1] != 0, reg), what
    assert B.same_bits(got[:, 0].view(F32), want[:, 0]).all(), (what, "q")
    assert not got[~reg][:, 1:].any(), (what, "words written outside the regime")
    if not reg.any():
        return 0, 0.0
    g, w = got[reg], want[reg]
    for col in (14,):
        assert np.array_equal(g[:, col] != 0, w[:, col] != 0), (what, col)
    for col in [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 19]:
        ok = B.same_bits(g[:, col].view(F32), w[:, col])
        assert ok.all(), (what, col, np.nonzero(~ok)[0][:5], g[~ok][:2, col].view(F32), w[~ok][:2, col])
    # the properties of every in-regime operand
    f = g.view(F32)
    assert not np.isnan(f[:, [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 17, 18, 19]]).any(), what
    dev = np.abs(f[:, 19].astype(np.float64) - 1)
    assert dev.max() <= 2.0 ** -18, (what, dev.max())
    facing = g[:, 14] != 0
    # W = fl(x ip) with x = fl(cs (omc + omc)) < 2 for a unit n: omc <= 1 - 2^-12 at the largest q below 1, which outweighs the few
    # ulps by which a rounded unit normal's cs can exceed 1; rounding is monotone, so W <= fl(2 ip) = 2 ip exactly
    W, ipr = f[:, 15].astype(np.float64), np.broadcast_to(np.asarray(ip, F32), (len(r),))[reg].astype(np.float64)
    assert np.all(W[facing] >= 0) and np.all(W[facing] <= 2 * ipr[facing]), (what, W[facing].max())
    return int(reg.sum()), float(dev.max())


def _pairs(g, m):
    """m accepted pairs of Uniform(-1, 1) draws, float32, with s = x1 x1 + x2 x2 < 1 as the kernel forms it."""
    x = np.zeros((0, 2), F32)
    while len(x) < m:
        c = g.uniform(-1, 1, (2 * m, 2)).astype(F32)
        x = np.concatenate([x, c[(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) < F32(1)]])
    x = x[:m]
    return x[:, 0].copy(), x[:, 1].copy(), (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]).astype(F32)


def test_structured_operands_equal_the_restatement(lib):
    """Every axis, both signs of zero in w.z, s at its ends, q at the regime's ends (P at the origin and c a unit axis vector: dc2 = 1
    exactly and q = r r), degenerate radii and distances."""
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 0, -0.0), (0, 1, -0.0), (-1, 0, -0.0), (0.6, 0.8, 0.0),
            (0.6, 0.0, -0.8), (0.0, 0.28, 0.96)]
    tiny = F32(2.0 ** -75)                                                  # s = 2^-150 rounds to 0 ... and 2^-149 is the smallest s
    pairs = [(0.0, 0.0), (tiny, 0.0), (0.0, -tiny), (F32(2.0 ** -74.5), 0.0), (_nb(1, False), 0.0), (F32(0.70710677), F32(0.70710671)),
             (-0.6, 0.79999995), (0.3, -0.4), (-0.0, 0.0)]
    lo = F32(2.0 ** -5)                                                     # r = 2^-5: q = 2^-10 exactly
    radii = [0.0, 1e-41, _nb(lo, False), lo, _nb(lo, True), 0.3, 0.9, _nb(1, False), 1.0, _nb(1, True), 1.5, np.inf, np.nan]
    rows = [(a, p, r) for a in axes for p in pairs for r in radii]
    m = len(rows)
    c = np.array([a for a, _, _ in rows], F32)
    x1, x2 = np.array([p[0] for _, p, _ in rows], F32), np.array([p[1] for _, p, _ in rows], F32)
    s = (x1 * x1 + x2 * x2).astype(F32)
    r = np.array([r for _, _, r in rows], F32)
    assert (s == 0).sum() >= 3 * len(axes) * len(radii) and (s == F32(2.0 ** -149)).any()
    assert np.signbit(c[:, 2]).any() and (c[:, 2] == 0).any()
    P = np.zeros((m, 3), F32)
    n_in, _ = _assert_samples(lib, P, c, r, x1, x2, s, c.copy(), F32(33), "structured")
    assert n_in >= 9 * len(pairs) * 5          # on the nine exact axes: lo, its upper neighbour, 0.3, 0.9 and the largest r below 1
    # s exactly at its ends, whatever pair would give it
    for sv in (0.0, 2.0 ** -149, float(_nb(1, False))):
        k = len(axes)
        _assert_samples(lib, np.zeros((k, 3), F32), np.array(axes, F32), np.full(k, 0.5, F32), np.full(k, 0.6, F32), np.full(k, -0.8, F32),
                        np.full(k, sv, F32), np.array(axes, F32), F32(2), ("s", sv))
    # dc2 = 0, inf, NaN and subnormal: never in the regime, whatever the radius
    far = np.array([(0, 0, 0), (np.inf, 0, 0), (np.nan, 0, 0), (1e30, 1e30, 0), (1e-30, 0, 0), (3e-23, 0, 0)], F32)
    k = len(far)
    got = _host_samples(lib, np.zeros((k, 3), F32), far, np.full(k, 0.5, F32), np.full(k, 0.1, F32), np.full(k, 0.2, F32),
                        np.full(k, 0.05, F32), np.tile(np.array([1, 0, 0], F32), (k, 1)), F32(2))
    assert not got[:, 1].any()
    _assert_samples(lib, np.zeros((k, 3), F32), far, np.full(k, 0.5, F32), np.full(k, 0.1, F32), np.full(k, 0.2, F32), np.full(k, 0.05, F32),
                    np.tile(np.array([1, 0, 0], F32), (k, 1)), F32(2), "degenerate distances")


def test_seeded_operands_equal_the_restatement(lib):
    g = np.random.default_rng(2020)
    m = 1 << 16
    P = g.uniform(-5, 5, (m, 3)).astype(F32)
    w = g.normal(size=(m, 3))
    w /= np.linalg.norm(w, axis=1)[:, None]
    r = (10.0 ** g.uniform(-2, 1, m)).astype(F32)
    ratio = np.where(g.random(m) < 0.15, g.uniform(0.02, 0.04, m), g.uniform(0.02, 1.1, m))     # r / dc, the regime's ends well covered
    c = (P + w * (r / ratio)[:, None]).astype(F32)
    x1, x2, s = _pairs(g, m)
    n = g.normal(size=(m, 3))
    n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(F32)
    ip = np.where(g.random(m) < 0.5, g.integers(1, 40, m), 1 / g.uniform(0.01, 1, m)).astype(F32)
    n_in, dev = _assert_samples(lib, P, c, r, x1, x2, s, n, ip, "seeded")
    print(f"{n_in} of {m} operands in the regime; largest |v.v - 1| = {dev:.3g} (bound 2^-18 = {2.0 ** -18:.3g})")
    assert n_in > 0.7 * m and m - n_in > 0.05 * m


# ---------------------------------------------------------------- (c) the view
def test_views_equal_the_restatement(lib):
    g = np.random.default_rng(2021)
    m = 20000
    o = g.uniform(-5, 5, (m, 3)).astype(F32)
    w = g.normal(size=(m, 3))
    w /= np.linalg.norm(w, axis=1)[:, None]
    r = (10.0 ** g.uniform(-2, 1, m)).astype(F32)
    ratio = g.uniform(0.02, 1.2, m)
    ratio[:6] = [1 / 32, 1 / 32 * (1 - 1e-7), 1 / 32 * (1 + 1e-7), 1.0, 1 - 1e-7, 1 + 1e-7]
    c = (o + w * (r / ratio)[:, None]).astype(F32)
    c[6], r[6] = o[6], 0.5                                                  # dc2 = 0
    r[7] = 0.0
    d = (w + g.normal(0, 0.1, (m, 3)))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F32)
    n = g.normal(size=(m, 3))
    n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(F32)
    ip = g.integers(1, 40, m).astype(F32)
    rec = np.zeros((m, VIEW_IN), F32)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12], rec[:, 12], rec[:, 13] = o, n, d, c, r, ip
    out = np.zeros((m, VIEW_OUT), np.uint32)
    lib.cone_views(m, rec.ctypes.data, out.ctypes.data)
    cs, omc, reg, samplable = CN.emitter_view_cone(o.T.copy(), n.T.copy(), d.T.copy(), c.T.copy(), r)
    W = CN.cone_weight(cs, omc, ip)
    f = out.view(F32)
    assert np.array_equal(out[:, 2] != 0, reg) and np.array_equal(out[:, 3] != 0, samplable)
    assert B.same_bits(f[:, 0], cs).all() and B.same_bits(f[:, 1], omc).all() and B.same_bits(f[:, 4], W).all()
    assert 0.6 * m < reg.sum() < m and 0 < samplable.sum() < reg.sum() and not reg[6] and not reg[7]
    assert np.all(f[:, 4][samplable] <= 2 * ip[samplable]) and np.all(f[:, 4][samplable] > 0)
    # the sample at P and the view from o = P speak of the same omc
    x1, x2, s = _pairs(g, m)
    smp = _host_samples(lib, o, c, r, x1, x2, s, n, ip)
    assert np.array_equal(smp[:, 1] != 0, reg) and np.array_equal(smp[reg][:, 5], out[reg][:, 1])


# ---------------------------------------------------------------- (d) unbiased against the closed form
@pytest.mark.parametrize("ratio,tilt", [(0.3, 0.0), (0.8, 0.1), (0.05, 1.2)])
def test_mean_weight_is_the_closed_form(lib, ratio, tilt):
    """The cone of half-angle asin(r / dc) about w lies wholly above the horizon of n when the angle between n and w is below
    pi / 2 - asin(r / dc); then cs > 0 on all of it and E[cs * 2 omc] = (1 / pi) * integral of cos over the cone = q (n.w), q = (r /
    dc)^2.  W at ip = 1 is cs * 2 omc.  The sample standard error is that of the 2^20 W values themselves."""
    assert tilt + np.arcsin(ratio) < np.pi / 2 - 0.05
    g = np.random.default_rng(int(ratio * 1000))
    m = 1 << 20
    P = np.array([0.3, -0.2, 0.1], F32)
    w = np.array([0.36, 0.48, -0.8])
    r = F32(0.5)
    c = (P + w * (float(r) / ratio)).astype(F32)
    t = np.cross(w, [0.0, 0.0, 1.0])
    t /= np.linalg.norm(t)
    n = (np.cos(tilt) * w + np.sin(tilt) * t).astype(F32)
    x1, x2, s = _pairs(g, m)
    out = _host_samples(lib, np.tile(P, (m, 1)), np.tile(c, (m, 1)), np.full(m, r, F32), x1, x2, s, np.tile(n, (m, 1)), F32(1))
    assert out[:, 1].all() and out[:, 14].all()                             # every sample in the regime and facing
    W = out[:, 15].view(F32).astype(np.float64)
    a = c.astype(np.float64) - P.astype(np.float64)
    q = float(r) ** 2 / (a @ a)
    closed = q * (n.astype(np.float64) @ (a / np.sqrt(a @ a)))
    se = W.std(ddof=1) / np.sqrt(m)
    print(f"r/dc {ratio}: mean W {W.mean():.6g}, closed form {closed:.6g}, gap {abs(W.mean() - closed):.3g}, 5 standard errors {5 * se:.3g}; "
          f"variance {W.var(ddof=1):.3g}, largest W {W.max():.4g}")
    assert abs(W.mean() - closed) <= 5 * se
    assert W.max() <= 2.0


# ---------------------------------------------------------------- (e) the rim share
@pytest.mark.parametrize("ratio", [0.9, 0.3, 1 / 16, 1 / 32])
def test_rim_share(lib, oracle, ratio):
    """The light alone in the scene: nothing occludes, so a cone sample that does not hit the emitter left the cone by rounding (or met
    the sphere closer than t_min, which the distances here exclude).  At most 2^-14 of 2^19 samples may, at every ratio; 1/32 is the
    regime's edge, where points that round to q < 2^-10 take the area sample and are drawn again."""
    g = np.random.default_rng(int(ratio * 4096))
    m = 1 << 19
    sph = np.zeros(1, _abi.SPHERE_DTYPE)
    sph["cx"], sph["cy"], sph["cz"], sph["radius"], sph["emission"] = 0.25, -0.5, 1.5, 0.5, 4.0
    sph["albedo_r"], sph["albedo_g"], sph["albedo_b"] = 1.0, 1.0, 1.0
    c = np.array([0.25, -0.5, 1.5], F32)
    P = np.zeros((0, 3), F32)
    while len(P) < m:
        w = g.normal(size=(m, 3))
        w /= np.linalg.norm(w, axis=1)[:, None]
        cand = (c - w * (0.5 / ratio)).astype(F32)
        P = np.concatenate([P, cand[CN.cone_regime(CN.cone_axis(cand.T.copy(), c[:, None], F32(0.5))[3])]])
    P = np.ascontiguousarray(P[:m])
    x1, x2, s = _pairs(g, m)
    out = _host_samples(lib, P, np.tile(c, (m, 1)), np.full(m, 0.5, F32), x1, x2, s, np.tile(np.array([0, 1, 0], F32), (m, 1)), F32(1))
    assert out[:, 1].all()
    v = out[:, 2:5].view(F32)
    rays = np.zeros(m, _abi.RAY_DTYPE)
    rays["ox"], rays["oy"], rays["oz"], rays["dx"], rays["dy"], rays["dz"] = P[:, 0], P[:, 1], P[:, 2], v[:, 0], v[:, 1], v[:, 2]
    rays["t_min"], rays["t_max"] = 0.001, 1000.0
    e = oracle.intersect_batch(sph, B.NO_TRI, rays, backend=1)
    missed = int((~e["hit"]).sum())
    print(f"r/dc {ratio:.5f}: {missed} of {m} cone samples miss the emitter: share {missed / m:.3g} (cap 2^-14 = {2.0 ** -14:.3g})")
    assert missed / m <= 2.0 ** -14


# ---------------------------------------------------------------- (f) the drivers
@pytest.mark.parametrize("name", ["two_lights", "regimes"])
def test_drivers_without_the_setting_are_the_lightpick_restatement(oracle, name):
    if name == "two_lights":
        sph, tri, wi = LP.two_lights()
        rays = D.camera_rays(16, 10, 0.6, -0.1)
    else:
        sph, tri = CN.regimes_scene()
        wi = None
        rays = CN.regimes_rays(160)
    n = len(rays)
    st = R.states(n, 4100)
    step = B.step(oracle, sph, tri, rays, st, 1, wi)
    for by_power in (False, True):
        a = recorded(f"direct/_lightpick_np/{name}/p{int(by_power)}c0g0")    # (LP.direct of these hits and states, by_power=by_power)
        b = LN.direct(oracle, sph, tri, step["hits"], step["states"], 1, wi, by_power=by_power, cone=False)
        c = LN.direct(oracle, sph, tri, step["hits"], step["states"], 1, wi, by_power=by_power, cone=True)
        assert a["direct"].tobytes() == b["direct"].tobytes() and np.array_equal(a["states"], b["states"])
        assert np.array_equal(a["shadow"], b["shadow"]) and not b["in_cone"].any()
        assert np.array_equal(c["states"], a["states"]) and c["in_cone"].sum() > 20
        tri_rec = ~c["in_cone"]                                             # a record outside the regime, or of a triangle: AREA's bytes
        assert c["direct"][tri_rec].tobytes() == a["direct"][tri_rec].tobytes()
        assert (c["direct"]["status"] == D.FACING_AWAY).sum() < (a["direct"]["status"] == D.FACING_AWAY).sum()
        m = 60
        x = recorded(f"nee/_lightpick_np/{name}/p{int(by_power)}c0g0")       # (LP.nee of these rays and states, by_power=by_power)
        y = LN.nee(oracle, sph, tri, rays[:m], 2, 3, 1, wi, states=st[:m], by_power=by_power, cone=False)
        z = LN.nee(oracle, sph, tri, rays[:m], 2, 3, 1, wi, states=st[:m], by_power=by_power, cone=True)
        for mode in LN.MODES:
            assert x["rgb"][mode].tobytes() == y["rgb"][mode].tobytes()
        assert np.array_equal(x["segments"], y["segments"]) and np.array_equal(x["shadow"], y["shadow"]) and np.array_equal(x["states"], y["states"])
        assert np.array_equal(z["segments"], x["segments"]) and np.array_equal(z["states"], x["states"])


# ---------------------------------------------------------------- (g) under a sanitizer, stand-alone
def test_host_program_under_sanitizers(tmp_path):
    exe = tmp_path / "cone_host_san"
    r = subprocess.run(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCONE_HOST_MAIN", "-o",
                              str(exe), str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "CONE_HOST_OK" in run.stdout and not run.stderr, run.stdout + run.stderr
