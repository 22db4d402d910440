"""The density of the reference's scatter lobe (rt_tile.h "light samples at glossy hits"), checked in float64 numpy
with fixed seeds and 2^20 draws per estimate:
(a) p(w) = (b^2 + D) / (2 pi r sqrt(D)) is the density of normalize(c + r us): for h = 1 and h = w.a, the mean of sqrt(D) h(w) over
    scatter draws equals the integral of h (b^2 + D) / (2 pi r) over the lobe, estimated with uniform directions, within
    5 sqrt(se1^2 + se2^2), on five (d, n, rho) with rho in {0.05, 0.3, 0.7, 0.95} (sqrt(D) removes the 1 / sqrt(D) singularity from
    both sides, so both estimates have a finite variance);
(b) negative control: with the Lambertian cs / pi in the place of p(w) the same bound is violated at rho = 0.7;
(c) the rim: the share of scatter draws that the float32 restatement (tests/_lobe_np.py: the glossy direction, the lobe and the factor
    the kernel forms for the direction its scatter takes, lobe_factor_scatter) puts outside the lobe is measured and printed, and is
    below the cone rim's documented 2^-14.  Nothing else is asserted about it.  For the record the same share is measured for
    D = b b - kappa of the f32 direction, the form the contract first had: 4.2e-5, 9.5e-7, 5.1e-4, 1.6e-3 and 7.5e-4 on the five
    configurations, above 2^-14 on three — which is why the factor of the scatter's own direction is formed from its draw;
(d) lobe_factor_scatter is lobe_factor of the scattered direction: in float64 the two agree on 2^16 draws per configuration, and the
    float32 factor is within 2^-8 of the float64 one wherever D > 2^-12 kappa."""
import numpy as np
import pytest

import _lobe_np as L

N = 1 << 20
F32 = np.float32


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _config(k):
    """(d, n, rho): front-face hits from normal incidence to grazing"""
    g = np.random.default_rng(2100 + k)
    n = _unit(g.normal(size=3))
    t = _unit(np.cross(n, g.normal(size=3)))
    ang = (0.0, 0.5, 1.0, 1.4, 1.2)[k]
    d = -np.cos(ang) * n + np.sin(ang) * t
    return d, n, (0.05, 0.3, 0.7, 0.95, 0.7)[k]


CONFIGS = list(range(5))


def _lobe(d, n, rho):
    g = d - 2 * (d @ n) * n
    r = 1 - rho
    c = r * n + rho * g
    return c, r, c @ c - r * r


def _sphere(g, m):
    return _unit(g.normal(size=(m, 3)))


@pytest.mark.parametrize("k", CONFIGS)
def test_density_matches_the_scatter(k):
    d, n, rho = _config(k)
    c, r, kappa = _lobe(d, n, rho)
    assert kappa > 0
    g = np.random.default_rng(2200 + k)
    a = _unit(g.normal(size=3))
    ws = _unit(c + r * _sphere(g, N))                                      # scatter draws
    wu = _sphere(g, N)                                                     # uniform directions, density 1 / (4 pi)
    for name, h in (("1", lambda w: np.ones(len(w))), ("w.a", lambda w: w @ a)):
        bs = ws @ c
        Ds = bs * bs - kappa
        assert (bs > 0).all() and (Ds > -1e-12).all()
        x = np.sqrt(np.maximum(Ds, 0)) * h(ws)
        bu = wu @ c
        Du = bu * bu - kappa
        inl = (bu > 0) & (Du > 0)
        y = np.where(inl, 4 * np.pi * h(wu) * (bu * bu + Du) / (2 * np.pi * r), 0.0)
        m1, m2 = x.mean(), y.mean()
        se = np.sqrt(x.var(ddof=1) / N + y.var(ddof=1) / N)
        print(f"config {k} rho {rho} h {name}: scatter {m1:.6f} lobe integral {m2:.6f} gap {abs(m1 - m2):.2e} bound {5 * se:.2e}")
        assert abs(m1 - m2) <= 5 * se, (k, name, m1, m2, se)


def test_negative_control_the_lambertian_density_fails_at_rho_0_7():
    d, n, rho = _config(2)
    assert rho == 0.7
    c, r, kappa = _lobe(d, n, rho)
    g = np.random.default_rng(2300)
    ws = _unit(c + r * _sphere(g, N))
    wu = _sphere(g, N)
    bs = ws @ c
    x = np.sqrt(np.maximum(bs * bs - kappa, 0))
    bu = wu @ c
    Du = bu * bu - kappa
    inl = (bu > 0) & (Du > 0)
    cs = wu @ n
    y = np.where(inl & (cs > 0), 4 * np.pi * np.sqrt(np.maximum(Du, 0)) * cs / np.pi, 0.0)   # sqrt(D) h p with p = cs / pi
    se = np.sqrt(x.var(ddof=1) / N + y.var(ddof=1) / N)
    print("negative control: scatter", x.mean(), "Lambertian", y.mean(), "bound", 5 * se)
    assert abs(x.mean() - y.mean()) > 5 * se


def rim_share(k, m=N):
    """(share, count) of the scatter draws of configuration k that the float32 arithmetic puts outside the lobe, the operands rounded to
    f32, the lobe and the factor by the restatement — by lobe_factor_scatter of the draw, which is what the kernel forms for a bounce
    direction — and (share, count) by lobe_factor of the direction formed as the path step forms it (diffuse + rho (glossy -
    diffuse), normalised by a reciprocal and then by a division), the contract's first form."""
    d, n, rho = _config(k)
    g = np.random.default_rng(2400 + k)
    d32, n32 = (d.astype(F32)[:, None], n.astype(F32)[:, None])
    rho32 = F32(rho)
    us = _sphere(g, m).T.astype(F32)
    with np.errstate(all="ignore"):
        gl = L.glossy_dir(d32, n32)
        diffuse = (us + n32).astype(F32)
        pre = (diffuse + rho32 * (gl - diffuse)).astype(F32)
        rcp = F32(1) / np.sqrt(L.D.dot(pre, pre))
        x = (pre * rcp).astype(F32)
        w = (x / np.sqrt(L.D.dot(x, x))).astype(F32)
        lobe = L.lobe_of(n32[:, 0], gl[:, 0], rho32)
        b, Dd, inl, cg = L.lobe_factor((lobe[0][:, None], lobe[1], lobe[2]), w)
        ins = L.lobe_factor_scatter((lobe[0][:, None], lobe[1], lobe[2]), us)[3]
    return (float((~ins).mean()), int((~ins).sum())), (float((~inl).mean()), int((~inl).sum()))


def test_rim_share_in_f32_is_below_the_cone_rims():
    shares = []
    for k in CONFIGS:
        (share, count), (old, old_count) = rim_share(k)
        rho = _config(k)[2]
        print(f"config {k} rho {rho}: {count} of {N} scatter draws outside the lobe in f32, share {share:.3e}; by D = b b - kappa of the "
              f"f32 direction {old_count}, share {old:.3e}")
        shares.append(share)
    print("largest share", max(shares), "2^-14 =", 2.0 ** -14)
    assert max(shares) < 2.0 ** -14, shares


@pytest.mark.parametrize("k", CONFIGS)
def test_scatter_factor_is_the_factor_of_the_scattered_direction(k):
    d, n, rho = _config(k)
    c, r, kappa = _lobe(d, n, rho)
    g = np.random.default_rng(2500 + k)
    us = _sphere(g, 1 << 16)
    X = c + r * us
    t = np.linalg.norm(X, axis=1)
    w = X / t[:, None]
    b = w @ c
    Dd = b * b - kappa
    m = r * (us @ c + r)
    assert np.allclose(t * t, kappa + 2 * m, rtol=1e-12, atol=1e-15) and np.allclose(np.sqrt(np.maximum(Dd, 0)), np.abs(m) / t, atol=1e-7)
    cg_s = ((kappa + m) ** 2 + m * m) / (2 * r * np.abs(m) * t)
    ok = Dd > 1e-6 * kappa                                                 # (b b - kappa cancels in float64 too, next to the rim)
    cg_w = (b * b + Dd) / (2 * r * np.sqrt(np.where(ok, Dd, 1.0)))
    assert ok.mean() > 0.95 and (np.abs(cg_s - cg_w)[ok] <= 1e-8 * cg_s[ok]).all()
    # float32 against float64, away from the rim: m carries an absolute error of about 2^-22 |c| r, which is relative to |m| in cg
    d32, n32 = d.astype(F32), n.astype(F32)
    gl = L.glossy_dir(d32, n32)
    lobe = L.lobe_of(n32, gl, F32(rho))
    _, _, cg32, in32 = L.lobe_factor_scatter((lobe[0][:, None], lobe[1], lobe[2]), us.T.astype(F32))
    far = Dd > 2.0 ** -12 * kappa
    assert in32.all() and far.mean() > 0.5
    assert (np.abs(cg32[far] - cg_s[far]) <= 2.0 ** -8 * cg_s[far]).all(), float((np.abs(cg32 - cg_s) / cg_s)[far].max())
