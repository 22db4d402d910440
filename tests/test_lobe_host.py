"""Light samples at glossy hits off the GPU, through the g++ harness tests/host/lobe_host.cpp:
(a) the sampled-class rule (csrc/rt_lobe_math.h sampled_class) on its boundaries: rho at 0, -0, 2^-24, 1 - 2^-24, 1 and beyond, negative,
    NaN and inf, each with gn at 0, above and below it;
(b) the glossy direction, the lobe, its factor of a direction and its factor of the scatter's own draw equal the numpy restatement of rt_tile.h (tests/_lobe_np.py) bit for bit on the
    operand corpus of tests/_lobe_cases.py — the directed records, every enumerated class at least FLOOR times, and 2^16 seeded ones.
    cg == cs is NOT asserted at rho = 0: that hit takes the diffuse path and never the lobe formula;
(c) at every lobe-sampled seeded record kappa >= 0 (the origin lies outside the sphere, or on it) and kappa is within 2^-19 of its terms
    of the header's formula in float64, which is |c|^2 - r^2 up to r^2 (n.n - 1); in the lobe cg > 0 and is no NaN;
(d) the restatement's driver (tests/_lights_np.py) with glossy=False gives the bytes recorded from tests/_cone_np.py's `nee` that it
    replaced (tests/test_light_restatement.py); with glossy=True on the glossy room it meets every class, drops some lobe samples, and a scene whose roughnesses are 0 and 1 only gives glossy=False's RT_NEE_MIS bytes;
(e) the harness as a stand-alone program under -fsanitize=address,undefined."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _bounce_np as B
import _direct_np as D
import _lights_np as LN
import _lobe_cases as LC
import _lobe_np as L
from test_light_restatement import assert_recorded, scene

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
SRC = ROOT / "tests" / "host" / "lobe_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "liblobe_host.so"
DEPS = [SRC, CSRC / "rt_lobe_math.h", CSRC / "rt_direct_math.h", CSRC / "rt_consts.h"]
GXX = ["g++", "-std=c++17", "-ffp-contract=off", "-pthread", f"-I{CSRC}", f"-I{ROOT / 'include'}"]
F32 = np.float32
R = B.R


@pytest.fixture(scope="module")
def lib():
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(GXX + ["-O2", "-fPIC", "-shared", "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    l.lobe_records.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    return l


def _host(lib, rec):
    rec = np.ascontiguousarray(rec, F32)
    out = np.zeros((len(rec), LC.WORDS[1]), np.uint32)
    lib.lobe_records(len(rec), rec.ctypes.data, out.ctypes.data)
    return out


# ---------------------------------------------------------------- (a) the class rule
def test_class_rule_on_its_boundaries(lib):
    up = [0.0, 1.0, 0.0]
    dirs = {"front": [0.6, -0.8, 0.0], "grazing": [1.0, 0.0, 0.0], "back": [0.6, 0.8, 0.0]}
    rhos = [(0.0, 1), (-0.0, 1), (1e-45, 2), (2.0 ** -24, 2), (0.5, 2), (1 - 2.0 ** -24, 2), (1.0, 0), (1 + 2.0 ** -23, 0), (-1e-45, 0),
            (-0.5, 0), (np.nan, 0), (np.inf, 0), (-np.inf, 0)]
    rec, want = [], []
    for rho, cls in rhos:
        for name, d in dirs.items():
            rec.append(LC._rec(up, d, rho, up))
            want.append(cls if (name != "back" or cls == L.DIFFUSE) else L.NONE)
    rec = np.array(rec, F32)
    got = _host(lib, rec)
    assert got[:, 0].tolist() == want
    gn = got[:, 4].view(F32).reshape(-1, 3)
    assert (gn[:, 0] > 0).all() and (gn[:, 1] == 0).all() and (gn[:, 2] < 0).all()
    assert LC.expected(rec)[:, 0].tolist() == want
    assert [int(L.sampled_class(F32(r), F32(g))) for r, g in ((0.5, np.nan), (0.5, -0.0), (0.0, np.nan))] == [L.NONE, L.LOBE, L.DIFFUSE]


# ---------------------------------------------------------------- (b) the header under g++ against the restatement
def test_directed_corpus_holds_every_class():
    rec = LC.directed()
    m = LC.classify(rec, LC.expected(rec))
    short = {k: int(v.sum()) for k, v in m.items() if v.sum() < LC.FLOOR}
    assert not short, short


def test_harness_equals_the_restatement_bit_for_bit(lib):
    rec = LC.records(1 << 16)
    want = LC.expected(rec)
    got = _host(lib, rec)
    ok = LC.words_equal(got, want)
    bad = ~ok.all(1)
    i = int(np.nonzero(bad)[0][0]) if bad.any() else 0
    assert not bad.any(), (int(bad.sum()), i, rec[i].tolist(), np.nonzero(~ok[i])[0].tolist(), [hex(x) for x in got[i]], [hex(x) for x in want[i]])
    m = LC.classify(rec, want)
    assert m["in lobe"].sum() > 5000 and m["class lobe"].sum() > 20000 and m["class none"].sum() > 5000


# ---------------------------------------------------------------- (c) properties
def test_kappa_is_positive_and_accurate_at_lobe_sampled_hits(lib):
    rec = LC.seeded(1 << 16, seed=1700)
    got = _host(lib, rec)
    f = got.view(F32)
    lobe = got[:, 0] == L.LOBE
    assert lobe.sum() > 20000
    n, d, rho = (rec[:, 0:3].astype(np.float64), rec[:, 3:6].astype(np.float64), rec[:, 6].astype(np.float64))
    g = d - 2 * np.einsum("ij,ij->i", d, n)[:, None] * n
    gn, gg, r = np.einsum("ij,ij->i", n, g), np.einsum("ij,ij->i", g, g), 1 - rho
    kappa = rho * (rho * gg + 2 * r * gn)                                   # the header's formula in float64 ...
    cc = np.einsum("ij,ij->i", (r[:, None] * n + rho[:, None] * g), (r[:, None] * n + rho[:, None] * g))
    nn = np.einsum("ij,ij->i", n, n)
    # ... which is |c|^2 - r^2 up to r^2 (n.n - 1): a normal rounded to f32 is a unit vector to 2^-23 only
    assert (np.abs(kappa - (cc - r * r) - r * r * (1 - nn)) <= 1e-15).all() and (np.abs(nn - 1) <= 2.0 ** -22).all()
    assert (f[lobe, 9] >= 0).all() and (f[lobe & (rho > 1e-6) & (gn > 1e-6), 9] > 0).all()
    # g carries three roundings per component (an absolute 2^-22 in gn and gg), kappa five more of terms no larger than
    # rho (rho gg + 2 r): 2^-19 of that covers both
    assert (np.abs(f[lobe, 9] - kappa[lobe]) <= 2.0 ** -19 * (rho * (rho * gg + 2 * r))[lobe] + 1e-45).all()
    inl = got[:, 12] != 0
    assert (f[inl & lobe, 13] > 0).all() and not np.isnan(f[inl, 13]).any() and (f[~inl, 13] == 0).all()
    assert not (got[:, 14] != 0)[~inl].any()


# ---------------------------------------------------------------- (d) the restatement's driver
def _glossy_room():
    from test_gpu_nee import _rooms
    return _rooms("glossy")


def test_driver_without_the_setting_is_the_cone_restatement_and_with_it_meets_every_class(oracle):
    sph, tri = _glossy_room()
    rays = D.camera_rays(12, 8, 0.6, -0.1)
    n = len(rays)
    st = R.states(n, 1800)
    held = scene("glossy")["nee"]                                           # the rays of this batch whose results are recorded
    for cone in (False, True):
        a = LN.nee(oracle, sph, tri, rays, 2, 3, 1, None, states=st, cone=cone, glossy=False)
        assert_recorded(a, f"nee/_cone_np/glossy/p0c{int(cone)}g0", held)    # (CN.nee of these rays and states, cone=cone)
        z = LN.nee(oracle, sph, tri, rays, 2, 3, 1, None, states=st, cone=cone, glossy=True)
        assert_recorded(z, f"nee/_lobe_np/glossy/p0c{int(cone)}g1", held)
        cnt = z["counts"]
        assert cnt["lobe"] > 20 and cnt["diffuse"] > 5 and cnt["none"] > 5 and cnt["dropped"] > 0, cnt
        assert cnt["dropped"] < cnt["lobe"] and z["shadow"].sum() > a["shadow"].sum()
        assert not np.array_equal(z["states"], a["states"]) and z["rgb"][LN.MIS].tobytes() != a["rgb"][LN.MIS].tobytes()
        assert np.isfinite(z["rgb"][LN.MIS]).all()
    # roughnesses 0 and 1 only: no hit is lobe-sampled, RT_GLOSSY_BOUNCE's bytes
    sph2 = sph.copy()
    sph2["roughness"][:4] = [1.0, 0.0, 1.0, 0.0]
    a = LN.nee(oracle, sph2, tri, rays, 2, 3, 1, None, states=st, cone=False, glossy=False)
    assert_recorded(a, "nee/_cone_np/rough01/p0c0g0", held)
    z = LN.nee(oracle, sph2, tri, rays, 2, 3, 1, None, states=st, cone=False, glossy=True)
    assert z["counts"]["lobe"] == 0 and z["rgb"][LN.MIS].tobytes() == a["rgb"][LN.MIS].tobytes()
    assert np.array_equal(z["states"], a["states"]) and np.array_equal(z["shadow"], a["shadow"])


# ---------------------------------------------------------------- (e) under a sanitizer, stand-alone
def test_host_program_under_sanitizers(tmp_path):
    exe = tmp_path / "lobe_host_san"
    r = subprocess.run(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLOBE_HOST_MAIN", "-o",
                              str(exe), str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "LOBE_HOST_OK" in run.stdout and not run.stderr, run.stdout + run.stderr
