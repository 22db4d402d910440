"""The operand corpus of tests/_sampling_cases.py — everything that samples a light or scatters a ray — without a GPU:
(a) every class the module lists holds at least FLOOR directed records, counted by the classifier alone — so the GPU tests of
    tests/test_gpu_sampling_operands.py cannot pass without the device having met each regime end, degenerate distance, fold, pick
    and weight edge at least FLOOR times;
(b) on the whole directed corpus and 2^16 seeded records per family the g++ builds of the product's own lines (tests/host/
    {direct,lightpick,cone,nee}_host.cpp over csrc/rt_direct_math.h and csrc/rt_nee_math.h) equal the numpy restatement bit for bit
    (flags as booleans, a word one side leaves unwritten as 0): the words the device is held to are the g++ build's.  SCATTER and SKY
    have no host form (rt_path_steps.hip.h is device code): their restatement is held to tests/_bounce_np.py's scatter_dir — the
    lines `step` runs, factored out of it — and to its unit_sphere_vec and sky_colour, restatements `step` does not call (it takes
    both from the oracle), which are held to oracle.draw and oracle.sky here;
(c) negative controls: numpy twins with one mutation each differ from the restatement on the directed corpus, and only in the
    classes named here:
      the last product of dot3 fused (float64, rounded once)      only where that product is inexact           "dot inexact"
      x / len as x * (1 / len)                                     only where 1 / len is inexact                "rcp inexact"
      subnormal inputs and results flushed to zero                 only where an operation met a subnormal      "subnormal"
      q > 2^-10 for q >= 2^-10                                     exactly the records of                        "q==2^-10"
      u1 + u2 >= 1 for u1 + u2 > 1                                 only in                                       "u1+u2==1"
      x <= c[k] for x < c[k]                                       only in                                       "x on a running sum"
      pick_light without its clamp                                 exactly the records of                        "u==1"
(d) what the restatement promises on the corpus: on every record in the cone regime no NaN but from a NaN normal, and the bounds
    of tests/test_cone_host.py, 0 <= W <= 2 ip where facing and |v.v - 1| <= 2^-18; the search by power never returns an emitter
    without power; every pick is below M."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _bounce_np as B
import _sampling_cases as S

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
BUILD = ROOT / "tests" / "host" / "_build"
GXX = ["g++", "-std=c++17", "-ffp-contract=off", "-pthread", f"-I{CSRC}", f"-I{ROOT / 'include'}"]
F = np.float32
N_SEEDED = 1 << 16
FAMILIES = list(S.NAMES)
IDS = [S.NAMES[f] for f in FAMILIES]


def _host(name):
    """the g++ harness tests/host/<name>_host.cpp as a shared library (built as its own test builds it)"""
    src, out = ROOT / "tests" / "host" / f"{name}_host.cpp", BUILD / f"lib{name}_host.so"
    deps = [src] + sorted(CSRC.glob("*.h")) + [ROOT / "include" / "rt_tile.h"]
    BUILD.mkdir(exist_ok=True)
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(GXX + ["-O2", "-fPIC", "-shared", "-o", str(out), str(src)], check=True)
    return C.CDLL(str(out))


@pytest.fixture(scope="module")
def hosts():
    libs = {k: _host(k) for k in ("direct", "lightpick", "cone", "nee")}
    vp, u32 = C.c_void_p, C.c_uint32
    for lib, fn in (("direct", "direct_math"), ("lightpick", "lightpick_weights"), ("lightpick", "lightpick_pick_records"),
                    ("cone", "cone_samples"), ("cone", "cone_views"), ("nee", "nee_view"), ("nee", "nee_weights")):
        getattr(libs[lib], fn).argtypes = [u32, vp, vp]
        getattr(libs[lib], fn).restype = None
    return libs


_corpus = {}


def corpus(family):
    """(records: directed then 2^16 seeded, the number of directed ones, the restatement's words, the classes of the directed ones)"""
    if family not in _corpus:
        rec = S.records(family, N_SEEDED)
        nd = len(S.DIRECTED[family]())
        want = S.expected(family, rec)
        for a in (rec, want):
            a.setflags(write=False)
        _corpus[family] = (rec, nd, want, S.classify(family, rec[:nd]))
    return _corpus[family]


# ---------------------------------------------------------------- (a) the class counts
@pytest.mark.parametrize("family", FAMILIES, ids=IDS)
def test_every_class_holds_the_floor(family):
    rec, nd, _, c = corpus(family)
    assert rec.shape[1] == S.WORDS[family][0] and nd >= S.FLOOR
    short = {k: int(c[k].sum()) for k in S.CLASSES[family] if int(c[k].sum()) < S.FLOOR}
    assert not short, (S.NAMES[family], "classes below the floor of", S.FLOOR, short)


def test_the_units_carry_the_families_of_the_header():
    """Documentation only: the comment table of rt_unit_sampling.hip.h says what tests/_sampling_cases.py uses.  What the code does
    (unit_carries, the words per record) is pinned by tests/test_gpu_sampling_operands.py, which runs and refuses every pair."""
    text = (CSRC / "rt_unit_sampling.hip.h").read_text()
    for fam, (wi, wo) in S.WORDS.items():
        line = next(l for l in text.splitlines() if l.startswith(f"//   {fam:2d} "))
        assert f"in {wi:2d}:" in line and f"out {wo:2d}:" in line, line
        carried = {int(x) for x in line.split()[-2:] if x.isdigit()}
        assert carried == {u for name, u in S.UNITS.items() if fam in S.CARRIES[name]}, line


# ---------------------------------------------------------------- (b) g++ against numpy
def _call(fn, rec, words_out):
    rec = np.ascontiguousarray(rec)
    out = np.zeros((len(rec), words_out), np.uint32)
    fn(len(rec), rec.ctypes.data, out.ctypes.data)
    return out


def _host_words(hosts, family, rec):
    if family == S.DIRECT:
        return _call(hosts["direct"].direct_math, rec, 16)
    if family == S.WEIGHT_IP:
        return _call(hosts["lightpick"].lightpick_weights, rec, 2)
    if family == S.PICK_POWER:
        return _call(hosts["lightpick"].lightpick_pick_records, rec, 2)
    if family == S.CONE:
        return _call(hosts["cone"].cone_samples, rec, 20)
    if family == S.CONE_VIEW:
        return _call(hosts["cone"].cone_views, rec, 5)
    assert family == S.NEE_VIEW
    return np.concatenate([_call(hosts["nee"].nee_view, rec[:, :13], 6), _call(hosts["nee"].nee_weights, rec[:, 13:14], 2)], axis=1)


def _first(family, rec, nd, got, want, bad, what):
    i = int(np.nonzero(bad)[0][0])
    classes = S.describe(S.classify(family, np.ascontiguousarray(rec[i:i + 1])), 0)
    return (f"{S.NAMES[family]} {what}: {int(bad.sum())} of {len(rec)} records differ; first: record {i} "
            f"({'directed' if i < nd else 'seeded'}) = {rec[i].view(F).tolist()} (words {[hex(w) for w in rec[i]]}), classes {classes}, "
            f"got {[hex(w) for w in got[i]]}, restatement {[hex(w) for w in want[i]]}")


@pytest.mark.parametrize("family", [S.DIRECT, S.WEIGHT_IP, S.PICK_POWER, S.CONE, S.CONE_VIEW, S.NEE_VIEW],
                         ids=lambda f: S.NAMES[f])
def test_host_build_equals_the_restatement(hosts, family):
    rec, nd, want, _ = corpus(family)
    got = _host_words(hosts, family, rec)
    bad = ~S.words_equal(family, got, want).all(axis=1)
    assert not bad.any(), _first(family, rec, nd, got, want, bad, "g++ harness")


def test_scatter_and_sky_equal_the_path_step_and_the_oracle(oracle):
    rec, nd, want, _ = corpus(S.SCATTER)
    f = rec.view(F)
    with np.errstate(all="ignore"):
        us = B.unit_sphere_vec(f[:, 7], f[:, 8], f[:, 9])
        out, ok = B.scatter_dir(us, f[:, 3:6], f[:, 0:3], f[:, 6])
    got = np.concatenate([us.view(np.uint32), np.ascontiguousarray(out, F).view(np.uint32), (~ok).astype(np.uint32)[:, None]], axis=1)
    bad = ~S.words_equal(S.SCATTER, got, want).all(axis=1)
    assert not bad.any(), _first(S.SCATTER, rec, nd, got, want, bad, "_bounce_np.scatter_dir")
    # the UnitSphere vector of the pairs the oracle itself accepts: two Uniform(-1, 1) draws per round, then its own UnitSphere draw
    states = B.R.states(2048, 99)
    for st in states:
        chk = st.copy()
        while True:
            x1, x2 = F(oracle.draw(st, 1)[0]), F(oracle.draw(st, 1)[0])
            sm = F(x1 * x1 + x2 * x2)
            if not (sm >= F(1)):
                break
        mine = B.unit_sphere_vec(np.array([x1]), np.array([x2]), np.array([sm]))[0]
        assert np.array_equal(mine.view(np.uint32), oracle.draw(chk, 3).astype(F).view(np.uint32)) and np.array_equal(chk, st)
    rec, nd, want, _ = corpus(S.SKY)
    with np.errstate(all="ignore"):
        sky = B.sky_colour(rec.view(F))
    got = np.ascontiguousarray(sky, F).view(np.uint32)
    bad = ~S.words_equal(S.SKY, got, want).all(axis=1)
    assert not bad.any(), _first(S.SKY, rec, nd, got, want, bad, "_bounce_np.sky_colour")
    ref = np.stack([oracle.sky(d) for d in rec.view(F)]).view(np.uint32)
    bad = ~S.words_equal(S.SKY, got, ref).all(axis=1)
    assert not bad.any(), _first(S.SKY, rec, nd, got, ref, bad, "oracle.sky")


# ---------------------------------------------------------------- (c) the negative controls
def _changed(family, ops=S.PLAIN, mut=()):
    """(the directed records whose words a twin changes, the classes of the directed records)"""
    rec, nd, want, c = corpus(family)
    got, _ = S.RESTATE[family](np.ascontiguousarray(rec[:nd]), ops, mut)
    return ~S.words_equal(family, got, want[:nd]).all(axis=1), c


BROAD = {"dot inexact": (S.FusedDot, (S.DIRECT, S.CONE, S.CONE_VIEW, S.NEE_VIEW, S.SCATTER, S.SKY)),
         "rcp inexact": (S.RcpDiv, (S.DIRECT, S.CONE, S.SCATTER)),
         "subnormal": (S.FlushOps, (S.DIRECT, S.WEIGHT_IP, S.CONE, S.CONE_VIEW, S.NEE_VIEW, S.SCATTER, S.SKY))}


@pytest.mark.parametrize("name", list(BROAD))
def test_an_arithmetic_mutation_shows_and_only_in_its_class(name):
    """a fused dot, a reciprocal for a division, flushed subnormals: in every family that has the operation at least FLOOR directed
    records change a word, all of them records where the restatement met the operand class that names the mutation"""
    ops, families = BROAD[name]
    for family in families:
        changed, c = _changed(family, ops())
        assert int(changed.sum()) >= S.FLOOR, (name, S.NAMES[family], int(changed.sum()))
        stray = changed & ~c[name]
        assert not stray.any(), (name, S.NAMES[family], int(stray.sum()), S.describe(c, int(np.nonzero(stray)[0][0])))
    for family in FAMILIES:
        if family not in families:                                             # the family has no such operation
            assert not _changed(family, ops())[0].any(), (name, S.NAMES[family])


def test_a_comparison_mutation_shows_and_only_in_its_class():
    for family in (S.CONE, S.CONE_VIEW):
        changed, c = _changed(family, mut=("q >",))
        assert np.array_equal(changed, c["q==2^-10"]) and int(changed.sum()) >= S.FLOOR, S.NAMES[family]
    changed, c = _changed(S.DIRECT, mut=("fold >=",))
    assert int(changed.sum()) >= S.FLOOR and not (changed & ~c["u1+u2==1"]).any()
    changed, c = _changed(S.PICK_POWER, mut=("x <= c",))
    assert int(changed.sum()) >= S.FLOOR and not (changed & ~c["x on a running sum"]).any()
    for family in (S.DIRECT, S.PICK_POWER):
        changed, c = _changed(family, mut=("no clamp",))
        assert np.array_equal(changed, c["u==1"]) and int(changed.sum()) >= S.FLOOR, S.NAMES[family]


def test_the_clamp_of_the_uniform_pick_is_dead_for_every_u_below_one():
    """u (float)M for the largest u01 is M - M 2^-24, at least half a spacing below M: it never rounds up to M, so for u < 1 the
    clamp of pick_light takes nothing.  Checked on every M of the corpus and on a sweep up to 2^23."""
    M = np.unique(np.concatenate([np.arange(1, 1 << 16), np.arange((1 << 23) - (1 << 16), (1 << 23) + 1),
                                  (1 << np.arange(0, 24)), (1 << np.arange(1, 24)) + 1, (1 << np.arange(1, 24)) - 1]))
    k = (S.U_LAST * M.astype(F)).astype(np.int64)
    assert (k <= M - 1).all() and (k[M > 1] == M[M > 1] - 1).sum() > 0


# ---------------------------------------------------------------- (d) what the restatement promises
def test_cone_invariants_hold_on_the_restatement():
    rec, nd, want, _ = corpus(S.CONE)
    classes = S.classify(S.CONE, rec, trace=False)
    n_reg, n_fac = S.cone_invariants(rec, want, classes)
    assert n_reg >= (1 << 15) and n_fac >= (1 << 14)
    # the bounds cover the edge classes too: directed records in the regime with a subnormal dc2 or r r, s at both ends, w.z = -1
    reg = want[:, 1] != 0
    deep = classes["in the regime, dc2<2^-130"]
    for k in ("dc2 subnormal", "r*r subnormal", "s==0", "s==pred(1)", "w.z==-1", "h clamped"):
        assert int((reg & classes[k] & ~deep).sum()) >= S.FLOOR, k
    # ... and the premise of the v.v bound is needed: below 2^-130 the restatement itself (the g++ build's words) breaks it
    dev = np.abs(want.view(F)[deep, 19].astype(np.float64) - 1.0)
    assert int(deep.sum()) >= S.FLOOR and dev.max() > 2.0 ** -18


def test_the_picks_are_in_range_and_skip_emitters_without_power():
    rec, nd, want, _ = corpus(S.PICK_POWER)
    _, i = S.restate_pick_power(rec)
    M, k, u = i["M"].astype(np.int64), want[:, 0].astype(np.int64), i["u"]
    inside = i["valid"] & (u < F(1))
    assert (k[inside] < M[inside]).all() and (want[inside, 1] < i["M_big"][inside]).all()
    # the search: the pick's own power c[k] - c[k - 1] is positive whenever x lies below the last sum
    c = i["c"]
    n = len(rec)
    found = i["valid"] & ~i["degenerate"] & ~i["lower"] & (i["first"] < M)
    own = c[np.arange(n), np.clip(k, 0, 15)]
    before = np.where(k > 0, c[np.arange(n), np.clip(k - 1, 0, 15)], F(0))
    assert int(found.sum()) >= (1 << 14) and (own[found] > before[found]).all()
    rec, nd, want, _ = corpus(S.DIRECT)
    ok = rec.view(F)[:, 2] < F(1)
    assert (want[ok, 0] < rec[ok, 1]).all()
