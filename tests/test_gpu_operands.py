"""The device functions of the closest-hit arithmetic against the oracle, operand by operand and bit for bit.

rt_debug_unit (test library; ray_tracer_s8_amd/csrc/rt_unit.hip.h) runs one lane per record through exact_sphere, exact_triangle,
intersects_aabb / intersects_aabb_finite, normalize / try_normalize, f32_as_u8 or the RNG, as the translation unit named compiles
them (lin: the compiler's square root and SLP vectorisation; trav and query: sqrt_rn, no SLP).  The records are the directed corpus
of tests/_operand_cases.py — every decision of the reference at least 64 times, tests/test_operand_corpus.py — plus 2^20 seeded
random records; the expected words come from the oracle's nested forms (oracle.operands_batch), computed once per family.
A failure prints the first offending record, the classes it belongs to, and both bit patterns."""
import ctypes as C

import numpy as np
import pytest

from ray_tracer_s8_amd import _abi

import _operand_cases as OC

pytestmark = pytest.mark.gpu

N_RANDOM = 1 << 20
ORACLE_THREADS = 16
UNITS = {"lin": 0, "trav": 1, "query": 2}


@pytest.fixture(scope="module")
def dbg(ndev):
    lib = _abi.load_debug()
    n = C.c_int(0)
    assert lib.rt_init(C.byref(n)) == 0 and n.value >= 1
    return lib


def run_unit(lib, unit, family, rec):
    rec = np.ascontiguousarray(rec)
    assert rec.dtype.itemsize == 4 and rec.shape[1] == OC.WORDS[family][0]
    out = np.zeros((len(rec), OC.WORDS[family][1]), np.uint32)
    rc = lib.rt_debug_unit(0, UNITS[unit], family, len(rec), rec.ctypes.data, out.ctypes.data)
    assert rc == 0, (rc, lib.rt_last_error().decode())
    return out


def _records(family):
    if family in (OC.SPHERE, OC.SPHERE_NORM):
        return np.concatenate([OC.sphere_directed(), OC.sphere_random(N_RANDOM)])
    if family == OC.TRIANGLE:
        return np.concatenate([OC.triangle_directed(), OC.triangle_random(N_RANDOM)])
    if family == OC.AABB:
        return np.concatenate([OC.aabb_directed(), OC.aabb_random(N_RANDOM)])
    if family == OC.CHAIN:
        return OC.chain_records(np.concatenate([OC.aabb_directed(), OC.aabb_random(N_RANDOM)]))
    if family == OC.NORMALIZE:
        return np.concatenate([OC.normalize_directed(), OC.normalize_random(N_RANDOM)])
    if family == OC.AS_U8:
        return np.concatenate([OC.as_u8_directed(), OC.as_u8_random(N_RANDOM)])
    return OC.rng_seeds(1 << 16)


_CLASSIFY = {OC.SPHERE: OC.classify_sphere, OC.SPHERE_NORM: lambda r: OC.classify_sphere(r, True), OC.TRIANGLE: OC.classify_triangle,
             OC.AABB: OC.classify_aabb, OC.CHAIN: lambda r: OC.classify_aabb(np.ascontiguousarray(r[:, :12])),
             OC.AS_U8: OC.classify_as_u8}
_cache = {}


@pytest.fixture(scope="module")
def expected(oracle):
    """family -> (records, the oracle's words): computed on first use, shared by the units, never written to"""
    def get(family):
        if family not in _cache:
            rec = _records(family)
            want = oracle.operands_batch(family, rec, nthreads=ORACLE_THREADS)
            rec.setflags(write=False)
            want.setflags(write=False)
            _cache[family] = (rec, want)
        return _cache[family]
    return get


def _report(family, rec, got, want, bad, what):
    i = int(np.nonzero(bad)[0][0])
    one = np.ascontiguousarray(rec[i:i + 1])
    classes = OC.describe(_CLASSIFY[family](one), 0) if family in _CLASSIFY else ()
    return (f"{what}: {int(bad.sum())} of {len(rec)} records differ; first: record {i} = {one[0].tolist()} "
            f"(words {[hex(w) for w in one.view(np.uint32)[0]]}), classes {classes}, "
            f"device {[hex(w) for w in got[i]]}, oracle {[hex(w) for w in want[i]]}")


def _word_eq(a, b):
    """float words: equal bits, or NaN on both sides"""
    fa, fb = a.view(np.float32), b.view(np.float32)
    return (a == b) | (np.isnan(fa) & np.isnan(fb))


def _check(family, rec, got, want, bad, what):
    assert not bad.any(), _report(family, rec, got, want, bad, what)


@pytest.mark.parametrize("unit", list(UNITS))
@pytest.mark.parametrize("family", [OC.SPHERE, OC.SPHERE_NORM, OC.TRIANGLE], ids=["sphere", "sphere_norm", "triangle"])
def test_hit_and_t(dbg, expected, family, unit):
    rec, want = expected(family)
    got = run_unit(dbg, unit, family, rec)
    hit = want[:, 0] != 0
    assert int(hit.sum()) >= 1 << 16 and int((~hit).sum()) >= 1 << 16, "the records do not both hit and miss"
    _check(family, rec, got, want, got[:, 0] != want[:, 0], f"{unit} hit flag")
    _check(family, rec, got, want, hit & ~_word_eq(got[:, 1], want[:, 1]), f"{unit} t")
    if family == OC.SPHERE_NORM:                                      # Ray::new's direction: defined for every record
        for k in range(3):
            _check(family, rec, got, want, ~_word_eq(got[:, 2 + k], want[:, 2 + k]), f"{unit} normalised direction [{k}]")


def test_sphere_bits_are_the_same_in_every_unit(dbg, expected):
    """the units differ in flags and in the square root they use: the stored words (t of a miss included) do not"""
    for family in (OC.SPHERE, OC.SPHERE_NORM):
        rec, _ = expected(family)
        outs = [run_unit(dbg, u, family, rec) for u in UNITS]
        for u, o in zip(list(UNITS)[1:], outs[1:]):
            bad = ~np.all(_word_eq(o, outs[0]), axis=1)
            _check(family, rec, o, outs[0], bad, f"{u} against lin")


@pytest.mark.parametrize("unit", list(UNITS))
def test_both_box_tests(dbg, expected, unit):
    rec, want = expected(OC.AABB)
    got = run_unit(dbg, unit, OC.AABB, rec)
    c = OC.classify_aabb(rec)
    _check(OC.AABB, rec, got, want, got[:, 2] != want[:, 2], f"{unit} RayAux::finite")
    _check(OC.AABB, rec, got, want, got[:, 0] != want[:, 0], f"{unit} intersects_aabb")
    # a finite inverse direction and lo <= hi on every axis — and no NaN among the slab products (a NaN origin component): the
    # reference's `if x < y` min / max keep or drop that NaN by its operand position, fminf / fmaxf always drop it;
    # _operand_cases "NaN slab product" holds the counter-examples, compared on intersects_aabb only (above)
    claimed = (want[:, 2] != 0) & c["ordered"] & ~c["NaN slab product"]
    outside = (want[:, 2] != 0) & c["ordered"] & c["NaN slab product"]
    assert int(outside.sum()) >= OC.FLOOR and int((want[:, 0] == 0)[outside].sum()) >= OC.FLOOR
    assert int(claimed.sum()) >= 1 << 19 and int((want[:, 0] != 0)[claimed].sum()) >= 1 << 16
    _check(OC.AABB, rec, got, want, claimed & (got[:, 1] != want[:, 0]), f"{unit} intersects_aabb_finite")
    nd = len(OC.aabb_directed())
    assert int((got[:nd, 2] == 0).sum()) >= OC.FLOOR
    for k in OC.AABB_CLASSES:
        if k not in OC.AABB_ZERO_DIR:
            assert int(((got[:nd, 2] != 0) & c[k][:nd]).sum()) >= OC.FLOOR, k


@pytest.mark.parametrize("unit", list(UNITS))
def test_leaf_box_passing_implies_outer_box_passing(dbg, expected, unit):
    rec, want = expected(OC.CHAIN)
    got = run_unit(dbg, unit, OC.CHAIN, rec)
    _check(OC.CHAIN, rec, got, want, np.any(got != want, axis=1), f"{unit} chain")
    fin, leaf, outer = got[:, 2] != 0, got[:, 0] != 0, got[:, 1] != 0
    assert int((fin & leaf).sum()) >= 1 << 16, int((fin & leaf).sum())
    _check(OC.CHAIN, rec, got, want, fin & leaf & ~outer, f"{unit} monotonicity lemma of bvh_reaches")


@pytest.mark.parametrize("unit", list(UNITS))
def test_normalize_as_u8_and_rng(dbg, expected, unit):
    rec, want = expected(OC.NORMALIZE)
    got = run_unit(dbg, unit, OC.NORMALIZE, rec)
    ok = want[:, 3] != 0
    assert int(ok.sum()) >= 1 << 19 and int((~ok).sum()) >= OC.FLOOR
    _check(OC.NORMALIZE, rec, got, want, got[:, 3] != want[:, 3], f"{unit} try_normalize's boolean")
    _check(OC.NORMALIZE, rec, got, want, ~np.all(_word_eq(got, want), axis=1), f"{unit} normalised vectors")
    rec, want = expected(OC.AS_U8)
    got = run_unit(dbg, unit, OC.AS_U8, rec)
    assert len(np.unique(want)) == 256
    _check(OC.AS_U8, rec, got, want, got[:, 0] != want[:, 0], f"{unit} f32_as_u8")
    rec, want = expected(OC.RNG)
    assert len(rec) == 1 << 16
    got = run_unit(dbg, unit, OC.RNG, rec)
    _check(OC.RNG, rec, got, want, np.any(got != want, axis=1), f"{unit} seed_state and the draws")
