"""The device functions that sample a light or scatter a ray against their numpy restatement, operand by operand and bit for bit.

rt_debug_unit (test library; ray_tracer_s8_amd/csrc/rt_unit_sampling.hip.h) runs one lane per record through the lines of
csrc/rt_direct_math.h, csrc/rt_nee_math.h and the shade lines of csrc/rt_path_steps.hip.h, as the translation unit named compiles
them: `direct` and `nee` (pick_light, pick_light_power, the point on a sphere or a triangle light, light_geometry, the weights, the
cone sample; `nee` alone the two views of an emitter the bounce reached and the MIS weights), `bounce` and `trace` (unit_sphere_vec,
scattered_dir, sky_colour).  The records are the directed corpus of tests/_sampling_cases.py — every regime end, degenerate
distance, fold, pick and weight edge at least 64 times, tests/test_sampling_corpus.py — plus 2^20 seeded records; the expected words
are the numpy restatement's, which tests/test_sampling_corpus.py holds to the g++ build of the same lines, computed once per family
and shared by the units.  Every word is compared: counts as integers, flags as booleans, floats bit for bit with NaN matching NaN.
A failure prints the first offending record, the classes it belongs to, and both bit patterns."""
import ctypes as C

import numpy as np
import pytest

from ray_tracer_s8_amd import _abi

import _sampling_cases as S

pytestmark = pytest.mark.gpu

N_RANDOM = 1 << 20
PAIRS = [(unit, family) for unit in S.UNITS for family in S.CARRIES[unit]]


@pytest.fixture(scope="module")
def dbg(ndev):
    lib = _abi.load_debug()
    n = C.c_int(0)
    assert lib.rt_init(C.byref(n)) == 0 and n.value >= 1
    return lib


def run_unit(lib, unit, family, rec):
    rec = np.ascontiguousarray(rec)
    assert rec.dtype.itemsize == 4 and rec.shape[1] == S.WORDS[family][0]
    out = np.zeros((len(rec), S.WORDS[family][1]), np.uint32)
    rc = lib.rt_debug_unit(0, S.UNITS[unit], family, len(rec), rec.ctypes.data, out.ctypes.data)
    assert rc == 0, (rc, lib.rt_last_error().decode())
    return out


_cache = {}


def expected(family):
    """(records, the restatement's words): computed on first use, shared by the units, never written to"""
    if family not in _cache:
        rec = S.records(family, N_RANDOM)
        want = S.expected(family, rec)
        rec.setflags(write=False)
        want.setflags(write=False)
        _cache[family] = (rec, want)
    return _cache[family]


def _report(family, unit, rec, got, want, bad):
    i = int(np.nonzero(bad)[0][0])
    one = np.ascontiguousarray(rec[i:i + 1])
    nd = len(S.DIRECTED[family]())
    words = np.nonzero(~S.words_equal(family, got[i:i + 1], want[i:i + 1])[0])[0].tolist()
    return (f"{unit} {S.NAMES[family]}: {int(bad.sum())} of {len(rec)} records differ; first: record {i} "
            f"({'directed' if i < nd else 'seeded'}) = {one.view(np.float32)[0].tolist()} (words {[hex(w) for w in one[0]]}), "
            f"classes {S.describe(S.classify(family, one), 0)}, output words {words} differ: "
            f"device {[hex(w) for w in got[i]]}, restatement {[hex(w) for w in want[i]]}")


@pytest.mark.parametrize("unit,family", PAIRS, ids=[f"{u}-{S.NAMES[f]}" for u, f in PAIRS])
def test_device_words_equal_the_restatement(dbg, unit, family):
    rec, want = expected(family)
    got = run_unit(dbg, unit, family, rec)
    bad = ~S.words_equal(family, got, want).all(axis=1)
    assert not bad.any(), _report(family, unit, rec, got, want, bad)
    if family == S.CONE:
        # the bounds tests/test_cone_host.py derives, on the device's own words, for every record in the regime
        if "cone classes" not in _cache:
            _cache["cone classes"] = S.classify(S.CONE, rec, trace=False)
        n_reg, n_fac = S.cone_invariants(rec, got, _cache["cone classes"])
        assert n_reg >= (1 << 19) and n_fac >= (1 << 18), (n_reg, n_fac)


def test_a_pair_that_is_not_instantiated_is_refused_and_no_records_is_ok(dbg):
    one = {f: np.ascontiguousarray(S.DIRECTED[f]()[:1]) for f in S.NAMES}
    out = np.zeros(64, np.uint32)
    for unit, uid in S.UNITS.items():
        for family in S.NAMES:
            rec = one[family]
            if family in S.CARRIES[unit]:
                assert dbg.rt_debug_unit(0, uid, family, 0, rec.ctypes.data, out.ctypes.data) == _abi.RT_OK
                assert dbg.rt_debug_unit(0, uid, family, 0, None, None) == _abi.RT_OK
            else:
                out[:] = 0xdeadbeef
                assert dbg.rt_debug_unit(0, uid, family, 1, rec.ctypes.data, out.ctypes.data) == _abi.RT_ERR_BAD_ARG, (unit, family)
                assert dbg.rt_debug_unit(0, uid, family, 0, rec.ctypes.data, out.ctypes.data) == _abi.RT_ERR_BAD_ARG, (unit, family)
                assert (out == 0xdeadbeef).all()
        for family in range(8):                                        # the closest-hit families live in units 0 .. 2 only
            assert dbg.rt_debug_unit(0, uid, family, 1, one[S.SKY].ctypes.data, out.ctypes.data) == _abi.RT_ERR_BAD_ARG
    for uid in (0, 1, 2, 7, -1):                                           # ... and the sampling families in units 3 .. 6 only
        for family in list(S.NAMES) + [16, -1]:
            assert dbg.rt_debug_unit(0, uid, family, 1, one[S.SKY].ctypes.data, out.ctypes.data) == _abi.RT_ERR_BAD_ARG, (uid, family)
