"""The lobe arithmetic of the light samples at glossy hits on the device against its numpy restatement, operand by operand and bit for
bit.  rt_debug_unit (test library; family 16 of ray_tracer_s8_amd/csrc/rt_unit_sampling.hip.h, carried by the unit `nee`) runs one lane
per record through sampled_class, glossy_dir, lobe_of, lobe_factor, lobe_sample_taken and lobe_factor_scatter of csrc/rt_lobe_math.h as the translation
unit of the integrator compiles them.  The records are the directed corpus of tests/_lobe_cases.py — roughness at 2^-24, 0.5 and
1 - 2^-24, gn at 0 and 1, w on the rim to the ulp on both sides of D = 0, b <= 0, a non-unit d, NaN and inf, every class at least 16
times (tests/test_lobe_host.py) — plus 2^20 seeded records; the expected words are the restatement's, which tests/test_lobe_host.py
holds to the g++ build of the same lines."""
import ctypes as C

import numpy as np
import pytest

from ray_tracer_s8_amd import _abi

import _lobe_cases as LC

pytestmark = pytest.mark.gpu

N_RANDOM = 1 << 20


@pytest.fixture(scope="module")
def dbg(ndev):
    lib = _abi.load_debug()
    n = C.c_int(0)
    assert lib.rt_init(C.byref(n)) == 0 and n.value >= 1
    return lib


def test_device_words_equal_the_restatement(dbg):
    rec = LC.records(N_RANDOM)
    want = LC.expected(rec)
    got = np.zeros((len(rec), LC.WORDS[1]), np.uint32)
    rc = dbg.rt_debug_unit(0, LC.UNIT_NEE, LC.LOBE, len(rec), rec.ctypes.data, got.ctypes.data)
    assert rc == 0, (rc, dbg.rt_last_error().decode())
    ok = LC.words_equal(got, want)
    bad = ~ok.all(1)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        cls = [k for k, v in LC.classify(rec[i:i + 1], want[i:i + 1]).items() if v[0]]
        raise AssertionError(f"{int(bad.sum())} of {len(rec)} records differ; first: record {i} = {rec[i].tolist()}, classes {cls}, output words "
                             f"{np.nonzero(~ok[i])[0].tolist()} differ: device {[hex(w) for w in got[i]]}, restatement {[hex(w) for w in want[i]]}")
    m = LC.classify(rec, want)
    assert m["in lobe"].sum() > (1 << 16) and m["class lobe"].sum() > (1 << 18)


def test_other_units_refuse_the_family(dbg):
    one = np.ascontiguousarray(LC.directed()[:1])
    out = np.full(64, 0xdeadbeef, np.uint32)
    for uid in (0, 1, 2, 3, 5, 6, 7):
        assert dbg.rt_debug_unit(0, uid, LC.LOBE, 1, one.ctypes.data, out.ctypes.data) == _abi.RT_ERR_BAD_ARG, uid
    assert (out == 0xdeadbeef).all()
    assert dbg.rt_debug_unit(0, LC.UNIT_NEE, LC.LOBE, 0, None, None) == _abi.RT_OK
    assert dbg.rt_debug_unit(0, LC.UNIT_NEE, 17, 1, one.ctypes.data, out.ctypes.data) == _abi.RT_ERR_BAD_ARG
