"""The film's host side without a GPU (ray_tracer_s8_amd/film.py):
1. sample_chunks covers [begin, end) exactly once, in order, no sub-range above max_records // pixels samples;
2. check_job refuses, with ValueError, what is not one request or the strips of one frame, an unknown integrator or mode, and a strip
   that does not fit max_records;
3. the module imports without torch, and Film is exported;
4. the fold on CPU tensors equals the numpy loop tot = (tot + v[:, j]).astype(float32) bit for bit, subnormals, signed zeros and mixed
   magnitudes included (in a child process: torch stays out of this one);
5. a Film constructed after the library bound its HIP runtime without torch raises _abi.check_single_hip_runtime's error.
Without the feature every test here fails: there is no ray_tracer_s8_amd.film."""
import subprocess
import sys
from pathlib import Path

import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

ROOT = Path(__file__).resolve().parent.parent


def _strips(n=3, first=0, **kw):
    base = dict(width=48, height=27, divisions=3, spp=5, max_bounces=6, seed=0xC0FFEE)
    base.update(kw)
    return [_abi.default_request(division_no=first + k, **base) for k in range(n)]


@pytest.mark.parametrize("pixels, begin, end, max_records", [
    (432, 0, 5, 432), (432, 0, 5, 863), (432, 0, 5, 864), (432, 2, 5, 432 * 2), (432, 0, 5, 432 * 5), (432, 0, 5, 1 << 22),
    (1, 0, 1, 1), (7, 3, 4, 7), (7, 0, 4096, 100), (256, 1, 4, 600), (5, 2, 2, 5)])
def test_sample_chunks_cover_the_range_once_in_order(pixels, begin, end, max_records):
    from ray_tracer_s8_amd import film
    chunks = film.sample_chunks(pixels, begin, end, max_records)
    k = max_records // pixels
    samples = [s for b, e in chunks for s in range(b, e)]
    assert samples == list(range(begin, end))
    assert all(0 < e - b <= k for b, e in chunks)
    assert all(pixels * (e - b) <= max_records for b, e in chunks)
    # no more sub-ranges than it takes
    assert len(chunks) == -(-(end - begin) // k)


def test_sample_chunks_edges():
    from ray_tracer_s8_amd import film
    assert film.sample_chunks(100, 0, 1, 100) == [(0, 1)]                       # one sample, max_records == pixels
    assert film.sample_chunks(100, 0, 3, 100) == [(0, 1), (1, 2), (2, 3)]
    assert film.sample_chunks(100, 0, 3, 199) == [(0, 1), (1, 2), (2, 3)]
    assert film.sample_chunks(100, 1, 4, 200) == [(1, 3), (3, 4)]
    with pytest.raises(ValueError):
        film.sample_chunks(101, 0, 1, 100)                                      # pixels > max_records
    with pytest.raises(ValueError):
        film.sample_chunks(100, 3, 2, 100)
    with pytest.raises(ValueError):
        film.sample_chunks(0, 0, 1, 100)


def test_check_job_accepts_one_request_and_the_strips_of_a_frame():
    from ray_tracer_s8_amd import film
    plan = film.check_job(_strips())
    assert (plan.hs, plan.width, plan.rows, plan.spp, plan.k) == (9, 48, 27, 5, 5)
    assert [r.division_no for r in plan.reqs] == [0, 1, 2]
    plan = film.check_job(_strips(2, first=1), "path", max_records=432 * 2)     # a part of the frame, k below spp
    assert (plan.rows, plan.k) == (18, 2) and [r.division_no for r in plan.reqs] == [1, 2]
    one = _strips()[1]
    plan = film.check_job(one, "nee", _abi.RT_NEE_LIGHT_ONLY, 432)
    assert (plan.rows, plan.k) == (9, 1)
    # the plan holds copies: the caller's request may change afterwards
    one.seed = 1
    assert plan.reqs[0].seed == 0xC0FFEE


def test_check_job_refuses_what_is_not_one_frame():
    from ray_tracer_s8_amd import film
    s = _strips()
    bad = {
        "descending": s[::-1],
        "non-consecutive": [s[0], s[2]],
        "repeated": [s[0], s[0]],
        "spp": [s[0], _strips(spp=6)[1]],
        "seed": [s[0], _strips(seed=1)[1]],
        "width": [s[0], _strips(width=47)[1]],
        "flags": [s[0], _strips(flags=_abi.RT_FLAG_NO_BVH_CULL)[1]],
        "max_bounces": [s[0], _strips(max_bounces=5)[1]],
        "beyond the frame": _strips(2, first=2),
        "empty": [],
        "not a request": [s[0], "strip"],
        "no rows": _strips(1, height=2),
    }
    for what, reqs in bad.items():
        with pytest.raises(ValueError):
            film.check_job(reqs)
            pytest.fail(what)
    for kw in (dict(integrator="bidir"), dict(integrator=None), dict(mode=2), dict(max_records=431), dict(max_records=0)):
        with pytest.raises(ValueError):
            film.check_job(s, **kw)
            pytest.fail(str(kw))
    # Film makes the same checks before it touches torch, the scene or the GPU
    for reqs, kw in ((s[::-1], {}), (s, dict(integrator="bidir")), (s, dict(max_records=431))):
        with pytest.raises(ValueError):
            rt.Film(None, reqs, **kw)


def test_module_imports_without_torch_and_film_is_exported():
    r = subprocess.run([sys.executable, "-c",
                        "import sys; import ray_tracer_s8_amd as rt; import ray_tracer_s8_amd.film as film; "
                        "assert 'torch' not in sys.modules; assert 'Film' in rt.__all__ and rt.Film is film.Film; print('ok')"],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "Film" in rt.__all__


_FOLD_CHILD = r"""
import numpy as np
import torch
from ray_tracer_s8_amd import film
rng = np.random.default_rng(0xF11)
P, K = 257, 7
tiny = np.float32(1e-45)
v = (rng.standard_normal((P, K, 3)) * 10.0 ** rng.integers(-12, 12, (P, K, 3))).astype(np.float32)
pick = rng.integers(0, 8, (P, K, 3))
v[pick == 0] = (rng.integers(-2000, 2000, (P, K, 3)).astype(np.float32) * tiny)[pick == 0]      # subnormals
v[pick == 1] = 0.0
v[pick == 2] = -0.0
v[0, :, :] = -0.0                                                                                # +0 + -0 ... stays +0
v[1, :, 0] = [1e30, 1.0, -1e30, 1e-30, 3.0, -3.0, tiny]                                          # the order shows
v[2, :, 0] = [3.4e38, 3.4e38, -3.4e38, 0, 0, 0, 0]                                               # overflow to inf, inf - x
assert (np.abs(v[pick == 0]) < 1.2e-38).all() and (v[pick == 0] != 0).any()
tot = np.zeros((P, 3), np.float32)
with np.errstate(all="ignore"):
    for j in range(K):
        tot = (tot + v[:, j]).astype(np.float32)
acc = torch.zeros((P, 3), dtype=torch.float32)
film.fold(acc, torch.from_numpy(v))
got = acc.numpy()
assert got.view(np.uint32).tobytes() == tot.view(np.uint32).tobytes(), np.argwhere(got.view(np.uint32) != tot.view(np.uint32))[:5]
# ... and it is the ORDER that is pinned: the reversed fold differs
rev = torch.zeros((P, 3), dtype=torch.float32)
film.fold(rev, torch.from_numpy(v[:, ::-1].copy()))
assert rev.numpy().view(np.uint32).tobytes() != tot.view(np.uint32).tobytes()
# cut into sub-ranges, the running sum carried: the same bytes
cut = torch.zeros((P, 3), dtype=torch.float32)
for b, e in film.sample_chunks(P, 0, K, 3 * P):
    film.fold(cut, torch.from_numpy(np.ascontiguousarray(v[:, b:e])))
assert cut.numpy().view(np.uint32).tobytes() == tot.view(np.uint32).tobytes()
# a strip's view of a frame-shaped accum, records as a view of a larger scratch: what render_pass hands over
frame = torch.zeros((3 * P, 1, 3), dtype=torch.float32)
scratch = torch.from_numpy(np.concatenate([v.reshape(-1, 3), np.ones((5, 3), np.float32)]))
film.fold(frame[P:2 * P].view(P, 3), scratch[:P * K].view(P, K, 3))
assert frame[P:2 * P].numpy().view(np.uint32).tobytes() == tot.view(np.uint32).tobytes()
assert not frame[:P].any() and not frame[2 * P:].any()
print("ok")
"""


def test_fold_equals_the_numpy_loop_bit_for_bit():
    r = subprocess.run([sys.executable, "-c", _FOLD_CHILD], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


_ORDER_CHILD = r"""
import sys
from ray_tracer_s8_amd import _abi, film
bound = _abi.hip_runtime_path()                     # the library is loaded and bound to a HIP runtime; torch is not imported yet
assert "torch" not in sys.modules
rq = _abi.default_request(width=16, height=8, divisions=2, spp=2)
try:
    film.Film(None, rq)                             # (the check comes before the scene is touched)
    print("ACCEPTED", bound)
except RuntimeError as e:
    print("REFUSED", "two HIP runtimes" in str(e), bound)
"""


def test_film_after_the_library_bound_its_runtime_raises_the_runtime_check():
    """tests/test_abi.py::test_two_hip_runtimes_in_one_process_are_refused, through Film: the error is check_single_hip_runtime's, raised
    before any HIP call."""
    r = subprocess.run([sys.executable, "-c", _ORDER_CHILD], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "REFUSED True" in r.stdout, r.stdout + r.stderr
