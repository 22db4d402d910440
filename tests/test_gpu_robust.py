"""The robust film on the GPU (ray_tracer_s8_amd/film_robust.py, robust_csrc/), whole tensors compared bit for bit
(NaN where NaN) with the restatement tests/_robust_np.py, and inputs read back unchanged:
1. rtr_fold with no scene: strips of 37 x 5 pixels (two full waves and a ragged third) and 67 x 9 (three blocks, the last ragged), the
   middle one of three strips in one (K, R, W, 3) tensor prefilled with a pattern, K in {3, 9, 15}, the calls (first, n) = (0, 1),
   (1, 2), (3, 20), (23, 4): after every call the whole tensor equals numpy's, so the other strips' rows and the buckets no sample
   fell into keep their bytes, and the end equals one call (0, 27);
2. rtr_resolve on 67 x 9 pixels: all seven K, three counts, "gini" and "trim" with c in {0, 1, h}, the corpora of the host test with
   the extreme tier; every output together, and each output alone into sentinel-filled tensors;
3. end to end on c2 at 64 x 36 in 3 strips, 20 samples in sub-ranges of 7 and passes (0, 5) and (5, 20), both integrators, K in {3, 9}:
   the buckets equal the numpy fold of the records a second tap cloned; the film's accum (and moments) equal those of a film with no
   tap; estimate() and state() equal the restatement on the buckets read back; preview() is the film's resolve of state(); reset()
   zeroes the buckets and the same passes give the same bytes; the refusals.
Every body runs in a child process that imports torch first.  Without the feature every test here fails: there is no rt.FilmRobust
and no librt_robust.so.  No timing is asserted."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

_PRELUDE = r"""
import sys
import numpy as np
import torch                                                      # first: the libraries then bind to torch's HIP runtime
sys.path.insert(0, "tests")
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, _robust_lib as rl, film_robust as fr, scenes
import _extreme_planes as xp
import _robust_np as rnp

f32 = np.float32
dev = torch.device("cuda", 0)

def refused(call, *a, **kw):
    try:
        call(*a, **kw)
    except ValueError:
        return True
    return False
"""


def _child(body, *args, timeout=600):
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body, *map(str, args)], capture_output=True, text=True, cwd=ROOT,
                       timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    return r.stdout


# ------------------------------------------------------------------------------------------- 1. the fold, no scene

_FOLD_CHILD = r"""
W, HS = (int(v) for v in sys.argv[1:3])
lib = rl.load()
stream = torch.cuda.Stream(device=dev)
P, R = W * HS, 3 * HS
CALLS = ((0, 1), (1, 2), (3, 20), (23, 4))
for K in (3, 9, 15):
    rec = rnp.records(100 + K, P, 27)
    rng = np.random.default_rng(K)
    start = rng.uniform(-4.0, 4.0, (K, R, W, 3)).astype(f32)        # the pattern; the middle strip starts from +0
    start[:, HS:2 * HS] = 0
    stride = R * W * 3

    def fold(t, first, n):
        # exactly the sub-range's records, pixel major, in a tensor of their own
        r = np.ascontiguousarray(rec[:, first:first + n])
        with torch.cuda.stream(stream):
            d = torch.from_numpy(r).to(dev)
            a = rl.FoldArgs(pixels=P, n=n, first=first, K=K, bucket_stride=stride, records=d.data_ptr(), buckets=t[0, HS:2 * HS].data_ptr())
            rl.check("rtr_fold", lib.rtr_fold(a, stream.cuda_stream))
        stream.synchronize()
        xp.identical(d.cpu().numpy(), r, ("the records", K, first, n))

    def np_fold(ref, first, n):
        mid = np.ascontiguousarray(ref[:, HS:2 * HS]).reshape(K, P, 3)
        rnp.fold(mid, rec[:, first:first + n], first)
        ref[:, HS:2 * HS] = mid.reshape(K, HS, W, 3)

    with torch.cuda.stream(stream):
        cut, whole = torch.from_numpy(start).to(dev), torch.from_numpy(start).to(dev)
    ref = start.copy()
    for first, n in CALLS:
        fold(cut, first, n)
        np_fold(ref, first, n)
        xp.identical(cut.cpu().numpy(), ref, ("after the call", K, first, n))
    fold(whole, 0, 27)
    xp.identical(whole.cpu().numpy(), ref, ("one call", K))
    one = start.copy()
    np_fold(one, 0, 27)
    xp.identical(one, ref, ("numpy, one call", K))
    assert (ref[:, :HS] == start[:, :HS]).all() and (ref[:, 2 * HS:] == start[:, 2 * HS:]).all()
    assert (ref[:, HS:2 * HS] != 0).any()
print("ok")
"""


@pytest.mark.parametrize("W,hs", [(37, 5), (67, 9)])
def test_the_fold_kernel(ndev, W, hs):
    _child(_FOLD_CHILD, W, hs)


# ------------------------------------------------------------------------------------------- 2. the resolve, no scene

_RESOLVE_CHILD = r"""
K = int(sys.argv[1])
W, R = 67, 9
N = W * R
lib = rl.load()
stream = torch.cuda.Stream(device=dev)
SHAPES = dict(linear=(R, W, 3), gini=(R, W), kept=(R, W), variance=(R, W), accum=(R, W, 3), moments=(R, W, 2))
SENTINEL = 7
calls = 0
for e in rnp.sample_counts(K):
    B, parts = rnp.corpus(K, e, N)
    with torch.cuda.stream(stream):
        d_B = torch.from_numpy(B).to(dev)
    for mode, c in rnp.widths(K):
        want = rnp.resolve(B, e, mode, c)
        for asked in (rnp.OUTPUTS,) + tuple((o,) for o in rnp.OUTPUTS):
            with torch.cuda.stream(stream):
                out = {o: torch.full(SHAPES[o], SENTINEL, dtype=torch.int32 if o == "kept" else torch.float32, device=dev)
                       for o in rnp.OUTPUTS}
                a = rl.ResolveArgs(W=W, R=R, K=K, samples=e, mode=mode, c=c, buckets=d_B.data_ptr(),
                                   **{"out_" + o: out[o].data_ptr() for o in asked})
                rl.check("rtr_resolve", lib.rtr_resolve(a, stream.cuda_stream))
            stream.synchronize()
            calls += 1
            for o in rnp.OUTPUTS:
                got = out[o].cpu().numpy()
                if o in asked:
                    xp.same(got, want[o].reshape(SHAPES[o]), (K, e, mode, c, asked, o))
                else:
                    assert (got == SENTINEL).all(), (K, e, mode, c, asked, o, "the sentinel")
    xp.identical(d_B.cpu().numpy(), B, ("the buckets", K, e))
assert calls == 3 * len(rnp.widths(K)) * 7
print("ok")
"""


@pytest.mark.parametrize("K", (3, 5, 7, 9, 11, 13, 15))
def test_the_resolve_kernel(ndev, K):
    _child(_RESOLVE_CHILD, K)


# ------------------------------------------------------------------------------------------- 3. end to end

_FILM_CHILD = r"""
INTEGRATOR, K = sys.argv[1], int(sys.argv[2])
MOMENTS = K == 9
W, H, DIV, SPP = 64, 36, 3, 20
HS = H // DIV
PASSES = ((0, 5), (5, 20))
sph, rq = scenes.config("c2")
strips = [rt.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=rq.max_bounces, seed=rq.seed)
          for k in range(DIV)]

class Clones:
    # a second tap: keeps a copy of every sub-range it is shown
    def __init__(self):
        self.seen = []
    def _on_records(self, i, b, e, records):
        self.seen.append((i, b, e, records.clone()))
    def _on_reset(self):
        self.seen.append("reset")

def host(film, t):
    film.sync()
    return t.cpu().numpy()

with rt.Scene(0, rt.World(sph)) as scene:
    kw = dict(integrator=INTEGRATOR, max_records=W * HS * 7, moments=MOMENTS)
    with rt.Film(scene, strips, **kw) as plain:
        for b, e in PASSES:
            plain.render_pass(b, e)
        accum0 = host(plain, plain.accum).copy()
        moments0 = host(plain, plain.moments).copy() if MOMENTS else None
    with rt.Film(scene, strips, **kw) as film, rt.FilmRobust(film, buckets=K) as robust:
        assert film._taps == [robust] and robust.buckets.shape == (K, H, W, 3) and robust.samples == 0
        clones = Clones()
        film._taps.append(clones)
        assert refused(robust.estimate) and refused(robust.state) and refused(robust.preview)              # no samples yet
        first = None
        for attempt in range(2):
            for b, e in PASSES:
                film.render_pass(b, e)
                assert robust.samples == film.samples == e
                if e < K:
                    assert refused(robust.estimate) and refused(robust.state)                               # samples < K
            # the tap saw every strip's sub-ranges of 7 samples, in order, and the buckets are their fold
            assert [(i, b, e) for i, b, e, _ in clones.seen] == \
                [(i, b, e) for lo, hi in PASSES for i in range(DIV) for b, e in ((0, 5), (5, 12), (12, 19), (19, 20)) if lo <= b < hi]
            ref = np.zeros((K, H, W, 3), f32)
            for i, b, e, t in clones.seen:
                r = host(film, t)
                assert r.shape == (W * HS, e - b, 3)
                mid = np.ascontiguousarray(ref[:, i * HS:(i + 1) * HS]).reshape(K, W * HS, 3)
                rnp.fold(mid, r, b)
                ref[:, i * HS:(i + 1) * HS] = mid.reshape(K, HS, W, 3)
            B = host(film, robust.buckets).copy()
            xp.identical(B, ref, "the buckets against the numpy fold of the records")
            # the film is what it is without a tap
            xp.identical(host(film, film.accum), accum0, "accum")
            if MOMENTS:
                xp.identical(host(film, film.moments), moments0, "moments")
            # the sum of the buckets is the film's sum up to the order of the adds: a loose sanity check of the layout
            assert np.allclose(B.sum(0), accum0, rtol=1e-4, atol=1e-4)
            if first is None:
                first = B
                film.reset()
                assert robust.samples == 0 and film.samples == 0 and clones.seen[-1] == "reset"
                assert not host(film, robust.buckets).any()
                clones.seen.clear()
            else:
                xp.identical(B, first, "the buckets after reset() and the same passes")
        # the estimate and the restated sums, against the restatement on the buckets read back
        want = rnp.resolve(B.reshape(K, H * W, 3), SPP, rnp.GINI, 0)
        out = robust.estimate(fr.OUTPUTS)
        for o in fr.OUTPUTS:
            xp.same(host(film, out[o]), want[o].reshape(out[o].shape), o)
        assert set(robust.estimate()) == {"linear"}
        acc, mom = robust.state()
        xp.same(host(film, acc), want["accum"].reshape(H, W, 3), "state: accum")
        xp.same(host(film, mom), want["moments"].reshape(H, W, 2), "state: moments")
        assert np.isfinite(want["linear"]).all() and (want["kept"] >= 1).all() and (want["kept"] <= K).all()
        # construction on a film that already holds samples
        assert refused(rt.FilmRobust, film, buckets=K)
        # preview() is the film's resolve of state()
        a = host(film, robust.preview()["rgb"]).copy()
        b = host(film, film.resolve(rt.DenoiseRequest.defaults(iterations=0), None, ("rgb",), _state=robust.state())["rgb"])
        assert a.dtype == np.uint8 and a.shape == (H, W, 3) and a.tobytes() == b.tobytes() and a.std() > 1.0
        lin = host(film, robust.resolve(rt.DenoiseRequest.defaults(iterations=0), None, ("linear",))["linear"])
        r = want["linear"].reshape(H, W, 3)
        assert (np.abs(lin - r) <= 2 * np.spacing(np.abs(r))).all()     # (r e_f) / e_f: two roundings, each within 2^-24 of r
        if MOMENTS:
            v = host(film, robust.variance())
            assert v.shape == (H, W) and np.isfinite(v).all() and (v >= 0).all()
            g = host(film, robust.resolve_guided(outputs=("rgb",))["rgb"])
            assert g.shape == (H, W, 3) and g.std() > 1.0
        else:
            assert refused(robust.variance) and refused(robust.resolve_guided)
        xp.identical(host(film, robust.buckets), B, "the buckets after the resolves")
        # a film advanced while the tap was removed
        film.reset()
        film.render_pass(0, K)
        film._taps.remove(robust)
        film.render_pass(K, K + 1)
        film._taps.insert(0, robust)
        assert robust.samples == K and film.samples == K + 1
        assert refused(robust.estimate) and refused(robust.state) and refused(robust.preview)
        film.reset()
        film.render_pass(0, K)
        assert not refused(robust.estimate)
        robust.close()
        assert robust not in film._taps and refused(robust.estimate)
        film.render_pass(K, K + 1)                                          # the film goes on without it
print("ok")
"""


@pytest.mark.parametrize("K", (3, 9))
@pytest.mark.parametrize("integrator", ("path", "nee"))
def test_a_film_with_a_robust_tap(ndev, integrator, K):
    _child(_FILM_CHILD, integrator, K)
