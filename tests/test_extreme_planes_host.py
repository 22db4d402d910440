"""The film stage on extreme planes, off the GPU: the corpus of tests/_extreme_planes.py (subnormals and signed zeros;
values whose squares overflow; infinities, NaNs and negative sums; inconsistent integer planes) through the product's per-pixel lines
in the g++ harnesses of the denoiser, the guided resolve, the history, its clip and the upsampler, against the numpy restatements.
The rule: a float is NaN in one exactly where it is NaN in the other, every other float is bit-equal (signed zeros and infinities
too), uint8 and integer planes are equal.  A NaN's payload and sign are not compared: the headers do not promise them.

The same file holds the conditions on the inputs, checked on the restatements alone, so that the GPU tests
(tests/test_gpu_film_extremes.py), which run the same cases, inherit inputs known to be discriminating: at most half of the pixels
of a run have a NaN in any output; a non-finite case has a NaN and a finite pixel beside one; a small case has no NaN and at least
1 % subnormal output values; each library has a -0 and a +-inf among its outputs; every branch the harnesses count
(history, clip, upsample) is taken over the corpus.  The measured shares are printed (pytest -s) and recorded in DESIGN.md 4.28."""
import numpy as np
import pytest

import _denoise_np as dn
import _extreme_planes as xp
import _film_np as fnp
import _history_np as hnp
import _upsample_np as unp
import test_denoise_host as tdh
import test_film_guided_host as tfh
import test_history_clip_host as tch
import test_history_host as thh
import test_upsample_host as tuh
from ray_tracer_s8_amd import _abi

f32 = np.float32
TIERS = xp.TIERS


def floats(outs):
    return [a for a in outs if a is not None and a.dtype == np.float32]


def conditions(runs, library):
    """The input conditions over a library's runs [(tier, what, [output arrays])], each held run by run; prints the measured
    shares.  A run is one call (or one frame of a sequence): one set of planes, constants and iterations."""
    shares = {t: xp.Shares() for t in TIERS}
    worst, least = (0.0, None), (1.0, None)
    for tier, what, outs in runs:
        outs = floats(outs)
        shares[tier].add(outs)
        nan = xp.pixel_nan(outs)
        assert nan.mean() <= 0.5, (library, tier, what, "NaN pixels", float(nan.mean()))
        worst = max(worst, (float(nan.mean()), (tier,) + tuple(what)), key=lambda w: w[0])
        if tier == "nonfinite":
            assert nan.any() and xp.finite_beside_nan(nan), (library, tier, what, int(nan.sum()))
        if tier == "small":
            assert not nan.any(), (library, tier, what, int(nan.sum()))
            one = xp.Shares()
            one.add(outs)
            assert one.subnormal >= 0.01 * one.values, (library, tier, what, one.subnormal, one.values)
            least = min(least, (one.subnormal / one.values, tuple(what)), key=lambda w: w[0])
    for t in TIERS:
        print(shares[t].line(library, t))
    print(f"{library}: the largest NaN share of a run is {100 * worst[0]:.1f} % of its pixels, in {worst[1]}")
    print(f"{library}: the least subnormal share of a small run is {100 * least[0]:.1f} % of its values, in {least[1]}")
    # (a -0 somewhere in the library's cases: the upsampler's small tier cannot make one, its colours being non-negative there)
    assert sum(s.neg_zero for s in shares.values()) > 0, library
    assert sum(s.inf for s in shares.values()) > 0, library
    return shares


# ---- the denoiser --------------------------------------------------------------------------------------------------------------------
def dn_planes(planes, names):
    return dict(A=planes["A"] if "A" in names else None, N=planes["N"] if "N" in names else None,
                D=planes["D"] if "D" in names else None, hits=planes["hits"] if "hits" in names else None)


@pytest.fixture(scope="module")
def denoise_runs():
    """[(tier, case, what, planes, kw, want)]: every case of the corpus at 0, 1 and 3 iterations, restated once."""
    runs = []
    for tier in TIERS:
        for c, (name, names, planes) in enumerate(xp.denoise_cases(tier)):
            for kc, kn, kd in xp.denoise_consts(tier):
                for it in xp.SPARSE_ITERATIONS:
                    kw = dict(iterations=it, k=xp.K, k_color=kc, k_normal=kn, k_depth=kd, **dn_planes(planes, names))
                    want = dn.denoise(planes["C"], xp.E, **{k: f32(v) if k.startswith("k_") else v for k, v in kw.items()})
                    runs.append((tier, c, (name, names, kc, it), planes, kw, want))
    return runs


def test_denoiser_inputs_are_discriminating(denoise_runs):
    conditions([(t, w, [want[o] for o in ("linear", "f32")]) for t, c, w, _, _, want in denoise_runs], "denoiser")


@pytest.mark.parametrize("tier", TIERS)
def test_denoiser_lines_equal_the_restatement(denoise_runs, tier):
    lib = tdh.load_lib()
    n = 0
    for t, _, what, planes, kw, want in denoise_runs:
        if t != tier:
            continue
        got = tdh.host_denoise(lib, planes["C"], xp.E, **kw)
        for o in ("linear", "f32", "rgb"):
            xp.same(got[o], want[o], ("denoiser", tier, what, o))
        n += 1
    assert n >= 9


# ---- the guided resolve ----------------------------------------------------------------------------------------------------------------
FILM_OUTPUTS = ("linear", "f32", "rgb", "variance")


@pytest.fixture(scope="module")
def film_runs():
    runs = []
    for tier in TIERS:
        for c, (name, (normal, depth), planes) in enumerate(xp.film_cases(tier)):
            for sl, ve, kn, kd in xp.film_consts(tier):
                for it in xp.SPARSE_ITERATIONS:
                    kw = dict(iterations=it, sigma_l=sl, var_eps=ve, k_normal=kn, k_depth=kd, **tfh.planes_of(planes, normal, depth))
                    want = fnp.resolve(planes["C"], planes["M"], xp.E,
                                       **{k: f32(v) if k in ("sigma_l", "var_eps", "k_normal", "k_depth") else v for k, v in kw.items()})
                    runs.append((tier, c, (name, normal, depth, sl, it), planes, kw, want))
    return runs


def test_guided_resolve_inputs_are_discriminating(film_runs):
    conditions([(t, w, [want[o] for o in ("linear", "f32", "variance")]) for t, c, w, _, _, want in film_runs], "guided")


@pytest.mark.parametrize("tier", TIERS)
def test_guided_resolve_lines_equal_the_restatement(film_runs, tier):
    lib = tfh.load_lib()
    n = 0
    for t, _, what, planes, kw, want in film_runs:
        if t != tier:
            continue
        got = tfh.host_resolve(lib, planes["C"], planes["M"], xp.E, **kw)
        for o in FILM_OUTPUTS:
            xp.same(got[o], want[o], ("guided", tier, what, o))
        n += 1
    assert n >= 18


# ---- the history and its clip ----------------------------------------------------------------------------------------------------------
CLIP_GAMMAS, CLIP_RADII = (0.5, 3.0), (1, 2)
STATE_F32 = ("accum", "moments", "length", "depth", "normal")


def history_rq():
    W, H, div = xp.HISTORY_FILM
    return _abi.default_request(width=W, height=H, divisions=div, division_no=0, spp=xp.HISTORY_SAMPLES)


def history_sequences():
    """[(tier, what, consts, [(rq, pose, frame)])] of the corpus."""
    out = []
    for tier in TIERS:
        rq = history_rq()
        for name, path, consts, frames in xp.history_cases(tier, rq):
            out.append((tier, (name, path, consts), consts, [(rq, pose, fr) for pose, fr in frames]))
    return out


def callers_state(tier, consts):
    """A second frame against a state of the caller's making, as test_history_host's "zeroed lengths": the first frame's state with a
    fifth of its lengths 0 (those taps are skipped) and a fifth 7 (above every n_max here), under the "half a pixel" step; both frames
    carry the tier's specials on every plane."""
    rq = history_rq()
    frames = [c for c in xp.history_cases(tier, rq) if c[1] == "half a pixel" and c[2] == consts][-1][3]      # its "every plane" case
    (p0, f0), (p1, f1) = frames[:2]
    return rq, p0, f0, p1, f1


def state_outs(st):
    return [st[n] for n in STATE_F32 + ("clip",) if st.get(n) is not None]


@pytest.fixture(scope="module")
def history_runs():
    """[(tier, what, consts, frames, [the restatement's state after every frame])]"""
    return [(tier, what, consts, frames, thh.restate(frames, consts)) for tier, what, consts, frames in history_sequences()]


def test_history_inputs_are_discriminating(history_runs):
    conditions([(t, (w, i), state_outs(st)) for t, w, _, _, states in history_runs for i, st in enumerate(states)], "history")


def test_history_lines_equal_the_restatement_and_every_branch_is_taken(history_runs):
    lib = thh.load_lib()
    counts = np.zeros(len(thh.BRANCHES), np.uint64)
    for tier, what, consts, frames, want in history_runs:
        prev, last = None, None
        for i, (rq, pose, frame) in enumerate(frames):
            prev = thh.host_frame(lib, rq, pose, last[0] if last else None, last[1] if last else None, frame, prev, consts, counts)
            for n in hnp.STATE:
                if want[i][n] is not None:
                    xp.same(prev[n], want[i][n], ("history", tier, what, i, n))
            last = (rq, pose)
    for tier in TIERS:
        for consts in xp.HISTORY_CONSTS:
            rq, p0, f0, p1, f1 = callers_state(tier, consts)
            prev = hnp.accumulate(hnp.cameras(rq, p0), f0, None, *consts)
            pick = np.random.default_rng(32).random(prev["length"].shape)
            prev["length"][pick < 0.2] = 0
            prev["length"][pick > 0.8] = 7
            want = hnp.accumulate(hnp.cameras(rq, p1, rq, p0), f1, prev, *consts)
            got = thh.host_frame(lib, rq, p1, rq, p0, f1, prev, consts, counts)
            for n in hnp.STATE:
                if want[n] is not None:
                    xp.same(got[n], want[n], ("history, the caller's state", tier, consts, n))
    never = [b for b, c in zip(thh.BRANCHES, counts) if c == 0]
    assert not never, (never, dict(zip(thh.BRANCHES, counts.tolist())))


@pytest.fixture(scope="module")
def clip_runs():
    """[(tier, what, consts, gamma, radius, frames, [states])]"""
    runs = []
    for tier, what, consts, frames in history_sequences():
        for gamma in CLIP_GAMMAS:
            for radius in CLIP_RADII:
                runs.append((tier, what + (gamma, radius), consts, gamma, radius, frames, tch.restate(frames, consts, gamma, radius)))
    return runs


def test_clip_inputs_are_discriminating(clip_runs):
    conditions([(t, (w, i), state_outs(st)) for t, w, _, _, _, _, states in clip_runs for i, st in enumerate(states)], "clip")


def test_clip_lines_equal_the_restatement_and_every_branch_is_taken(clip_runs):
    lib = tch.load_lib()
    counts, clip_counts = np.zeros(len(thh.BRANCHES), np.uint64), np.zeros(len(tch.CLIP_BRANCHES), np.uint64)
    for tier, what, consts, gamma, radius, frames, want in clip_runs:
        prev, last = None, None
        for i, (rq, pose, frame) in enumerate(frames):
            prev = tch.host_frame(lib, rq, pose, last[0] if last else None, last[1] if last else None, frame, prev, consts, gamma,
                                  radius, counts, clip_counts)
            for n in hnp.STATE + ("clip",):
                if want[i].get(n) is not None:
                    xp.same(prev[n], want[i][n], ("clip", tier, what, i, n))
            last = (rq, pose)
    never = [b for b, c in zip(tch.CLIP_BRANCHES, clip_counts) if c == 0]
    assert not never, (never, dict(zip(tch.CLIP_BRANCHES, clip_counts.tolist())))


# ---- the upsampler ---------------------------------------------------------------------------------------------------------------------
UP_OUTPUTS = ("linear", "f32", "rgb", "cls")


@pytest.fixture(scope="module")
def upsample_runs():
    runs = []
    for tier in TIERS:
        for s in xp.UPSAMPLE_SCALES:
            for name, L, lo, hi, geom, kl, kh in xp.upsample_cases(tier, s):
                assert geom["y0l"] > 0
                for names in xp.UPSAMPLE_SETS:
                    if name not in names + ("every plane", "colour"):
                        continue                                   # (the case's special plane is not among the call's)
                    args = (L, unp.take(lo, names), unp.take(hi, names), geom)
                    want = unp.upsample(*args, unp.K_DEPTH, unp.K_NORMAL, unp.EPS, kl, kh)
                    runs.append((tier, (name, s, names), args, (kl, kh), want))
    return runs


def test_upsampler_inputs_are_discriminating(upsample_runs):
    conditions([(t, w, [want[o] for o in ("linear", "f32")]) for t, w, _, _, want in upsample_runs], "upsampler")


def test_upsampler_lines_equal_the_restatement_and_every_branch_is_taken(upsample_runs):
    lib = tuh.load_lib()
    total = dict.fromkeys(tuh.BRANCHES, 0)
    for tier, what, args, (kl, kh), want in upsample_runs:
        got = tuh.host(lib, *args, kl, kh)
        for o in UP_OUTPUTS:
            xp.same(got[o], want[o], ("upsampler", tier, what, o))
        assert got["counts"] == want["counts"], (tier, what, got["counts"], want["counts"])
        for b in tuh.BRANCHES:
            total[b] += got["counts"][b]
    assert all(total.values()), total


# ---- the corpus itself -----------------------------------------------------------------------------------------------------------------
def test_every_hits_plane_carries_every_special_and_every_index_plane_a_none():
    """In every tier, on every hits plane of every library, the low side of the upsampler's 33 x 7 film too: hits of 0, 1, 2^24,
    2^24 + 1 and 0xFFFFFFFF, a 0 among them under a depth that is not zero; RT_HIT_NONE on every index plane, under hits > 0
    somewhere.  And in the filters' non-finite tier every plane whose values reach the outputs takes each of its NaN-making values
    in some case of every plane set that has the plane."""
    def held(hits, depth=None, index=None, what=None):
        assert set(xp.HITS_SPECIALS) <= set(np.unique(hits).tolist()), (what, np.unique(hits)[-4:])
        if depth is not None:
            assert ((hits == 0) & (depth != 0)).any(), what
        if index is not None:
            assert ((index == xp.NONE) & (hits > 0)).any(), what
    for tier in TIERS:
        for name, names, planes in xp.denoise_cases(tier):
            held(planes["hits"], planes["D"], what=("denoiser", tier, name))
        for name, sub, planes in xp.film_cases(tier):
            held(planes["hits"], planes["D"], what=("guided", tier, name))
        for name, path, consts, frames in xp.history_cases(tier, history_rq()):
            for pose, fr in frames:
                held(fr["hits"], fr["depth"], fr["index"], ("history", tier, name))
        for s in xp.UPSAMPLE_SCALES:
            for name, L, lo, hi, geom, kl, kh in xp.upsample_cases(tier, s):
                held(lo["hits"], lo["depth"], what=("upsampler, low", tier, s, name))
                held(hi["hits"], hi["depth"], hi["index"], ("upsampler, high", tier, s, name))
                y, x = xp.lattice(*lo["index"].shape, xp.ORIGINS["index"], xp.INT_PITCH)[0]
                assert lo["index"][y, x] == xp.NONE
    bits_of = lambda a: set(np.ascontiguousarray(a, f32).view(np.uint32).ravel().tolist())
    for cases, key, planes_of in ((xp.denoise_cases, dict(colour="C", albedo="A"), lambda names: ("C",) + tuple(n for n in names if n == "A")),
                                  (xp.film_cases, dict(colour="C", moments="M"), lambda sub: ("C", "M"))):
        seen = {}
        for name, sub, planes in cases("nonfinite"):
            for p in planes_of(sub):
                seen.setdefault((sub, p), set()).update(bits_of(planes[p]))
        for (sub, p), bits in seen.items():
            role = {v: k for k, v in key.items()}[p]
            zero = f32(-(xp.DENOISE_EPS * f32(xp.K))) if role == "albedo" else None
            want = bits_of(xp.makers(xp.values("nonfinite", role, zero)))
            assert want <= bits, (sub, p, [hex(b) for b in want - bits])
