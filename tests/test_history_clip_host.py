"""The film history's clip off the GPU (rt_history.h step 5a): the product's per-pixel lines
(history_csrc/rt_history_math.h accumulate_pixel_clip, through the g++ harness tests/host/history_clip_host.cpp) equal the numpy
restatement (tests/_history_clip_np.py) bit for bit on the seeded synthetic frames of tests/_history_np.py, whole films and bands,
along four of test_history_host.py's camera paths, with and without normals, three widths of the box and both radii, and every
branch of the clip is taken; both outcomes of the clip occur in numbers; properties of the contract hold on the restatement; a
ghost is removed; the harness as a stand-alone program runs clean under the address and undefined-behaviour sanitizers.  Without the
feature every test here fails: there is no accumulate_pixel_clip and no tests/_history_clip_np.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _history_clip_np as cnp
import _history_np as hnp
from ray_tracer_s8_amd import _abi
from test_history_host import BRANCHES, BUILD, DEPS, GXX, PATHS, ROOT, SIZES, _camera, _new_state, film_of, sequence

SRC = ROOT / "tests" / "host" / "history_clip_host.cpp"
OUT = BUILD / "libhistory_clip_host.so"
f32 = np.float32
E = 4                                                # synthetic_frame's sample count
CLIP_BRANCHES = ("TAP_OUT", "TAP_IN", "SPREAD_ZERO", "SPREAD_POS", "LO", "HI", "INSIDE", "UNTOUCHED", "TOUCHED", "S1_ZERO", "S1_POS",
                 "S2_ZERO", "S2_POS")
CLIP_PATHS = ("identical", "half a pixel", "translated", "rotated")
CONSTS = ((0.4, 3.0, 0.05, 0.9), (0.05, 8.0, 0.1, None))
GAMMAS = (0.5, 1.0, 3.0)
RADII = (1, 2)


def load_lib():
    """The harness as a library, built if it is missing or older than its sources (tests/test_extreme_planes_host.py loads it too)."""
    BUILD.mkdir(exist_ok=True)
    deps = [SRC] + DEPS[1:]
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run([*GXX, "-fPIC", "-shared", "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    vp = C.c_void_p
    l.history_clip_frame_host.argtypes = [C.c_uint32, C.c_uint32, vp, C.c_uint32, C.POINTER(_abi.TileRequest), C.POINTER(_abi.Camera),
                                          C.POINTER(_abi.TileRequest), C.POINTER(_abi.Camera)] + [vp] * 6 + \
                                         [C.POINTER(vp), C.POINTER(vp), vp, vp, vp]
    l.history_clip_frame_host.restype = C.c_int
    assert l.history_clip_branch_count() == len(CLIP_BRANCHES) and l.history_clip_base_branch_count() == len(BRANCHES)
    return l


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def host_frame(lib, rq, pose, prev_rq, prev_pose, frame, prev, consts, gamma, radius, counts, clip_counts):
    """One frame through the harness: the next state as a dict of new arrays, "clip" among them."""
    R, W = frame["depth"].shape
    normals = consts[3] is not None
    nxt = _new_state(R, W)
    amount = np.full((R, W), np.nan, f32)
    fp = np.array([consts[0], consts[1], consts[2], consts[3] if normals else 0.0, gamma, E], f32)
    pack = lambda s: (C.c_void_p * 6)(*[s[n].ctypes.data if s.get(n) is not None else None for n in hnp.STATE])
    arr = [np.ascontiguousarray(frame[n]) for n in ("C", "M", "depth", "hits", "index")]
    nrm = np.ascontiguousarray(frame["normal"]) if normals else None
    cam, pcam = _camera(pose), _camera(prev_pose)
    rc = lib.history_clip_frame_host(W, R, fp.ctypes.data, radius, C.byref(rq), C.byref(cam) if cam else None,
                                     C.byref(prev_rq) if prev is not None else None, C.byref(pcam) if pcam else None,
                                     *[a.ctypes.data for a in arr], nrm.ctypes.data if normals else None,
                                     pack(prev if prev is not None else nxt), pack(nxt), amount.ctypes.data, counts.ctypes.data,
                                     clip_counts.ctypes.data)
    assert rc == 0
    if not normals:
        nxt["normal"] = None
    nxt["clip"] = amount
    return nxt


def _eq(got, want, what):
    for n in hnp.STATE + ("clip",):
        if want.get(n) is None:
            continue
        bad = np.argwhere(got[n].view(np.uint32) != want[n].view(np.uint32))
        assert len(bad) == 0, (what, n, len(bad), bad[:4].tolist(), got[n][tuple(bad[0])], want[n][tuple(bad[0])])


def restate(frames, consts, gamma, radius, debug=None):
    """The states of a path through the restatement; debug: a list that receives every frame's debug dict."""
    states, prev, last = [], None, None
    for rq, pose, frame in frames:
        cam = hnp.cameras(rq, pose, last[0] if last else None, last[1] if last else None)
        dbg = {}
        prev = cnp.accumulate(cam, frame, prev, *consts, clip=gamma, clip_radius=radius, samples=E, debug=dbg)
        states.append(prev)
        if debug is not None:
            debug.append(dbg)
        last = (rq, pose)
    return states


def _run(lib, frames, consts, gamma, radius, counts, clip_counts, what):
    want = restate(frames, consts, gamma, radius)
    prev, last = None, None
    for i, (rq, pose, frame) in enumerate(frames):
        prev = host_frame(lib, rq, pose, last[0] if last else None, last[1] if last else None, frame, prev, consts, gamma, radius,
                          counts, clip_counts)
        _eq(prev, want[i], (what, i))
        last = (rq, pose)


def _crafted(consts, seed=41):
    """Two frames of 70 x 9 under the "half a pixel" step that reach the clip's rare branches, none of which the library's own
    states of the synthetic frames reach: the second frame has a region of one colour (no spread, and rounding can leave
    B / n - mu mu just below 0) and a region of zeros; the state it reads is the caller's, with S1 far below the colour sums in
    places (the shift takes S1h' below 0) and S2 = 0 in places (the shift takes S2h' below 0)."""
    rq_of, R = film_of(70, 9, 3, False)
    frames = sequence(rq_of, R, PATHS["half a pixel"][:2], consts, seed)
    prev = hnp.accumulate(hnp.cameras(frames[0][0], frames[0][1]), frames[0][2], None, *consts)
    rng = np.random.default_rng(seed + 1)
    pick = rng.random((R, 70))
    prev["moments"][..., 0][pick < 0.2] *= f32(0.01)
    prev["moments"][..., 1][(pick >= 0.2) & (pick < 0.4)] = 0
    fr = dict(frames[1][2])
    fr["C"] = fr["C"].copy()
    fr["C"][:, 20:34] = np.array([0.3, 1.7, 0.1], f32)
    fr["C"][:, 40:50] = 0
    return frames[0], (frames[1][0], frames[1][1], fr), prev


def test_host_lines_equal_the_restatement_and_every_clip_branch_is_taken(lib):
    counts, clip_counts = np.zeros(len(BRANCHES), np.uint64), np.zeros(len(CLIP_BRANCHES), np.uint64)
    for W, H, div in SIZES:
        for band in ((False, True) if div >= 3 else (False,)):
            rq_of, R = film_of(W, H, div, band)
            for k, name in enumerate(CLIP_PATHS):
                for consts in CONSTS:
                    frames = sequence(rq_of, R, PATHS[name], consts, 1000 * W + 10 * k + band)
                    for gamma in GAMMAS:
                        for radius in RADII:
                            _run(lib, frames, consts, gamma, radius, counts, clip_counts, (W, H, band, name, consts, gamma, radius))
    synthetic = dict(zip(CLIP_BRANCHES, clip_counts.tolist()))
    for consts in CONSTS:
        for radius in RADII:
            (rq0, pose0, _), (rq1, pose1, frame), prev = _crafted(consts)
            want = cnp.accumulate(hnp.cameras(rq1, pose1, rq0, pose0), frame, prev, *consts, clip=1.0, clip_radius=radius, samples=E)
            _eq(host_frame(lib, rq1, pose1, rq0, pose0, frame, prev, consts, 1.0, radius, counts, clip_counts), want,
                ("crafted", consts, radius))
    never = [b for b, c in zip(CLIP_BRANCHES, clip_counts) if c == 0]
    assert not never, (never, dict(zip(CLIP_BRANCHES, clip_counts.tolist())), synthetic)


@pytest.mark.parametrize("W,H,div", [(70, 9, 3), (130, 70, 5)])
@pytest.mark.parametrize("radius", RADII)
def test_both_outcomes_of_the_clip_occur(W, H, div, radius):
    """At gamma = 1 under the "half a pixel" step, over the four frames: at least a tenth of the pixels with history are clipped and
    at least a tenth are not."""
    consts = CONSTS[1]
    rq_of, R = film_of(W, H, div, False)
    frames = sequence(rq_of, R, PATHS["half a pixel"], consts, 1000 * W + 10)
    debug = []
    restate(frames, consts, 1.0, radius, debug)
    has = sum(int(d["gathered"]["has"].sum()) for d in debug[1:])
    touched = sum(int((d["clipped"]["touched"] & d["gathered"]["has"]).sum()) for d in debug[1:])
    print(f"{W} x {H}, radius {radius}: {touched} of {has} pixels with history clipped")
    assert has > 300 and 0.1 * has <= touched <= 0.9 * has, (touched, has)


# ---- properties of the contract, on the restatement -------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32).tobytes()


def _frames(consts, name="half a pixel", W=70, H=9, div=3, seed=9):
    rq_of, R = film_of(W, H, div, False)
    return sequence(rq_of, R, PATHS[name], consts, seed)


@pytest.mark.parametrize("consts", CONSTS)
def test_without_clip_the_bytes_are_the_plain_historys(consts):
    frames = _frames(consts)
    prev, mine, last = None, None, None
    for rq, pose, frame in frames:
        cam = hnp.cameras(rq, pose, last[0] if last else None, last[1] if last else None)
        prev = hnp.accumulate(cam, frame, prev, *consts)
        mine = cnp.accumulate(cam, frame, mine, *consts, clip=None)
        assert "clip" not in mine
        for n in hnp.STATE:
            assert (prev[n] is None and mine[n] is None) or _bits(prev[n]) == _bits(mine[n]), n
        last = (rq, pose)


@pytest.mark.parametrize("radius", RADII)
def test_a_box_too_wide_to_clip_gives_the_unclipped_bytes_and_a_plane_of_zeros(radius):
    consts = CONSTS[0]
    frames = _frames(consts)
    plain = restate(frames, consts, None, radius)
    wide = restate(frames, consts, 1e30, radius)
    for a, b in zip(plain, wide):
        for n in hnp.STATE:
            assert _bits(a[n]) == _bits(b[n]), n
        assert _bits(b["clip"]) == _bits(np.zeros_like(b["clip"]))
    assert (wide[-1]["length"] > 1).sum() > 100


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("radius", RADII)
def test_clipped_colours_lie_in_the_box_and_untouched_pixels_keep_their_moments(gamma, radius):
    consts = CONSTS[1]
    debug = []
    restate(_frames(consts), consts, gamma, radius, debug)
    seen = 0
    for d in debug[1:]:
        g, c = d["gathered"], d["clipped"]
        t, u = g["has"] & c["touched"], g["has"] & ~c["touched"]
        assert ((c["Ch"][t] >= c["lo"][t]) & (c["Ch"][t] <= c["hi"][t])).all()
        assert _bits(c["Ch"][u]) == _bits(g["Ch"][u]) and _bits(c["S1h"][u]) == _bits(g["S1h"][u])
        assert _bits(c["S2h"][u]) == _bits(g["S2h"][u]) and not c["amount"][u].any()
        assert (c["amount"][t] > 0).all()
        seen += int(t.sum())
    assert seen > 0                                  # (not vacuous: at gamma = 3 few pixels are clipped)


@pytest.mark.parametrize("radius", RADII)
def test_touched_pixels_keep_their_spread_to_the_stated_roundings(radius):
    """rt_history.h step 5a "What the shift keeps": |(S2h' - S1h'^2 / e) - (S2h - S1h^2 / e)| <= 2^-23 S2h' + 2^-22 (S1h^2 + S1h'^2) / e
    wherever S2h' was not clamped; evaluated in float64, whose own roundings are 2^-29 of these."""
    consts = CONSTS[1]
    debug = []
    restate(_frames(consts, W=130, H=70, div=5), consts, 1.0, radius, debug)
    seen = 0
    for d in debug[1:]:
        g, c = d["gathered"], d["clipped"]
        t = g["has"] & c["touched"] & (c["S2h"] > 0)
        s1, s2, s1c, s2c = (a[t].astype(np.float64) for a in (g["S1h"], g["S2h"], c["S1h"], c["S2h"]))
        drift = np.abs((s2c - s1c * s1c / E) - (s2 - s1 * s1 / E))
        bound = 2.0 ** -23 * s2c + 2.0 ** -22 * (s1 * s1 + s1c * s1c) / E
        assert (drift <= bound).all(), float((drift / bound).max())
        seen += int(t.sum())
    assert seen > 1000


@pytest.mark.parametrize("radius", RADII)
def test_a_window_of_one_colour_pulls_any_history_to_it(radius):
    """The current frame is one colour everywhere, with sums that are exact (powers of two: k c and k c c are exact for k <= 25), so
    mu is the colour and the spread is 0: whatever the history held, the clipped history IS the colour, and the output b c + a c is
    within 1 ulp of it.  (With a colour whose sums round, B / n - mu mu is of the size of n roundings and the box of its square
    root: some 2^-10 of the colour wide, not 0.)"""
    consts = CONSTS[1]
    frames = _frames(consts, name="identical")
    colour = np.array([0.5, 2.0, 0.125], f32)                # powers of two: n colour and n colour^2 are exact for n <= 25
    (rq0, pose0, fr0), (rq1, pose1, fr1) = frames[:2]
    fr1 = dict(fr1)
    fr1["C"] = np.broadcast_to(colour, fr1["C"].shape).copy()
    prev = cnp.accumulate(hnp.cameras(rq0, pose0), fr0, None, *consts, clip=1.0, clip_radius=radius, samples=E)
    dbg = {}
    out = cnp.accumulate(hnp.cameras(rq1, pose1, rq0, pose0), fr1, prev, *consts, clip=1.0, clip_radius=radius, samples=E, debug=dbg)
    has = dbg["gathered"]["has"]
    assert has.sum() > 300
    # the sums are exact, so mu is the colour and the spread is 0: the clipped history IS the colour
    assert _bits(dbg["clipped"]["Ch"][has]) == _bits(np.broadcast_to(colour, fr1["C"].shape)[has])
    # ... and the blend b c + a c of it is within 1 ulp of c
    ulp = np.spacing(colour)
    assert (np.abs(out["accum"][has] - colour) <= ulp).all()
    # the history was something else
    assert (np.abs(dbg["gathered"]["Ch"][has] - colour) > 0.01).any()


# ---- the ghost ---------------------------------------------------------------------------------------------------------------------
GHOST_CONSTS = (0.05, 32.0, 0.1, None)
GHOST_LENGTH = 31.0


def ghost_frames(W=40, H=24):
    """Two frames under the reference camera with identical planes: every pixel hit, one primitive, a wall at distance 5 along
    every centre ray, one colour everywhere; frame 1 has a 6 x 6 patch 40 times as bright, frame 2 does not.  The colour sums are
    powers of two, so a bilinear mean of equal values is that value exactly and a pixel that no patch value reaches holds the
    colour to the bit, in the history and in the box."""
    rq = _abi.default_request(width=W, height=H, divisions=1, division_no=0, spp=E)
    hits = np.full((H, W), E, np.uint32)
    planes = dict(depth=(f32(5.0) * hits.astype(f32)).astype(f32), hits=hits, index=np.full((H, W), 3, np.uint32),
                  normal=np.zeros((H, W, 3), f32))
    patch = np.zeros((H, W), bool)
    patch[8:14, 15:21] = True
    frames = []
    for i in range(2):
        Cc = np.broadcast_to(np.array([1.0, 2.0, 0.5], f32), (H, W, 3)).copy()
        if i == 0:
            Cc[patch] *= f32(40.0)
        y = ((Cc[..., 0] + Cc[..., 1]) + Cc[..., 2]).astype(f32)
        M = np.stack([y, (y * y / f32(E)) * f32(1.1)], -1).astype(f32)
        frames.append((rq, None, dict(C=Cc, M=M, **planes)))
    return frames, patch


@pytest.mark.parametrize("radius", RADII)
def test_the_clip_removes_a_ghost(radius):
    """A still camera, identical planes, alpha = 0.05, and a history that is already long: the first frame's state with its length
    set to 31, as after many frames, so that the blend is at alpha.  Unclipped, the patch pixels keep more than 0.9 of the patch's
    excess; with gamma = 1 every patch pixel ends at or below its window's hi; pixels more than the radius away from the patch have
    the unclipped bytes (a pixel next to the patch differs: a pixel reprojects onto itself only up to the roundings of its ray, and
    the sliver of weight that goes to a neighbour brings some of the patch, which the clip removes)."""
    frames, patch = ghost_frames()
    (rq0, _, fr0), (rq1, _, fr1) = frames
    first = cnp.accumulate(hnp.cameras(rq0, None), fr0, None, *GHOST_CONSTS)
    first["length"][...] = GHOST_LENGTH
    cam = hnp.cameras(rq1, None, rq0, None)
    plain = cnp.accumulate(cam, fr1, first, *GHOST_CONSTS)
    dbg = {}
    clipped = cnp.accumulate(cam, fr1, first, *GHOST_CONSTS, clip=1.0, clip_radius=radius, samples=E, debug=dbg)
    assert dbg["gathered"]["has"].all()
    hi = cnp.box(fr1["C"], 1.0, radius)[1]
    assert _bits(hi) == _bits(dbg["clipped"]["hi"])
    assert_ghost(fr0["C"], fr1["C"], patch, plain, clipped, hi, radius)


def assert_ghost(first, second, patch, plain, clipped, hi, radius):
    """The three statements of the ghost test on a plain and a clipped state of the second frame (the GPU test's too)."""
    excess = first[patch].astype(np.float64) - second[patch]
    kept = (plain["accum"][patch] - second[patch]) / excess
    assert (kept > 0.9).all(), float(kept.min())
    assert (clipped["accum"][patch] <= hi[patch]).all()
    assert (clipped["clip"][patch] > 0).all()
    ys, xs = np.nonzero(patch)
    far = np.ones_like(patch)
    far[max(ys.min() - radius, 0):ys.max() + radius + 1, max(xs.min() - radius, 0):xs.max() + radius + 1] = False
    assert far.sum() > 100
    for n in ("accum", "moments", "length"):
        assert _bits(clipped[n][far]) == _bits(plain[n][far]), n
    assert not clipped["clip"][far].any()


# ---- the harness as a stand-alone program under the sanitizers ---------------------------------------------------------------------
def test_the_stand_alone_harness_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "history_clip_host"
    r = subprocess.run([*GXX, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DHISTORY_CLIP_HOST_MAIN",
                        "-o", str(exe), str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pixels blended" in r.stdout, r.stdout + r.stderr
