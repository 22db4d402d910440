"""Every launch-path knob must render the oracle's bytes (the output is a function of scene and request only).

The sample-unit scheduler of csrc/rt_kernel.hip.h — slots, out-of-order commits, the queue of whole tiles and parts, the refill
threshold, output staging — has free parameters, the process-level knobs of csrc/rt_api.hip (DebugKnob).  The other GPU tests run
each scheduler branch only at the value the host rule picks for their shape; here every knob is set away from the rule, on frames
of a few hundred pixels chosen so that each branch is reached (tests/_knob_matrix.py: the requests, the settings, and what each
reaches; tests/test_launch_plan.py checks the same tuples' plans on the CPU).  Every comparison is a bit comparison.

The knob values and why a wave always progresses under them (nothing outside the kernel's domain is ever launched)
------------------------------------------------------------------------------------------------------------------------------
RT_SLOTS.  plan_launch takes 1 ... SLOTS_MAX (more: SLOTS_MAX; <= 0: the host rule), so 1 is the smallest value there is, and one
slot is enough.  A lane without a unit takes the next unit of the issue tile; units of a slot that is open come from that slot
(cur_slot), a unit that starts a slot needs a free one.  The step takes min(want, units left in the tile, slot_room) units, where
slot_room = (k_open + n_free) U - tile_u counts the units the open slot and the free slots still hold.  With no free slot and
the open slot fully issued slot_room is 0: the step takes nothing and the acquisition loop is left (`stall`).  The slots in use
then hold only units that lanes are tracing; a path ends after at most max_bounces + 1 segments and its lane deposits the colour
and decrements the slot's counter, so some slot's counter reaches 0 after finitely many rounds: the slot is complete.  The commit
test is n_complete >= commit_slots, or n_complete != 0 and (popcount(freem) < 2 or issue_over): with every slot in use popcount(freem)
is 0, so the first complete slot is committed and freed whatever commit_slots says, and the next acquisition has slot_room >= U.
At n_slots = 1 that reads: the wave traces one slot's units (at least 8), commits it, and opens it again.  A wave leaves the loop
when no lane is active, every slot is free and nothing is left to issue; a slot that is not free is open or in flight, so it
completes and is committed (issue_over commits whatever is complete once the queue is drained).
RT_COMMIT_SLOTS is min-ed with n_slots by plan_launch; the disjunction above makes any value >= 1 safe.
RT_TAIL_TILES is min-ed with the launch's tiles by plan_queue.
RT_REFILL_EIGHTHS 1 ... 8: the walk loop is left when no lane walks, or when walking * 8 <= live * eighths and walking < live; a
walking lane steps in every round of the loop, so the loop ends for every value, and 8 means "as soon as one lane has finished".
RT_NO_STAGE, RT_COMPACT, RT_STRIP_COST, RT_LDS_TREE, RT_CULL_WALK, RT_REORDER choose between code paths that other tests run.
"""
import contextlib

import numpy as np
import pytest

import _denoise_np as dn
import _knob_matrix as M
import ray_tracer_s8_amd as rt
from _ray_cases import pile_world
from ray_tracer_s8_amd import _abi, scenes
from test_denoise_host import synthetic
from test_gpu_progressive import ENGINES, _expected_engine, _run_passes, _world

pytestmark = pytest.mark.gpu

T, E = _abi.RT_FLAG_BVH_TRAVERSE, _abi.RT_FLAG_EXACT_NODES


@contextlib.contextmanager
def knobs(values):
    """Set launch-path knobs of the TEST library (inside `with _abi.debug_library()`) and restore the previous values on exit."""
    prev = {}
    try:
        for name, v in values.items():
            prev[name] = _abi.debug_set(name, v)
        yield
    finally:
        for name, v in prev.items():
            _abi.debug_set(name, v)


def _requests(w, h, spp, flags):
    return [_abi.default_request(width=w, height=h, divisions=M.DIVISIONS, division_no=k, spp=spp, max_bounces=M.MAX_BOUNCES,
                                 seed=M.SEED, flags=flags) for k in range(M.DIVISIONS)]


def _backend(flags):
    return 0 if (flags & _abi.RT_FLAG_NO_BVH_CULL) else 1            # (as tests/test_gpu_parity.py _compare)


@pytest.fixture(scope="module")
def references(oracle):
    """want(scene name, spheres, triangles, world_index, request) -> the oracle's (rgb, f32, ray segments) of the strip, computed
    once per (scene, request) for the whole module; the arrays are handed out read-only."""
    cache = {}

    def want(name, world, rq):
        key = (name, rq.width, rq.height, rq.divisions, rq.division_no, rq.spp, rq.max_bounces, rq.seed, _backend(rq.flags))
        if key not in cache:
            sph = world.spheres if len(world.spheres) else None
            tri = world.triangles if len(world.triangles) else None
            rgb, f32, info = oracle.render(rq, sph, tri, backend=key[-1], want_f32=True, world_index=world.world_index)
            rgb.setflags(write=False)
            f32.setflags(write=False)
            cache[key] = (rgb, f32, info["ray_segments"])
        return cache[key]

    return want


def _bits(a):
    return np.asarray(a).view(np.uint32)


class _Check:
    """Collects every failing (engine, request, setting) of a test, so that one GPU run names them all."""

    def __init__(self, engine):
        self.engine, self.bad, self.n = engine, [], 0

    def __call__(self, ok, rq_name, setting, what):
        self.n += 1
        if not ok:
            self.bad.append((self.engine, rq_name, setting, what))

    def done(self):
        assert not self.bad, f"{len(self.bad)} of {self.n} checks failed: {self.bad[:40]}"


def _render_frame_and_strip(sc, reqs, name, world, want, engine, rq_name, setting, check, base):
    """The frame's strips in one batched launch and strip 1 alone, against the oracle and the default-knob f32 (`base`, filled by
    the first call).  Returns nothing; failures go to `check`."""
    hs, w, spp = reqs[0].height // reqs[0].divisions, reqs[0].width, reqs[0].spp
    outs, outf, st = sc.render_tiles(reqs, want_f32=True)
    rgb1, f1, st1 = sc.render_tile(reqs[1], want_f32=True)
    refs = [want(name, world, r) for r in reqs]
    for k, (o, f) in enumerate(zip(outs, outf)):
        check(np.array_equal(o, refs[k][0]), rq_name, setting, f"batched strip {k}: {int((o != refs[k][0]).sum())} RGB8 bytes differ")
    check(np.array_equal(rgb1, refs[1][0]), rq_name, setting, f"strip 1 alone: {int((rgb1 != refs[1][0]).sum())} RGB8 bytes differ")
    key = (rq_name,)
    if key not in base:                                           # the default knobs: also the oracle's f32, bit for bit
        base[key] = ([f.copy() for f in outf], f1.copy())
        for k, f in enumerate(outf):
            check(np.array_equal(_bits(f), _bits(refs[k][1])), rq_name, setting, f"batched strip {k}: f32 differs from the oracle's")
    bf, b1 = base[key]
    for k, f in enumerate(outf):
        check(np.array_equal(_bits(f), _bits(bf[k])), rq_name, setting, f"batched strip {k}: f32 differs from the default knobs'")
    check(np.array_equal(_bits(f1), _bits(b1)), rq_name, setting, "strip 1 alone: f32 differs from the default knobs'")
    check(np.array_equal(_bits(f1), _bits(outf[1])), rq_name, setting, "strip 1 alone differs from strip 1 of the batch")
    check(st.ray_segments == sum(r[2] for r in refs) and st1.ray_segments == refs[1][2], rq_name, setting,
          f"ray segments {st.ray_segments}, {st1.ray_segments}")
    check(st.primary_rays == len(reqs) * hs * w * spp and st1.primary_rays == hs * w * spp, rq_name, setting, "primary rays")
    check(st.n_launches == 1 and st1.n_launches == 1, rq_name, setting, f"launches {st.n_launches}, {st1.n_launches}")
    want_engine = st.engine if engine is None else _expected_engine(engine, st.engine)       # (None: whatever the flags give)
    check(st.engine == want_engine == st1.engine, rq_name, setting, f"engine {st.engine}, {st1.engine}")


def _engine_row(key):
    engine = int(str(key)[0])
    scene, flags = ENGINES[engine]
    return engine, scene, flags, (M.CAPPED if isinstance(key, str) else {})


@pytest.mark.parametrize("key", M.ENGINE_KEYS, ids=[f"engine{k}" for k in M.ENGINE_KEYS])
def test_every_setting_renders_the_oracles_bytes(ndev, references, key):
    """Engine x request x setting (tests/_knob_matrix.py): both strips of the frame in one launch and strip 1 alone; the progressive
    job in three passes; then the same scene built with RT_REORDER=0 (its records in the caller's order) under the default knobs.
    Whole-tile queue entries (RT_TAIL_TILES 0 and 1), slot counts away from the host rule and the capped-stack kernels included."""
    engine, name, flags, capped = _engine_row(key)
    world = _world(name)
    check = _Check(key)
    pw, ph, pspp, passes = M.PASS_JOB
    prq = _requests(pw, ph, pspp, flags)[1]
    with _abi.debug_library():
        rt.init()
        with knobs(capped):
            base, acc0 = {}, None
            with rt.Scene(0, world) as sc:
                for setting in M.settings_for(key):
                    with knobs(M.SETTINGS[setting][0]):
                        for rq_name, (w, h, spp, _, _) in M.REQUESTS.items():
                            _render_frame_and_strip(sc, _requests(w, h, spp, flags), name, world, references, engine, rq_name, setting,
                                                    check, base)
                        rgb, f32, acc, segs, st = _run_passes(sc, prq, passes)
                    ref = references(name, world, prq)
                    if acc0 is None:
                        acc0, f0 = acc.copy(), f32.copy()
                        check(np.array_equal(_bits(f32), _bits(ref[1])), "passes", setting, "f32 differs from the oracle's")
                    check(np.array_equal(rgb, ref[0]), "passes", setting, f"{int((rgb != ref[0]).sum())} RGB8 bytes differ")
                    check(np.array_equal(_bits(acc), _bits(acc0)), "passes", setting, "accum differs from the default knobs'")
                    check(np.array_equal(_bits(f32), _bits(f0)), "passes", setting, "f32 differs from the default knobs'")
                    check(segs == ref[2] and st.engine == _expected_engine(engine, st.engine), "passes", setting, f"segments {segs}")
            if len(world.spheres) + len(world.triangles) >= 64:       # (REORDER_MIN_PRIMS: below it the records are never reordered)
                with knobs({"RT_REORDER": 0}):                        # read when the scene is created
                    with rt.Scene(0, world) as sc:
                        for rq_name, (w, h, spp, _, _) in M.REQUESTS.items():
                            _render_frame_and_strip(sc, _requests(w, h, spp, flags), name, world, references, engine, rq_name,
                                                    "reorder_0", check, base)
    check.done()


def _tie_world(permuted):
    """A 128-sphere cut of the pile of test_gpu_ray_fuzz.test_thousands_of_coincident_spheres: 63 copies of one sphere, 64 of
    another and the ground.  Every hit on a pile is an exact distance tie; the first leaf in depth-first order wins."""
    p = pile_world()
    sph = np.concatenate([p[:63], p[2000:2064], p[4000:]])
    assert len(sph) == 128
    wi = np.random.default_rng(6).permutation(len(sph)).astype(np.uint32) if permuted else None
    return rt.World(sph, None, wi)


@pytest.mark.parametrize("permuted", [False, True])
def test_reorder_knob_keeps_the_tie_rule(ndev, references, permuted):
    """RT_REORDER stores the records of a scene of 64 primitives and more in the tree's leaf order; the winner of an exact distance
    tie must not depend on it, in the caller's order and in a permuted world, through every engine such a scene can take."""
    world = _tie_world(permuted)
    name = f"ties{int(permuted)}"
    check = _Check(name)
    rows = {e: ENGINES[e][1] for e in (0, 2, 3, 4, 5, 7)}             # (128 spheres: no streamed scan, no triangles)
    with _abi.debug_library():
        rt.init()
        for reorder in (1, 0):
            with knobs({"RT_REORDER": reorder}):
                sc = rt.Scene(0, world)
            with sc:
                for engine, flags in rows.items():
                    base = {}
                    for rq_name in ("150x6x1", "70x6x3"):
                        w, h, spp, _, _ = M.REQUESTS[rq_name]
                        reqs = _requests(w, h, spp, flags)
                        # (no engine asserted: the ground sphere may keep the pile out of the culled or the quantised walk)
                        _render_frame_and_strip(sc, reqs, name, world, references, None, rq_name, f"reorder_{reorder} engine {engine}",
                                                check, base)
    piles = references(name, world, _requests(70, 6, 3, 0)[1])[0]
    assert piles.std() > 1.0                                          # (the piles are in the picture)
    check.done()


def test_engine_knobs_choose_the_engine_and_keep_the_bytes(ndev, references):
    """RT_LDS_TREE and RT_CULL_WALK on requests without engine flags (rand1024, whose tree fits LDS): the engine moves exactly as a
    request flag would move it (plan_launch: RT_LDS_TREE=0 is RT_FLAG_NO_LDS_TREE for the process, RT_CULL_WALK=0 / 1 is
    RT_FLAG_NO_CULL_WALK / RT_FLAG_CULL_WALK), an explicit cull flag still wins over the knob (cull_wanted), the bytes stay."""
    world = _world("rand1024")
    check = _Check("rand1024")
    NOLT, CW, NCW = _abi.RT_FLAG_NO_LDS_TREE, _abi.RT_FLAG_CULL_WALK, _abi.RT_FLAG_NO_CULL_WALK
    w, h, spp, _, _ = M.REQUESTS["70x6x3"]
    want = [references("rand1024", world, r) for r in _requests(w, h, spp, 0)]

    def engine_of(sc, flags, what):
        outs, outf, st = sc.render_tiles(_requests(w, h, spp, flags), want_f32=True)
        for k in range(M.DIVISIONS):
            check(np.array_equal(outs[k], want[k][0]) and np.array_equal(_bits(outf[k]), _bits(want[k][1])), "70x6x3", what,
                  f"strip {k} differs from the oracle")
        check(st.ray_segments == sum(r[2] for r in want), "70x6x3", what, "ray segments")
        return int(st.engine)

    with _abi.debug_library():
        rt.init()
        with rt.Scene(0, world) as sc:
            by_flag = {f: engine_of(sc, f, f"flags {f:#x}") for f in (0, NOLT, CW, NCW, NOLT | CW, NOLT | NCW, T | E, T | E | NOLT)}
            assert by_flag[0] in (4, 7) and by_flag[CW] == 7 and by_flag[NCW] == 4           # the LDS-resident tree, plain or culled
            assert by_flag[NOLT] in (2, 3, 5) and by_flag[T | E | NOLT] == 2 and by_flag[T | E] in (4, 7)
            with knobs({"RT_LDS_TREE": 0}):
                assert engine_of(sc, 0, "RT_LDS_TREE=0") == by_flag[NOLT]
                assert engine_of(sc, T | E, "RT_LDS_TREE=0, exact nodes") == 2
                assert engine_of(sc, CW, "RT_LDS_TREE=0, cull flag") == by_flag[NOLT | CW]
                assert engine_of(sc, NCW, "RT_LDS_TREE=0, no-cull flag") == by_flag[NOLT | NCW]
            for knob, flag, other in ((0, NCW, CW), (1, CW, NCW)):
                with knobs({"RT_CULL_WALK": knob}):
                    assert engine_of(sc, 0, f"RT_CULL_WALK={knob}") == by_flag[flag] == (7 if knob else 4)
                    assert engine_of(sc, other, f"RT_CULL_WALK={knob} against the flag") == by_flag[other]     # the flag wins
                    assert engine_of(sc, flag, f"RT_CULL_WALK={knob} with the flag") == by_flag[flag]
                    with knobs({"RT_LDS_TREE": 0}):
                        assert engine_of(sc, other, f"RT_CULL_WALK={knob}, RT_LDS_TREE=0 against the flag") == by_flag[NOLT | other]
                        assert engine_of(sc, 0, f"RT_CULL_WALK={knob}, RT_LDS_TREE=0") == by_flag[NOLT | flag]
    check.done()


def test_frame_context_without_strip_costs_keeps_the_snake(ndev, oracle):
    """RT_STRIP_COST=0: the kernels count nothing, so a frame leaves no measurement behind.  All-zero costs used to count as one
    (cost_valid), and longest-first over them put every strip on entry 0: every frame after the first ran on one of the eight
    entries.  Now each frame is a snake frame (assignment 1) and every entry renders."""
    sph, rq = scenes.config("c3")
    rq.width, rq.height, rq.divisions, rq.spp = 320, 256, 32, 4        # (the request of the balance test, tests/test_gpu_parity.py)
    one = rq.copy()
    one.divisions = 1
    want, _, info = oracle.render(one, sph, backend=1)
    seen = []
    with _abi.debug_library():
        rt.init()
        with knobs({"RT_STRIP_COST": 0}):
            with rt.FrameContext(devices=[0] * 8, world=rt.World(sph)) as fc:
                for frame in range(3):
                    img, fs = fc.render(rq)
                    per = list(fs.entry_segments)[:8]
                    seen.append((int(fs.assignment), per, bool(np.array_equal(img.reshape(-1), want)), int(fs.totals.ray_segments)))
    for frame, (assignment, per, same, segs) in enumerate(seen):
        assert assignment == 1, (frame, seen)
        assert all(s > 0 for s in per) and sum(per) == segs == info["ray_segments"], (frame, per)
        assert same, frame


# ---------------------------------------------------------------------------------------------------- the denoiser's split

DN_PLANES = {"albedo": "A", "normal": "N", "depth": "D", "hits": "hits"}


@pytest.mark.parametrize("R,W,n", [(12, 67, 4), (40, 129, 2)])
@pytest.mark.parametrize("names", [(), tuple(DN_PLANES)], ids=["plain", "guided"])
def test_denoiser_split_between_lds_and_l2(ndev, R, W, n, names):
    """RT_DENOISE_LDS_STEP moves iterations between the LDS-window kernel and the L2-gather kernel; five iterations (steps 1 ... 16)
    with the largest LDS step at 0 (all through L2), 1, 4, 8 and 16: bit for bit tests/_denoise_np.py whatever the split.  (The
    plans of these values: tests/test_denoise_host.py.)"""
    rng = np.random.default_rng(R * 7919 + W * 31 + n + len(names))
    s = synthetic(rng, R, W)
    dq = _abi.DenoiseRequest.defaults(iterations=5)
    f32 = np.float32
    want = dn.denoise(s["C"], 8, k=4, iterations=5, k_color=f32(dq.k_color), color_step_scale=f32(dq.color_step_scale),
                      k_normal=f32(dq.k_normal), k_depth=f32(dq.k_depth), albedo_eps=f32(dq.albedo_eps),
                      **{DN_PLANES[k]: s[DN_PLANES[k]] for k in names})
    reqs = [_abi.default_request(width=W, height=R, divisions=n, division_no=i, spp=16, seed=3) for i in range(n)]
    planes = [{k: np.split(s[DN_PLANES[k]], n, axis=0)[i] for k in names} for i in range(n)]
    check = _Check("denoise")
    with _abi.debug_library():
        rt.init()
        with rt.Scene(0, rt.World(scenes.single_sphere())) as sc:
            for step in (0, 1, 4, 8, 16):
                with knobs({"RT_DENOISE_LDS_STEP": step}):
                    got, st = sc.denoise(reqs, np.split(s["C"], n, axis=0), planes, 8, 4, dq, outputs=("rgb", "linear", "f32"))
                for o in ("rgb", "linear", "f32"):
                    g = np.concatenate([x[o] for x in got], 0)
                    same = np.array_equal(g, want[o]) if o == "rgb" else np.array_equal(_bits(g), _bits(want[o]))
                    check(same, f"{R}x{W}", f"lds_step_{step}", o)
    check.done()
