"""The frame context's decisions off the GPU (csrc/rt_frame_plan.h, the product's functions through the g++ harness
tests/host/frame_plan_host.cpp): the cut of a frame into strips, the key under which last frame's strip costs still hold, the
assignment mode, the page-lock step, the launch groups of a call and the folds of the strip costs and of the entries' statistics.
Reference: the controller fires one request per strip of the wire format's `divisions` and stitches them by division_no
(C/main.rs:47-75, 109-115).  Every expected value is written out from the rule, none comes from the function under test."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ray_tracer_s8_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "host" / "frame_plan_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "libframe_plan_host.so"
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
HDRS = [CSRC / "rt_frame_plan.h", CSRC / "rt_assign.h", CSRC / "rt_plan.h", CSRC / "rt_consts.h", ROOT / "include" / "rt_tile.h"]
STATIC, SNAKE, BY_COST, QUEUE = 0, 1, 2, 3
MIB = 1 << 20
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def lib():
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(p.stat().st_mtime for p in [SRC, *HDRS]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(OUT), str(SRC)],
                       check=True)
    l = C.CDLL(str(OUT))
    rqp, fp = C.POINTER(_abi.TileRequest), C.POINTER(C.c_float)
    for name, res, args in [
        ("fp_max_batch", C.c_uint32, []),
        ("fp_cost_copies", C.c_uint32, []),
        ("fp_strips", C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int]),
        ("fp_mem_new", C.c_void_p, []),
        ("fp_mem_free", None, [C.c_void_p]),
        ("fp_mem_forget", None, [C.c_void_p]),
        ("fp_mem_usable", C.c_int, [C.c_void_p, rqp, fp]),
        ("fp_mem_remember", None, [C.c_void_p, rqp, fp, u64p, C.c_uint32, C.c_int]),
        ("fp_plan", C.c_uint32, [C.c_void_p, rqp, C.c_uint32, fp, rqp, u64p, u32p, u32p]),
        ("fp_remember_frame", None, [C.c_void_p, rqp, C.c_uint32, fp, u64p, C.c_uint32, C.c_int]),
        ("fp_pin_step", C.c_uint32, [C.c_int, C.c_size_t, C.c_uint64, C.c_size_t, C.c_uint64]),
        ("fp_launch_groups", C.c_uint32, [C.c_uint32, C.c_uint64, u32p]),
        ("fp_fold_strip_costs", None, [u64p, u32p, C.c_uint32, u64p]),
        ("fp_fold_frame_stats", None, [C.POINTER(_abi.TileStats), fp, C.c_uint32, C.c_int, C.POINTER(_abi.FrameStats)]),
    ]:
        getattr(l, name).restype, getattr(l, name).argtypes = res, args
    assert l.fp_max_batch() == 64 and l.fp_cost_copies() == 16          # the sizes the cases below are written for
    return l


# ---------------------------------------------------------------- the cut of a frame into strips
RECUT = [((256, 32, 8), 64), ((180, 6, 2), 12), ((144, 12, 2), 12), ((1080, 16, 8), 54), ((1080, 32, 8), 54), ((2160, 32, 8), 48),
         ((1080, 16, 16), 108), ((1000, 8, 3), 20), ((54, 3, 8), 54), ((64, 64, 2), 64),
         ((7, 7, 2), 7),       # none found: the request is kept
         ((97, 1, 2), 1),      # a prime height: 97 itself is beyond 4 * 12
         ((96, 4, 1), 4)]      # one entry


def recut(height, divisions, n, queue=False, static=False):
    """rt_tile.h "Strip assignment": at least six strips per entry, the first count from max(divisions, 6 n) up to four times that
    (and no more than the height) that divides the height; the request's own strips for the queue, the static split and one entry."""
    if queue or static or n <= 1:
        return divisions
    want = max(divisions, 6 * n)
    return next((dv for dv in range(want, min(height, 4 * want) + 1) if height % dv == 0), divisions)


@pytest.mark.parametrize("case,strips", RECUT)
def test_recut_cases(lib, case, strips):
    h, dv, n = case
    assert lib.fp_strips(h, dv, n, 0, 0) == strips
    for queue, static in [(1, 0), (0, 1), (1, 1)]:
        assert lib.fp_strips(h, dv, n, queue, static) == dv


def test_recut_against_the_rule_for_all_small_frames(lib):
    for h in range(1, 129):
        for dv in [d for d in range(1, h + 1) if h % d == 0]:
            for n in range(1, 10):
                got = lib.fp_strips(h, dv, n, 0, 0)
                assert got == recut(h, dv, n), (h, dv, n)
                assert h % got == 0 and got >= dv
                assert lib.fp_strips(h, dv, n, 1, 0) == dv and lib.fp_strips(h, dv, n, 0, 1) == dv


def test_recut_never_looks_past_the_height(lib):
    """The range ends at min(height, 4 want).  A count above the height never divides it, so the only frame on which that bound
    shows is the empty one (which the entry points reject before any plan): it has no count in range, and keeps the request's."""
    assert lib.fp_strips(0, 4, 2, 0, 0) == 4


# ---------------------------------------------------------------- the cost memory
def request(**kw):
    r = _abi.TileRequest(width=256, height=144, divisions=12, division_no=0, spp=4, max_bounces=10, aperture=0.1, focus_distance=1.0,
                         fov=1.5, focal_length=1.0, t_min=0.001, t_max=1000.0, seed=7, flags=0, reserved=0)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def pose(x=0.0):
    return (C.c_float * 12)(x, 1, 2, 1, 0, 0, 0, 1, 0, 0, 0, 1)


def costs(values):
    a = (C.c_uint64 * len(values))(*values)
    return a, len(values)


class Mem:
    def __init__(self, lib):
        self.lib, self.h = lib, C.c_void_p(lib.fp_mem_new())

    def __del__(self):
        self.lib.fp_mem_free(self.h)

    def usable(self, rq, ps=None):
        return bool(self.lib.fp_mem_usable(self.h, C.byref(rq), ps))

    def remember(self, rq, ps, values, counting_on=True):
        self.lib.fp_mem_remember(self.h, C.byref(rq), ps, *costs(values), int(counting_on))

    def plan(self, rq, n, ps=None):
        out, nbytes, mode = _abi.TileRequest(), C.c_uint64(), C.c_uint32()
        owner = (C.c_uint32 * (4 * max(rq.divisions, 6 * n) + 1))()
        strips = self.lib.fp_plan(self.h, C.byref(rq), n, ps, C.byref(out), C.byref(nbytes), C.byref(mode), owner)
        return out, nbytes.value, mode.value, list(owner[:strips])

    def remember_frame(self, rq, n, ps, values, counting_on=True):
        self.lib.fp_remember_frame(self.h, C.byref(rq), n, ps, *costs(values), int(counting_on))


def test_cost_memory_key(lib):
    m, rq, ps = Mem(lib), request(), pose()
    assert not m.usable(rq, ps) and not m.usable(rq)                   # a fresh object
    m.remember(rq, ps, range(1, 13))
    assert m.usable(rq, ps)
    # the seed changes the paths, not where the expensive rows are; division_no and the flags are no part of the key
    assert m.usable(request(seed=8), ps) and m.usable(request(division_no=5), ps)
    for flags in (_abi.RT_FLAG_FRAME_NO_PIN, _abi.RT_FLAG_FRAME_STATIC, _abi.RT_FLAG_FRAME_QUEUE | _abi.RT_FLAG_FRAME_NO_PIN):
        assert m.usable(request(flags=flags), ps)
    # the frame's geometry is
    for change in (dict(spp=5), dict(width=257), dict(max_bounces=9), dict(t_max=999.0), dict(height=288), dict(fov=1.25),
                   dict(aperture=0.2), dict(focus_distance=2.0), dict(focal_length=2.0), dict(t_min=0.01)):
        assert not m.usable(request(**change), ps), change
    assert not m.usable(rq, pose(0.5))                                 # another pose
    assert not m.usable(rq, None)                                      # pose present when measured, absent now
    assert not m.usable(request(divisions=24), ps)                     # another strip count
    m.lib.fp_mem_forget(m.h)
    assert not m.usable(rq, ps)
    # ... and measured without a pose: usable without one only (the pose's bytes are not compared then)
    m.remember(rq, None, range(1, 13))
    assert m.usable(rq, None) and not m.usable(rq, ps)


def test_a_request_with_a_nan_knob_is_of_its_own_frame(lib):
    """same_frame is also what admits a batch of strips: a knob that is NaN in both requests agrees (a single strip with a NaN fov or
    aperture is a frame of NaN rays, not a batch that disagrees with itself), and still differs from every number."""
    nan = float("nan")
    for knob in ("aperture", "focus_distance", "fov", "focal_length", "t_min", "t_max"):
        m, rq, ps = Mem(lib), request(**{knob: nan}), pose()
        m.remember(rq, ps, range(1, 13))
        assert m.usable(rq, ps) and m.usable(request(**{knob: nan, "seed": 8}), ps), knob
        assert not m.usable(request(), ps) and not m.usable(request(**{knob: 0.0}), ps), knob
        other = "fov" if knob != "fov" else "aperture"
        assert not m.usable(request(**{knob: nan, other: 0.75}), ps), knob


def test_cost_memory_takes_only_a_measurement(lib):
    m, rq, ps = Mem(lib), request(), pose()
    m.remember(rq, ps, range(1, 13), counting_on=False)                # counting off
    assert not m.usable(rq, ps)
    m.remember(rq, ps, [0] * 12)                                       # all-zero costs
    assert not m.usable(rq, ps)
    m.remember(rq, ps, [0] * 11 + [1])
    assert m.usable(rq, ps)
    m.remember(rq, ps, [0] * 12)                                       # ... and a frame that measured nothing takes it away again
    assert not m.usable(rq, ps)


def test_queue_frame_leaves_the_memory_alone(lib):
    """144 rows in 12 strips over 2 entries stay 12 strips (six per entry).  One heavy strip on top: longest-first gives it an entry
    of its own, as long as the memory holds THAT measurement."""
    m, rq, ps = Mem(lib), request(), pose()
    heavy_top = [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    m.remember_frame(rq, 2, ps, [12] + [1] * 11)
    assert m.plan(rq, 2, ps)[2:] == (BY_COST, heavy_top)
    q = request(flags=_abi.RT_FLAG_FRAME_QUEUE)
    m.remember_frame(q, 2, ps, [1] * 11 + [12])                       # another profile, through a queue frame: not taken
    assert m.plan(rq, 2, ps)[2:] == (BY_COST, heavy_top)
    m.remember_frame(q, 2, ps, [0] * 12)                              # nor does a queue frame invalidate
    assert m.plan(rq, 2, ps)[2:] == (BY_COST, heavy_top)
    m.remember_frame(request(flags=_abi.RT_FLAG_FRAME_STATIC), 2, ps, [1] * 11 + [12])     # a static frame measures
    assert m.plan(rq, 2, ps)[2:] == (BY_COST, [1] * 11 + [0])


# ---------------------------------------------------------------- the plan of a frame
@pytest.mark.parametrize("queue,static,usable", list(itertools.product([False, True], repeat=3)))
def test_mode_and_owners(lib, queue, static, usable):
    """A frame of 180 rows in 6 strips over 2 entries: 12 strips for the balanced assignments, the request's 6 for the queue and the
    static split.  Queue wins over static, static over the costs, the costs over the snake."""
    m, ps = Mem(lib), pose()
    flags = _abi.RT_FLAG_COUNT_STEPS | _abi.RT_FLAG_FRAME_NO_PIN | (_abi.RT_FLAG_FRAME_QUEUE if queue else 0) | (_abi.RT_FLAG_FRAME_STATIC if static else 0)
    rq = request(height=180, divisions=6, division_no=3, flags=flags)
    strips = 6 if queue or static else 12
    cut = request(height=180, divisions=strips)
    if usable:
        m.remember(cut, ps, [9] + [1] * (strips - 1))
    assert m.usable(cut, ps) == usable
    out, nbytes, mode, owner = m.plan(rq, 2, ps)
    assert (out.divisions, out.division_no, out.flags) == (strips, 0, _abi.RT_FLAG_COUNT_STEPS)        # the kernels' request
    assert (out.width, out.height, out.spp, out.seed) == (256, 180, 4, 7)
    assert nbytes == (180 // strips) * 256 * 3
    if queue or static:
        assert mode == (QUEUE if queue else STATIC) and owner == [k % 2 for k in range(6)]
    elif usable:
        assert mode == BY_COST and owner == [0] + [1] * 9 + [0, 1]     # 9 | 1 x 9, then the loads are equal: the lower entry first
    else:
        assert mode == SNAKE and owner == [0, 1, 1, 0] * 3
    assert m.usable(cut, ps) == usable                                  # planning does not touch the memory


def test_one_entry_owns_everything(lib):
    out, nbytes, mode, owner = Mem(lib).plan(request(height=96, divisions=4), 1)
    assert (out.divisions, nbytes, mode, owner) == (4, 24 * 256 * 3, SNAKE, [0] * 4)


# ---------------------------------------------------------------- the page-lock step
def parent_pin(want, held_ptr, held_len, out, frame_bytes):
    """rt_frame_ctx_render's two conditions as they stood before rt_frame_plan.h, word for word."""
    release = acquire = False
    if (not want) or held_ptr != out or held_len < frame_bytes:
        if held_ptr and not (want and held_ptr == out and held_len >= frame_bytes):
            release = True
        if want:
            acquire = True
    return release, acquire


def test_pin_step_truth_table(lib):
    out, other, nbytes = 0x10000, 0x20000, 4096
    table = {}
    for want, held, held_len in itertools.product([False, True], [0, out, other], [nbytes - 1, nbytes, nbytes + 1]):
        got = lib.fp_pin_step(int(want), held, held_len, out, nbytes)
        got = (bool(got & 1), bool(got & 2))
        assert got == parent_pin(want, held, held_len, out, nbytes), (want, held, held_len)
        table[want, held, held_len >= nbytes] = got
    # ... and the table of the header's comment: (release, acquire)
    for long_enough in (False, True):
        assert table[False, 0, long_enough] == (False, False)
        assert table[False, out, long_enough] == table[False, other, long_enough] == (True, False)
        assert table[True, 0, long_enough] == (False, True)
        assert table[True, other, long_enough] == (True, True)
    assert table[True, out, True] == (False, False) and table[True, out, False] == (True, True)


# ---------------------------------------------------------------- launch groups and the strip costs
def groups(lib, n, strip_bytes):
    buf = (C.c_uint32 * (2 * (n // 64 + 2)))()
    k = lib.fp_launch_groups(n, strip_bytes, buf)
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(k)]


@pytest.mark.parametrize("n,strip_bytes,want", [
    (6, 1000, [(0, 6)]), (1, 1000, [(0, 1)]), (1, 200 * MIB, [(0, 1)]), (3, 40 * MIB, [(0, 3)]), (4, 17 * MIB, [(0, 3), (3, 1)]),
    (100, MIB, [(0, 64), (64, 11), (75, 25)]), (300, MIB, [(0, 64), (64, 64), (128, 64), (192, 33), (225, 64), (289, 11)]),
    (4, 16 * MIB, [(0, 4)]), (64, MIB, [(0, 64)]),              # exactly 64 MiB: one launch
    (4, 16 * MIB + 1, [(0, 3), (3, 1)]), (8, 8 * MIB + 1, [(0, 6), (6, 2)]),
])
def test_launch_groups(lib, n, strip_bytes, want):
    assert groups(lib, n, strip_bytes) == want


def test_launch_groups_tile_the_call(lib):
    for strip_bytes in (1000, MIB, 33 * MIB):
        for n in range(1, 301):
            g = groups(lib, n, strip_bytes)
            at = 0
            for first, count in g:
                assert first == at and 1 <= count <= 64
                at += count
            assert at == n
            split = n >= 4 and n * strip_bytes > 64 * MIB
            assert len(g) == (-(-(n - n // 4) // 64) + -(-(n // 4) // 64) if split else -(-n // 64))
            if split:
                assert n - n // 4 in [first for first, _ in g]                   # the last quarter starts a launch of its own


def test_fold_strip_costs(lib):
    g = [(0, 64), (64, 11), (75, 25)]
    raw = (np.arange(3 * 16 * 64, dtype=np.uint64) * np.uint64(1000003)) % np.uint64(999983) + np.uint64(1)      # distinct partial counters
    assert len(set(raw.tolist())) == raw.size
    out = np.full(100, 2**64 - 1, np.uint64)
    flat = np.array(g, np.uint32).ravel()
    lib.fp_fold_strip_costs(raw.ctypes.data_as(u64p), flat.ctypes.data_as(u32p), 3, out.ctypes.data_as(u64p))
    blocks = raw.reshape(3, 16, 64)                                      # [group][copy][strip of the group]
    for gi, (first, count) in enumerate(g):
        for i in range(count):
            assert out[first + i] == sum(int(blocks[gi, c, i]) for c in range(16)), (gi, i)


# ---------------------------------------------------------------- the entries' statistics
def fold(lib, entries, queue=False):
    st = (_abi.TileStats * len(entries))()
    busy = (C.c_float * len(entries))()
    for i, e in enumerate(entries):
        e = dict(e)
        busy[i] = e.pop("busy_ms")
        for k, v in e.items():
            setattr(st[i], k, v)
    fs = _abi.FrameStats()
    C.memset(C.byref(fs), 0xff, C.sizeof(fs))
    lib.fp_fold_frame_stats(st, busy, len(entries), int(queue), C.byref(fs))
    return fs


THREE = [      # (times are binary fractions: the comparisons below are exact)
    dict(ray_segments=100, primary_rays=10, broad_candidates=5, exact_fallbacks=1, node_steps=7, kernel_ms=3.0, h2d_ms=0.5, d2h_ms=0.875,
         n_launches=1, engine=4, broad_form=0, busy_ms=5.0),
    dict(ray_segments=300, primary_rays=20, broad_candidates=6, exact_fallbacks=2, node_steps=8, kernel_ms=2.0, h2d_ms=0.125, d2h_ms=0.25,
         n_launches=2, engine=3, broad_form=1, busy_ms=6.0),           # finishes last, with neither the longest kernel nor download
    dict(ray_segments=200, primary_rays=30, broad_candidates=7, exact_fallbacks=3, node_steps=9, kernel_ms=1.0, h2d_ms=0.75, d2h_ms=0.5,
         n_launches=0, engine=9, broad_form=5, busy_ms=1.0),           # launched nothing: its engine is no one's
]


@pytest.mark.parametrize("queue", [False, True])
def test_fold_frame_stats_three_entries(lib, queue):
    fs = fold(lib, THREE, queue)
    t = fs.totals
    assert (t.ray_segments, t.primary_rays, t.broad_candidates, t.exact_fallbacks, t.node_steps, t.n_launches) == (600, 60, 18, 6, 24, 3)
    assert (t.kernel_ms, t.h2d_ms, t.d2h_ms) == (3.0, 0.75, 0.875)      # the entries run concurrently: the largest, not the sum
    assert (t.engine, t.broad_form) == (3, 1)                           # of the last entry that launched
    # of the entry that finished last; the strip queue books that dispatcher's wall time and no exposed download
    assert (fs.kernel_ms, fs.d2h_exposed_ms) == ((6.0, 0.0) if queue else (2.0, 0.25))
    assert list(fs.entry_segments) == [100, 300, 200] + [0] * 13
    assert fs.balance_max_over_mean == 1.5                              # 300 / (600 / 3)
    # the caller's part is zeroed, not filled
    assert (fs.wall_ms, fs.pin_ms, fs.scene_ms, fs.host_ms, fs.n_devices, fs.pinned, fs.assignment) == (0, 0, 0, 0, 0, 0, 0)


def test_fold_frame_stats_first_of_equal_finishers(lib):
    a = dict(THREE[0], busy_ms=6.0)
    fs = fold(lib, [a, THREE[1]])
    assert (fs.kernel_ms, fs.d2h_exposed_ms) == (3.0, 0.875)


def test_fold_frame_stats_twenty_entries(lib):
    """rt_frame_stats has room for 16 entries' segments; the balance is taken over all twenty (the busiest is the last)."""
    segs = [10 + e for e in range(19)] + [1000]
    fs = fold(lib, [dict(ray_segments=s, n_launches=1, engine=2, busy_ms=1.0) for s in segs])
    assert list(fs.entry_segments) == segs[:16]
    assert fs.totals.ray_segments == sum(segs) and fs.totals.n_launches == 20
    assert fs.balance_max_over_mean == np.float32(1000 * 20 / sum(segs))
    fs = fold(lib, [dict(ray_segments=s, n_launches=1, engine=2, busy_ms=1.0) for s in segs[:16]])
    assert list(fs.entry_segments) == segs[:16]                         # sixteen fill it
    fs = fold(lib, [dict(ray_segments=s, n_launches=1, engine=2, busy_ms=1.0) for s in segs[:15]])
    assert list(fs.entry_segments) == segs[:15] + [0]


def test_fold_frame_stats_without_segments(lib):
    fs = fold(lib, [dict(busy_ms=1.0), dict(busy_ms=2.0)])
    assert fs.balance_max_over_mean == 0.0 and fs.totals.ray_segments == 0
    assert (fs.totals.engine, fs.totals.broad_form, fs.totals.n_launches) == (0, 0, 0)
