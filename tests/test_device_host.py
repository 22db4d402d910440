"""The owners of the host layer's device resources off the GPU (csrc/rt_device.h: DevArray, Event, Stream, GrowBuf, EventPool), the
product's header through the g++ harness tests/host/device_host.cpp, which DEFINES the HIP functions the header calls as counting
fakes (a link seam: no runtime, no template parameter in the product).  A double free or an unknown handle is a violation (the
stand-alone program aborts on it; here every test ends by asserting that there was none); the fakes log every call as one letter and
can fail the k-th fallible call:
    M hipMalloc   F hipFree   C hipMemcpyAsync   E hipEventCreateWithFlags   D hipEventDestroy   W hipEventSynchronize
    R hipEventRecord   S hipStreamCreateWithFlags   X hipStreamDestroy
(a) failure injection, exhaustive: a sequence shaped like the scene upload followed by two shaped like a host form, with every one of
    its calls failing in turn, returns a failure and leaves no allocation, event or stream alive; so does the clean run;
(b) GrowBuf: no call when large enough, the wait before the free, pointer and size after a failed wait and a failed allocation;
(c) EventPool: both events or none, a dropped lease is reused without a create call, a pending pair does not return until collected;
(d) moves free nothing twice and leave the source empty;
(e) the harness as a stand-alone program under -fsanitize=address,undefined."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "host" / "device_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "libdevice_host.so"
HDR = ROOT / "ray_tracer_s8_amd" / "csrc" / "rt_device.h"
GXX = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{HDR.parent}"]
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def lib():
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.run(GXX + ["-O2", "-fPIC", "-shared", "-o", str(OUT), str(SRC)], check=True)
    l = C.CDLL(str(OUT))
    for name, res, args in [
        ("dh_reset", None, [C.c_long]),
        ("dh_calls", C.c_long, []),
        ("dh_violation", C.c_char_p, []),
        ("dh_forget", None, []),
        ("dh_log", C.c_char_p, []),
        ("dh_live", None, [u64p]),
        ("dh_run_sequences", C.c_int, []),
        ("dh_moves", C.c_int, []),
        ("dh_grow_new", C.c_void_p, []),
        ("dh_grow_free", None, [C.c_void_p]),
        ("dh_grow", C.c_int, [C.c_void_p, C.c_uint64]),
        ("dh_grow_make_done", C.c_int, [C.c_void_p]),
        ("dh_grow_size", C.c_uint64, [C.c_void_p]),
        ("dh_grow_data", C.c_uint64, [C.c_void_p]),
        ("dh_pool_new", C.c_void_p, []),
        ("dh_pool_free", None, [C.c_void_p]),
        ("dh_lease", C.c_void_p, [C.c_void_p, C.POINTER(C.c_int)]),
        ("dh_lease_events", None, [C.c_void_p, u64p]),
        ("dh_lease_drop", None, [C.c_void_p]),
        ("dh_lease_to_pending", None, [C.c_void_p]),
        ("dh_pool_pending", C.c_uint64, [C.c_void_p, u64p, C.c_uint64]),
        ("dh_pool_collected", None, [C.c_void_p]),
    ]:
        getattr(l, name).restype, getattr(l, name).argtypes = res, args
    return l


@pytest.fixture(autouse=True)
def no_violation(lib):
    lib.dh_forget()
    yield
    assert lib.dh_violation() == b""


def live(lib):
    out = (C.c_uint64 * 3)()
    lib.dh_live(out)
    return tuple(out)


def log(lib):
    return lib.dh_log().decode()


def lease(lib, pool):
    """(handle or None, status, (a, b))"""
    st = C.c_int(99)
    h = lib.dh_lease(pool, C.byref(st))
    ev = (C.c_uint64 * 2)()
    if h:
        lib.dh_lease_events(h, ev)
    return h, st.value, tuple(ev)


def pending(lib, pool):
    out = (C.c_uint64 * 16)()
    n = lib.dh_pool_pending(pool, out, 8)
    return [(out[2 * i], out[2 * i + 1]) for i in range(n)]


# ---------------------------------------------------------------- (a) failure injection
# What the clean run calls, written out from the sequences in the harness, not taken from a run:
#   the upload: two streams, two events, a record, five uploads (allocation and copy each, the empty one too), the counters, a record
#   and the wait; its two timing events are destroyed when it returns;
UPLOAD = "SS" "EE" "R" + "MC" * 5 + "M" "R" "W" "DD"
#   the first host form: the staging, two pairs made (E E each), a record; the first launch makes its pair, the ring and the ring's
#   event, and records three times; the second launch makes a pair, waits for the ring's event, frees and allocates, records three times;
#   the closing record; two waits for the pending pairs;
FORM_1 = "M" "EE" "EE" "R" + ("EE" "M" "E" "RRR") + ("EE" "W" "F" "M" "RRR") + "R" "WW"
#   the second: nothing made, nothing grown (the four pairs are reused): the records and the waits only;
FORM_2 = "R" + "RRR" * 2 + "R" "WW"
#   scope exit, in reverse order of declaration: the scene (pool: four pairs; stage; ring and its event; counters, rank, big (empty:
#   no call), emis, nodes, geom), then the copy stream and the stream.
EXIT = "DD" * 4 + "F" + "DF" + "F" * 5 + "XX"


def test_clean_run_calls_what_the_sequences_say_and_leaves_nothing(lib):
    lib.dh_reset(-1)
    assert lib.dh_run_sequences() == 0
    assert live(lib) == (0, 0, 0)
    got = log(lib)
    body = UPLOAD + FORM_1 + FORM_2
    assert got[:len(body)] == body
    assert sorted(got[len(body):]) == sorted(EXIT)             # (the order of the members' destructors is the struct's business)
    assert lib.dh_calls() == sum(body.count(c) for c in "MCEWRS")


def test_every_call_failing_in_turn_fails_the_run_and_leaks_nothing(lib):
    lib.dh_reset(-1)
    assert lib.dh_run_sequences() == 0
    n = lib.dh_calls()
    assert n == 18 + 23 + 10                                   # the fallible calls of UPLOAD, FORM_1 and FORM_2 (all letters but F and D)
    for k in range(n):                                         # every one of them, not a sample
        lib.dh_reset(k)
        assert lib.dh_run_sequences() != 0, k
        assert live(lib) == (0, 0, 0), (k, log(lib))
        assert lib.dh_calls() == k + 1, k                      # the run stopped at the call that failed
    lib.dh_reset(n)                                            # one past the last call: nothing fails
    assert lib.dh_run_sequences() == 0 and live(lib) == (0, 0, 0)


# ---------------------------------------------------------------- (b) GrowBuf
def test_growbuf_makes_no_call_when_it_is_large_enough(lib):
    lib.dh_reset(-1)
    g = lib.dh_grow_new()
    assert lib.dh_grow(g, 0) == 0 and log(lib) == ""           # nothing asked, nothing done
    assert lib.dh_grow(g, 1000) == 0 and log(lib) == "M"       # the first area: nothing to wait for, nothing to free
    p = lib.dh_grow_data(g)
    assert p and lib.dh_grow_size(g) == 1000
    for bytes_ in (1000, 999, 1, 0):
        assert lib.dh_grow(g, bytes_) == 0
    assert log(lib) == "M" and lib.dh_grow_data(g) == p and lib.dh_grow_size(g) == 1000
    lib.dh_grow_free(g)
    assert log(lib) == "MF" and live(lib) == (0, 0, 0)


def test_growbuf_waits_for_its_event_before_it_frees(lib):
    lib.dh_reset(-1)
    g = lib.dh_grow_new()
    assert lib.dh_grow(g, 100) == 0
    assert lib.dh_grow(g, 200) == 0                            # no event yet (a staging buffer): free, allocate
    assert log(lib) == "M" "FM"
    assert lib.dh_grow_make_done(g) == 0
    assert lib.dh_grow(g, 300) == 0                            # with its event: wait, free, allocate
    assert log(lib) == "M" "FM" "E" "WFM"
    assert lib.dh_grow_size(g) == 300
    lib.dh_grow_free(g)
    assert live(lib) == (0, 0, 0)


def test_growbuf_without_an_area_does_not_wait(lib):
    lib.dh_reset(-1)
    g = lib.dh_grow_new()
    assert lib.dh_grow_make_done(g) == 0
    assert lib.dh_grow(g, 64) == 0 and log(lib) == "EM"        # the event exists, the area does not: nothing is in flight on it
    lib.dh_grow_free(g)
    assert live(lib) == (0, 0, 0)


def test_growbuf_after_a_failed_allocation_is_empty_and_grows_again(lib):
    lib.dh_reset(-1)
    g = lib.dh_grow_new()
    assert lib.dh_grow(g, 100) == 0 and lib.dh_grow_make_done(g) == 0
    lib.dh_reset(1)                                            # the wait (call 0) succeeds, the allocation (call 1) fails
    assert lib.dh_grow(g, 200) != 0
    assert log(lib) == "WFM"
    assert lib.dh_grow_data(g) == 0 and lib.dh_grow_size(g) == 0
    assert live(lib) == (0, 1, 0)                              # the old area is gone, the event stays
    lib.dh_reset(-1)
    assert lib.dh_grow(g, 50) == 0                             # smaller than the area it once had: it has none now
    assert log(lib) == "M" and lib.dh_grow_data(g) and lib.dh_grow_size(g) == 50
    lib.dh_grow_free(g)
    assert live(lib) == (0, 0, 0)


def test_growbuf_after_a_failed_wait_keeps_its_area(lib):
    lib.dh_reset(-1)
    g = lib.dh_grow_new()
    assert lib.dh_grow(g, 100) == 0 and lib.dh_grow_make_done(g) == 0
    p = lib.dh_grow_data(g)
    lib.dh_reset(0)
    assert lib.dh_grow(g, 200) != 0
    assert log(lib) == "W"                                     # a launch may still use the area: it is not freed
    assert lib.dh_grow_data(g) == p and lib.dh_grow_size(g) == 100
    lib.dh_grow_free(g)
    assert live(lib) == (0, 0, 0)


# ---------------------------------------------------------------- (c) EventPool
def test_pool_pair_is_both_events_or_none(lib):
    for k, left in ((0, "E"), (1, "EED")):                     # the first create fails / the second: the first event is destroyed
        lib.dh_reset(k)
        pool = lib.dh_pool_new()
        h, st, _ = lease(lib, pool)
        assert h is None and st > 0                            # (st == -1: a failed lease that holds something)
        assert log(lib) == left and live(lib) == (0, 0, 0)
        assert pending(lib, pool) == []
        lib.dh_reset(-1)
        h, st, (a, b) = lease(lib, pool)                       # the pool is as good as new
        assert h and st == 0 and a and b and a != b and live(lib) == (0, 2, 0)
        lib.dh_lease_drop(h)
        lib.dh_pool_free(pool)
        assert live(lib) == (0, 0, 0)


def test_dropped_lease_returns_to_the_pool_and_is_reused_without_a_create(lib):
    lib.dh_reset(-1)
    pool = lib.dh_pool_new()
    h1, _, ev1 = lease(lib, pool)
    h2, _, ev2 = lease(lib, pool)
    assert log(lib) == "EEEE" and len(set(ev1 + ev2)) == 4
    lib.dh_lease_drop(h1)
    assert log(lib) == "EEEE" and live(lib) == (0, 4, 0)       # returned, not destroyed
    h3, st, ev3 = lease(lib, pool)
    assert st == 0 and ev3 == ev1 and log(lib) == "EEEE"       # the same pair, no create call
    h4, _, ev4 = lease(lib, pool)                              # the pool is empty again: a new pair
    assert log(lib) == "EEEEEE" and not set(ev4) & set(ev1 + ev2)
    for h in (h2, h3, h4):
        lib.dh_lease_drop(h)
    lib.dh_pool_free(pool)
    assert log(lib) == "EEEEEE" + "D" * 6 and live(lib) == (0, 0, 0)


def test_pending_lease_does_not_return_until_collected(lib):
    lib.dh_reset(-1)
    pool = lib.dh_pool_new()
    h1, _, ev1 = lease(lib, pool)
    h2, _, ev2 = lease(lib, pool)
    lib.dh_lease_to_pending(h1)
    lib.dh_lease_to_pending(h2)
    assert pending(lib, pool) == [ev1, ev2]                    # in the order of the launches
    lib.dh_lease_drop(h1)                                      # the lease goes out of scope: its pair stays pending
    lib.dh_lease_drop(h2)
    assert pending(lib, pool) == [ev1, ev2]
    h3, _, ev3 = lease(lib, pool)                              # so the next lease is a NEW pair, not one a launch still records to
    assert log(lib) == "EEEEEE" and not set(ev3) & set(ev1 + ev2)
    lib.dh_pool_collected(pool)
    assert pending(lib, pool) == []
    got = []
    for _ in range(2):                                         # collecting returned both: two leases, no create call
        h, _, ev = lease(lib, pool)
        got.append(ev)
        lib.dh_lease_to_pending(h)                             # (and a pool destroyed with pairs pending destroys those too)
        lib.dh_lease_drop(h)
    assert sorted(got) == sorted([ev1, ev2]) and log(lib) == "EEEEEE"
    lib.dh_lease_drop(h3)
    lib.dh_pool_free(pool)
    assert log(lib) == "EEEEEE" + "D" * 6 and live(lib) == (0, 0, 0)


# ---------------------------------------------------------------- (d) moves
def test_moves_leave_the_source_empty_and_release_once(lib):
    lib.dh_reset(-1)
    assert lib.dh_moves() == 0                                 # (a second release of a handle is a violation)
    assert live(lib) == (0, 0, 0)
    made = log(lib)
    assert made.count("F") == made.count("M") and made.count("D") == made.count("E") and made.count("X") == made.count("S")


# ---------------------------------------------------------------- (e) under a sanitizer, stand-alone
def test_host_program_under_sanitizers(tmp_path):
    exe = tmp_path / "device_host_san"
    r = subprocess.run(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DDEVICE_HOST_MAIN", "-o", str(exe),
                              str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "DEVICE_HOST_OK" in run.stdout and not run.stderr, run.stdout + run.stderr
