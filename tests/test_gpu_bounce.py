"""Path steps of caller rays on the GPU (rt_scene_bounce, rt_scene_bounce_device), bit for bit throughout:
1. one step against the CPU reference tests/_bounce_np.py (pinned by tests/test_bounce_np.py): status, rgb, the rt_hit of the incoming
   ray, the ray written back and the state, under four configurations and both ray forms, on a sphere scene, a triangle scene and the
   mixed scene, every status occurring in each; the bytes of rays that MISSED or EMITTED untouched; the two exceptional arms of the
   scatter on constructed rays;
2. K steps through the device form, the active lists ping-ponged with no host read between the steps, folded right to left:
   Scene.trace(rng_state=..., spp=1, max_bounces=K - 1) and oracle.trace_batch, colours and final states; the rays stepped in all are
   the trace's segments; the seeded states against the seeded trace;
3. compaction and the active list for batch sizes around the wave and workgroup sizes: the set returned, the sentinel fill of every
   record outside the list, a device-side length shorter than the list, length 0, no next list, two streams at once;
4. the device form against the host form, the argument errors with a live scene, and the plain-C client examples/bounce_rays.c."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi

import _bounce_np as B
from test_bounce_surface import bad_arg_calls

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
F = _abi
WALK, SCAN = 2, 1
# name: (flags, engine, oracle backend)
CONFIGS = {
    "default": (0, WALK, 1),
    "no_bvh_cull": (F.RT_FLAG_NO_BVH_CULL, SCAN, 0),
    "exact_scan": (F.RT_FLAG_EXACT_SCAN, SCAN, 1),
    "full_chain": (F.RT_FLAG_FULL_CHAIN, WALK, 1),
}
N_RAYS = 640
FILL = 0xA5                                      # sentinel byte of the output buffers
SENTINEL_U32 = 0xA5A5A5A5


@pytest.fixture(scope="module")
def cases(oracle):
    return {name: B.population(oracle, name, N_RAYS, 600 + k) for k, name in enumerate(B.SCENE_NAMES)}


_REF = {}


def _ref_step(oracle, cases, name, backend, as_given):
    """The CPU reference of the first step of a scene's rays: computed once per (scene, backend, ray form), never modified."""
    key = (name, backend, as_given)
    if key not in _REF:
        sph, tri, wi, rays, st0 = cases[name]
        _REF[key] = B.step(oracle, sph, tri, rays, st0, backend, wi, as_given=as_given)
    return _REF[key]


_TRACE = {}


def _ref_trace(oracle, cases, name, backend, K):
    key = (name, backend, K)
    if key not in _TRACE:
        sph, tri, wi, rays, st0 = cases[name]
        _TRACE[key] = oracle.trace_batch(sph, tri, rays, spp=1, max_bounces=K - 1, backend=backend, world_index=wi, states=st0)
    return _TRACE[key]


def _assert_step_equals(got, want, idx, what):
    """The records of the rays `idx` of a step's result (a dict as Scene.bounce returns) against the reference's."""
    assert np.array_equal(got["bounce"]["status"][idx], want["bounce"]["status"][idx]), (what, "status")
    for key, ff, fi in (("bounce", B.BNC_F, ()), ("hits", B.HIT_F, ("index",)), ("rays", B.RAY_F, ())):
        ok = B.records_equal(got[key][idx], want[key][idx], ff, fi)
        assert ok.all(), (what, key, np.asarray(idx)[~ok][:5], got[key][idx][~ok][:2], want[key][idx][~ok][:2])
    assert np.array_equal(got["states"][idx], want["states"][idx]), (what, "states")


# ---------------------------------------------------------------- 1. one step against the CPU reference
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", B.SCENE_NAMES)
def test_one_step_is_bit_exact(ndev, oracle, cases, name, cfg):
    flags, engine, backend = CONFIGS[cfg]
    sph, tri, wi, rays, st0 = cases[name]
    every = np.arange(len(rays))
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        for as_given in (False, True):
            want = _ref_step(oracle, cases, name, backend, as_given)
            status = want["bounce"]["status"]
            assert {B.SCATTERED, B.EMITTED, B.MISSED} == set(status.tolist()), (name, cfg, "a status does not occur")
            got = sc.bounce(rays, st0, as_given=as_given, flags=flags, want_hits=True, want_next=True)
            _assert_step_equals(got, want, every, (name, cfg, as_given))
            still = status != B.SCATTERED                                  # EMITTED and MISSED: not a byte of the ray or the state
            assert still.any() and got["rays"][still].tobytes() == rays[still].tobytes()
            assert np.array_equal(got["states"][still], st0[still])
            assert np.all(np.any(got["states"][~still] != st0[~still], 1))
            assert np.array_equal(got["next"], np.nonzero(~still)[0])
            st = got["stats"]
            assert st.engine == engine and st.n_launches == 1 and st.ray_segments == len(rays) and st.primary_rays == 0
            assert st.broad_candidates > 0
            if engine == SCAN:
                assert st.broad_candidates == len(rays) * (len(sph) + len(tri))


@pytest.mark.parametrize("cfg", CONFIGS)
def test_exceptional_arms_of_the_scatter(ndev, oracle, cfg):
    """The zero normal as try_normalize's fallback (Ray::new's division gives NaN) and the roughness-1 mirror, on constructed rays
    (tests/_bounce_np.py exceptional_case; tests/test_bounce_np.py asserts that the reference takes those arms)."""
    flags, engine, backend = CONFIGS[cfg]
    sph, tri, rays = B.exceptional_case()
    st0 = B.R.states(len(rays), 5)
    want = B.step(oracle, sph, tri, rays, st0, backend)
    m = len(rays) // 3
    assert np.all(want["bounce"]["status"] == B.SCATTERED) and np.isnan(want["rays"]["dx"][:m]).all()
    assert np.all(want["hits"]["index"][2 * m:] == 0) and sph["roughness"][0] == 1.0
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        got = sc.bounce(rays, st0, flags=flags, want_hits=True)
        _assert_step_equals(got, want, np.arange(len(rays)), ("exceptional", cfg))
        assert np.isnan(got["rays"]["dx"][:m]).all() and got["stats"].engine == engine
        # the second step, as given: the NaN rays miss
        want2 = B.step(oracle, sph, tri, want["rays"], want["states"], backend, as_given=True)
        got2 = sc.bounce(got["rays"], got["states"], as_given=True, flags=flags, want_hits=True)
        _assert_step_equals(got2, want2, np.arange(len(rays)), ("exceptional, second step", cfg))
        assert np.all(got2["bounce"]["status"][:m] == B.MISSED)


# ---------------------------------------------------------------- device buffers through the library's own HIP runtime
class Dev:
    H2D, D2H = 1, 2

    def __init__(self):
        hip = self.hip = _abi.hip_runtime()
        vp = C.c_void_p
        hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
        hip.hipFree.argtypes = [vp]
        hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
        hip.hipMemset.argtypes = [vp, C.c_int, C.c_size_t]
        hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
        hip.hipStreamDestroy.argtypes = [vp]
        self.bufs, self.streams = [], []

    def alloc(self, nbytes, fill=None):
        d = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(d), max(int(nbytes), 4)) == 0
        self.bufs.append(d)
        if fill is not None:
            assert self.hip.hipMemset(d, fill, max(int(nbytes), 4)) == 0
        return d.value

    def put(self, a):
        a = np.ascontiguousarray(a)
        d = self.alloc(a.nbytes)
        if a.nbytes:
            assert self.hip.hipMemcpy(d, a.ctypes.data, a.nbytes, self.H2D) == 0
        return d

    def get(self, d, dtype, count):
        a = np.zeros(count, dtype)
        if a.nbytes:
            assert self.hip.hipMemcpy(a.ctypes.data, d, a.nbytes, self.D2H) == 0
        return a

    def stream(self):
        s = C.c_void_p()
        assert self.hip.hipStreamCreate(C.byref(s)) == 0
        self.streams.append(s)
        return s.value

    def sync(self):
        assert self.hip.hipDeviceSynchronize() == 0

    def close(self):
        self.sync()
        for s in self.streams:
            self.hip.hipStreamDestroy(s)
        for b in self.bufs:
            self.hip.hipFree(b)
        self.bufs, self.streams = [], []


@pytest.fixture
def dev(ndev):
    d = Dev()
    yield d
    d.close()


def _device_outputs(dev, n):
    """Sentinel-filled rt_bounce, rt_hit and next-list buffers and a next-list length of 99."""
    return dict(bounce=dev.alloc(16 * n, FILL), hits=dev.alloc(32 * n, FILL), next=dev.alloc(4 * n, FILL),
                n_next=dev.put(np.array([99], np.uint32)))


def _read_step(dev, d_rays, d_state, out, n):
    return dict(rays=dev.get(d_rays, _abi.RAY_DTYPE, n), states=dev.get(d_state, np.uint64, 4 * n).reshape(n, 4),
                bounce=dev.get(out["bounce"], _abi.BOUNCE_DTYPE, n), hits=dev.get(out["hits"], _abi.HIT_DTYPE, n),
                next=dev.get(out["next"], np.uint32, n), n_next=int(dev.get(out["n_next"], np.uint32, 1)[0]))


# ---------------------------------------------------------------- 2. K steps compose to the trace
def _device_fold(sc, dev, rays, st0, K, flags, seed=None, as_given=False):
    """K steps of the device form on the scene's stream, the next list of one step the active list of the following one, nothing
    read in between; then the right-to-left fold of the per-step records.  Returns (rgb, final states, collect() stats)."""
    n = len(rays)
    d_rays, d_state = dev.put(rays), dev.put(st0)
    d_bnc = [dev.alloc(16 * n, FILL) for _ in range(K)]
    lists = [(dev.alloc(4 * n, FILL), dev.put(np.array([99], np.uint32))) for _ in range(2)]
    dev.sync()
    sc.collect()
    for k in range(K):
        act, n_act = lists[(k + 1) % 2] if k else (0, 0)
        nxt, n_nxt = lists[k % 2]
        sc.bounce_device(d_rays, n, d_state, d_bnc[k], d_active=act, d_n_active=n_act, d_next_active=nxt, d_n_next=n_nxt,
                         as_given=as_given or k > 0, flags=flags, seed=seed if k == 0 else None)
    st = sc.collect()
    acc = np.zeros((n, 3), np.float32)
    for k in range(K - 1, -1, -1):
        b = dev.get(d_bnc[k], _abi.BOUNCE_DTYPE, n)
        stepped = b["status"] != SENTINEL_U32
        assert set(b["status"][stepped].tolist()) <= {B.SCATTERED, B.EMITTED, B.MISSED}
        rgb = B.rgb_of(b)
        with np.errstate(all="ignore"):
            acc = np.where(stepped[:, None], np.where((b["status"] == B.SCATTERED)[:, None], rgb * acc, rgb), acc).astype(np.float32)
    return acc, dev.get(d_state, np.uint64, 4 * n).reshape(n, 4), st


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", ["spheres", "mixed"])
def test_k_steps_compose_to_the_trace(ndev, oracle, cases, dev, name, cfg):
    flags, engine, backend = CONFIGS[cfg]
    sph, tri, wi, rays, st0 = cases[name]
    o, d = B.R.od(rays)
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        for K in (1, 2, 4, 11):
            rgb, segs, _, st1 = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=K - 1, rng_state=st0, flags=flags)
            acc, states, st = _device_fold(sc, dev, rays, st0, K, flags)
            ok = np.all(B.same_bits(acc, rgb), 1)
            assert ok.all(), (name, cfg, K, np.nonzero(~ok)[0][:5], acc[~ok][:3], rgb[~ok][:3])
            assert np.array_equal(states, st1), (name, cfg, K, "states")
            assert st.ray_segments == int(segs.sum()) and st.n_launches == K and st.engine == engine and st.primary_rays == 0
            want = _ref_trace(oracle, cases, name, backend, K)
            assert B.same_bits(acc, want[0]).all() and np.array_equal(states, want[2]), (name, cfg, K, "oracle")
        assert int(segs.max()) >= (11 if name == "spheres" else 4)          # some path is alive at the last step


@pytest.mark.parametrize("cfg", ["default", "no_bvh_cull"])
def test_seeded_states_compose_to_the_seeded_trace(ndev, oracle, cases, dev, cfg):
    flags, engine, backend = CONFIGS[cfg]
    sph, tri, wi, rays, st0 = cases["mixed"]
    o, d = B.R.od(rays)
    seed, K = 0xFEEDF00D5EED, 4
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        rgb, segs, _ = sc.trace(o, d, rays["t_min"], rays["t_max"], spp=1, max_bounces=K - 1, seed=seed, flags=flags)
        acc, states, st = _device_fold(sc, dev, rays, np.zeros_like(st0), K, flags, seed=seed)
        assert B.same_bits(acc, rgb).all() and st.ray_segments == int(segs.sum())
        want = oracle.trace_batch(sph, tri, rays, spp=1, max_bounces=K - 1, backend=backend, world_index=wi, seed=seed)
        assert B.same_bits(acc, want[0]).all()
        # one seeded step of the host form: the state of every ray is seeded, whatever its status
        one = sc.bounce(rays, None, seed=seed, flags=flags)
        ref = B.step(oracle, sph, tri, rays, np.zeros_like(st0), backend, wi, seed=seed)
        assert np.array_equal(one["states"], ref["states"]) and np.array_equal(one["bounce"]["status"], ref["bounce"]["status"])
        still = ref["bounce"]["status"] != B.SCATTERED
        assert np.array_equal(one["states"][still], B.seeded_states(seed, len(rays))[still])


# ---------------------------------------------------------------- 3. compaction and the active list
@pytest.fixture(scope="module")
def big(oracle):
    """5 000 rays on the sphere scene and, once a scene exists, the host form's step of all of them (the per-ray truth of this
    section: every result lives at the ray's own index, so any subset stepped in any order gives the same records)."""
    sph, tri, wi, rays, st0 = B.population(oracle, "spheres", 5000, 900)
    return dict(sph=sph, tri=tri, wi=wi, rays=rays, st0=st0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_compaction_and_the_active_list(ndev, oracle, big, dev, n):
    rays, st0 = big["rays"][:n], big["st0"][:n]
    with rt.Scene(0, rt.World(big["sph"], big["tri"], big["wi"])) as sc:
        full = sc.bounce(rays, st0, want_hits=True, want_next=True)
        want = B.step(oracle, big["sph"], big["tri"], rays, st0, 1)
        _assert_step_equals(full, want, np.arange(n), ("all", n))
        scat = np.nonzero(full["bounce"]["status"] == B.SCATTERED)[0]
        assert np.array_equal(full["next"], scat)                          # the set, sorted by the wrapper
        if n >= 63:
            assert 0 < len(scat) < n

        # (a) the device form, all rays: the host form's bytes, the list a permutation of the scattered set
        d_rays, d_state, out = dev.put(rays), dev.put(st0), _device_outputs(dev, n)
        sc.bounce_device(d_rays, n, d_state, out["bounce"], d_hits=out["hits"], d_next_active=out["next"], d_n_next=out["n_next"])
        sc.collect()
        got = _read_step(dev, d_rays, d_state, out, n)
        for k in ("rays", "states", "bounce", "hits"):
            assert got[k].tobytes() == full[k].tobytes(), (n, k)
        assert got["n_next"] == len(scat) and np.array_equal(np.sort(got["next"][:len(scat)]), scat)
        assert np.all(got["next"][len(scat):] == SENTINEL_U32)

        # (b) a strict subset, shuffled, in a list longer than its device-side length: only the first `used` entries are stepped
        g = np.random.default_rng(n)
        listed = g.permutation(np.arange(0, n, 3) if n > 1 else np.zeros(0, np.int64)).astype(np.uint32)
        used = len(listed) - len(listed) // 4
        stepped = np.sort(listed[:used]).astype(np.int64)
        rest = np.setdiff1d(np.arange(n), stepped)
        results = {}
        for with_next in (True, False):
            d_rays, d_state, out = dev.put(rays), dev.put(st0), _device_outputs(dev, n)
            d_list, d_len = dev.put(listed), dev.put(np.array([used], np.uint32))
            sc.bounce_device(d_rays, n, d_state, out["bounce"], d_hits=out["hits"], d_active=d_list, d_n_active=d_len,
                             d_next_active=out["next"] if with_next else 0, d_n_next=out["n_next"] if with_next else 0)
            st = sc.collect()
            assert st.ray_segments == used and st.n_launches == 1
            results[with_next] = got = _read_step(dev, d_rays, d_state, out, n)
            _assert_step_equals(got, full, stepped, ("subset", n, with_next))
            assert got["rays"][rest].tobytes() == rays[rest].tobytes() and np.array_equal(got["states"][rest], st0[rest])
            for k in ("bounce", "hits"):
                assert set(got[k][rest].tobytes()) <= {FILL}, (n, k, "a record outside the list was written")
        sub = np.intersect1d(scat, stepped)
        got = results[True]
        assert got["n_next"] == len(sub) and np.array_equal(np.sort(got["next"][:len(sub)]), sub)
        assert np.all(got["next"][len(sub):] == SENTINEL_U32)
        # (c) no next list: the step is otherwise identical, and the list and its length are not touched
        for k in ("rays", "states", "bounce", "hits"):
            assert results[False][k].tobytes() == results[True][k].tobytes(), (n, k)
        assert results[False]["n_next"] == 99 and np.all(results[False]["next"] == SENTINEL_U32)

        # (d) a device-side length of 0: n_next is 0 and nothing is written
        d_rays, d_state, out = dev.put(rays), dev.put(st0), _device_outputs(dev, n)
        d_list, d_len = dev.put(np.arange(n, dtype=np.uint32)), dev.put(np.array([0], np.uint32))
        sc.bounce_device(d_rays, n, d_state, out["bounce"], d_hits=out["hits"], d_active=d_list, d_n_active=d_len,
                         d_next_active=out["next"], d_n_next=out["n_next"])
        st = sc.collect()
        got = _read_step(dev, d_rays, d_state, out, n)
        assert got["n_next"] == 0 and st.ray_segments == 0 and st.n_launches == 1
        assert got["rays"].tobytes() == rays.tobytes() and np.array_equal(got["states"], st0)
        assert set(got["bounce"].tobytes()) | set(got["hits"].tobytes()) | set(got["next"].tobytes()) <= {FILL}

        # (e) the host form with an active list: the records outside it come back as they went in
        if len(stepped):
            h = sc.bounce(rays, st0, active=stepped, want_hits=True, want_next=True)
            _assert_step_equals(h, full, stepped, ("host subset", n))
            assert h["rays"][rest].tobytes() == rays[rest].tobytes() and np.array_equal(h["states"][rest], st0[rest])
            assert not any(h["bounce"][rest].tobytes()) and not any(h["hits"][rest].tobytes())
            assert np.array_equal(h["next"], sub) and h["stats"].ray_segments == len(stepped)
        h = sc.bounce(rays, st0, active=[], want_next=True)
        assert len(h["next"]) == 0 and h["stats"].ray_segments == 0 and h["rays"].tobytes() == rays.tobytes()


def test_two_streams_at_once(ndev, big, dev):
    """Two steps on two streams at once give the bytes of one after the other: there is no per-scene scratch."""
    n = 5000
    rays, st0 = big["rays"], big["st0"]
    st_b = B.R.states(n, 901)
    with rt.Scene(0, rt.World(big["sph"], big["tri"], big["wi"])) as sc:
        seq = [sc.bounce(rays, s, flags=f, want_hits=True, want_next=True) for s, f in ((st0, 0), (st_b, F.RT_FLAG_EXACT_SCAN))]
        runs = []
        for s, f in ((st0, 0), (st_b, F.RT_FLAG_EXACT_SCAN)):
            runs.append((dev.put(rays), dev.put(s), _device_outputs(dev, n), dev.stream(), f))
        dev.sync()
        sc.collect()
        for d_rays, d_state, out, stream, f in runs:
            sc.bounce_device(d_rays, n, d_state, out["bounce"], d_hits=out["hits"], d_next_active=out["next"], d_n_next=out["n_next"],
                             flags=f, stream=stream)
        dev.sync()
        st = sc.collect()
        assert st.n_launches == 2 and st.ray_segments == 2 * n
        for (d_rays, d_state, out, _, _), want in zip(runs, seq):
            got = _read_step(dev, d_rays, d_state, out, n)
            for k in ("rays", "states", "bounce", "hits"):
                assert got[k].tobytes() == want[k].tobytes(), k
            assert np.array_equal(np.sort(got["next"][:got["n_next"]]), want["next"])


# ---------------------------------------------------------------- 4. errors and the plain-C client
def test_argument_errors_launch_nothing(ndev, cases):
    lib = _abi.load()
    sph, tri, wi, rays, st0 = cases["spheres"]
    with rt.Scene(0, rt.World(sph, tri, wi)) as sc:
        sc.collect()
        for what, status in bad_arg_calls(lib, sc._h):
            assert status == _abi.RT_ERR_BAD_ARG, what
        st = sc.collect()
        assert st.n_launches == 0 and st.ray_segments == 0
        with pytest.raises(ValueError):
            sc.bounce(rays, st0[:-1])
        with pytest.raises(ValueError):
            sc.bounce(rays, None)
        with pytest.raises(_abi.RtError):
            sc.bounce(rays, st0, active=[len(rays)])
        assert sc.bounce(rays, st0)["stats"].n_launches == 1                # the scene still works


def test_plain_c_bounce_client(ndev, tmp_path):
    """examples/bounce_rays.c through the C-ABI only: K host-form steps with the active list, folded right to left, against
    rt_scene_trace of the same rays and states."""
    exe = tmp_path / "bounce_rays"
    lib = _abi.lib_path().parent
    r = subprocess.run([shutil.which("gcc"), "-std=c99", "-O2", "-Wall", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "bounce_rays.c"),
                        f"-L{lib}", "-lrt_s8", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "BOUNCE_OK" in run.stdout, run.stdout + run.stderr
