"""The film sampler on the GPU (ray_tracer_s8_amd/film_sampler.py, sampler_csrc/), bytes compared throughout:
1. rts_select on uploaded moments and counts with no scene: one pixel, one strip, three strips with a partial last workgroup, two
   strips whose scan spans many workgroups; no pixel noisy, all, the first only, the last only, seeded random; dilate 0 and 1; lists,
   counts and err equal tests/_sampler_np.py;
2. rts_gather and rts_fold at 0, 1, 63 and 257 active pixels and 1 and 3 samples, on adversarial records, into strip views of
   frame-shaped tensors; pixels that are not active keep their bytes;
3. on the glossy room of tests/test_gpu_film.py, "nee" MIS and "path", a floor of 4 of 12 samples and rounds of (4, 4) and (1, 3, 4)
   under a threshold that is the median error after the floor: after every round the lists, counts, accum and moments equal the
   restatement run over the host composition's per-(pixel, sample) records; an always active pixel has a uniform film's bytes, a
   never active one the floor's; the film itself is untouched; a max_records that forces sub-ranges gives the same bytes;
4. threshold = inf samples nothing and every resolve is the film's own; after rounds, the normalised sums equal the restatement and
   resolve_guided and variance equal tests/_film_np.py on them;
5. refused calls change nothing;
6. examples/film_adaptive.py writes its three files.
Every body runs in a child process that imports torch first.  Without the feature every test here fails: there is no rt.FilmSampler.
No timing is asserted."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _direct_np as D

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

_PRELUDE = r"""
import sys
import numpy as np
import torch                                                      # first: the libraries then bind to torch's HIP runtime
sys.path.insert(0, "tests")
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, _sampler_lib as sl, film as film_mod, film_sampler, scenes
import _film_np as fnp
import _sampler_np as snp

f32 = np.float32

def host(film, t):
    film.sync()                                                   # (.cpu() copies on torch's current stream, not the film's)
    return t.cpu().numpy()

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).tobytes() if a.dtype == np.float32 else a.tobytes()

def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if bits(got) != bits(want):
        g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
        bad = np.argwhere(g != w)
        raise AssertionError((what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))

def refused(call, *a, **kw):
    try:
        call(*a, **kw)
    except ValueError:
        return True
    return False

def lists_of(sampler):
    # the strips' lists as the sampler holds them after a select: uint32 strip indices
    P = sampler.film.hs * sampler.film.width
    act = host(sampler.film, sampler.active).view(np.uint32)
    return [act[i * P:i * P + n].copy() for i, n in enumerate(sampler.last_active)]
"""


def _child(body, *args, timeout=600):
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body, *map(str, args)], capture_output=True, text=True, cwd=ROOT,
                       timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    """The glossy room of tests/test_gpu_film.py."""
    path = tmp_path_factory.mktemp("film_sampler") / "room.npz"
    sph, tri = D.lit_room()
    sph["roughness"][:4] = [0.5, 0.0, 0.5, 1.0]
    np.savez(path, sph=sph, tri=tri)
    return path


# ------------------------------------------------------------------------------------------- 1. the select, no scene

_SELECT_CHILD = r"""
W, R, HS = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
lib = sl.load()
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
P, strips = HS * W, R // HS
SENTINEL = 0x7FFFFFFF

def run(M, counts, thr, dilate, eps, what):
    with torch.cuda.stream(stream):
        mom, cnt = torch.from_numpy(M).to(dev), torch.from_numpy(counts).to(dev)
        err = torch.full((R, W), 7.0, dtype=torch.float32, device=dev)
        active = torch.full((R * W,), SENTINEL, dtype=torch.int32, device=dev)
        sc = torch.full((strips,), SENTINEL, dtype=torch.int32, device=dev)
        scratch = torch.empty(sl.scratch_bytes(W, R, HS), dtype=torch.uint8, device=dev)
        a = sl.SelectArgs(W=W, R=R, Hs=HS, dilate=dilate, threshold=float(thr), eps=eps, moments=mom.data_ptr(), counts=cnt.data_ptr(),
                          err=err.data_ptr(), active=active.data_ptr(), strip_counts=sc.data_ptr(), scratch=scratch.data_ptr(),
                          scratch_bytes=scratch.numel())
        sl.check("rts_select", lib.rts_select(a, stream.cuda_stream))
    stream.synchronize()
    err, active, sc = err.cpu().numpy(), active.cpu().numpy().view(np.uint32), sc.cpu().numpy().view(np.uint32)
    werr, wlists, wsc = snp.select(M, counts, HS, thr, dilate, eps)
    same(err, werr, (what, "err"))
    same(sc, wsc, (what, "strip counts"))
    for i, w in enumerate(wlists):
        same(active[i * P:i * P + len(w)], w, (what, "list", i))
        assert (active[i * P + len(w):(i + 1) * P] == SENTINEL).all(), (what, "behind the list", i)
    return int(wsc.sum())

rng = np.random.default_rng(1000 * R + W)
for name in ("none", "all", "first", "last", "random"):
    flags = snp.pattern(name, rng, R, W)
    M, counts, thr, eps = snp.moments_for(flags)
    for dilate in (0, 1):
        n = run(M, counts, thr, dilate, eps, (name, dilate))
        assert dilate or n == int(flags.sum())
        assert n == {"none": 0, "all": R * W}.get(name, n)
# seeded sums at mixed counts around the median of their error, and the adversarial image's sums tiled over this one
counts = rng.integers(2, 30, (R, W)).astype(np.int32)
M = snp.moments_of(rng, R, W, counts)
thr = np.median(snp.pixel_error(M, counts, 2.0 ** -6))
aM, an, aeps = snp.adversarial()
tM = np.ascontiguousarray(np.tile(aM, (R // 6 + 1, W // 8 + 1, 1))[:R, :W])
tn = np.ascontiguousarray(np.tile(an, (R // 6 + 1, W // 8 + 1))[:R, :W])
for dilate in (0, 1):
    n = run(M, counts, thr, dilate, 2.0 ** -6, ("seeded", dilate))
    assert R * W == 1 or 0 < n and (dilate or n < R * W)
    run(tM, tn, f32(0.05), dilate, aeps, ("adversarial", dilate))
    assert run(tM, tn, f32(np.inf), dilate, aeps, ("adversarial, inf", dilate)) == 0
print("ok")
"""


@pytest.mark.parametrize("W,R,hs", [(1, 1, 1), (70, 9, 9), (50, 48, 16), (130, 70, 35)])
def test_select_on_synthetic_moments(ndev, W, R, hs):
    _child(_SELECT_CHILD, W, R, hs)


# ------------------------------------------------------------------------------------------- 2. gather and fold, no scene

_GATHER_FOLD_CHILD = r"""
lib = sl.load()
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
W, HS, STRIPS = 30, 10, 3
P = W * HS
rng = np.random.default_rng(0x6A7)
for n_active in (0, 1, 63, 257):
    for k in (1, 3):
        act = np.sort(rng.permutation(P)[:n_active]).astype(np.uint32)
        if n_active >= 2:
            act[0], act[-1] = 0, P - 1                                      # the strip's first and last pixel
        rays = rng.integers(0, 256, (P * k, 32)).astype(np.uint8)
        states = rng.integers(0, 256, (P * k, 32)).astype(np.uint8)
        rgb = fnp.adversarial_records(max(n_active, 1), k)[:n_active].reshape(-1, 3)
        acc0 = fnp.adversarial_records(STRIPS * P, 1, seed=3)[:, 0].reshape(STRIPS * HS, W, 3).copy()
        mom0 = rng.standard_normal((STRIPS * HS, W, 2)).astype(f32)
        cnt0 = rng.integers(2, 50, (STRIPS * HS, W)).astype(np.int32)
        with torch.cuda.stream(stream):
            d_act = torch.from_numpy(np.concatenate([act, np.zeros(1, np.uint32)]).view(np.int32)).to(dev)
            d_rays, d_states = torch.from_numpy(rays).to(dev), torch.from_numpy(states).to(dev)
            o_rays = torch.full((P * k, 32), 0xAB, dtype=torch.uint8, device=dev)
            o_states = torch.full((P * k, 32), 0xCD, dtype=torch.uint8, device=dev)
            d_rgb = torch.from_numpy(np.concatenate([rgb, np.ones((1, 3), f32)])).to(dev)
            acc, mom, cnt = torch.from_numpy(acc0).to(dev), torch.from_numpy(mom0).to(dev), torch.from_numpy(cnt0).to(dev)
            g = sl.GatherArgs(n_active=n_active, k=k, pixels=P, active=d_act.data_ptr(), rays=d_rays.data_ptr(),
                              states=d_states.data_ptr(), out_rays=o_rays.data_ptr(), out_states=o_states.data_ptr())
            sl.check("rts_gather", lib.rts_gather(g, stream.cuda_stream))
            # strip 1's view of the frame-shaped tensors
            f = sl.FoldArgs(n_active=n_active, k=k, pixels=P, active=d_act.data_ptr(), rgb=d_rgb.data_ptr(),
                            accum=acc[HS:2 * HS].data_ptr(), moments=mom[HS:2 * HS].data_ptr(), counts=cnt[HS:2 * HS].data_ptr())
            sl.check("rts_fold", lib.rts_fold(f, stream.cuda_stream))
        stream.synchronize()
        o_rays, o_states = o_rays.cpu().numpy(), o_states.cpu().numpy()
        n = n_active * k
        same(o_rays[:n], snp.gather(act, k, rays), ("rays", n_active, k))
        same(o_states[:n], snp.gather(act, k, states), ("states", n_active, k))
        assert (o_rays[n:] == 0xAB).all() and (o_states[n:] == 0xCD).all()
        same(d_rays.cpu().numpy(), rays, "the strip's rays")
        acc, mom, cnt = acc.cpu().numpy(), mom.cpu().numpy(), cnt.cpu().numpy()
        wa, wm, wc = snp.fold(acc0[HS:2 * HS].reshape(P, 3), mom0[HS:2 * HS].reshape(P, 2), cnt0[HS:2 * HS].reshape(P), act, rgb, k)
        want_acc, want_mom, want_cnt = acc0.copy(), mom0.copy(), cnt0.copy()
        want_acc[HS:2 * HS], want_mom[HS:2 * HS], want_cnt[HS:2 * HS] = wa.reshape(HS, W, 3), wm.reshape(HS, W, 2), wc.reshape(HS, W)
        same(acc, want_acc, ("accum", n_active, k))
        same(mom, want_mom, ("moments", n_active, k))
        same(cnt, want_cnt, ("counts", n_active, k))
        idle = np.ones(P, bool)
        idle[act.astype(int)] = False                                       # untouched pixels keep their bytes
        same(acc[HS:2 * HS].reshape(P, 3)[idle], acc0[HS:2 * HS].reshape(P, 3)[idle], "idle accum")
        assert (cnt[HS:2 * HS].reshape(P)[~idle] == cnt0[HS:2 * HS].reshape(P)[~idle] + k).all()
print("ok")
"""


def test_gather_and_fold_on_adversarial_records(ndev):
    _child(_GATHER_FOLD_CHILD)


# ------------------------------------------------------------------------------------------- 3. rounds on the glossy room

_SCENE = r"""
room = np.load(sys.argv[1])
integrator = sys.argv[2]
W, H, DIV, SPP, MB, FLOOR = 48, 36, 3, 12, 3, 4
EPS = f32(film_sampler.EPS)
rqs = [_abi.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=MB, seed=0x5A3F) for k in range(DIV)]
hs = H // DIV
pixels = hs * W

def composition(sc):
    # the integrator's colour of every (pixel, sample), from the host calls: (H, W, SPP, 3)
    out = []
    for rq in rqs:
        rays, states, _ = sc.camera_rays(rq, 0, SPP)
        o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)
        d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)
        kw = dict(spp=1, max_bounces=MB, rng_state=states, as_given=True)
        if integrator == "nee":
            rgb = sc.trace_nee(o, d, rays["t_min"], rays["t_max"], mode=_abi.RT_NEE_MIS, **kw)[0]
        else:
            rgb = sc.trace(o, d, rays["t_min"], rays["t_max"], **kw)[0]
        out.append(rgb.reshape(hs, W, SPP, 3))
    return np.concatenate(out)

def scene():
    sc = rt.Scene(0, rt.World(room["sph"], room["tri"]))
    sc.set_light_sampling(_abi.RT_LIGHTS_CONE)
    sc.set_glossy_sampling(_abi.RT_GLOSSY_MIS)
    return sc

def floor_threshold(film):
    # the median of the error plane after the floor, from the downloaded moments with numpy
    err = snp.pixel_error(host(film, film.moments), np.full((H, W), FLOOR, np.int32), EPS)
    return f32(np.median(err))
"""

_ROUNDS_CHILD = _SCENE + r"""
with scene() as sc:
    records = composition(sc)
    assert np.isfinite(records).all()
    with rt.Film(sc, rqs, integrator=integrator, moments=True) as film, rt.Film(sc, rqs, integrator=integrator, moments=True) as uni, \
            rt.Film(sc, rqs, integrator=integrator, moments=True, max_records=pixels) as cut:
        assert cut.k == 1 and film.k == SPP
        film.render_pass(0, FLOOR)
        film.sync()
        cut.render_pass(0, FLOOR)
        cut.sync()
        floor = dict(accum=host(film, film.accum).copy(), moments=host(film, film.moments).copy())
        thr = floor_threshold(film)
        for dilate in (0, 1):
            for schedule in ((4, 4), (1, 3, 4)):
                want = snp.Rounds(records, hs, FLOOR, thr, dilate, EPS)
                same(want.accum, floor["accum"], "the floor")
                same(want.moments, floor["moments"], "the floor's moments")
                uni.reset()
                uni.render_pass(0, FLOOR)
                uni.sync()
                with rt.FilmSampler(film, threshold=float(thr), dilate=dilate) as sampler, \
                        rt.FilmSampler(cut, threshold=float(thr), dilate=dilate) as sampler_cut:
                    sampler.begin()
                    sampler_cut.begin()
                    assert sampler.samples == FLOOR and (host(film, sampler.counts) == FLOOR).all()
                    always, never = np.ones((H, W), bool), np.ones((H, W), bool)
                    for r, n in enumerate(schedule):
                        got_n = sampler.render_pass(n)
                        want_n = want.render_pass(n)
                        what = (dilate, schedule, r)
                        assert got_n == want_n and sampler.samples == want.samples, (what, got_n, want_n)
                        if r == 0 and dilate == 0:
                            assert 0 < got_n < H * W, (what, got_n)              # a condition of the test: the selection is not trivial
                        assert got_n > 0, what
                        assert sampler.active_fraction == got_n / (H * W)
                        for i, (g, w) in enumerate(zip(lists_of(sampler), want.lists)):
                            same(g, w, (what, "list", i))
                        same(host(film, sampler.error), want.err, (what, "err"))
                        same(host(film, sampler.counts), want.counts, (what, "counts"))
                        same(host(film, sampler.accum), want.accum, (what, "accum"))
                        same(host(film, sampler.moments), want.moments, (what, "moments"))
                        act = np.zeros((H, W), bool)
                        for i, l in enumerate(want.lists):
                            act[i * hs:(i + 1) * hs].reshape(-1)[l.astype(int)] = True
                        always &= act
                        never &= ~act
                        uni.render_pass(uni.samples, want.samples)
                        ua, um = host(uni, uni.accum), host(uni, uni.moments)
                        ga, gm = host(film, sampler.accum), host(film, sampler.moments)
                        same(ga[always], ua[always], (what, "always active: the uniform film's accum"))
                        same(gm[always], um[always], (what, "always active: the uniform film's moments"))
                        same(ga[never], floor["accum"][never], (what, "never active: the floor's accum"))
                        same(gm[never], floor["moments"][never], (what, "never active: the floor's moments"))
                        assert (want.counts[always] == want.samples).all() and (want.counts[never] == FLOOR).all()
                        # the film is the floor still
                        assert film.samples == FLOOR
                        same(host(film, film.accum), floor["accum"], (what, "the film's accum"))
                        same(host(film, film.moments), floor["moments"], (what, "the film's moments"))
                        # one sample index a launch: the same bytes
                        assert sampler_cut.render_pass(n) == got_n
                        same(host(cut, sampler_cut.accum), ga, (what, "accum under max_records"))
                        same(host(cut, sampler_cut.moments), gm, (what, "moments under max_records"))
                        same(host(cut, sampler_cut.counts), want.counts, (what, "counts under max_records"))
                    assert sampler.samples == SPP and sampler.render_pass(1) == 0 and sampler.samples == SPP    # the indices ran out
                    assert always.any() and (dilate or never.any())
            # render(): rounds until nothing is active or the indices run out; the same sums as the rounds one by one
            want = snp.Rounds(records, hs, FLOOR, thr, 1, EPS)
            rounds = 0
            while want.render_pass(3):
                rounds += 1
            with rt.FilmSampler(film, threshold=float(thr)) as sampler:
                sampler.begin()
                assert sampler.render(3) == rounds == sampler.rounds
                same(host(film, sampler.accum), want.accum, "render() accum")
                same(host(film, sampler.counts), want.counts, "render() counts")
        assert film.collect().n_launches > 0
print("ok")
"""


@pytest.mark.parametrize("integrator", ["nee", "path"])
def test_rounds_equal_the_restatement_over_the_host_composition(ndev, room, integrator):
    _child(_ROUNDS_CHILD, room, integrator)


# ------------------------------------------------------------------------------------------- 4. the resolves

_RESOLVE_CHILD = _SCENE + r"""
OUTPUTS = ("rgb", "linear", "f32", "variance")
DEFAULTS = dict(sigma_l=f32(film_mod.SIGMA_L), var_eps=f32(film_mod.VAR_EPS), k_normal=f32(1.0), k_depth=f32(4.0))
with scene() as sc:
    with rt.Film(sc, rqs, integrator=integrator, moments=True) as film:
        film.render_pass(0, FLOOR)
        planes = film.features(2)
        guide = {n: planes[n] for n in ("normal", "depth", "hits")}
        got = {n: host(film, t) for n, t in planes.items()}
        np_guide = dict(N=got["normal"], D=got["depth"], hits=got["hits"].view(np.uint32))
        keep = lambda d: {o: host(film, t).copy() for o, t in d.items()}
        own = dict(resolve=keep(film.resolve(planes=guide, outputs=("rgb", "linear", "f32"))), preview=keep(film.preview(("rgb", "f32"))),
                   guided=keep(film.resolve_guided(guide, OUTPUTS)), variance=host(film, film.variance()).copy())
        # threshold = inf: nothing is sampled, and every resolve is the film's own
        with rt.FilmSampler(film, threshold=float("inf")) as sampler:
            sampler.begin()
            assert sampler.render_pass(4) == 0 and sampler.samples == FLOOR and sampler.render(4) == 0 and sampler.active_fraction == 0.0
            assert (host(film, sampler.counts) == FLOOR).all()
            na, nm = sampler.normalised()
            same(host(film, na), host(film, film.accum), "normalised accum at the floor")
            same(host(film, nm), host(film, film.moments), "normalised moments at the floor")
            for o, w in own["resolve"].items():
                same(host(film, sampler.resolve(planes=guide, outputs=(o,))[o]), w, ("resolve", o))
            for o, w in own["preview"].items():
                same(host(film, sampler.preview((o,))[o]), w, ("preview", o))
            for o, w in own["guided"].items():
                same(host(film, sampler.resolve_guided(guide, (o,))[o]), w, ("resolve_guided", o))
            same(host(film, sampler.variance()), own["variance"], "variance")
        # after rounds: the normalised sums are the restatement's, and the film's resolves on them are _film_np's
        thr = floor_threshold(film)
        with rt.FilmSampler(film, threshold=float(thr), dilate=0) as sampler:
            sampler.begin()
            assert 0 < sampler.render_pass(3) < H * W and sampler.render_pass(5) > 0
            acc, mom, cnt = host(film, sampler.accum), host(film, sampler.moments), host(film, sampler.counts)
            assert cnt.min() == FLOOR and cnt.max() == SPP and set(np.unique(cnt)) <= {FLOOR, FLOOR + 3, FLOOR + 5, SPP}
            na, nm = sampler.normalised()
            na, nm = host(film, na).copy(), host(film, nm).copy()
            wa, wm = snp.normalise(acc, mom, cnt, FLOOR)
            same(na, wa, "normalised accum")
            same(nm, wm, "normalised moments")
            at = cnt == FLOOR
            same(na[at], acc[at], "a pixel at the film's count")
            var = host(film, sampler.variance()).copy()
            same(var, fnp.entry_variance(nm, FLOOR), "variance()")
            v_true = snp.true_variance(mom, cnt)
            assert (np.abs(var.astype(np.float64) - v_true) <= snp.variance_bound(v_true, nm, FLOOR)).all()   # rt_sampler.h's bound
            assert bits(var) != bits(own["variance"])
            for it, g in ((0, {}), (3, np_guide), (5, {})):
                out = sampler.resolve_guided(guide if g else None, OUTPUTS, iterations=it)
                want = fnp.resolve(na, nm, FLOOR, iterations=it, **DEFAULTS, **g)
                for o in OUTPUTS:
                    same(host(film, out[o]), want[o], ("resolve_guided", it, bool(g), o))
            want = fnp.resolve(na, nm, FLOOR, iterations=0, **DEFAULTS)
            prev = sampler.preview(("rgb", "f32"))
            same(host(film, prev["rgb"]), want["rgb"], "preview rgb")
            same(host(film, prev["f32"]), want["f32"], "preview f32")
            res = sampler.resolve(planes=guide, outputs=("f32",))
            mine = host(film, res["f32"]).copy()
            same(mine, host(film, film.resolve(None, guide, ("f32",), _state=sampler.normalised())["f32"]), "resolve")
            assert bits(mine) != bits(own["resolve"]["f32"])
print("ok")
"""


def test_resolves_on_the_normalised_sums(ndev, room):
    _child(_RESOLVE_CHILD, room, "nee")


# ------------------------------------------------------------------------------------------- 5. discipline

_DISCIPLINE_CHILD = _SCENE + r"""
with scene() as sc:
    with rt.Film(sc, rqs, integrator=integrator) as plain:
        assert refused(rt.FilmSampler, plain)                                        # a film without moments
    with rt.Film(sc, rqs, integrator=integrator, moments=True) as film:
        for kw in (dict(threshold=-1.0), dict(threshold=float("nan")), dict(dilate=2), dict(eps=0.0), dict(eps=float("inf"))):
            assert refused(rt.FilmSampler, film, **kw), kw
        sampler = rt.FilmSampler(film, threshold=0.0)
        state = lambda: (sampler.samples, film.samples, bits(host(film, sampler.accum)), bits(host(film, sampler.moments)),
                         bits(host(film, sampler.counts)), bits(host(film, film.accum)), bits(host(film, film.moments)))
        s0 = state()
        assert refused(sampler.begin) and refused(sampler.render_pass, 1) and refused(sampler.resolve) and refused(sampler.variance)
        film.render_pass(0, 1)
        s1 = state()
        assert refused(sampler.begin) and refused(sampler.render_pass, 1)            # one sample is no floor
        assert state() == s1 and s1[:1] == s0[:1]
        film.render_pass(1, FLOOR)
        sampler.begin()
        s4 = state()
        for n in (0, -1, True, 1.5, None, "4"):
            assert refused(sampler.render_pass, n), n
            assert state() == s4, n
        assert sampler.render_pass(2) > 0                                            # threshold 0: every pixel with a spread
        s6 = state()
        assert s6[2] != s4[2] and s6[5:] == s4[5:] and sampler.samples == FLOOR + 2
        # the film moved on: the sampler's floor is stale until begin() again
        film.render_pass(FLOOR, FLOOR + 1)
        s_moved = state()
        assert refused(sampler.render_pass, 1) and refused(sampler.resolve) and refused(sampler.resolve_guided) and refused(sampler.variance)
        assert state() == s_moved
        sampler.begin()
        assert sampler.samples == FLOOR + 1 and sampler.rounds == 0
        same(host(film, sampler.accum), host(film, film.accum), "begin() again")
        sampler.reset()
        assert refused(sampler.render_pass, 1) and sampler.samples == 0
        sampler.begin()
        assert sampler.render(64) == 1 and sampler.samples == SPP and sampler.render_pass(1) == 0
        sampler.close()
        sampler.close()
        assert sampler.accum is None and refused(sampler.begin) and refused(sampler.render_pass, 1) and refused(sampler.resolve)
        assert film.accum is not None and film.samples == FLOOR + 1
    with rt.Film(sc, rqs, integrator=integrator, moments=True) as film:
        film.render_pass(0, 2)
        with rt.FilmSampler(film) as sampler:
            sampler.begin()
        assert sampler.accum is None
        sampler = rt.FilmSampler(film)
        sampler.begin()
    assert refused(sampler.render_pass, 1)                                           # the film is closed
print("ok")
"""


def test_refused_calls_change_nothing(ndev, room):
    _child(_DISCIPLINE_CHILD, room, "nee")


# ------------------------------------------------------------------------------------------- 6. the example

_EXAMPLE_CHILD = r"""
import runpy
out_dir, example = sys.argv[1], sys.argv[2]
sys.argv = [example, out_dir, "--width", "64", "--height", "36", "--divisions", "2", "--spp", "10", "--floor", "4", "--round", "3",
            "--threshold", "0.1"]
runpy.run_path(example, run_name="__main__")
got = {n: np.load(f"{out_dir}/{n}.npy") for n in ("resolve", "counts", "err")}
assert got["resolve"].shape == (36, 64, 3) and got["resolve"].dtype == np.uint8
assert got["counts"].shape == (36, 64) and got["counts"].dtype == np.int32 and got["err"].shape == (36, 64) and got["err"].dtype == np.float32
assert got["counts"].min() >= 4 and got["counts"].max() <= 10 and set(np.unique(got["counts"])) <= {4, 7, 10}
assert got["counts"].max() > 4 and got["resolve"].std() > 1
sph, rq = scenes.config("c2")
rqs = [_abi.default_request(width=64, height=36, divisions=2, division_no=k, spp=10, max_bounces=rq.max_bounces, seed=rq.seed) for k in range(2)]
with rt.Scene(0, rt.World(sph)) as sc:
    sc.set_light_sampling(_abi.RT_LIGHTS_CONE)
    sc.set_glossy_sampling(_abi.RT_GLOSSY_MIS)
    with rt.Film(sc, rqs, integrator="nee", moments=True) as film, rt.FilmSampler(film, threshold=0.1) as sampler:
        film.render_pass(0, 4)
        sampler.begin()
        sampler.render(3)
        planes = film.features(1)
        out = sampler.resolve_guided({n: planes[n] for n in ("normal", "depth", "hits")})
        same(host(film, out["rgb"]), got["resolve"], "resolve.npy")
        same(host(film, sampler.counts), got["counts"], "counts.npy")
        same(host(film, sampler.error), got["err"], "err.npy")
print("ok")
"""


def test_example_film_adaptive(ndev, tmp_path):
    _child(_EXAMPLE_CHILD, tmp_path, ROOT / "examples" / "film_adaptive.py")
