"""The a-trous denoiser on the GPU (rt_scene_denoise, rt_scene_denoise_device), bit for bit against the numpy restatement of rt_tile.h
(tests/_denoise_np.py) throughout:
1. synthetic images (sizes of 1 .. 3 and odd ones, sky and partial hits, zero normals and albedo channels, fireflies) under every
   combination of planes and several iteration counts and k, through the host form (here) and the device form (child process);
2. real inputs: the progressive accum and render_aov planes of c2, c3, quad_room and a terrain strip, at e != k;
3. the anchor to the renderer: no iteration and no albedo give the progressive pass's preview, at e = S and at e < S;
4. strips: a frame as n strips equals it as one strip, a run of middle strips equals the restatement on their union, 66 strips;
5. host form == device form, two streams with their own scratch, repeated calls;
6. quality with the defaults: half the MSE of the noisy mean against a 1024-spp render, on c2 and quad_room;
7. argument errors, with the outputs untouched; a scratch one byte short."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _denoise_np as dn
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes
from test_denoise_host import synthetic

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
OUTS = ("rgb", "linear", "f32")


def _eq(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype == np.uint8:
        bad = np.argwhere(a != b)
    else:
        bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert len(bad) == 0, (what, len(bad), bad[:4], a[tuple(bad[0])], b[tuple(bad[0])])


def _dq(**kw):
    return _abi.DenoiseRequest.defaults(**kw)


def _np_kw(dq):
    return dict(iterations=dq.iterations, k_color=f32(dq.k_color), color_step_scale=f32(dq.color_step_scale),
                k_normal=f32(dq.k_normal), k_depth=f32(dq.k_depth), albedo_eps=f32(dq.albedo_eps))


def _split(a, n):
    return list(np.split(a, n, axis=0))


def _strip_planes(s, names, n):
    """the per-strip plane dicts of a synthetic image stacked from n strips"""
    parts = {k: _split(s[k], n) for k in names}
    return [{k: parts[k][i] for k in names} for i in range(n)]


def _np_planes(s, names):
    m = {"albedo": "A", "normal": "N", "depth": "D", "hits": "hits"}
    return {m[k]: s[k] for k in names}


@pytest.fixture(scope="module")
def scene(ndev):
    with rt.Scene(0, rt.World(scenes.single_sphere())) as sc:
        yield sc


def _frame(W, R, n):
    return [_abi.default_request(width=W, height=R, divisions=n, division_no=i, spp=16, seed=3) for i in range(n)]


PLANE_SETS = [(), ("albedo",), ("normal",), ("hits",), ("depth", "hits"), ("albedo", "normal"), ("normal", "depth", "hits"),
              ("albedo", "normal", "depth", "hits")]


@pytest.mark.parametrize("R,W,n", [(1, 1, 1), (2, 3, 1), (3, 2, 1), (3, 1, 3), (12, 67, 4), (40, 129, 2)])
@pytest.mark.parametrize("names", PLANE_SETS)
def test_synthetic_images_equal_the_restatement(scene, R, W, n, names):
    rng = np.random.default_rng(R * 7919 + W * 31 + n + len(names))
    s = synthetic(rng, R, W)
    s = {"C": s["C"], "albedo": s["A"], "normal": s["N"], "depth": s["D"], "hits": s["hits"]}
    for it, kc, kn, kd in [(0, 1.0, 4.0, 16.0), (1, 1.0, 4.0, 16.0), (3, 0.5, 2.0, 8.0), (5, 1.0, 4.0, 16.0), (8, 1.0, 4.0, 16.0),
                           (3, 0.0, 0.0, 0.0), (2, 1e6, 1e6, 1e6)]:
        dq = _dq(iterations=it, k_color=kc, k_normal=kn, k_depth=kd)
        got, st = scene.denoise(_frame(W, R, n), _split(s["C"], n), _strip_planes(s, names, n), 8, 4, dq, outputs=OUTS)
        want = dn.denoise(s["C"], 8, k=4, **_np_planes(s, names), **_np_kw(dq))
        for o in OUTS:
            _eq(np.concatenate([g[o] for g in got], 0), want[o], (R, W, n, names, it, kc, o))
        assert st.n_launches >= 2 and st.kernel_ms > 0 and st.ray_segments == 0 and st.primary_rays == 0 and st.engine == 0


def _render(sc, rq, e, k):
    """beauty accum after [0, e) of rq.spp and the planes after [0, k)"""
    _, _, acc, _ = sc.render_tile_pass(rq, 0, e)
    planes, _ = sc.render_aov(rq, 0, k, planes=("albedo", "normal", "depth", "hits"))
    return acc, planes


def _real(name):
    if name in ("c2", "c3"):
        return scenes.config(name)[0], None
    return scenes.quad_room() if name == "quad_room" else scenes.tri_terrain()


@pytest.mark.parametrize("name", ["c2", "c3", "quad_room", "terrain"])
def test_real_inputs_equal_the_restatement(ndev, name):
    sph, tri = _real(name)
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        rq = _abi.default_request(width=96, height=64, divisions=4, division_no=2, spp=16, max_bounces=6, seed=0xD0E5)
        acc, planes = _render(sc, rq, 16, 4)
        for dq in (_dq(), _dq(iterations=3, k_color=0.25, k_normal=1.0, k_depth=4.0)):
            got, _ = sc.denoise(rq, acc, planes, 16, 4, dq, outputs=OUTS)
            want = dn.denoise(acc, 16, A=planes["albedo"], k=4, N=planes["normal"], D=planes["depth"], hits=planes["hits"],
                              **_np_kw(dq))
            for o in OUTS:
                _eq(got[o], want[o], (name, dq.iterations, o))


def test_no_iteration_is_the_progressive_preview(ndev):
    sph, rq = scenes.config("c2")
    rq.width, rq.height, rq.divisions, rq.division_no, rq.spp = 80, 48, 2, 1, 12
    with rt.Scene(0, rt.World(sph)) as sc:
        planes, _ = sc.render_aov(rq, 0, 3, planes=("normal", "depth", "hits"))
        for e in (5, 12):                                                   # e < S, e = S
            rgb, f, acc, _ = sc.render_tile_pass(rq, 0, e, want_f32=True)
            for pl in ({}, planes):
                got, _ = sc.denoise(rq, acc, pl, e, 3, _dq(iterations=0), outputs=OUTS)
                _eq(got["f32"].ravel(), f, ("f32", e, len(pl)))
                _eq(got["rgb"].ravel(), rgb, ("rgb", e, len(pl)))


def test_strips_equal_one_strip_and_the_union(scene):
    rng = np.random.default_rng(21)
    W, R, n = 37, 64, 8
    s = synthetic(rng, R, W)
    s = {"C": s["C"], "albedo": s["A"], "normal": s["N"], "depth": s["D"], "hits": s["hits"]}
    names = ("albedo", "normal", "depth", "hits")
    dq = _dq()
    whole, _ = scene.denoise(_frame(W, R, 1)[0], s["C"], {k: s[k] for k in names}, 8, 4, dq, outputs=OUTS)
    strips, _ = scene.denoise(_frame(W, R, n), _split(s["C"], n), _strip_planes(s, names, n), 8, 4, dq, outputs=OUTS)
    for o in OUTS:
        _eq(np.concatenate([g[o] for g in strips], 0), whole[o], ("strips", o))
    # strips 2, 3, 4 of 8: the restatement on their 24 rows (their top and bottom rows are borders)
    mid, _ = scene.denoise(_frame(W, R, n)[2:5], _split(s["C"], n)[2:5], _strip_planes(s, names, n)[2:5], 8, 4, dq, outputs=OUTS)
    rows = slice(16, 40)
    want = dn.denoise(s["C"][rows], 8, k=4, **_np_planes({k: s[k][rows] for k in names}, names), **_np_kw(dq))
    for o in OUTS:
        _eq(np.concatenate([g[o] for g in mid], 0), want[o], ("middle", o))


def test_66_strips_in_one_call(scene):
    rng = np.random.default_rng(66)
    W, n = 9, 66
    R = 2 * n
    s = synthetic(rng, R, W)
    s = {"C": s["C"], "albedo": s["A"], "normal": s["N"], "depth": s["D"], "hits": s["hits"]}
    names = ("albedo", "normal", "depth", "hits")
    dq = _dq(iterations=6)
    got, st = scene.denoise(_frame(W, R, n), _split(s["C"], n), _strip_planes(s, names, n), 8, 4, dq, outputs=OUTS)
    want = dn.denoise(s["C"], 8, k=4, **_np_planes(s, names), **_np_kw(dq))
    for o in OUTS:
        _eq(np.concatenate([g[o] for g in got], 0), want[o], ("66", o))
    bands = (n + 31) // 32
    assert st.n_launches == bands + 5 + bands, st.n_launches


def _mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("name", ["c2", "quad_room"])
def test_quality_with_the_defaults(ndev, name):
    """c2's camera at 192 x 108: 4 spp beauty and planes over [0, 4) against a 1024-spp render of another seed (the reference
    linear mean).  The denoised linear mean has at most half the MSE of the noisy one (DESIGN.md 4.14 records the ratios)."""
    sph, tri = _real(name)
    _, rq = scenes.config("c2")
    rq.width, rq.height, rq.divisions, rq.division_no = 192, 108, 1, 0
    with rt.Scene(0, rt.World(sph, tri)) as sc:
        rq.spp = 4
        acc, planes = _render(sc, rq, 4, 4)
        ref_rq = _abi.TileRequest.from_buffer_copy(rq)
        ref_rq.spp, ref_rq.seed = 1024, rq.seed ^ 0x5A5A5A5A
        _, _, ref_acc, _ = sc.render_tile_pass(ref_rq, 0, 1024)
        ref = ref_acc / f32(1024)
        got, _ = sc.denoise(rq, acc, planes, 4, 4, None, outputs=("linear",))
    noisy = acc / f32(4)
    ratio = _mse(noisy, ref) / _mse(got["linear"], ref)
    print(f"{name}: MSE noisy {_mse(noisy, ref):.5g}  denoised {_mse(got['linear'], ref):.5g}  ratio {ratio:.2f}")
    assert ratio >= 2.0, ratio


def test_argument_errors_leave_the_outputs_alone(scene):
    rng = np.random.default_rng(3)
    W, R = 16, 8
    s = synthetic(rng, R, W)
    rq = _frame(W, R, 1)[0]
    lib = scene._lib
    n = 1
    acc = np.ascontiguousarray(s["C"])
    out = np.full((R, W, 3), 77, np.uint8)
    outf = np.full((R, W, 3), -3.0, f32)
    vp = C.c_void_p
    arr = (_abi.TileRequest * 1)(rq)
    acc_p = (vp * 1)(acc.ctypes.data)
    hits = s["hits"].copy()

    def call(dq=None, reqs=arr, nn=n, accp=acc_p, planes=None, rgb=True, f=True, out_len=R * W * 3, sc=scene._h):
        pl = planes if planes is not None else (_abi.AovPlanes * 1)(_abi.AovPlanes(None, None, None, hits.ctypes.data, None))
        dq = dq if dq is not None else _dq(color_samples=8)
        return lib.rt_scene_denoise(sc, reqs, nn, C.byref(dq) if dq is not False else None, accp, pl,
                                    (vp * 1)(out.ctypes.data) if rgb else None, out_len, (vp * 1)(outf.ctypes.data) if f else None,
                                    None, None)

    BAD, LIMIT, SMALL = _abi.RT_ERR_BAD_ARG, _abi.RT_ERR_LIMIT, _abi.RT_ERR_BUFFER_TOO_SMALL
    dep = s["D"].copy()
    cases = [
        (BAD, dict(sc=None)), (BAD, dict(dq=False)), (BAD, dict(accp=None)), (BAD, dict(accp=(vp * 1)(None))),
        (BAD, dict(rgb=False, f=False)),
        (BAD, dict(planes=(_abi.AovPlanes * 1)(_abi.AovPlanes(None, None, dep.ctypes.data, None, None)))),
        (BAD, dict(dq=_dq(color_samples=0))), (BAD, dict(dq=_dq(color_samples=8, iterations=9))),
        (BAD, dict(dq=_dq(color_samples=8, flags=1))), (BAD, dict(dq=_dq(color_samples=8, reserved=1))),
        (BAD, dict(dq=_dq(color_samples=8, k_color=-1.0))), (BAD, dict(dq=_dq(color_samples=8, k_normal=float("inf")))),
        (BAD, dict(dq=_dq(color_samples=8, k_depth=float("nan")))), (BAD, dict(dq=_dq(color_samples=8, color_step_scale=0.0))),
        (BAD, dict(dq=_dq(color_samples=8, albedo_eps=0.0))),
        (LIMIT, dict(dq=_dq(color_samples=4097))),
        (SMALL, dict(out_len=R * W * 3 - 1)),
    ]
    for want, kw in cases:
        assert call(**kw) == want, kw
    # albedo given: aov_samples checked
    alb = s["A"].copy()
    pla = (_abi.AovPlanes * 1)(_abi.AovPlanes(alb.ctypes.data, None, None, None, None))
    assert call(dq=_dq(color_samples=8, aov_samples=0), planes=pla) == BAD
    assert call(dq=_dq(color_samples=8, aov_samples=5000), planes=pla) == LIMIT
    # strips: not consecutive, differing in a frame-level field, different sets of planes
    two = _frame(W, 2 * R, 2)
    acc2 = (vp * 2)(acc.ctypes.data, acc.ctypes.data)
    gap = (_abi.TileRequest * 2)(*_frame(W, 3 * R, 3)[0::2])
    pl2 = (_abi.AovPlanes * 2)(_abi.AovPlanes(None, None, None, hits.ctypes.data, None), _abi.AovPlanes(None, None, None, None, None))
    pl_same = (_abi.AovPlanes * 2)(_abi.AovPlanes(), _abi.AovPlanes())
    rq_b = _frame(W, 2 * R, 2)[1]
    rq_b.max_bounces += 1
    for reqs, pl in (((_abi.TileRequest * 2)(*two[::-1]), pl_same), (gap, pl_same), ((_abi.TileRequest * 2)(two[0], rq_b), pl_same),
                     ((_abi.TileRequest * 2)(*two), pl2)):
        assert lib.rt_scene_denoise(scene._h, reqs, 2, C.byref(_dq(color_samples=8)), acc2, pl, (vp * 2)(out.ctypes.data, out.ctypes.data),
                                    R * W * 3, None, None, None) == BAD
    # an output array with a NULL entry
    assert lib.rt_scene_denoise(scene._h, (_abi.TileRequest * 2)(*two), 2, C.byref(_dq(color_samples=8)), acc2, pl_same,
                                (vp * 2)(out.ctypes.data, None), R * W * 3, None, None, None) == BAD
    assert np.all(out == 77) and np.all(outf == f32(-3.0))
    # and a good call writes them
    assert call() == _abi.RT_OK and not np.all(out == 77)


_DEVICE_CHILD = r"""
import sys
import numpy as np
import torch                                                      # first: the library then binds to torch's HIP runtime
sys.path.insert(0, "tests")
import _denoise_np as dn
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _abi, scenes
from test_denoise_host import synthetic
rt.init()
dev = torch.device("cuda", 0)
f32 = np.float32
NAMES = ("albedo", "normal", "depth", "hits")
OUTS = ("rgb", "linear", "f32")


def frame(W, R, n):
    return [_abi.default_request(width=W, height=R, divisions=n, division_no=i, spp=16, seed=3) for i in range(n)]


def kw_np(dq):
    return dict(iterations=dq.iterations, k_color=f32(dq.k_color), color_step_scale=f32(dq.color_step_scale),
                k_normal=f32(dq.k_normal), k_depth=f32(dq.k_depth), albedo_eps=f32(dq.albedo_eps))


def upload(s, n, names):
    acc = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in np.split(s["C"], n, 0)]
    pl = []
    for i in range(n):
        d = {}
        for k in names:
            a = np.ascontiguousarray(np.split(s[k], n, 0)[i])
            if a.dtype == np.uint32:
                a = a.view(np.int32)
            d[k] = torch.from_numpy(a).to(dev)
        pl.append(d)
    return acc, pl


def outputs(n, hs, W):
    return [{"rgb": torch.full((hs, W, 3), 9, dtype=torch.uint8, device=dev),
             "linear": torch.full((hs, W, 3), -1.0, dtype=torch.float32, device=dev),
             "f32": torch.full((hs, W, 3), -1.0, dtype=torch.float32, device=dev)} for _ in range(n)]


def run(sc, reqs, dq, acc, pl, outs, scratch, nbytes=None, stream=0):
    sc.denoise_device(reqs, dq, [a.data_ptr() for a in acc], [{k: v.data_ptr() for k, v in d.items()} for d in pl],
                      scratch.data_ptr(), scratch.numel() if nbytes is None else nbytes,
                      d_rgb=[o["rgb"].data_ptr() for o in outs], d_f32=[o["f32"].data_ptr() for o in outs],
                      d_linear=[o["linear"].data_ptr() for o in outs], stream=stream)


def check(outs, want, what):
    for o in OUTS:
        got = np.concatenate([t[o].cpu().numpy() for t in outs], 0)
        g = got if got.dtype == np.uint8 else got.view(np.uint32)
        w = want[o] if want[o].dtype == np.uint8 else want[o].view(np.uint32)
        assert g.shape == w.shape and np.array_equal(g, w), (what, o, int((g != w).sum()))


with rt.Scene(0, rt.World(scenes.single_sphere())) as sc:
    for (R, W, n), names, it in [((1, 1, 1), NAMES, 3), ((3, 2, 1), (), 2), ((12, 67, 4), NAMES, 5), ((40, 129, 2), ("normal",), 8),
                                 ((66 * 2, 9, 66), NAMES, 5), ((24, 130, 3), ("albedo",), 0)]:
        rng = np.random.default_rng(R + W + n)
        s0 = synthetic(rng, R, W)
        s = {"C": s0["C"], "albedo": s0["A"], "normal": s0["N"], "depth": s0["D"], "hits": s0["hits"]}
        dq = _abi.DenoiseRequest.defaults(color_samples=8, aov_samples=4, iterations=it)
        want = dn.denoise(s["C"], 8, k=4, **{m: s[k] for k, m in zip(NAMES, ("A", "N", "D", "hits")) if k in names}, **kw_np(dq))
        acc, pl = upload(s, n, names)
        hs = R // n
        scratch = torch.empty(rt.denoise_scratch_bytes(W, R), dtype=torch.uint8, device=dev)
        outs = outputs(n, hs, W)
        torch.cuda.synchronize()
        sc.collect()
        run(sc, frame(W, R, n), dq, acc, pl, outs, scratch)
        torch.cuda.synchronize()
        st = sc.collect()
        assert st.n_launches >= 2 and st.kernel_ms > 0 and st.ray_segments == 0
        check(outs, want, ("device", R, W, n, names, it))
        # host form of the same call
        host, _ = sc.denoise(frame(W, R, n), np.split(s["C"], n, 0),
                             [{k: np.split(s[k], n, 0)[i] for k in names} for i in range(n)], 8, 4, dq, outputs=OUTS)
        for o in OUTS:
            assert np.concatenate([h[o] for h in host], 0).tobytes() == want[o].tobytes(), ("host", o)
        # repeated: the same bits
        outs2 = outputs(n, hs, W)
        run(sc, frame(W, R, n), dq, acc, pl, outs2, scratch)
        torch.cuda.synchronize()
        check(outs2, want, ("repeat", R, W))
        # a scratch one byte short: refused, nothing written
        outs3 = outputs(n, hs, W)
        try:
            run(sc, frame(W, R, n), dq, acc, pl, outs3, scratch, nbytes=scratch.numel() - 1)
            raise AssertionError("short scratch accepted")
        except rt.RtError as e:
            assert e.status == _abi.RT_ERR_BAD_ARG, e
        torch.cuda.synchronize()
        assert all(bool(torch.all(o["rgb"] == 9)) and bool(torch.all(o["f32"] == -1.0)) for o in outs3)

    # two streams, separate scratch, enqueued back to back: both match
    R, W, n = 256, 320, 4
    rng = np.random.default_rng(99)
    cases = []
    for j in range(2):
        s0 = synthetic(rng, R, W)
        s = {"C": s0["C"], "albedo": s0["A"], "normal": s0["N"], "depth": s0["D"], "hits": s0["hits"]}
        dq = _abi.DenoiseRequest.defaults(color_samples=8, aov_samples=4, iterations=5 - j)
        want = dn.denoise(s["C"], 8, k=4, A=s["albedo"], N=s["normal"], D=s["depth"], hits=s["hits"], **kw_np(dq))
        acc, pl = upload(s, n, NAMES)
        cases.append((dq, want, acc, pl, outputs(n, R // n, W),
                      torch.empty(rt.denoise_scratch_bytes(W, R), dtype=torch.uint8, device=dev), torch.cuda.Stream(device=dev)))
    torch.cuda.synchronize()
    for dq, want, acc, pl, outs, scratch, stream in cases:
        run(sc, frame(W, R, n), dq, acc, pl, outs, scratch, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    sc.collect()
    for j, (dq, want, acc, pl, outs, scratch, stream) in enumerate(cases):
        check(outs, want, ("stream", j))
print("DEVICE OK")
"""


def test_device_form_streams_and_repeats(ndev):
    """rt_scene_denoise_device on torch tensors: bit-exact, equal to the host form, repeatable, two streams with their own scratch,
    a scratch one byte short refused (in a child process that imports torch first: one HIP runtime for both)."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _DEVICE_CHILD], capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    assert r.returncode == 0 and "DEVICE OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
